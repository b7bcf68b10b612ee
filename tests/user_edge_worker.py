"""Runs one user-model library (SSME_PF_LIB = a build of one of the headers of tests/user_edge_cases.py) in a process of its own -- a
process binds ONE libssme_pf.so -- over the lists of that file and writes what tests/test_user_edges_gpu.py compares with the oracle.
    python tests/user_edge_worker.py HEADER PART OUTDIR          PART: "edges" (the degenerate cases) or "book" (series bookkeeping)
The output is one pickled dict of numpy arrays per result key (user_edge_cases.key_file) in OUTDIR, read only by the test that started
the worker."""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssme_amd  # noqa: E402
from ssme_amd import _capi  # noqa: E402
import user_edge_cases as uc  # noqa: E402

header, part, out = sys.argv[1], sys.argv[2], sys.argv[3]
S = uc.HEADERS[header]
L = _capi.lib()
assert L.ssme_pf_user_model_dim_cov() == S["K"] and L.ssme_pf_user_model_has_first() == int(S["first"])
assert int(L.ssme_pf_user_model_n_h()) == S["n_h"]


class _Out(dict):
    def __setitem__(self, key, value):
        with open(os.path.join(out, uc.key_file(key)), "wb") as f:
            pickle.dump(value, f, protocol=pickle.HIGHEST_PROTOCOL)


res = _Out()


def make(case, route, rs, debug, graph=None):
    b = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, route["n"], case["R"], uc.SEED, rs, case["sched"], tile=route["tile"])
    assert b._dims() == (S["dx"], S["dy"]) and (b.tile, b.n_tiles) == uc.shape(case, route)[1:3]
    b.set_small_series(bool(route["small"]))
    b.set_debug(debug, debug, split_level2=route["split"])
    if graph is not None:
        b.set_graph_mode(graph)
    b.set_params(np.asarray(case["theta"], dtype=np.float64))
    return b


def states(b, R, debug):
    """Every filter's download, stacked: x [R, dx, N], (logw, anc in debug mode), cdf, A, mb, m, S, rshift."""
    sts = [b.state(r, ancestors=debug, logw=debug) for r in range(R)]
    o = dict(x=np.stack([np.asarray(s["x"]).reshape(S["dx"], -1) for s in sts]), cdf=np.stack([s["cdf"] for s in sts]),
             A=np.stack([s["A"] for s in sts]), mb=np.stack([s["mb"] for s in sts]), m=np.array([s["m"] for s in sts]),
             S=np.array([s["S"] for s in sts], dtype=np.uint64), rshift=np.array([s["rshift"] for s in sts]))
    if debug:
        o["logw"], o["anc"] = np.stack([s["logw"] for s in sts]), np.stack([s["anc"] for s in sts])
    return o


def stepped(b, y, Z, R):
    """The step API over a series (covariates by value): per step the log conditional likelihoods, every state and the functionals."""
    steps = []
    for t in range(len(y)):
        ll = b.step(y[t], None if Z is None else Z[t])
        steps.append(dict(ll=ll, ue=b.user_expectations() if S["n_h"] else None, **states(b, R, True)))
    return steps


def series(b, y, Z, R):
    """run_series (covariates from the table): the sum, per_step(), every state and the functionals."""
    tot = b.run_series(y, Z)
    return dict(tot=tot, per=b.per_step(), ue=b.user_expectations() if S["n_h"] else None, **states(b, R, False))


if part == "edges":
    for case, route in uc.pairs(header):
        pid = uc.pair_id((case, route))
        y, Z = uc.series(header, case)
        yc, Zc = uc.series(header, uc.clean(case))
        R = case["R"]
        if route["kind"] != "small":
            # GENERAL form: the step API in debug mode, resamplers 0-3; a clean_tail case goes on after reset() with the healthy series
            for rs in (0, 1, 2, 3):
                b = make(case, route, rs, True)
                g = dict(steps=stepped(b, y, Z, R), loglik=b.loglik())
                if case["clean_tail"]:
                    b.reset()
                    g["tail"] = stepped(b, yc, Zc, R)
                res[f"G|{pid}|{rs}"] = g
                b.close()
        # HOT form: run_series without debug flags, resamplers 0 and 1, eager and captured graph (the whole-series kernels are not
        # captured: the small routes run eagerly only); second pass on the same handle (the healthy series for a clean_tail case)
        for rs in (0, 1):
            for graph in ((False,) if route["kind"] == "small" else (False, True)):
                b = make(case, route, rs, False, graph)
                h = dict(first=series(b, y, Z, R))
                h["second"] = series(b, yc, Zc, R) if case["clean_tail"] else series(b, y, Z, R)
                if route["kind"] == "small":
                    b.set_small_series(False)          # the same handle, now through the tiled kernel
                    h["small_off"] = series(b, y, Z, R)
                elif header in uc.VECTOR and route["n"] <= 2048 and not graph:
                    b.set_small_series(True)           # a vector model has no whole-series kernel: the switch is ignored
                    h["small_on"] = series(b, y, Z, R)
                res[f"H|{pid}|{rs}|{int(graph)}"] = h
                b.close()
elif part == "book":
    R = uc.BOOK_R
    th = S["theta"]
    case = dict(R=R, T=0, sched=1, theta=th)
    for n, tile, small in uc.BOOK_SHAPES:
        route = dict(n=n, tile=tile, small=small, split=None)
        for graph in (False, True):
            key = f"B|{n}|{tile}|{int(small)}|{int(graph)}"
            for T in (1, 2):                                     # the shortest series, each on a fresh handle
                b = make(case, route, 0, False, graph)
                y, Z = uc.book_series(header, T)
                res[f"{key}|fresh{T}"] = series(b, y, Z, R)
                b.close()
            for with_z in (True, False):                         # 2, then 40, then 6 steps on ONE handle: zbuf regrows at K per row, the graph is recaptured
                b = make(case, route, 0, False, graph)
                for T in uc.BOOK_LENGTHS:
                    y, Z = uc.book_series(header, T, with_z)
                    res[f"{key}|chain{int(with_z)}|{T}"] = series(b, y, Z, R)
                if with_z:                                       # and the has_z flag of the graph key: NULL after Z and Z after NULL, same length
                    y, Z = uc.book_series(header, 6)
                    res[f"{key}|flip|null"] = series(b, y, None, R)
                    res[f"{key}|flip|z"] = series(b, y, Z, R)
                b.close()
            # run_series(T = 3), three more steps through the step API, reset(), one step: `first` at step 0 only, and again after reset
            b = make(case, route, 0, False, graph)
            y, Z = uc.book_series(header, 6)
            d = dict(head=series(b, y[:3], Z[:3], R))
            d["ll"] = np.stack([b.step(y[t], Z[t]) for t in (3, 4, 5)])
            d["after"] = states(b, R, False)
            d["ue"] = b.user_expectations()
            b.reset()
            d["ll0"] = b.step(y[0], Z[0])
            res[f"{key}|continue"] = d
            b.close()
else:
    raise SystemExit("PART is edges or book")
