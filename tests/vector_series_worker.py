"""Runs one library in a process of its own (a process binds ONE libssme_pf.so: SSME_PF_LIB = a build of one of the headers of
tests/vector_series_cases.py, or unset for the stock library) over the lists of that file and pickles what
tests/test_vector_series_gpu.py compares.
    python tests/vector_series_worker.py LIB PART OUT.pkl
PART: route | parity | long | edges | handover | forecast | stock"""
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
import vector_series_cases as vc  # noqa: E402

lib, part, out = sys.argv[1], sys.argv[2], sys.argv[3]
S = vc.LIBS.get(lib) or vc.FORECAST_LIBS.get(lib)
res = {}


def make(n, R, rs, sched, theta, debug=False, tile=0):
    b = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, n, R, vc.SEED, rs, sched, tile=tile)
    assert b._dims() == (S["dx"], S["dy"])
    if debug:
        b.set_debug(True, True)
    b.set_params(np.asarray(theta, dtype=np.float64))
    return b


def states(b, R, debug):
    sts = [b.state(r, ancestors=debug, logw=debug) for r in range(R)]
    o = dict(x=np.stack([np.asarray(s["x"]).reshape(S["dx"], -1) for s in sts]), cdf=np.stack([s["cdf"] for s in sts]),
             A=np.stack([s["A"] for s in sts]), mb=np.stack([s["mb"] for s in sts]), m=np.array([s["m"] for s in sts]),
             S=np.array([s["S"] for s in sts], dtype=np.uint64), rshift=np.array([s["rshift"] for s in sts]))
    if debug:
        o["logw"], o["anc"] = np.stack([s["logw"] for s in sts]), np.stack([s["anc"] for s in sts])
    return o


def run(b, y, Z, R, debug=False):
    tot = b.run_series(y, Z)
    return dict(tot=tot, per=b.per_step(), route=b.series_route(), **states(b, R, debug))


def three_passes(b, y, Z, R, debug=False):
    """The whole-series route, then the tiled kernel on the same handle, then the whole-series route again."""
    b.set_small_series(True)
    first = run(b, y, Z, R, debug)
    b.set_small_series(False)
    tiled = run(b, y, Z, R, debug)
    b.set_small_series(True)
    return dict(series=first, tiled=tiled, again=run(b, y, Z, R, debug))


if part == "stock":
    L = _capi.lib()
    b = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_SVOL, 100, 1, seed=1)
    res["svol-100"] = b.series_route()
    b.set_small_series(False)
    res["svol-100-off"] = b.series_route()
    import ctypes as C
    r, t = C.c_int32(), C.c_int32()
    res["null-handle"] = L.ssme_pf_get_series_route(None, C.byref(r), C.byref(t))
    res["null-route"] = L.ssme_pf_get_series_route(b._h, None, C.byref(t))
    res["null-threads"] = L.ssme_pf_get_series_route(b._h, C.byref(r), None)
    b.close()
    sh = C.c_void_p()
    cfg = _capi.Config(model=0, n_particles=4096, n_filters=1, dtype=0, resampler=0, resamp_sched=1, seed=1, device=0, first_filter_id=0,
                       tile_particles=0, n_filters_total=0)
    _capi.check(L.ssme_pf_shard_create(C.byref(cfg), 0, 2, C.byref(sh)))
    res["sharded"] = L.ssme_pf_get_series_route(sh, C.byref(r), C.byref(t))
    L.ssme_pf_destroy(sh)
elif part == "route":
    th = S["theta"][0]
    for key, n, tile in (("n500", 500, 0), ("n1500", 1500, 0), ("n2049", 2049, 0), ("n500-tile512", 500, 512), ("n64", 64, 0), ("n65", 65, 0)):
        b = make(n, 1, 0, 1, th, tile=tile)
        d = dict(fresh=b.series_route())                    # no prior step, no set_small_series
        b.set_small_series(True)
        d["on"] = b.series_route()
        b.set_small_series(False)
        d["off"] = b.series_route()
        res[key] = d
        b.close()
elif part == "parity":
    y, Z = vc.series(lib, vc.T)
    for n in vc.SIZES:
        for rs in vc.RESAMPLERS:
            for sched in vc.SCHEDULES:
                for debug in (False, True):
                    b = make(n, vc.R, rs, sched, S["theta"], debug)
                    res[(n, rs, sched, debug)] = three_passes(b, y, Z, vc.R, debug)
                    b.close()
elif part == "long":
    c = vc.LONG
    b = make(c["n"], c["R"], 0, 1, S["theta"][:c["R"]])
    for i, T in enumerate((c["T"],) + c["then"]):
        y, Z = vc.series(lib, T)
        res[(i, T)] = three_passes(b, y, Z, c["R"])
    b.close()
elif part == "edges":
    for name in vc.EDGE_CASES[lib]:
        case = uc.case_of(S["edge"], name)
        y, Z = uc.series(S["edge"], case)
        yc, Zc = uc.series(S["edge"], uc.clean(case))
        for n in vc.EDGE_SHAPES:
            for rs in vc.EDGE_RESAMPLERS:
                b = make(n, case["R"], rs, case["sched"], case["theta"], True)
                d = three_passes(b, y, Z, case["R"], True)
                if case["clean_tail"]:                      # the healthy series after reset() on the same handle
                    b.reset()
                    d["tail"] = run(b, yc, Zc, case["R"], True)
                res[(name, n, rs)] = d
                b.close()
elif part == "handover":
    y, Z = vc.series(lib, 6)
    z = lambda t: None if Z is None else Z[t]
    for n in (300, 1500):
        for small in (True, False):
            b = make(n, vc.R, 0, 1, S["theta"])
            b.set_small_series(small)
            d = dict(head=run(b, y[:3], None if Z is None else Z[:3], vc.R))
            d["ue"] = b.user_expectations() if int(_capi.lib().ssme_pf_user_model_n_h()) else None
            d["ll"] = np.stack([b.step(y[t], z(t)) for t in (3, 4, 5)])
            d["after"] = states(b, vc.R, False)
            b.reset()
            d["ll0"] = b.step(y[0], z(0))
            d["after0"] = states(b, vc.R, False)
            res[(n, small)] = d
            b.close()
elif part == "forecast":
    y, Z = vc.series(lib, 5)
    for n in (300, 1500):
        for small in (True, False):
            b = make(n, len(S["theta"]), 0, 1, S["theta"])
            b.set_small_series(small)
            d = dict(head=run(b, y, Z, len(S["theta"])))
            if ssme_amd.user_model_has_gsamp():
                zf = None if Z is None else np.arange(3 * S["K"], dtype=np.float64).reshape(3, S["K"]) * 0.125
                d["fc"] = b.sim_future_obs(3, last_obs=y[-1, 0], states=True, start=True, z_future=zf)
            res[(n, small)] = d
            b.close()
else:
    raise SystemExit("unknown PART")

with open(out, "wb") as f:
    pickle.dump(res, f, protocol=pickle.HIGHEST_PROTOCOL)
