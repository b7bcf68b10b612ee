"""The MODEL_USER0 instantiations of the step kernels (csrc/pf_kernels.h: k_filter_step with VEC / KC > 0; csrc/pf_small.h:
k_filter_series_lane, k_filter_series_small with KC > 0; csrc/model_api.h: cov_step, first / first_logw) at the degenerate inputs of
tests/user_edge_cases.py, on the routes that file lists, and the series bookkeeping of a covariate table with K values per row
(csrc/pf_api.hip: zbuf, set_last_z, the graph keyed by T and has_z).  Six headers (scalar, VEC 2x2, VEC 3x1, scalar K = 3 with and
without `first`, VEC 2x2 K = 4 with `first`), every one run ONCE per part in a process of its own (user_edge_worker.py with
SSME_PF_LIB; a process binds one libssme_pf.so, each under its own timeout); the tests compare what it wrote with the oracle closures
of user_edge_cases.py (proved equal to those of user_cov_ref.py / oracle_models.py in test_user_edges_cpu.py), bit for bit, NaN for
NaN, every filter of the handle:
  * GENERAL form -- the step API with set_debug(True, True, split_level2 = route), resamplers 0-3, covariates BY VALUE (z_now,
    z_now_v[j - 1]; y_now, y_now_v[d - 1]): after every step x (all planes), log-weights, integer cdf, ancestors, tile sums and
    maxima, m, S and the log conditional likelihood; loglik();
  * HOT form -- run_series without debug flags, resamplers 0 and 1, eager and captured graph (the small routes eagerly only),
    covariates FROM THE TABLE (a.z[yi * KC + j]; the prefetch of pf_small.h): per_step(), the sum, final x, cdf, tile sums, m, S; a
    second pass on the same handle; on the small routes a third pass with set_small_series(False) on the same handle; for the vector
    headers at N <= 2048 a pass with set_small_series(True), which must change nothing;
  * user_expectations() of the headers with n_h: all NaN where the step left S = 0, within expect_ref.budget_fixed_point of
    expect_ref.expect_fixed_point on the downloaded state, with the covariates of that step, where it left weight;
  * a case whose cloud is NaN to the end of the series (clean_tail) goes on on the same handle: reset() and the healthy series through
    the step API, the healthy series as the second run_series -- both against the oracle.

    route                  N        tile  B     hot form of a SCALAR header (KC = 0 and KC = 3)         hot form of a VECTOR header
    small-1 / -64          1, 64    2048  1     k_filter_series_lane<64>                                -- (scalar headers only)
    small-100              100      2048  1     k_filter_series_lane<128>                               --
    small-200              200      2048  1     k_filter_series_lane<256>                               --
    small-300              300      2048  1     k_filter_series_lane<512>                               --
    small-1000             1000     2048  1     k_filter_series_small<512, 1>                           --
    small-2000             2000     2048  1     k_filter_series_small<512, 2>                           --
    edge-n1 .. edge-n2049  1..2049  2048  1, 2  k_filter_step<512, BIG=0, 2048, RS, WL2=1> (small off)  the same, VEC (switch ignored)
    wl2-512                1613     512   4     k_filter_step<256, BIG=0, 512, RS, WL2=1>               the same, VEC
    wl2-2048               6221     2048  4     k_filter_step<512, BIG=0, 2048, RS, WL2=1>              the same, VEC
    split-forced-5         2125     512   5     k_filter_step<256, BIG=1, 512, RS, WL2=0>               the same, VEC
    tables-5               2125     512   5     k_filter_step<256, BIG=1, 512, RS, WL2=0> + k_level2_plan  the same, VEC
All of them are MODEL = MODEL_USER0.  With svol_reg_cov.h and svol_reg_cov_nofirst.h the six whole-series rows are the KC = 3
instantiations -- k_filter_series_lane<64 | 128 | 256 | 512> and k_filter_series_small<512, 1 | 2> with the covariate prefetch and
cov_step -- which RUN here (before, only lane<512> did); with svol_two_factor_cov.h the tiled rows are VEC with KC = 4.  RS = 0 / 1 for
resamplers 0 / 1 from step 1 on (step 0, every step of schedule 3 and the general form run RS = -1); the small routes with
set_small_series(False) and the general form at N <= 2048 run k_filter_step<512, BIG=0, 2048, RS, WL2=1>.

Why no address depends on data in what a user model adds (read from the code before the first run; the searches, level-2 kernels and
their clamps are those of the stock path, argued in test_bootstrap_edges_gpu.py):
  * `srcv`, the index at which components d >= 1 are gathered (a.x_in[d * xplane + rowoff + srcv]), is 0 and UNREAD at the first step
    (xv[d] = first_step ? 0.0 : ...); on a step that does not resample it is the particle's own index i_first + 2 (k NT + tid) + c
    < B * TILE <= N_pad, a function of the thread alone (beyond N it reads the zeroed padding of the plane and the result is overwritten
    by the ragged block); on a resampling step it is the ancestor AFTER the clamp to N - 1 (staged path: `anc < a.N - 1 ? anc : a.N - 1`;
    probe path: probe_ancestor clamps).  A plane is R * N_pad doubles and the buffer dim_x planes (pf_api.hip: own_alloc of np * dx), so
    d * xplane + rowoff + srcv < dim_x * R * N_pad for every d < dim_x.
  * the table indices are a.y[yi * DY + d] and a.z[yi * KC + j] with yi < T <= Tcap, d < DY, j < KC: below Tcap * dim_y and
    Tcap * K, the sizes ensure_series_buffers allocates (kz = K per row).  The whole-series kernels read row 0 before the loop and row
    t + 1 under `t + 1 < T`; a.z == NULL is tested before every read.
  * by value, y_now_v[d - 1] and z_now_v[j - 1] are indexed by the unrolled loop counters d < DY <= 4, j < KC <= 4: arrays of 3.
  * particles beyond N (ragged last tile): component 0 and every plane d >= 1 are stored as 0, the log-weight as -inf, whatever the
    model returned for them -- NaN included.
  * a NaN or infinite y, z, x or log-weight is only ever a VALUE: cov_step, first, first_logw, prop and logg compute on it; `bad` selects
    -inf after the model calls.  user_expect.h evaluates h under j < nvalid only.
The reading found no unclamped index and no unguarded load.  (The SSME_F32 staging of ssme_pf_run_series rounds T values of y: it
relies on ssme_pf_create refusing SSME_F32 for every model with dim_x > 1 or dim_y > 1, so dim_y = 1 there.)
The NaN, infinite and `bad` cases run first when the module is run in two invocations (-k "not bookkeeping" / -k bookkeeping)."""
import atexit
import os
import pickle
import shutil
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import expect_ref as er
import user_edge_cases as uc
from test_liu_west_edges_gpu import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "models")
pytestmark = pytest.mark.gpu

ITEMS = [(h, p, form) for h in uc.HEADERS for p in uc.pairs(h) for form in ("general", "hot") if not (form == "general" and p[1]["kind"] == "small")]


def _iid(it):
    return f"{it[0]}-{uc.pair_id(it[1])}-{it[2]}"


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a HIP device"
    import ssme_amd
    return ssme_amd


_TMP = []


_WORKERS = {}


def _run(header, part):
    """The directory the worker wrote for one library and part: built once, STARTED once per session.  A worker that failed -- a
    non-zero exit, a signal, its time limit -- is not started again, and no OTHER worker is started after it either: every later
    test that needs one fails with the first error, so that this module runs nothing more on the device after a fault."""
    key = (header, part)
    first = next((e for e in _WORKERS.values() if isinstance(e, Exception)), None)
    if key not in _WORKERS and first is not None:
        _WORKERS[key] = first
    if key not in _WORKERS:
        try:
            from ssme_amd import build
            so = build.build_user_model(os.path.join(MODELS, header + ".h"), uc.HEADERS[header]["lib"])
            out = tempfile.mkdtemp(prefix=f"user_edges_{header}_{part}_")
            if not _TMP:
                atexit.register(lambda: [shutil.rmtree(d, ignore_errors=True) for d in _TMP])
            _TMP.append(out)
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "user_edge_worker.py"), header, part, out],
                           env=dict(os.environ, SSME_PF_LIB=so), check=True, timeout=600)
            _WORKERS[key] = out
        except Exception as e:          # remembered, not retried
            _WORKERS[key] = e
    if isinstance(_WORKERS[key], Exception):
        raise RuntimeError(f"a worker failed and none is started after it ({header}, {part}): {_WORKERS[key]!r}") from _WORKERS[key]
    return _WORKERS[key]


def _load(header, part, key):
    with open(os.path.join(_run(header, part), uc.key_file(key)), "rb") as f:
        return pickle.load(f)


_LAST = [None]


def _oracle_run(oracle, header, case, route, rs):
    if _LAST[0] != header:                      # the tests are header-major: one header's oracle runs are held at a time
        uc.forget_runs()
        _LAST[0] = header
    return uc.oracle_run(oracle, header, case, route, rs)


def compare_state(g, r, o, name, debug, anc):
    """Filter r of the worker's stacked download against the oracle's state, bit for bit."""
    same_bits(g["x"][r], o["x"], name + ": particles, all planes")
    if debug:
        same_bits(g["logw"][r], o["logw"], name + ": log-weights")
        if anc:
            np.testing.assert_array_equal(g["anc"][r], o["anc"], err_msg=name + ": ancestors")
    np.testing.assert_array_equal(g["cdf"][r], o["cdf"], err_msg=name + ": integer cdf")
    np.testing.assert_array_equal(g["A"][r], o["A"], err_msg=name + ": tile sums")
    same_bits(g["mb"][r], o["mb"], name + ": tile maxima")
    same_bits([g["m"][r]], [o["m"]], name + ": maximum")
    assert int(g["S"][r]) == o["S"] and int(g["rshift"][r]) == o["rshift"], (name, g["S"][r], o["S"])


def check_functionals(oracle, header, ue, g, r, o, th, zc, tile, name):
    """user_expectations() of filter r against the state the device downloaded (equal to the oracle's `o`: compared before)."""
    s = uc.HEADERS[header]
    assert ue.shape[0] == s["n_h"]
    if o["S"] == 0:
        assert np.isnan(ue[:, r]).all(), (name, ue[:, r])
        return 0
    # (the log-weights enter the budget alone; run_series without debug flags keeps none on the device, so they are the oracle's)
    st = er.make_state(oracle, dict(x=g["x"][r][0], cdf=g["cdf"][r], A=g["A"][r], mb=g["mb"][r], m=float(g["m"][r]), logw=o["logw"]), tile)
    h = uc.h_rows(oracle, header, th, g["x"][r], zc)
    assert np.isfinite(h).all(), name
    eq, bud = er.expect_fixed_point(h, st), er.budget_fixed_point(h, st)
    for k in range(s["n_h"]):
        err = float(abs(Fraction(float(ue[k, r])) - eq[k]))
        print("FUNCTIONAL", name, "h", k, "device", ue[k, r], "E_q", float(eq[k]), "error", err, "budget_fixed_point", float(bud[k]))
        assert err <= bud[k], (name, k, ue[k, r], float(eq[k]), err, bud[k])
    return 1


def _zrow(header, Z, t):
    return np.zeros(max(uc.HEADERS[header]["K"], 1)) if Z is None else Z[t]


def _general(oracle, header, case, route):
    n, tile, B, T = uc.shape(case, route)
    R, pid = case["R"], uc.pair_id((case, route))
    y, Z = uc.series(header, case)
    probes = uc.probes(case) if uc.HEADERS[header]["n_h"] and n <= uc.FUNCTIONAL_MAX_N else ()
    checked = 0
    for rs in (0, 1, 2, 3):
        assert uc.route_of(header, case, route, "general", rs)[4] == -1
        g = _load(header, "edges", f"G|{pid}|{rs}")
        legs = [(g["steps"], _oracle_run(oracle, header, case, route, rs), Z, "")]
        if case["clean_tail"]:
            cc = uc.clean(case)
            legs.append((g["tail"], _oracle_run(oracle, header, cc, route, rs), uc.series(header, cc)[1], " after reset()"))
        for steps, run, Zl, tag in legs:
            for t in range(T):
                name = f"{header} {pid} rs={rs}{tag} t={t}"
                same_bits(steps[t]["ll"], run[t][0], name + ": log conditional likelihood")
                resampled = t > 0 and t % case["sched"] == 0
                for r in range(R):
                    compare_state(steps[t], r, run[t][1][r], f"{name} r={r}", True, resampled)
                    if resampled:
                        assert steps[t]["anc"][r].max() < n
                    if rs == 0 and t in probes:
                        checked += check_functionals(oracle, header, steps[t]["ue"], steps[t], r, run[t][1][r], case["theta"][r], _zrow(header, Zl, t),
                                                     tile, f"{name} r={r}")
        run = legs[0][1]                          # (loglik() was read before the reset of a clean_tail case)
        same_bits(g["loglik"], np.array([sum((run[t][0][r] for t in range(T)), 0.0) for r in range(R)]), f"{header} {pid} rs={rs}: loglik()")
    if probes:
        assert checked >= 1, "a functional was compared where weight was left"


def _series_leg(oracle, header, got, run, R, T, name):
    want_ll = np.array([[run[t][0][r] for t in range(T)] for r in range(R)])
    want_sum = np.array([sum((run[t][0][r] for t in range(T)), 0.0) for r in range(R)])
    same_bits(got["per"], want_ll, name + ": per_step()")
    same_bits(got["tot"], want_sum, name + ": the returned sum")
    assert (np.isnan(got["tot"]) == np.isnan(want_ll).any(axis=1)).all(), name
    for r in range(R):
        compare_state(got, r, run[T - 1][1][r], f"{name} r={r}", False, False)


def _hot(oracle, header, case, route):
    n, tile, B, T = uc.shape(case, route)
    R, pid = case["R"], uc.pair_id((case, route))
    y, Z = uc.series(header, case)
    s = uc.HEADERS[header]
    for rs in (0, 1):
        run = _oracle_run(oracle, header, case, route, rs)
        kern = uc.route_of(header, case, route, "hot", rs)[0]
        assert kern.startswith("k_filter_series") == (route["kind"] == "small")
        second, Z2 = (run, Z)
        if case["clean_tail"]:
            cc = uc.clean(case)
            second, Z2 = _oracle_run(oracle, header, cc, route, rs), uc.series(header, cc)[1]
        for graph in ((False,) if route["kind"] == "small" else (False, True)):
            h = _load(header, "edges", f"H|{pid}|{rs}|{int(graph)}")
            name = f"{header} {pid} rs={rs} {'graph' if graph else 'eager'} ({kern})"
            _series_leg(oracle, header, h["first"], run, R, T, name)
            _series_leg(oracle, header, h["second"], second, R, T, name + " (second pass)")
            assert ("small_off" in h) == (route["kind"] == "small")
            if "small_off" in h:
                _series_leg(oracle, header, h["small_off"], run, R, T, name + " (set_small_series(False), same handle)")
            assert ("small_on" in h) == (header in uc.VECTOR and n <= 2048 and not graph)
            if "small_on" in h:
                _series_leg(oracle, header, h["small_on"], run, R, T, name + " (set_small_series(True) on a vector model)")
            if s["n_h"] and rs == 0 and not graph and n <= uc.FUNCTIONAL_MAX_N and case["name"] not in uc.NO_FUNCTIONALS:
                for r in range(R):
                    check_functionals(oracle, header, h["first"]["ue"], h["first"], r, run[T - 1][1][r], case["theta"][r], _zrow(header, Z, T - 1), tile,
                                      f"{name} r={r} after run_series")
                    check_functionals(oracle, header, h["second"]["ue"], h["second"], r, second[T - 1][1][r], case["theta"][r], _zrow(header, Z2, T - 1),
                                      tile, f"{name} r={r} after the second pass")


@pytest.mark.parametrize("item", ITEMS, ids=_iid)
def test_pair(sa, oracle, item):
    header, (case, route), form = item
    (_general if form == "general" else _hot)(oracle, header, case, route)


# ---- series bookkeeping ----------------------------------------------------------------------------------------------------------
BOOK = [(h, shp, graph) for h in uc.BOOK_HEADERS for shp in uc.BOOK_SHAPES for graph in (False, True)]


def _book_leg(oracle, header, got, n, tile, T, with_z, name, t_used=None):
    """One run_series of `T` steps against a FRESH oracle pair of that length (covariates drawn per length)."""
    per, sts = uc.book_oracle(oracle, header, n, tile, T, with_z)
    R = uc.BOOK_R
    same_bits(got["per"], per, name + ": per_step()")
    same_bits(got["tot"], np.array([sum((per[r, t] for t in range(T)), 0.0) for r in range(R)]), name + ": the returned sum")
    assert np.isfinite(per).all()
    Z = uc.book_series(header, T, with_z)[1]
    for r in range(R):
        compare_state(got, r, sts[r], f"{name} r={r}", False, False)
        check_functionals(oracle, header, got["ue"], got, r, sts[r], uc.HEADERS[header]["theta"][r], _zrow(header, Z, T - 1), tile,
                          f"{name} r={r}: functionals with row T - 1")


@pytest.mark.parametrize("header,shp,graph", BOOK, ids=lambda v: str(v).replace(" ", ""))
def test_series_bookkeeping(sa, oracle, header, shp, graph):
    """T = 1 and T = 2 on fresh handles; 2, then 40, then 6 steps on ONE handle with Z and with z = NULL (each equal to the fresh oracle
    pair of that length, covariates drawn per length so that a stale or mis-strided row changes the bits; the functionals receive row
    T - 1); z = NULL after Z and Z after NULL at one length; run_series(3) + three steps == six steps, `first` at step 0 only and again
    after reset()."""
    n, tile, small = shp
    if _LAST[0] != header:
        uc.forget_runs()
        _LAST[0] = header
    key = f"B|{n}|{tile}|{int(small)}|{int(graph)}"
    tag = f"{header} N={n} tile={tile} small={small} {'graph' if graph else 'eager'}"
    for T in (1, 2):
        _book_leg(oracle, header, _load(header, "book", f"{key}|fresh{T}"), n, tile, T, True, f"{tag} fresh T={T}")
    for with_z in (True, False):
        for T in uc.BOOK_LENGTHS:
            _book_leg(oracle, header, _load(header, "book", f"{key}|chain{int(with_z)}|{T}"), n, tile, T, with_z,
                      f"{tag} T={T} in the chain 2, 40, 6 ({'Z' if with_z else 'z = NULL'})")
    _book_leg(oracle, header, _load(header, "book", f"{key}|flip|null"), n, tile, 6, False, f"{tag} z = NULL after Z")
    _book_leg(oracle, header, _load(header, "book", f"{key}|flip|z"), n, tile, 6, True, f"{tag} Z after z = NULL")
    # a stale row would show: the lengths' covariates differ, and Z differs from zeros
    a, b = uc.book_oracle(oracle, header, n, tile, 6, True)[0], uc.book_oracle(oracle, header, n, tile, 6, False)[0]
    assert not np.array_equal(a, b)
    assert not np.array_equal(uc.book_series(header, 6)[1][:2], uc.book_series(header, 2)[1])
    # run_series(T = 3), three steps, reset(), one step
    d = _load(header, "book", f"{key}|continue")
    per, sts = uc.book_oracle(oracle, header, n, tile, 6, True)
    same_bits(d["head"]["per"], per[:, :3], tag + ": run_series(T = 3)")
    same_bits(d["ll"].T, per[:, 3:], tag + ": three steps after run_series(T = 3)")
    Z = uc.book_series(header, 6)[1]
    for r in range(uc.BOOK_R):
        compare_state(d["after"], r, sts[r], f"{tag} r={r}: state after run_series(3) + 3 steps", False, False)
        check_functionals(oracle, header, d["ue"], d["after"], r, sts[r], uc.HEADERS[header]["theta"][r], Z[5], tile, f"{tag} r={r}: functionals after the steps")
    same_bits(d["ll0"], per[:, 0], tag + ": the first step after reset() takes `first` again")
