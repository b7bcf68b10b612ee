"""The whole-series kernels (pf_small.h) of VECTOR user models at N <= 2048: the route query, both routes bit for bit on one handle,
the oracle, a long series, degenerate inputs and the hand-over to the step API, the functionals and the forecast.  The lists are
tests/vector_series_cases.py; one process per library runs them (tests/vector_series_worker.py).  Every comparison is exact.

test_route_of_vector_handles is the test that fails without the feature: the query is missing there, and a vector handle would
answer ROUTE_TILED.  The stock handle and the SSME_ERR_* statuses are in test_route_query_stock_and_statuses."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import user_edge_cases as uc
import vector_series_cases as vc
from test_liu_west_edges_gpu import same_bits
from test_user_edges_gpu import compare_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "models")
pytestmark = pytest.mark.gpu
TIMEOUT = {"stock": 120, "route": 120, "parity": 420, "long": 120, "edges": 300, "handover": 120, "forecast": 120}
_DONE = {}


def _worker(lib, part, tmp_path_factory):
    """What the worker pickled for (lib, part): started once per session; a worker that failed is not started again, and none after it."""
    key = (lib, part)
    first = next((e for e in _DONE.values() if isinstance(e, Exception)), None)
    if key not in _DONE and first is not None:
        _DONE[key] = first
    if key not in _DONE:
        try:
            env = dict(os.environ)
            if lib != "stock":
                from ssme_amd import build
                s = vc.LIBS.get(lib) or vc.FORECAST_LIBS[lib]
                env["SSME_PF_LIB"] = build.build_user_model(os.path.join(MODELS, s["header"] + ".h"), lib)
            else:
                env.pop("SSME_PF_LIB", None)
            out = str(tmp_path_factory.mktemp(f"vs_{lib}_{part}") / "res.pkl")
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vector_series_worker.py"), lib, part, out], env=env, check=True,
                           timeout=TIMEOUT[part])
            with open(out, "rb") as f:
                _DONE[key] = pickle.load(f)
        except Exception as e:          # remembered, not retried
            _DONE[key] = e
    if isinstance(_DONE[key], Exception):
        raise RuntimeError(f"a worker failed and none is started after it ({lib}, {part}): {_DONE[key]!r}") from _DONE[key]
    return _DONE[key]


def same_run(a, b, name, debug=False):
    """Two passes (worker's run()) equal bit for bit: sums, per_step(), every plane of x, cdf, tile sum and maximum, m and S."""
    same_bits(a["tot"], b["tot"], name + ": sums")
    same_bits(a["per"], b["per"], name + ": per_step()")
    same_state(a, b, name, debug)


def same_state(a, b, name, debug=False):
    same_bits(a["x"], b["x"], name + ": particles, all planes")
    np.testing.assert_array_equal(a["cdf"], b["cdf"], err_msg=name + ": integer cdf")
    np.testing.assert_array_equal(a["A"], b["A"], err_msg=name + ": tile sums")
    same_bits(a["mb"], b["mb"], name + ": tile maxima")
    same_bits(a["m"], b["m"], name + ": m")
    np.testing.assert_array_equal(a["S"], b["S"], err_msg=name + ": S")
    if debug:
        same_bits(a["logw"], b["logw"], name + ": log-weights")
        np.testing.assert_array_equal(a["anc"], b["anc"], err_msg=name + ": ancestors")


def three_equal(d, name, n, debug=False):
    """series -> tiled -> series on one handle: the routes the worker asked for were taken, and all three passes are the same bits."""
    assert tuple(d["series"]["route"]) == vc.expected_route(n) and tuple(d["again"]["route"]) == vc.expected_route(n), (name, d["series"]["route"])
    assert d["tiled"]["route"][0] == vc.ROUTE_TILED, name
    same_run(d["series"], d["tiled"], name + ": whole-series == tiled", debug)
    same_run(d["again"], d["tiled"], name + ": whole-series again == tiled", debug)


# ---- route --------------------------------------------------------------------------------------------------------------------------
def test_route_of_vector_handles(tmp_path_factory):
    """FAILS WITHOUT THE FEATURE.  A fresh two_factor handle (no step, no switch): the lane kernel with 512 threads at N = 500, the pair
    kernel at N = 1500, the tiled kernel at N = 2049 and with 512-particle tiles; set_small_series(False) -> tiled.  The default of
    every (kernel, dim_x) class is the whole-series route (profiles/vector_series_timing.txt)."""
    r = _worker("two_factor", "route", tmp_path_factory)
    assert tuple(r["n500"]["fresh"]) == (vc.ROUTE_SERIES_LANE, 512)
    assert tuple(r["n1500"]["fresh"]) == (vc.ROUTE_SERIES_PAIR, 512)
    assert tuple(r["n64"]["fresh"]) == (vc.ROUTE_SERIES_LANE, 64) and tuple(r["n65"]["fresh"]) == (vc.ROUTE_SERIES_LANE, 128)
    for key in ("n2049", "n500-tile512"):
        assert all(r[key][k][0] == vc.ROUTE_TILED for k in ("fresh", "on", "off")), (key, r[key])
    for key, n in (("n500", 500), ("n1500", 1500), ("n64", 64), ("n65", 65)):
        assert tuple(r[key]["on"]) == vc.expected_route(n) and r[key]["off"][0] == vc.ROUTE_TILED, (key, r[key])


def test_route_query_stock_and_statuses(tmp_path_factory):
    """A stock SVOL handle at N = 100: the lane kernel with 128 threads; NULL arguments and a sharded handle."""
    from ssme_amd import _capi
    r = _worker("stock", "stock", tmp_path_factory)
    assert tuple(r["svol-100"]) == (vc.ROUTE_SERIES_LANE, 128) and r["svol-100-off"][0] == vc.ROUTE_TILED
    assert r["null-handle"] == r["null-route"] == r["null-threads"] == _capi.ERR_INVALID_ARG
    assert r["sharded"] == _capi.ERR_STATE


# ---- both routes, bit for bit, on one handle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", list(vc.LIBS))
def test_both_routes_same_bits_on_one_handle(lib, tmp_path_factory):
    r = _worker(lib, "parity", tmp_path_factory)
    for n in vc.SIZES:
        for rs in vc.RESAMPLERS:
            for sched in vc.SCHEDULES:
                for debug in (False, True):
                    three_equal(r[(n, rs, sched, debug)], f"{lib} N={n} rs={rs} sched={sched} debug={debug}", n, debug)


@pytest.mark.parametrize("lib", list(vc.LIBS))
def test_whole_series_route_matches_oracle(lib, oracle, tmp_path_factory):
    """oracle.UserVectorModelFilter for every filter (lin_gauss_4d_h through oracle_models._lin_gauss_4d_oracle)."""
    r = _worker(lib, "parity", tmp_path_factory)
    for n in vc.ORACLE_SIZES:
        for rs in vc.ORACLE_RESAMPLERS:
            for sched in ((1, 3) if n in (65, 1025) else (1,)):
                per, sts = vc.oracle_series(oracle, lib, n, rs, sched)
                g = r[(n, rs, sched, True)]["series"]
                name = f"{lib} N={n} rs={rs} sched={sched}"
                same_bits(g["per"], per, name + ": per_step()")
                for f in range(vc.R):
                    same_bits([g["tot"][f]], [vc.series_sum(per[f])], name + f" filter {f}: sum")
                    compare_state(g, f, sts[f], name + f" filter {f}", True, sched == 1)


# ---- long series ----------------------------------------------------------------------------------------------------------------------
def test_long_series_accounting_and_buffer_reuse(oracle, tmp_path_factory):
    """T = 300 (series_accounting replays five 64-step loads), then T = 40 and T = 300 again on the same handle."""
    c = vc.LONG
    r = _worker(c["lib"], "long", tmp_path_factory)
    for i, T in enumerate((c["T"],) + c["then"]):
        three_equal(r[(i, T)], f"long pass {i} T={T}", c["n"])
        per, sts = vc.oracle_series(oracle, c["lib"], c["n"], 0, 1, T=T, nfilters=c["R"])
        g = r[(i, T)]["series"]
        same_bits(g["per"], per, f"long pass {i} T={T}: per_step()")
        for f in range(c["R"]):
            same_bits([g["tot"][f]], [vc.series_sum(per[f])], f"long pass {i} T={T} filter {f}: the series sum")
            compare_state(g, f, sts[f], f"long pass {i} T={T} filter {f}", False, False)


# ---- degenerate inputs ----------------------------------------------------------------------------------------------------------------
_nan_eq = same_bits            # NaN for NaN, everything else bit for bit


def _edge_vs_oracle(g, steps, R, T, name):
    """A worker pass of T steps against the oracle's steps (user_edge_cases.oracle_run): NaN for NaN, everything else bit for bit."""
    per = np.array([[steps[t][0][f] for t in range(T)] for f in range(R)])
    _nan_eq(g["per"], per, name + ": per_step()")
    for f in range(R):
        _nan_eq([g["tot"][f]], [vc.series_sum(per[f])], name + f" filter {f}: sum")
        o = steps[T - 1][1][f]
        _nan_eq(g["x"][f], o["x"], name + f" filter {f}: particles, all planes")
        _nan_eq(g["logw"][f], o["logw"], name + f" filter {f}: log-weights")
        np.testing.assert_array_equal(g["cdf"][f], o["cdf"], err_msg=name + ": integer cdf")
        np.testing.assert_array_equal(g["A"][f], o["A"], err_msg=name + ": tile sums")
        _nan_eq(g["mb"][f], o["mb"], name + ": tile maxima")
        _nan_eq([g["m"][f]], [o["m"]], name + ": m")
        assert int(g["S"][f]) == o["S"], name


@pytest.mark.parametrize("lib", list(vc.EDGE_CASES))
def test_degenerate_inputs_both_kernels(lib, oracle, tmp_path_factory):
    r = _worker(lib, "edges", tmp_path_factory)
    header = vc.LIBS[lib]["edge"]
    uc.forget_runs()
    for name in vc.EDGE_CASES[lib]:
        case = uc.case_of(header, name)
        for n in vc.EDGE_SHAPES:
            for rs in vc.EDGE_RESAMPLERS:
                d, tag = r[(name, n, rs)], f"{lib} {name} N={n} rs={rs}"
                assert tuple(d["series"]["route"]) == vc.expected_route(n) and d["tiled"]["route"][0] == vc.ROUTE_TILED, tag
                for k in ("series", "tiled", "again"):
                    _edge_vs_oracle(d[k], uc.oracle_run(oracle, header, case, vc.edge_route(n), rs), case["R"], case["T"], f"{tag} ({k})")
                if case["clean_tail"]:
                    _edge_vs_oracle(d["tail"], uc.oracle_run(oracle, header, uc.clean(case), vc.edge_route(n), rs), case["R"], case["T"],
                                    tag + " (healthy series after reset)")
    uc.forget_runs()


# ---- hand-over ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["two_factor", "svol_two_factor_cov", "lin_gauss_4d_h"])
def test_hand_over_to_step_api_and_functionals(lib, tmp_path_factory):
    """run_series(T = 3), three step() calls, reset() and one step; user_expectations() after the series: the same after both routes."""
    r = _worker(lib, "handover", tmp_path_factory)
    for n in (300, 1500):
        s, t = r[(n, True)], r[(n, False)]
        assert tuple(s["head"]["route"]) == vc.expected_route(n) and t["head"]["route"][0] == vc.ROUTE_TILED
        same_run(s["head"], t["head"], f"{lib} N={n}: head")
        same_bits(s["ll"], t["ll"], f"{lib} N={n}: three steps after the series")
        same_state(s["after"], t["after"], f"{lib} N={n}: state after the steps")
        same_bits(s["ll0"], t["ll0"], f"{lib} N={n}: first step after reset()")
        same_state(s["after0"], t["after0"], f"{lib} N={n}: state after reset() and one step")
        assert (s["ue"] is None) == (lib == "two_factor")
        if s["ue"] is not None:
            assert np.isfinite(s["ue"]).all()
            same_bits(s["ue"], t["ue"], f"{lib} N={n}: user_expectations() after the series")


@pytest.mark.parametrize("lib", ["two_factor_g", "lin_gauss_4d_g", "svol_two_factor_cov"])
def test_forecast_after_series(lib, tmp_path_factory):
    """sim_future_obs(H = 3) (observations, states, start draw) after a series on either route."""
    r = _worker(lib, "forecast", tmp_path_factory)
    for n in (300, 1500):
        s, t = r[(n, True)], r[(n, False)]
        assert tuple(s["head"]["route"]) == vc.expected_route(n) and t["head"]["route"][0] == vc.ROUTE_TILED
        same_run(s["head"], t["head"], f"{lib} N={n}: series")
        assert "fc" in s and "fc" in t, "the header declares its observation draw"
        for a, b, what in zip(s["fc"], t["fc"], ("y", "x", "start")):
            assert np.isfinite(np.asarray(a, dtype=np.float64)).all()
            same_bits(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), f"{lib} N={n}: forecast {what}")
