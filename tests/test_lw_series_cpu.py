"""The whole-series Liu-West route without a GPU: the C ABI surface (declared, exported, argument checks before any HIP call) and the
case list of tests/lw_series_cases.py through the oracle alone -- every case reaches what it is listed for.
test_lw_series_gpu.py then asks the device for the same bits on the series route, the tiled route and the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lw_edge_cases as lc
import lw_series_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssme_lw_set_small_series", "ssme_lw_get_series_route")


def test_header_declares_and_library_exports_the_two_functions():
    text = open(os.path.join(ROOT, "include", "ssme_pf.h")).read()
    assert re.search(r"int\s+ssme_lw_set_small_series\(ssme_lw_handle h, int32_t enable\);", text)
    assert re.search(r"int\s+ssme_lw_get_series_route\(ssme_lw_handle h, int32_t\* route, int32_t\* threads_per_block\);", text)
    assert re.search(r"SSME_ROUTE_LW_SERIES\s*=\s*3", text)
    from ssme_amd import _capi
    assert _capi.ROUTE_LW_SERIES == 3
    L = _capi.lib()
    for name in NEW:
        assert name in _capi.EXPORTS
        assert getattr(L, name) is not None


def test_null_arguments_are_refused_before_any_hip_call():
    from ssme_amd import _capi
    L = _capi.lib()
    route, threads = C.c_int32(-1), C.c_int32(-1)
    assert L.ssme_lw_set_small_series(None, 1) == _capi.ERR_INVALID_ARG
    assert L.ssme_lw_set_small_series(None, 0) == _capi.ERR_INVALID_ARG
    assert L.ssme_lw_get_series_route(None, C.byref(route), C.byref(threads)) == _capi.ERR_INVALID_ARG
    assert (route.value, threads.value) == (-1, -1)


def test_python_surface():
    import ssme_amd
    for cls in (ssme_amd.svol_lw_1_par, ssme_amd.svol_lw_2_par):
        assert callable(cls.set_small_series) and callable(cls.series_route)
    assert ssme_amd.ROUTE_LW_SERIES == 3


def test_the_list_covers_what_the_kernel_can_get_wrong():
    names = {c["name"] for c in sc.all_cases()}
    assert len(names) == len(sc.all_cases())
    assert set(sc.SIZES) == {1, 2, 3, 63, 64, 65, 500, 1023, 1024, 1025, 2047, 2048} and max(sc.SIZES) == sc.ONE_TILE == lc.TILE
    assert lc.tiles(sc.ONE_TILE) == 1 and lc.tiles(sc.TILED_ONLY) == 2
    for c in sc.all_cases():
        assert lc.tiles(c["n"]) == 1 and c["form"] in (0, 1)
    assert {c["base"] for c in sc.degenerate_cases()} == set(sc.DEGENERATE)
    by = {c["name"]: c for c in sc.degenerate_cases()}
    assert by["huge-y-3030-form0"]["transforms"] == (3, 0, 3, 0)            # not the compiled-in set: the run-time switch
    assert by["nan-y-R3-form1"]["R"] == 3


@pytest.mark.parametrize("case", sc.all_cases(), ids=lambda c: c["name"])
def test_case_reaches_what_it_is_listed_for(oracle, case):
    run = lc.oracle_run(oracle, case)
    exp, T, n = case["expect"], case["T"], case["n"]
    ll = np.array([lls for lls, _ in run])
    assert ll.shape == (T, case["R"])
    if "nan_steps" in exp:
        for r in range(case["R"]):
            assert tuple(np.flatnonzero(np.isnan(ll[:, r]))) == tuple(exp["nan_steps"]), (case["name"], ll[:, r])
    if "big_step" in exp:
        assert ll[exp["big_step"], 0] < -1e5
    if exp.get("clamped_last"):                  # N = 1: every target's count is clamped to the last particle, N - 1 = 0
        for t in range(1, T):
            st = run[t][1][0]
            assert st["anc"].tolist() == [0] and st["kidx"].tolist() == [0] and not np.tril(st["L"]).any()
    for t in exp.get("no_draw_steps", ()):        # a step without a resampling draw: everyone continues itself
        assert np.array_equal(run[t][1][0]["anc"], np.arange(n)), t
    if case["rs"] > 1:
        for t in range(1, T):
            assert np.array_equal(run[t][1][0]["anc"], np.arange(n)) == (t % case["rs"] != 0), t
        assert any(not np.array_equal(run[t][1][0]["anc"], np.arange(n)) for t in range(1, T))
    if exp.get("L_zero") == "all":               # an all-zero Cholesky factor
        for t in range(1, T):
            assert not np.tril(run[t][1][0]["L"]).any()
    if "L_zero_diag" in exp:                     # mu == 0: moments that are exactly zero, the row and column of L that the guard zeroes
        for t in range(1, T):
            st = run[t][1][0]
            assert tuple(np.flatnonzero(np.diag(st["L"]) == 0.0)) == tuple(exp["L_zero_diag"])
            assert st["thetabar"][1] == 0.0
    if "collapsed_after" in exp:
        st = run[exp["collapsed_after"] + 1][1][0]
        assert np.unique(st["anc"]).size == 1 and lc.zero_denominator(run[exp["collapsed_after"]][1][0])
    if exp.get("x_nan_last"):
        assert np.isnan(run[-1][1][0]["x"]).all()
    if case["R"] > 1:                            # filters differ, so a leak between them would show
        assert len({run[-1][1][r]["theta"].tobytes() for r in range(case["R"])}) == case["R"]
