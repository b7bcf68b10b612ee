"""Recorded series (ssme_pf_set_series_expectations) without a GPU: the three entry points are exported and declared, validate their
arguments before any HIP call, and the adaptor's program compiles and links.  On the GPU: tests/test_series_expectations_gpu.py."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssme_pf_set_series_expectations", "ssme_pf_get_series_expectations", "ssme_pf_get_series_user_expectations")
SRC = os.path.join(ROOT, "tests", "cpp", "test_series_expect.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_series_expect")


def build_program(so=None, exe=EXE, user=False):
    """tests/cpp/test_series_expect.cpp against the stock library, or (user) against a library with svol_reg_cov.h compiled in."""
    from ssme_amd import build
    so = so or build.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread"] + (["-DSERIES_EXPECT_USER"] if user else []) +
                          [SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    return exe


def test_symbols_exported_and_declared():
    from ssme_amd import _capi
    L = _capi.lib()
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for n in NEW:
        assert n in _capi.EXPORTS and hasattr(L, n)
        assert getattr(L, n).restype is C.c_int
    assert list(L.ssme_pf_set_series_expectations.argtypes) == [C.c_void_p, i32p, C.c_int32, C.c_int32]
    assert list(L.ssme_pf_get_series_expectations.argtypes) == [C.c_void_p, dp, C.c_int32]
    assert list(L.ssme_pf_get_series_user_expectations.argtypes) == [C.c_void_p, dp, C.c_int32]
    hdr = open(os.path.join(ROOT, "include", "ssme_pf.h")).read()
    for n in NEW:
        assert f"int {n}(ssme_pf_handle h" in hdr


def test_null_handle_is_invalid_arg_without_a_device():
    from ssme_amd import _capi
    L = _capi.lib()
    ids = (C.c_int32 * 2)(0, 2)
    buf = (C.c_double * 8)()
    assert L.ssme_pf_set_series_expectations(None, ids, 2, 0) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_set_series_expectations(None, None, 0, 0) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_get_series_expectations(None, buf, 1) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_get_series_user_expectations(None, buf, 1) == _capi.ERR_INVALID_ARG


def test_python_interface_present():
    import ssme_amd
    for m in ("record_series_expectations", "series_expectations", "series_user_expectations"):
        assert callable(getattr(ssme_amd.ParticleFilterBank, m))


def test_adaptor_program_compiles_and_links():
    assert os.path.exists(build_program())


@pytest.mark.gpu
def test_adaptor_program_stock():
    """svol_log_like_evaluator: record_expectations / series_expectations against a stepped handle, lane and pair kernel."""
    exe = build_program()
    out = subprocess.check_output([exe, os.path.join(ROOT, "tests", "golden", "spy_returns.csv")], text=True, timeout=120)
    vals = dict(line.split(" ", 1) for line in out.strip().splitlines())
    for n in (500, 1500):
        assert int(vals[f"n{n}_rows"]) == 48
        assert int(vals[f"n{n}_equals_stepping"]) == 1 and int(vals[f"n{n}_loglik_unchanged"]) == 1
        assert float(vals[f"n{n}_vol_last"]) > 0.0
        assert int(vals[f"n{n}_off_throws"]) == 1
        # what a run recorded is read at ITS size whatever the evaluator was told since
        for k in ("off_then_read", "shrink_then_read", "bad_id_rejected", "after_rejection_x_alone", "grow_then_read"):
            assert int(vals[f"n{n}_{k}"]) == 1, (n, k)


@pytest.mark.gpu
def test_adaptor_program_user_model():
    """user_log_like_evaluator<1, 1, 3> on svol_reg_cov: built-ins and the header's functionals, lane, pair and tiled route."""
    from ssme_amd import build
    so = build.build_user_model(os.path.join(ROOT, "tests", "models", "svol_reg_cov.h"), "svol_reg_cov")
    exe = build_program(so, os.path.join(ROOT, "tests", "cpp", "test_user_series_expect"), user=True)
    out = subprocess.check_output([exe], text=True, timeout=120)
    vals = dict(line.split(" ", 1) for line in out.strip().splitlines())
    for n in (500, 1500, 3000):
        assert int(vals[f"n{n}_equals_stepping"]) == 1 and int(vals[f"n{n}_user_equals_stepping"]) == 1
        assert int(vals[f"n{n}_user_rows"]) == 12
        for k in ("off_then_read", "bad_id_rejected", "rejected_then_read", "grow_then_read", "user_off_throws"):
            assert int(vals[f"n{n}_{k}"]) == 1, (n, k)
        assert int(vals[f"n{n}_two_ids_rows"]) == 12
