"""Recorded Liu-West series without a GPU: the C ABI surface (declared, exported, every refusal that needs no handle returned with no
device present), the Python methods, the case list, and tests/cpp/test_lw_series_expect.cpp compiles and links.
test_lw_series_expect_gpu.py then asks the device for the rows."""
import ctypes as C
import os
import re

import numpy as np

import lw_edge_cases as lc
import lw_series_cases as sc
import lw_series_expect_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssme_lw_set_series_expectations", "ssme_lw_get_series_expectations")


def test_header_declares_and_library_exports_the_two_functions():
    text = open(os.path.join(ROOT, "include", "ssme_pf.h")).read()
    assert re.search(r"int\s+ssme_lw_set_series_expectations\(ssme_lw_handle h, int32_t enable\);", text)
    assert re.search(r"int\s+ssme_lw_get_series_expectations\(ssme_lw_handle h, const int32_t\* functionals, int32_t n,\s*"
                     r"double\* out(\s*/\*[^*]*\*/)?, int32_t T\);", text)
    from ssme_amd import _capi
    L = _capi.lib()
    for name in NEW:
        assert name in _capi.EXPORTS
        assert getattr(L, name) is not None


def test_refusals_with_no_device_present():
    """Everything that can be refused without a handle: a NULL handle comes first in both functions, whatever else is wrong."""
    from ssme_amd import _capi
    L = _capi.lib()
    for enable in (0, 1, 2, -1):
        assert L.ssme_lw_set_series_expectations(None, enable) == _capi.ERR_INVALID_ARG
    ids = np.arange(8, dtype=np.int32)
    ip = ids.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.full((2, 8, 1), -1.0)
    for args in ((ip, 8, _capi.dptr(out), 2), (None, 8, _capi.dptr(out), 2), (ip, 8, None, 2), (ip, 0, _capi.dptr(out), 2),
                 (ip, 9, _capi.dptr(out), 2), (ip, 8, _capi.dptr(out), 0)):
        assert L.ssme_lw_get_series_expectations(None, *args) == _capi.ERR_INVALID_ARG
    assert (out == -1.0).all()


def test_python_surface():
    import ssme_amd
    for cls in (ssme_amd.svol_lw_1_par, ssme_amd.svol_lw_2_par):
        for name in ("record_series_expectations", "series_expectations", "series_param_means"):
            assert callable(getattr(cls, name))


def test_the_list_covers_what_the_recording_can_get_wrong():
    names = [c["name"] for c in xc.all_cases()]
    assert len(set(names)) == len(names)
    assert xc.SIZES == (1, 2, 3, 63, 64, 65, 255, 256, 257, 500, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)
    assert all(c["T"] == 6 and lc.tiles(c["n"]) == 1 for c in xc.size_cases())
    assert {c["n"] for c in xc.size_cases()} == set(xc.SIZES) and max(xc.SIZES) == lc.TILE
    for v in (xc.VIRTUAL_THREADS // 4, xc.VIRTUAL_THREADS, 2 * xc.VIRTUAL_THREADS):       # a wave, one term -> two, 512
        assert {v - 1, v, v + 1} <= set(xc.SIZES)
    assert [(c["base"], c["rs"], c["T"]) for c in xc.schedule_cases() if c["form"] == 0] == [
        ("series-rs2", 2, 7), ("series-rs3", 3, 7), ("series-T1", 1, 1), ("series-T2", 1, 2)]
    assert {c["base"] for c in xc.degenerate_cases()} == set(sc.DEGENERATE)
    assert [(c["n"], lc.tiles(c["n"]), c["T"]) for c in xc.tiled_only_cases() if c["form"] == 0] == [(2049, 2, 4), (5000, 3, 4)]
    for group in (xc.size_cases(), xc.schedule_cases(), xc.degenerate_cases(), xc.tiled_only_cases(), xc.invisible_cases()):
        assert sorted(c["form"] for c in group) == [0] * (len(group) // 2) + [1] * (len(group) // 2)       # every case for both forms
    by = {c["name"]: c for c in xc.degenerate_cases()}
    assert by["nan-y-R3-form0"]["R"] == 3 and by["nan-y-R3-form0"]["y_set"] == {xc.NAN_Y_STEP: by["nan-y-R3-form0"]["y_set"][xc.NAN_Y_STEP]}
    assert {(c["rs"], c["form"]) for c in xc.invisible_cases()} == {(1, 0), (1, 1), (2, 0), (2, 1)}


def test_lw_series_expect_program_compiles_and_links():
    import test_lw_series_expect_cpp_gpu as cpp
    assert os.path.exists(cpp.build_program())
