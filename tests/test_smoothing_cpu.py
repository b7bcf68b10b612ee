"""Smoothing without a device: the five entry points are declared, exported and bound; every refusal that needs no device comes back
before any HIP call; tests/smooth_ref.py agrees with a genealogy written out by hand."""
import ctypes as C
import os
import re

import numpy as np

import smooth_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ssme_pf_set_series_history", "ssme_pf_series_history_bytes", "ssme_pf_sample_trajectories",
           "ssme_pf_get_smoothed_expectations", "ssme_pf_smoothing_elapsed_ms")


def test_symbols_declared_exported_and_bound():
    from ssme_amd import _capi
    header = open(os.path.join(ROOT, "include", "ssme_pf.h")).read()
    L = _capi.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in _capi.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    import ssme_amd
    for m in ("record_series_history", "series_history_bytes", "sample_trajectories", "smoothed_expectations"):
        assert callable(getattr(ssme_amd.ParticleFilterBank, m))
    hpp = open(os.path.join(ROOT, "include", "ssme_gpu", "bsfilter_gpu.hpp")).read()
    for m in ("record_history", "sample_trajectories", "smoothed_expectations"):
        assert hpp.count("    " + m + "(") + hpp.count(" " + m + "(std::") + hpp.count(" " + m + "(const") + hpp.count(" " + m + "(bool") >= 2, m


def test_refusals_that_need_no_device():
    """NULL handles and NULL outputs are SSME_ERR_INVALID_ARG.  With a handle (where a device exists) every argument check comes back
    before any HIP call and an unrecorded handle is SSME_ERR_STATE; without a device no handle can be made: SSME_ERR_HIP."""
    from ssme_amd import _capi
    L = _capi.lib()
    ids = (C.c_int32 * 4)(0, 1, 2, 3)
    buf = np.zeros(64)
    idx = np.zeros(64, dtype=np.uint32)
    b = C.c_uint64()
    ms = C.c_float()
    assert L.ssme_pf_set_series_history(None, 1) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_series_history_bytes(None, 4, C.byref(b)) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_sample_trajectories(None, 1, None, _capi.dptr(buf), None, 4) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_get_smoothed_expectations(None, ids, 1, _capi.dptr(buf), 4) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_smoothing_elapsed_ms(None, C.byref(ms), C.byref(ms)) == _capi.ERR_INVALID_ARG
    cfg = _capi.Config(model=0, n_particles=8, n_filters=2, dtype=0, resampler=0, resamp_sched=1, seed=1, device=0)
    h = C.c_void_p()
    rc = L.ssme_pf_create(C.byref(cfg), C.byref(h))
    assert rc in (_capi.OK, _capi.ERR_HIP)                 # no device: nothing computes on the CPU
    if rc != _capi.OK:
        assert not h.value
        return
    try:
        refusals_with_a_handle(L, h)
    finally:
        L.ssme_pf_destroy(h)


def refusals_with_a_handle(L, h, n=8, r=2):
    """Every refusal of a handle of r filters of n particles that has recorded nothing, checked before any HIP call (also run on the
    GPU: tests/test_smoothing_gpu.py)."""
    from ssme_amd import _capi
    ids = (C.c_int32 * 4)(0, 1, 2, 3)
    buf = np.zeros(4 * 4 * max(r, 16))
    idx = np.zeros(buf.size, dtype=np.uint32)
    b = C.c_uint64()
    tile, tiles = C.c_int32(), C.c_int32()
    assert L.ssme_pf_get_layout(h, C.byref(tile), C.byref(tiles)) == _capi.OK
    npad = tile.value * tiles.value
    assert L.ssme_pf_set_series_history(h, 2) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_set_series_history(h, -1) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_series_history_bytes(h, 0, C.byref(b)) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_series_history_bytes(h, 4, None) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_series_history_bytes(h, 4, C.byref(b)) == _capi.OK and b.value == 4 * r * npad * 12
    bad_term = np.zeros(r, dtype=np.uint32)
    bad_term[-1] = n
    for K, term, out in ((0, None, buf), (n + 1, None, buf), (1, None, None), (1, bad_term, buf)):
        assert L.ssme_pf_sample_trajectories(h, K, _capi.u32ptr(term), _capi.dptr(out), _capi.u32ptr(idx), 4) == _capi.ERR_INVALID_ARG
    for k, f, out in ((0, ids, buf), (5, ids, buf), (1, None, buf), (1, ids, None), (1, (C.c_int32 * 1)(4), buf), (1, (C.c_int32 * 1)(-1), buf)):
        assert L.ssme_pf_get_smoothed_expectations(h, f, k, _capi.dptr(out), 4) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_sample_trajectories(h, 1, None, _capi.dptr(buf), None, 4) == _capi.ERR_STATE       # nothing recorded
    assert L.ssme_pf_get_smoothed_expectations(h, ids, 1, _capi.dptr(buf), 4) == _capi.ERR_STATE
    assert L.ssme_pf_set_series_history(h, 1) == _capi.OK
    assert L.ssme_pf_get_smoothed_expectations(h, ids, 1, _capi.dptr(buf), 4) == _capi.ERR_STATE          # no run_series yet
    assert L.ssme_pf_set_series_history(h, 0) == _capi.OK


def test_history_state_rules_without_a_device(tmp_path):
    """ssme_amd/csrc/series_history.h, the host-side rules of when a history is in force, driven through run_series' sequences by a
    stand-alone program: after a REFUSED allocation of larger rows the earlier history is not in force (its rows are freed), a
    failed series records nothing, and the handle records again afterwards."""
    import subprocess
    exe = str(tmp_path / "test_history_state")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_history_state.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
    api = open(os.path.join(ROOT, "ssme_amd", "csrc", "pf_api.hip")).read()
    # the handle keeps no second copy of that state and asks query() before it touches the rows
    assert "SeriesHistoryState hist;" in api and "h->hist.query(h->hist_x && h->hist_anc, T)" in api
    assert not re.search(r"->hist_(T|cap|on)\b", api)


def test_genealogy_by_hand():
    """Four particles, three steps, resamp_sched = 2: step 1 does not resample (its debug ancestors are stale and must be ignored),
    step 2 does."""
    stale = np.array([3, 3, 3, 3])
    ancs = [np.array([9, 9, 9, 9]), stale, np.array([2, 0, 0, 3])]
    B = sr.genealogy(ancs, sched=2)
    np.testing.assert_array_equal(B, [[2, 0, 0, 3], [2, 0, 0, 3], [0, 1, 2, 3]])
    xs = [np.array([10.0, 11.0, 12.0, 13.0]), np.array([20.0, 21.0, 22.0, 23.0]), np.array([30.0, 31.0, 32.0, 33.0])]
    x = sr.lineage_states(xs, B)
    assert x.shape == (4, 3, 1)
    np.testing.assert_array_equal(x[:, :, 0], [[12, 22, 30], [10, 20, 31], [10, 20, 32], [13, 23, 33]])
    # every step resamples: both ancestor rows are chased
    B1 = sr.genealogy([ancs[0], np.array([1, 1, 2, 0]), ancs[2]], sched=1)
    np.testing.assert_array_equal(B1, [[2, 1, 1, 0], [2, 0, 0, 3], [0, 1, 2, 3]])
    # a vector state: both planes follow the one lineage
    xv = [np.stack([x0, -x0]) for x0 in xs]
    v = sr.lineage_states(xv, B)
    assert v.shape == (4, 3, 2)
    np.testing.assert_array_equal(v[:, :, 1], -v[:, :, 0])
    np.testing.assert_array_equal(v[:, :, 0], x[:, :, 0])
    assert not sr.resampled(0, 1) and sr.resampled(1, 1) and not sr.resampled(1, 2) and sr.resampled(2, 2)


def test_cpp_program_compiles():
    """tests/cpp/test_smoothing.cpp, which uses the new methods of both evaluators, compiles and links against the C ABI (the one
    build without a device; tests/test_cpp_smoothing.py runs the program on the GPU)."""
    import test_cpp_smoothing
    assert os.path.exists(test_cpp_smoothing._build())
