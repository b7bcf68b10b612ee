"""Marginal smoothing without a device: the new entry points are declared, exported and bound; every refusal that needs no device comes
back before any HIP call; tests/marginal_ref.py agrees with a brute-force Fraction evaluation on hand-built histories (N <= 4), a step
without weight and a column made degenerate by a NaN density included; the life cycle of the rows (ssme_amd/csrc/marginal_state.h)
holds in a stand-alone program; the C++ program of the adaptor test compiles and links."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np

import backward_ref as br
import marginal_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ssme_pf_marginal_smoothing_bytes", "ssme_pf_download_smoothing_weights", "ssme_pf_get_marginal_smoothed_expectations")


def test_symbols_declared_exported_and_bound():
    """Fails without the feature: none of the three symbols exists before it."""
    import ssme_amd
    from ssme_amd import _capi
    header = open(os.path.join(ROOT, "include", "ssme_pf.h")).read()
    L = _capi.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in _capi.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    for m in ("marginal_smoothing_bytes", "smoothing_weights", "marginal_smoothed_expectations"):
        assert callable(getattr(ssme_amd.ParticleFilterBank, m)), m
    hpp = open(os.path.join(ROOT, "include", "ssme_gpu", "bsfilter_gpu.hpp")).read()
    assert hpp.count(" smoothing_weights(std::size_t r, std::size_t t)") == 2 and hpp.count(" marginal_smoothed_expectations(const") == 2
    assert L.ssme_pf_version() >= 334


def test_refusals_that_need_no_device():
    from ssme_amd import _capi
    L = _capi.lib()
    ids = (C.c_int32 * 4)(0, 1, 2, 3)
    buf = np.zeros(64)
    b = C.c_uint64()
    assert L.ssme_pf_marginal_smoothing_bytes(None, 4, C.byref(b)) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_download_smoothing_weights(None, 0, 0, None, _capi.dptr(buf)) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_get_marginal_smoothed_expectations(None, ids, 1, _capi.dptr(buf), 4) == _capi.ERR_INVALID_ARG
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
    GPU: tests/test_marginal_gpu.py)."""
    from ssme_amd import _capi
    ids = (C.c_int32 * 4)(0, 1, 2, 3)
    bad_ids = (C.c_int32 * 2)(0, 4)
    neg_ids = (C.c_int32 * 1)(-1)
    buf = np.zeros(max(4 * 4 * max(r, 16), n))
    b = C.c_uint64()
    tile, tiles = C.c_int32(), C.c_int32()
    assert L.ssme_pf_get_layout(h, C.byref(tile), C.byref(tiles)) == _capi.OK
    npad = tile.value * tiles.value
    assert L.ssme_pf_marginal_smoothing_bytes(h, 0, C.byref(b)) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_marginal_smoothing_bytes(h, 4, None) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_marginal_smoothing_bytes(h, 4, C.byref(b)) == _capi.OK and b.value == 32 * 4 * r * npad
    shared = C.c_uint64()
    assert L.ssme_pf_backward_bytes(h, 4, C.byref(shared)) == _capi.OK and 4 * shared.value == b.value
    for f, t, out in ((-1, 0, buf), (r, 0, buf), (0, -1, buf), (0, 0, None)):
        assert L.ssme_pf_download_smoothing_weights(h, f, t, None, _capi.dptr(out)) == _capi.ERR_INVALID_ARG
    for fs, k, out, T in ((None, 1, buf, 4), (ids, 0, buf, 4), (ids, 5, buf, 4), (bad_ids, 2, buf, 4), (neg_ids, 1, buf, 4), (ids, 1, None, 4),
                          (ids, 1, buf, 0)):
        assert L.ssme_pf_get_marginal_smoothed_expectations(h, fs, k, _capi.dptr(out), T) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_download_smoothing_weights(h, 0, 0, None, _capi.dptr(buf)) == _capi.ERR_STATE         # nothing recorded
    assert L.ssme_pf_download_smoothing_weights(h, 0, 0, _capi.dptr(buf), _capi.dptr(buf)) == _capi.ERR_STATE
    assert L.ssme_pf_get_marginal_smoothed_expectations(h, ids, 4, _capi.dptr(buf), 4) == _capi.ERR_STATE


def test_rows_life_cycle_without_a_device(tmp_path):
    """ssme_amd/csrc/marginal_state.h: the rows are filled once per history, stale after every call that moves the handle on -- whether or
    not backward simulation refilled the log-weights in between -- and their buffer goes with the history rows
    (tests/cpp/test_marginal_state.cpp).  pf_api.hip tells the state of every event of the history's own state."""
    exe = str(tmp_path / "test_marginal_state")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_marginal_state.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
    api = open(os.path.join(ROOT, "ssme_amd", "csrc", "pf_api.hip")).read()
    # every event of the history's state is followed by the marginal rows' (on the same line or the next statement)
    for event, forwarded, least in ((r"h->hist\.moved_on\(\);", r"h->msm\.moved_on\(\);", 3), (r"h->hist\.rows_dropped\(\);", r"h->msm\.dropped\(\);", 2),
                                    (r"h->hist\.recorded\(T\);", r"h->msm\.moved_on\(\);", 1), (r"own_free\(h, h->bs_lw\);", r"own_free\(h, h->ms_rows\);", 2)):
        assert len(re.findall(event, api)) == len(re.findall(event + r"\s*" + forwarded, api)) >= least, event


# ---- the restatement against a brute-force evaluation --------------------------------------------------------------------------------
TH = (0.9, 0.7, 1.0)


def _hand_history(rng, T, n, dead_step=None, nan_column=None):
    """A hand-built history of one scalar filter.  dead_step = t: every log-weight of step t is -inf, so every column of step t + 1 is
    degenerate.  nan_column = (t, j): x_{t}[j] = NaN, so the density to it is NaN from every particle: column j of step t alone is."""
    xs = [rng.normal(size=(1, n)) for _ in range(T)]
    lws = [rng.normal(size=n) * 2.0 for _ in range(T)]
    if n > 1:
        for t in range(T):
            lws[t][rng.integers(n)] = -np.inf              # a dead particle per step
    if dead_step is not None:
        lws[dead_step][:] = -np.inf
    if nan_column is not None:
        xs[nan_column[0]][0, nan_column[1]] = np.nan
    ancs = [rng.integers(0, n, size=n) for _ in range(T)]
    w = np.abs(rng.normal(size=n)) + 0.01
    if n > 2:
        w[rng.integers(n)] = 0.0                           # a final particle without weight
    return xs, lws, ancs, w


def _check(O, T, n, sched, **kw):
    rng = np.random.default_rng(1000 * T + 10 * n + sched)
    xs, lws, ancs, w = _hand_history(rng, T, n, **kw)
    logf = br.logf_builtin(O, br.MODEL_LIN_GAUSS, TH)
    om, degenerate = mr.filter_rows(O, logf, xs, lws, ancs, sched, w)
    exact = mr.brute_force(O, logf, xs, lws, ancs, sched, w)
    assert om.shape == (T, n)
    assert np.array_equal(om[T - 1], w)
    for t in range(T):
        # one side of the device tolerance: the restatement's own roundings against the exact rational rows
        b = Fraction(mr.bound(T, n, t)) / 2
        for i in range(n):
            got, want = Fraction(float(om[t, i])), exact[t][i]
            assert (got == 0) == (want == 0), (t, i, got, want)
            assert abs(got - want) <= b * want, (t, i, float(got), float(want))
        assert sum(exact[t]) == sum(exact[T - 1]), t                            # the exact rows keep the mass exactly
    return degenerate, om


def test_restatement_against_brute_force():
    from oracle import oracle as O
    for T, n, sched in ((1, 1, 1), (2, 1, 1), (4, 1, 2), (2, 2, 1), (3, 2, 2), (4, 3, 1), (4, 3, 2), (3, 4, 1), (4, 4, 2)):
        assert _check(O, T, n, sched)[0] == 0, (T, n, sched)
    # N = 1: q = D = 2^sh, every row is w_0 to the bit
    om = _check(O, 4, 1, 1)[1]
    assert (om == om[3, 0]).all()


def test_restatement_pushes_a_step_without_weight_down_the_genealogy():
    from oracle import oracle as O
    for sched in (1, 2):
        rng = np.random.default_rng(1000 * 4 + 10 * 4 + sched)
        xs, lws, ancs, w = _hand_history(rng, 4, 4, dead_step=1)
        degenerate, om = _check(O, 4, 4, sched, dead_step=1)
        assert degenerate == 4                             # the four columns of step 2, into step 1
        want = np.zeros(4)
        for j in range(4):
            want[mr.parent(ancs, 1, j, 4, sched)] += om[2, j]
        # at most three additions of non-negative terms per entry, in another order
        np.testing.assert_allclose(om[1], want, rtol=3 * 2.0 ** -53, atol=0)
        assert mr.parent(ancs, 1, 2, 4, 1) == min(int(ancs[2][2]), 3) and mr.parent(ancs, 1, 2, 4, 3) == 2


def test_restatement_treats_a_nan_density_as_a_degenerate_column():
    from oracle import oracle as O
    for sched in (1, 2):
        degenerate, om = _check(O, 4, 4, sched, nan_column=(2, 1))
        # column 1 of step 2 is degenerate (into step 1); as a ROW of step 2 the particle has NaN densities to step 3: no weight
        assert degenerate == 1 and om[2, 1] == 0.0 and np.isfinite(om).all()


def test_chunked_columns_equal_one_chunk():
    """The restatement's chunks of columns are an order of summation, nothing more: 5 particles in chunks of 2 against one chunk."""
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    xs, lws, ancs, w = _hand_history(rng, 3, 5)
    logf = br.logf_builtin(O, br.MODEL_LIN_GAUSS, TH)
    one = mr.filter_rows(O, logf, xs, lws, ancs, 1, w)[0]
    keep = mr.CHUNK
    try:
        mr.CHUNK = 2
        two = mr.filter_rows(O, logf, xs, lws, ancs, 1, w)[0]
    finally:
        mr.CHUNK = keep
    np.testing.assert_allclose(two, one, rtol=8 * 2.0 ** -53, atol=0)


def test_cpp_program_compiles():
    """tests/cpp/test_marginal.cpp, which uses the new methods of both evaluators, compiles and links against the C ABI (the one build
    without a device; tests/test_cpp_marginal.py runs the program on the GPU)."""
    import test_cpp_marginal
    assert os.path.exists(test_cpp_marginal.build_program())
