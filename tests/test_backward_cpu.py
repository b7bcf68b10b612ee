"""Backward-simulation smoothing without a device: the new entry points are declared, exported and bound and the stock library
declares no user transition density; every refusal that needs no device comes back before any HIP call; tests/backward_ref.py agrees
with a brute-force Fraction evaluation on hand-built histories (N <= 8), a degenerate transition included; the life cycle of the
log-weight rows (ssme_amd/csrc/series_history.h) holds in a stand-alone program."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import backward_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ssme_pf_user_model_has_logf", "ssme_pf_backward_bytes", "ssme_pf_download_series_logweights",
           "ssme_pf_sample_trajectories_backward")


def test_symbols_declared_exported_and_bound():
    """Fails without the feature: none of the four symbols exists before it."""
    import ssme_amd
    from ssme_amd import _capi
    header = open(os.path.join(ROOT, "include", "ssme_pf.h")).read()
    L = _capi.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in _capi.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert L.ssme_pf_user_model_has_logf() == 0 and ssme_amd.filters.user_model_has_logf() is False     # the stock build
    for m in ("sample_trajectories_backward", "backward_bytes", "backward_smoothed_means", "user_model_has_logf", "series_logweights"):
        assert callable(getattr(ssme_amd.ParticleFilterBank, m)), m
    hpp = open(os.path.join(ROOT, "include", "ssme_gpu", "bsfilter_gpu.hpp")).read()
    assert hpp.count(" sample_backward(") >= 2
    api = open(os.path.join(ROOT, "ssme_amd", "csrc", "model_api.h")).read()
    assert "struct user_logf" in api and "logf_vec" in api


def test_refusals_that_need_no_device():
    from ssme_amd import _capi
    L = _capi.lib()
    buf = np.zeros(64)
    b = C.c_uint64()
    assert L.ssme_pf_backward_bytes(None, 4, C.byref(b)) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_download_series_logweights(None, 0, 0, _capi.dptr(buf)) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_sample_trajectories_backward(None, 1, None, _capi.dptr(buf), None, 4) == _capi.ERR_INVALID_ARG
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
    GPU: tests/test_backward_gpu.py)."""
    from ssme_amd import _capi
    buf = np.zeros(4 * 4 * max(r, 16))
    idx = np.zeros(buf.size, dtype=np.uint32)
    b = C.c_uint64()
    tile, tiles = C.c_int32(), C.c_int32()
    assert L.ssme_pf_get_layout(h, C.byref(tile), C.byref(tiles)) == _capi.OK
    npad = tile.value * tiles.value
    assert L.ssme_pf_backward_bytes(h, 0, C.byref(b)) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_backward_bytes(h, 4, None) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_backward_bytes(h, 4, C.byref(b)) == _capi.OK and b.value == 8 * 4 * r * npad
    bad_term = np.zeros(r, dtype=np.uint32)
    bad_term[-1] = n
    for K, term, out in ((0, None, buf), (n + 1, None, buf), (1, None, None), (1, bad_term, buf)):
        assert L.ssme_pf_sample_trajectories_backward(h, K, _capi.u32ptr(term), _capi.dptr(out), _capi.u32ptr(idx), 4) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_sample_trajectories_backward(h, 1, None, _capi.dptr(buf), None, 0) == _capi.ERR_INVALID_ARG
    for f, t, out in ((-1, 0, buf), (r, 0, buf), (0, -1, buf), (0, 0, None)):
        assert L.ssme_pf_download_series_logweights(h, f, t, _capi.dptr(out)) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_sample_trajectories_backward(h, 1, None, _capi.dptr(buf), None, 4) == _capi.ERR_STATE       # nothing recorded
    assert L.ssme_pf_download_series_logweights(h, 0, 0, _capi.dptr(buf)) == _capi.ERR_STATE


def test_weight_rows_life_cycle_without_a_device(tmp_path):
    """ssme_amd/csrc/series_history.h: the log-weight rows are filled once per history, stale after every call that moves the handle
    on, and their buffer goes with the history rows (tests/cpp/test_history_weights.cpp)."""
    exe = str(tmp_path / "test_history_weights")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_history_weights.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
    api = open(os.path.join(ROOT, "ssme_amd", "csrc", "pf_api.hip")).read()
    assert "h->hist.weights_query(" in api and "h->hist.weights_filled()" in api


# ---- the restatement against a brute-force evaluation --------------------------------------------------------------------------------
def _hand_history(rng, T, n, sched, degenerate_at=None):
    """A hand-built history of one scalar filter: populations, log-weights, ancestors.  degenerate_at = t: every log-weight of step t
    is -inf, so the draw of B_t has no weight to draw from."""
    xs = [rng.normal(size=(1, n)) for _ in range(T)]
    lws = [rng.normal(size=n) * 2.0 for _ in range(T)]
    for t in range(T):
        lws[t][rng.integers(n)] = -np.inf                  # a dead particle per step
    if degenerate_at is not None:
        lws[degenerate_at][:] = -np.inf
    ancs = [rng.integers(0, n, size=n) for _ in range(T)]
    return xs, lws, ancs


def _check_against_brute_force(O, T, n, sched, K, seed, rep, degenerate_at=None):
    rng = np.random.default_rng(100 * T + n + sched)
    xs, lws, ancs = _hand_history(rng, T, n, sched, degenerate_at)
    th = (0.9, 0.7, 1.0)
    logf = br.logf_builtin(O, br.MODEL_LIN_GAUSS, th)
    term = rng.integers(0, n, size=K)
    B, X, fb = br.backward_filter(O, logf, xs, lws, ancs, sched, term, seed, rep)
    sh = br.shift_of(n)
    n_fb = 0
    for k in range(K):
        assert B[k, T - 1] == term[k]
        for t in range(T - 2, -1, -1):
            b1 = int(B[k, t + 1])
            xn = float(xs[t + 1][0, b1])
            # a_i by plain Python floats: the linear Gaussian density needs no device function
            a = []
            for i in range(n):
                d = (xn - th[0] * float(xs[t][0, i])) / th[1]
                v = float(lws[t][i]) + (-0.5 * (d * d))
                a.append(-math.inf if v != v else v)
            m = max(a)
            pick = None
            if math.isfinite(m):
                q = O.quantize(np.array(a) - m, sh)
                pick = br.brute_force(q, br.draw_uniform(k, t, rep, seed), a, sh)
            if pick is None:
                n_fb += 1
                pick = int(ancs[t + 1][b1]) if (t + 1) % sched == 0 else b1
            assert B[k, t] == pick, (k, t, B[k, t], pick)
            assert X[k, t, 0] == xs[t][0, pick]
    assert fb == n_fb
    return fb


def test_restatement_against_brute_force():
    from oracle import oracle as O
    assert br.shift_of(1) == 41 and br.shift_of(2) == 41 and br.shift_of(2048) == 41 and br.shift_of(2049) == 40 and br.shift_of(4097) == 39
    for T, n, sched in ((1, 1, 1), (2, 2, 1), (5, 8, 1), (6, 7, 3), (4, 3, 2)):
        assert _check_against_brute_force(O, T, n, sched, K=min(n, 5), seed=0x1234567890, rep=3) == 0


def test_restatement_takes_the_genealogy_where_the_transition_is_degenerate():
    from oracle import oracle as O
    # step 2 of 5 has no weight: B_2 is the lineage of B_3 -- anc_3[B_3] with sched 1, B_3 itself where step 3 did not resample
    assert _check_against_brute_force(O, 5, 8, 1, K=4, seed=7, rep=0, degenerate_at=2) == 4
    assert _check_against_brute_force(O, 5, 8, 2, K=4, seed=7, rep=0, degenerate_at=2) == 4
