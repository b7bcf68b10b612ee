"""The windowed count of a particle pair's second resampling target (staged_search in csrc/pf_kernels.h).

The second target of a pair is counted inside a window of SSME_SEARCH_WINDOW (16) tile elements that starts at the first
target's count; a wave with a count that reaches the window's top repeats the full descent.  The scenario here (an
outlier observation, then an ordinary one: a few surviving particles, long runs of zero-weight particles between the
targets) makes that fallback happen on the staged-tile path, which the CPU test below proves from the oracle's ancestors
alone.  The GPU tests check ancestors, particles and the integer cdf bit for bit against the oracle at every tile size
and thread count, through the general kernel (debug recording) and the hot kernel (a whole series)."""
import numpy as np
import pytest

W = 16                                   # SSME_SEARCH_WINDOW of the shipped library
TH = [1.0, 0.95, 0.25]                   # stochastic volatility
YS = [0.01, 0.02, 6.0, 0.01, -8.0, 0.01]
SEED = 7
# (particles per tile, threads per tile, N): pairs per thread NK = 2, 4, 1 at 2048; 1 at 1024 and 512.  Ragged N.
SHAPES = [(2048, 512, 16384 + 100), (2048, 256, 16384), (2048, 1024, 12288 + 7), (1024, 512, 8000), (512, 256, 4000)]


def _assert_bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    bad = (a.view(np.uint64) != b.view(np.uint64)) & ~np.isnan(a)
    assert not bad.any(), f"{what}: {bad.sum()} of {a.size} values differ"


def _window_fallbacks(anc, n, tile):
    """Pairs whose second count the window cannot bracket, in output tiles whose sources span at most three cdf tiles
    (the staged path).  Mirrors staged_search: start = the first count (its tile's first element if the second target
    lies in a later tile), moved down to tile - W; not bracketed when the count reaches start + W - 1."""
    nopen = 0
    for b in range((n + tile - 1) // tile):
        a = anc[b * tile:min(n, (b + 1) * tile)].astype(np.int64)
        src = a // tile
        if src.max() - src.min() + 1 > 3:
            continue
        m = len(a) // 2 * 2
        a0, a1 = a[0:m:2], a[1:m:2]
        s0, s1 = a0 // tile, a1 // tile
        start = np.minimum(np.where(s0 == s1, a0 - s0 * tile, 0), tile - W)
        nopen += int(((a1 - s1 * tile) - start >= W - 1).sum())
    return nopen


@pytest.mark.parametrize("resampler", [0, 1, 2])
@pytest.mark.parametrize("tile,nt,n", SHAPES)
def test_scenario_forces_window_fallback(oracle, tile, nt, n, resampler):
    """Every shape of the GPU test below meets pairs that the window cannot bracket (oracle only, no device)."""
    of = oracle.Filter(oracle.MODEL_SVOL, n, TH, SEED, resampler=resampler, tile=tile)
    total = 0
    for t, y in enumerate(YS):
        of.step(y)
        if t > 0:
            total += _window_fallbacks(of.state()["anc"], n, tile)
    assert total > 0


@pytest.mark.gpu
@pytest.mark.parametrize("resampler", [0, 1, 2])
@pytest.mark.parametrize("tile,nt,n", SHAPES)
def test_window_fallback_bit_exact(oracle, tile, nt, n, resampler):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ssme_amd

    bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_SVOL, n, 1, SEED, resampler, tile=tile)
    bank.set_tuning(nt)
    bank.set_debug(True)
    bank.set_params(TH)
    of = oracle.Filter(oracle.MODEL_SVOL, n, TH, SEED, resampler=resampler, tile=tile)
    fallbacks = 0
    for t, y in enumerate(YS):
        assert bank.step(y)[0] == of.step(y), t
        g, o = bank.state(0, ancestors=True), of.state()
        _assert_bits_equal(g["x"], o["x"], f"particles t={t}")
        np.testing.assert_array_equal(g["cdf"], o["cdf"], err_msg=f"integer cdf t={t}")
        if t > 0:
            np.testing.assert_array_equal(g["anc"], o["anc"], err_msg=f"ancestors t={t}")
            fallbacks += _window_fallbacks(o["anc"], n, tile)
    assert fallbacks > 0
    bank.close()

    # the hot kernel (no recording, resampling every step): the whole series' log-likelihood
    bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_SVOL, n, 1, SEED, resampler, tile=tile)
    bank.set_tuning(nt)
    bank.set_params(TH)
    ll = bank.run_series(np.array(YS))[0]
    ref = oracle.Filter(oracle.MODEL_SVOL, n, TH, SEED, resampler=resampler, tile=tile).run_series(np.array(YS))[0]
    assert ll == ref, (ll, ref)
    bank.close()
