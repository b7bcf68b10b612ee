"""k_filter_step after the glue trim (csrc/pf_kernels.h): the gather's byte offset taken straight from the search position with the clamp to
N - 1 behind the uniform ragged-last-source-tile condition, block_scan_f64 without the shifted copy, the tile select of staged_search_pos
as a wave-uniform branch, and the schedule and store policy compiled in (RESIDENT) -- against oracle.Filter(..., tile=2048), bit for bit.

Shapes: N = 129 * 2048 and N = 129 * 2048 - 1000 with 2048-particle tiles.  More than 128 tiles, so the step kernels with the block-wide
level-2 run (k_filter_step<0, 512, false, 2048, RS, false, true>, the benchmark's instantiation), not the wave-local one; the second N has a ragged
last tile (the clamped gather, the masked spacings).  T = 6, multinomial and systematic resampling, the benchmark's theta and theta with
sigma = 3 and two |y| = 0.5 observations.  Through run_series (RS >= 0 kernels) the per-step log-likelihoods, the particles and the cdf; through
the step API with set_debug(True, True) (the RS = -1 kernel) the ancestors of every step as well.

Source tiles of an output tile and where a crossing between two of them falls, counted on the CPU with the oracle over steps 1 .. 5 (645
output tiles per run; thread tid of 512 holds particle pairs tid and 512 + tid, a wave 64 consecutive pairs):
    N       resampler    theta    tiles with 1 / 2 / 3 sources    crossings inside a pair / inside a wave / between two waves
    264192  multinomial  bench    31 / 591 / 23                   317 / 319 / 1
    264192  multinomial  sigma 3  36 / 580 / 29                   311 / 324 / 3
    264192  systematic   bench    25 / 603 / 17                   333 / 302 / 2
    264192  systematic   sigma 3  28 / 598 / 19                   340 / 295 / 1
    263192  multinomial  bench    34 / 582 / 29                   321 / 316 / 3
    263192  multinomial  sigma 3  39 / 575 / 31                   325 / 305 / 7
    263192  systematic   bench    31 / 593 / 21                   341 / 294 / 0
    263192  systematic   sigma 3  26 / 599 / 20                   323 / 312 / 4
so every run stages one, two and three tiles, and waves with no crossing (both uniform branches), with a crossing inside a pair and with one
between pairs all occur; a crossing between two waves (every wave uniform, neighbours in different tiles) in all runs but one.

One Liu-West case (N = 2^14, T = 4, auxiliary form) against oracle.LWFilter: block_scan_f64, multinomial_targets and staged_search are shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 20260101
NS = (129 * 2048, 129 * 2048 - 1000)
T = 6
THETA_BENCH = [1.0, 0.95, 0.25]
THETA_UNEVEN = [1.0, 0.95, 3.0]


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ssme_amd
    from ssme_amd import _capi
    assert _capi.lib() is not None        # the in-tree HIP library is what runs
    return ssme_amd


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _series(spy, which):
    y = np.array(spy[:T], dtype=np.float64)
    if which == "uneven":
        y[2], y[4] = 0.5, -0.5
    return y


def _theta(which):
    return THETA_UNEVEN if which == "uneven" else THETA_BENCH


@pytest.fixture(scope="module")
def oracle_runs(oracle, spy):
    """(n, resampler, which) -> (log-likelihood, per-step, state after the series), computed once per case and not changed."""
    cache = {}

    def get(n, rs, which):
        key = (n, rs, which)
        if key not in cache:
            f = oracle.Filter(oracle.MODEL_SVOL, n, _theta(which), SEED, rep=0, resampler=rs, tile=2048)
            ll, per = f.run_series(_series(spy, which))
            cache[key] = (ll, per, f.state())
        return cache[key]
    return get


def _same_state(g, o, what):
    assert np.array_equal(_bits(g["x"]), _bits(o["x"])), what + ": particles"
    np.testing.assert_array_equal(g["cdf"], o["cdf"], err_msg=what + ": integer cdf")
    np.testing.assert_array_equal(g["A"], o["A"], err_msg=what + ": tile sums")
    assert np.array_equal(_bits(g["mb"]), _bits(o["mb"])), what + ": tile maxima"
    assert g["S"] == o["S"] and g["rshift"] == o["rshift"], what + ": integer weight sum"


@pytest.mark.parametrize("which", ["bench", "uneven"])
@pytest.mark.parametrize("rs", [0, 1], ids=["multinomial", "systematic"])
@pytest.mark.parametrize("n", NS)
def test_series_equals_the_oracle(sa, oracle_runs, spy, n, rs, which):
    lo, po, so = oracle_runs(n, rs, which)
    assert np.all(np.isfinite(po))
    b = sa.ParticleFilterBank(sa.MODEL_SVOL, n, 1, SEED, rs, tile=2048)
    assert (b.tile, b.n_tiles) == (2048, 129)
    b.set_params(_theta(which))
    ll = b.run_series(_series(spy, which))[0]
    per = b.per_step()[0][:T].copy()
    g = b.state(0, ancestors=False, logw=False)
    b.close()
    assert np.array_equal(_bits(per), _bits(po)), (per.tolist(), po.tolist())
    assert ll == lo
    _same_state(g, so, f"n={n} rs={rs} {which}")


@pytest.mark.parametrize("rs", [0, 1], ids=["multinomial", "systematic"])
@pytest.mark.parametrize("n", NS)
def test_step_api_with_recording_equals_the_oracle_ancestors_included(sa, oracle, spy, n, rs):
    y = _series(spy, "uneven")
    of = oracle.Filter(oracle.MODEL_SVOL, n, THETA_UNEVEN, SEED, rep=0, resampler=rs, tile=2048)
    b = sa.ParticleFilterBank(sa.MODEL_SVOL, n, 1, SEED, rs, tile=2048)
    b.set_debug(True, True)
    b.set_params(THETA_UNEVEN)
    for t in range(T):
        lg, lo = b.step(y[t])[0], of.step(y[t])
        assert lg == lo, (t, lg, lo)
        g, o = b.state(0, ancestors=True, logw=True), of.state()
        _same_state(g, o, f"n={n} rs={rs} t={t}")
        assert np.array_equal(_bits(g["logw"]), _bits(o["logw"])), f"t={t}: log-weights"
        if t > 0:
            np.testing.assert_array_equal(g["anc"], o["anc"], err_msg=f"ancestors n={n} rs={rs} t={t}")
            assert g["anc"].max() < n
    b.close()


def test_liu_west_equals_its_oracle(sa, oracle, spy):
    n, steps = 1 << 14, 4
    lo, hi, tr = oracle.LW_PRIOR_LO, oracle.LW_PRIOR_HI, oracle.LW_TRANSFORMS
    g = sa.svol_lw_1_par(0.99, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], nparts=n, n_filters=1, seed=SEED, transforms=tr, rs=1)
    o = oracle.LWFilter(n, SEED, 0, 0.99, tr, lo, hi, 0, 1)
    for t in range(steps):
        z = spy[t - 1] if t else 0.0
        g.filter(spy[t], z)
        lc = o.step(spy[t], z)
        assert g.getLogCondLike() == lc, (t, g.getLogCondLike(), lc)
    gs, so = g.state(0), o.state()
    g.close()
    assert np.array_equal(_bits(gs["x"]), _bits(so["x"])), "particles"
    assert np.array_equal(_bits(gs["theta"]), _bits(so["theta"])), "parameters"
