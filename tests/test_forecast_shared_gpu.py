"""What ssme_pf_sim_future_obs and ssme_lw_sim_future_obs share on the host (csrc/handle_core.h: Forecast, forecast_prepare, forecast_plan,
forecast_finish, forecast_elapsed) and no other test pins: the regrow of the sample buffers on a Liu-West handle, and a bootstrap and a
Liu-West handle forecasting in turn in one process.  Every comparison is bit for bit against the same call on a fresh handle (or the same
handle before): no tolerance.  N = 2049: two tiles, an odd N, so the pad column of the Ns-long sample rows exists."""
import numpy as np
import pytest

import bs_edge_cases as bc
import fc_edge_cases as fc
import test_expectations_gpu as teg

pytestmark = pytest.mark.gpu
sa = teg.sa
N, STEPS = 2049, 2
Y, Z = bc.series(dict(fc.BENIGN, model=bc.MODEL_SVOL_LEVERAGE), STEPS)


def lev_bank(sa):
    b = sa.ParticleFilterBank(bc.MODEL_SVOL_LEVERAGE, N, 1, bc.SEED)
    b.set_params(bc.TH_LEV)
    for t in range(STEPS):
        b.step(Y[t], Z[t])
    return b


def lw_filter(sa):
    g = sa.svol_lw_1_par(0.99, 0.8, 0.99, -0.1, 0.1, 0.01, 0.1, -0.5, -0.01, nparts=N, seed=bc.SEED)
    for t in range(STEPS):
        g.filter(Y[t], Z[t])
    return g


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want, what):
    """tuples of arrays, or state() dictionaries: equal shapes and equal bits"""
    if isinstance(got, dict):
        assert got.keys() == want.keys(), what
        got, want = [got[k] for k in sorted(got)], [want[k] for k in sorted(want)]
    assert len(got) == len(want), what
    for i, (u, v) in enumerate(zip(got, want)):
        if u is None or v is None:
            assert u is None and v is None, (what, i)
            continue
        u, v = np.asarray(u), np.asarray(v)
        assert u.shape == v.shape and u.dtype == v.dtype and np.array_equal(bits(u), bits(v)), (what, i)


def test_liu_west_output_buffers_regrow_separately(sa):
    """The twin of test_output_buffers_regrow_separately on a Liu-West handle: H = 2 (y only), 17 with states, 2 with states, 1, each
    with the start draw and the proposal: each call equals the same call on a fresh handle."""
    one = lw_filter(sa)
    for H, states in ((2, False), (17, True), (2, True), (1, False)):
        got = one.sim_future_obs(H, Y[-1], states=states, start=True, prop=True)
        fresh = lw_filter(sa)
        want = fresh.sim_future_obs(H, Y[-1], states=states, start=True, prop=True)
        fresh.close()
        assert len(got) == (4 if states else 3) and got[0].shape == (1, H, N)
        same(got, want, (H, states))
    one.close()


def test_bootstrap_and_liu_west_handles_interleaved(sa):
    """A bootstrap leverage bank and a Liu-West filter alive together: bootstrap forecast, Liu-West forecast, bootstrap forecast.  The
    first and the third are equal, the Liu-West one equals a fresh handle's, neither filter's state() moves under the other's (or its
    own) forecast, and every handle reports the event times of its own last call."""
    H = 5
    b, g = lev_bank(sa), lw_filter(sa)
    sb, sg = b.state(0, logw=False), g.state(0)
    first = b.sim_future_obs(H, Y[-1], states=True, start=True)
    tb1 = b.forecast_elapsed_ms()
    same(g.state(0), sg, "Liu-West state after the bootstrap forecast")
    lw = g.sim_future_obs(H, Y[-1], states=True, start=True, prop=True)
    tg = g.forecast_elapsed_ms()
    same(b.state(0, logw=False), sb, "bootstrap state after the Liu-West forecast")
    assert b.forecast_elapsed_ms() == tb1, "the bootstrap handle's times after the Liu-West forecast"
    third = b.sim_future_obs(H, Y[-1], states=True, start=True)
    tb3 = b.forecast_elapsed_ms()
    same(third, first, "bootstrap forecast before and after the Liu-West one")
    same(g.state(0), sg, "Liu-West state after both forecasts")
    same(b.state(0, logw=False), sb, "bootstrap state after both forecasts")
    assert g.forecast_elapsed_ms() == tg, "the Liu-West handle's times after the bootstrap forecast"
    for hor, call in (tb1, tg, tb3):
        assert 0.0 < hor <= call, (tb1, tg, tb3)
    fresh = lw_filter(sa)
    same(lw, fresh.sim_future_obs(H, Y[-1], states=True, start=True, prop=True), "Liu-West forecast beside a bootstrap handle")
    fresh.close()
    b.close()
    g.close()
