"""ssme_pf_sim_future_obs / ssme_lw_sim_future_obs (csrc/forecast.h) against the numpy restatement of tests/forecast_ref.py, to the bit:
both sides are fixed IEEE operation sequences (-ffp-contract=off), the standard the step-kernel parity tests hold.  The bootstrap
reference starts from the device's own downloads (state(): particles, integer cdf, tile sums and maxima), the Liu-West one from an
oracle.LWFilter run in lock-step (the parity tests pin device == oracle for that state).  One anchor is independent of the
restatement: the forecast mean of the linear Gaussian model against phi^(k+1) E[x_t].
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import forecast_ref as fr
import test_expectations_gpu as teg
from test_liu_west_edges_gpu import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
sa = teg.sa
SEED = 0x5eed0000beef
THETA = {0: [[1.0, 0.95, 0.25], [0.8, 0.9, 0.3], [1.3, 0.97, 0.15]],                       # SVOL: beta, phi, sigma
         1: [[0.95, 0.01, 0.2, -0.3], [0.9, -0.02, 0.3, -0.1], [0.97, 0.0, 0.15, -0.5]],  # leverage: phi, mu, sigma, rho
         2: [[0.9, 0.4, 0.7], [0.8, 0.5, 0.5], [0.95, 0.3, 1.1]]}                          # linear Gaussian: phi, sigma, tau


def _bank(sa, model, n, r=1, tile=0, first=0, sched=1, dtype=0, resampler=0):
    bank = sa.ParticleFilterBank(model, n, r, seed=SEED, resampler=resampler, resamp_sched=sched, first_filter_id=first, tile=tile,
                                 dtype=dtype)
    bank.set_params(THETA[model][0] if r == 1 else THETA[model][:r])
    return bank


def _steps(bank, model, y, t_from, t_to):
    out = []
    for t in range(t_from, t_to):
        out.append(bank.step(y[t], (y[t - 1] if t else 0.0) if model == 1 else None))
    return out


def _check(oracle, bank, model, r, first, t0, H, last_obs, f32=False):
    """Device forecast of every filter == the reference started from the device's own state."""
    y, x, start = bank.sim_future_obs(H, last_obs, states=True, start=True)
    assert y.shape == (r, H, bank.n) and x.shape == y.shape and start.shape == (r, bank.n)
    for f in range(r):
        st = bank.state(f, logw=False)
        theta = THETA[model][f] if r > 1 else THETA[model][0]
        ws, wx, wy = fr.forecast_bs(oracle, model, theta, st, bank.n, bank.tile, SEED, first + f, t0, H, last_obs, f32=f32)
        assert np.array_equal(start[f], ws), ("start", f)
        same_bits(x[f], wx, f"x of filter {f}")
        same_bits(y[f], wy, f"y of filter {f}")
    return y, x, start


# N, tile, H, R: every N of the issue, B = 1, 2 and 13 (not a power of two; the ragged last tile holds 7 particles)
SHAPES = [(1, 0, 17, 1), (2, 0, 2, 3), (500, 0, 17, 3), (2048, 0, 1, 1), (2049, 0, 2, 3), (3 * 2048 + 7, 512, 1, 1)]


@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("n,tile,H,r", SHAPES, ids=lambda v: str(v))
def test_bootstrap_parity(sa, oracle, spy, model, n, tile, H, r):
    first = 5 if r > 1 else 0
    bank = _bank(sa, model, n, r, tile, first)
    _steps(bank, model, spy, 0, 4)
    y, _, start = _check(oracle, bank, model, r, first, 4, H, spy[3])
    assert np.isfinite(y).all()
    if n > 2048:
        assert len(set((start[0] // bank.tile).tolist())) > 1          # the draw crosses tiles
    bank.close()


def test_routes_agree(sa, oracle, spy):
    """N = 500 after run_series on the one-launch route, on the forced tiled route, and after the same steps through ssme_pf_step."""
    outs = []
    for route in ("small", "tiled", "step"):
        bank = _bank(sa, 1, 500)
        if route == "tiled":
            bank.set_small_series(False)
        if route == "step":
            _steps(bank, 1, spy, 0, 6)
        else:
            z = np.concatenate([[0.0], spy[:5]])
            bank.run_series(spy[:6], z)
        outs.append(_check(oracle, bank, 1, 1, 0, 6, 3, spy[5]))
        bank.close()
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)


def test_schedule_carried_and_fresh_weights(sa, oracle, spy):
    """resamp_sched = 3: after one step the weights are carried (no resampling at step 1), after three the cloud was just weighted
    afresh; the forecast draws from the weights of the last step either way."""
    bank = _bank(sa, 1, 2049, sched=3)
    _steps(bank, 1, spy, 0, 1)
    _check(oracle, bank, 1, 1, 0, 1, 2, spy[0])
    _steps(bank, 1, spy, 1, 3)
    _check(oracle, bank, 1, 1, 0, 3, 2, spy[2])
    bank.close()


def test_degenerate_weights(sa, oracle, spy):
    bank = _bank(sa, 0, 2049)
    _steps(bank, 0, spy, 0, 2)
    bank.step(40.0)                                                      # an observation 40 standard deviations out: few particles keep weight
    _, _, start = _check(oracle, bank, 0, 1, 0, 3, 2, 40.0)
    st = bank.state(0, logw=False)
    cdf = st["cdf"].astype(np.int64)
    q = np.diff(cdf, prepend=0)
    q[2048] = cdf[2048]
    assert (q == 0).any() and (q[start[0]] > 0).all()
    bank.close()


@pytest.mark.parametrize("model,bad_row,good_row", [(0, [-1.0, 0.95, 0.25], [1.0, 0.95, 0.25]),      # SVOL: scale beta < 0
                                                    (0, [0.0, 0.95, 0.25], [1.0, 0.95, 0.25]),       # SVOL: beta = 0
                                                    (2, [0.9, 0.4, -0.7], [0.9, 0.4, 0.7]),          # linear Gaussian: observation sigma tau < 0
                                                    (2, [0.9, 0.4, 0.0], [0.9, 0.4, 0.7])],          # ... tau = 0
                         ids=["svol-beta-neg", "svol-beta-0", "lg-tau-neg", "lg-tau-0"])
def test_bad_parameters_give_nan(sa, spy, model, bad_row, good_row):
    """Scale parameters that make `bad = 1` (every log-weight -inf, S = 0) for filter 0 only: all its outputs are NaN, its start draw
    is the zeros the search returns on an empty cdf, the call returns status 0, and the healthy filter beside it is untouched."""
    bank = sa.ParticleFilterBank(model, 2049, 2, seed=SEED)
    bank.set_params([bad_row, good_row])
    _steps(bank, model, spy, 0, 2)
    y, x, start = bank.sim_future_obs(3, states=True, start=True)          # status 0: no exception
    assert np.isnan(y[0]).all() and np.isnan(x[0]).all() and not start[0].any()
    assert np.isfinite(y[1]).all() and np.isfinite(x[1]).all() and start[1].any()
    alone = sa.ParticleFilterBank(model, 2049, 1, seed=SEED, first_filter_id=1, n_filters_total=2)
    alone.set_params(good_row)
    _steps(alone, model, spy, 0, 2)
    for got, want in zip((y[1], x[1], start[1]), alone.sim_future_obs(3, states=True, start=True)):
        assert np.array_equal(got, want[0])
    alone.close()
    bank.close()


def test_forecasts_leave_the_filter_alone(sa, spy):
    def series(with_forecasts):
        bank = _bank(sa, 1, 2049, 2, first=3)
        ll, fc = [], {}
        for t in range(12):
            ll.append(_steps(bank, 1, spy, t, t + 1)[0])
            if with_forecasts and t + 1 in (3, 7):
                a = bank.sim_future_obs(4, spy[t], states=True, start=True)
                b = bank.sim_future_obs(4, spy[t], states=True, start=True)
                for u, v in zip(a, b):
                    assert np.array_equal(u, v, equal_nan=True)          # two forecasts at one origin: the same bits
                fc[t + 1] = a
        st = [bank.state(f, logw=False) for f in range(2)]
        ex = bank.expectations_multi([0, 1, 2])
        bank.close()
        return np.array(ll), st, ex, fc
    ll0, st0, ex0, _ = series(False)
    ll1, st1, ex1, fc = series(True)
    assert np.array_equal(ll0, ll1) and np.array_equal(ex0, ex1)
    for a, b in zip(st0, st1):
        for k in ("x", "cdf", "A", "mb"):
            assert np.array_equal(a[k], b[k]), k
        assert a["m"] == b["m"] and a["S"] == b["S"]
    assert not np.array_equal(fc[3][0], fc[7][0]) and not np.array_equal(fc[3][2], fc[7][2])


def test_f32_handle_rounds_at_the_boundary(sa, oracle, spy):
    bank = _bank(sa, 1, 500, dtype=1)
    y32 = spy.astype(np.float32).astype(np.float64)
    _steps(bank, 1, y32, 0, 4)
    y, x, _ = _check(oracle, bank, 1, 1, 0, 4, 3, spy[3], f32=True)
    assert np.array_equal(y, y.astype(np.float32)) and np.array_equal(x, x.astype(np.float32))
    bank.close()


def test_linear_gaussian_anchor(sa):
    """Independent of the restatement: E[x_{t+k+1} | y_{1:t}] = phi^(k+1) E[x_t | y_{1:t}] for x' = phi x + sigma e.  The sample mean
    of the forecast states must be within 5 standard errors (sample sd / sqrt N) of it; an unweighted or misweighted start
    population misses by many (the filtered mean moves by about a prior standard deviation per step).  Fixed seed: not flaky."""
    n, phi, sigma, tau = 1 << 16, 0.9, 0.4, 0.3
    rng = np.random.default_rng(7)
    xt, ys = 0.0, []
    for _ in range(20):
        xt = phi * xt + sigma * rng.standard_normal()
        ys.append(xt + tau * rng.standard_normal())
    bank = sa.ParticleFilterBank(2, n, 1, seed=SEED)
    bank.set_params([phi, sigma, tau])
    bank.run_series(np.array(ys))
    ex = bank.expectations(0)[0]
    y, x = bank.sim_future_obs(4, states=True)
    for k in range(4):
        se = x[0, k].std(ddof=1) / np.sqrt(n)
        assert abs(x[0, k].mean() - phi ** (k + 1) * ex) <= 5.0 * se, (k, x[0, k].mean(), phi ** (k + 1) * ex, se)
        se_y = y[0, k].std(ddof=1) / np.sqrt(n)
        assert abs(y[0, k].mean() - phi ** (k + 1) * ex) <= 5.0 * se_y
    # the start population itself: unweighted mean of the cloud differs from the filtered mean by far more than that
    assert abs(bank.state(0, logw=False)["x"].mean() - ex) > 20.0 * x[0, 0].std(ddof=1) / np.sqrt(n)
    bank.close()


def test_status_codes(sa, tmp_path):
    import ctypes as C
    from ssme_amd import _capi
    L = _capi.lib()
    bank = sa.ParticleFilterBank(0, 100, 1, seed=1)
    bank.set_params(THETA[0][0])
    with pytest.raises(sa.SsmeError) as e:
        bank.sim_future_obs(2)
    assert e.value.status == _capi.ERR_STATE                             # before the first step
    bank.step(0.1)
    with pytest.raises(sa.SsmeError) as e:
        bank.sim_future_obs(65536)
    assert e.value.status == _capi.ERR_INVALID_ARG
    assert bank.sim_future_obs(65535 // 4096).shape == (1, 15, 100)
    bank.close()
    # a particle-sharded handle
    cfg = _capi.Config(model=0, n_particles=4096, n_filters=1, dtype=0, resampler=0, resamp_sched=1, seed=1, device=0,
                       first_filter_id=0, tile_particles=0, n_filters_total=0)
    h = C.c_void_p()
    assert L.ssme_pf_shard_create(C.byref(cfg), 0, 2, C.byref(h)) == _capi.OK
    y = np.zeros(4096)
    assert L.ssme_pf_sim_future_obs(h, 1, None, _capi.dptr(y), None, None) == _capi.ERR_UNSUPPORTED
    L.ssme_pf_destroy(h)
    # a library with a user model compiled in (a process of its own: SSME_PF_LIB is read when the package loads)
    from ssme_amd import build
    so = build.build_user_model(os.path.join(ROOT, "tests", "models", "svol_student_t.h"), "student_t")
    out = str(tmp_path / "status.txt")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "forecast_user_worker.py"), out], env=dict(os.environ, SSME_PF_LIB=so),
                   check=True, timeout=120)
    assert open(out).read().split() == [str(_capi.ERR_UNSUPPORTED), str(_capi.OK)]


# ---- Liu-West -----------------------------------------------------------------------------------------------------------------------
LW_DEFAULT = (fr.TR_LOGIT, fr.TR_NULL, fr.TR_LOG, fr.TR_TWICE_FISHER)
LW_OTHER = (fr.TR_TWICE_FISHER, fr.TR_NULL, fr.TR_LOG, fr.TR_TWICE_FISHER)
LW_LO, LW_HI, LW_DELTA = (0.8, -0.1, 0.01, -0.5), (0.99, 0.1, 0.1, -0.01), 0.97
# form, N, H, resamp_sched, transforms
LW_CASES = [(0, 1, 3, 1, LW_DEFAULT), (1, 1, 1, 2, LW_DEFAULT), (0, 500, 1, 2, LW_DEFAULT), (1, 500, 3, 1, LW_DEFAULT),
            (0, 2049, 3, 2, LW_DEFAULT), (1, 2049, 1, 1, LW_DEFAULT), (0, 5000, 1, 1, LW_DEFAULT), (1, 5000, 3, 2, LW_DEFAULT),
            (0, 500, 3, 1, LW_OTHER)]


def _lw(sa, form, n, rs, tr, r=1, first=0):
    cls = sa.svol_lw_2_par if form else sa.svol_lw_1_par
    return cls(LW_DELTA, LW_LO[0], LW_HI[0], LW_LO[1], LW_HI[1], LW_LO[2], LW_HI[2], LW_LO[3], LW_HI[3], nparts=n, n_filters=r, seed=SEED,
               first_filter_id=first, transforms=tr, rs=rs)


@pytest.mark.parametrize("form,n,H,rs,tr", LW_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_liu_west_parity(sa, oracle, spy, form, n, H, rs, tr):
    import expect_ref as er
    import lw_moments_ref as mr
    g = _lw(sa, form, n, rs, tr)
    o = oracle.LWFilter(n, SEED, 0, LW_DELTA, tr, LW_LO, LW_HI, form, rs)
    T = 3
    for t in range(T):
        z = spy[t - 1] if t else 0.0
        g.filter(spy[t], z)
        o.step(spy[t], z)
    so, gs = o.state(), g.state(0)
    same_bits(gs["x"], so["x"], "lock-step particles")
    same_bits(gs["theta"], so["theta"], "lock-step parameters")
    # the oracle's second-stage weights -> integer cdf, tile sums and maxima, as expect_ref.lw_state rebuilds them
    ls = er.lw_state(oracle, so)
    B = -(-n // 2048)
    cdf = np.concatenate([np.cumsum(ls["q"][s:s + 2048]) for s in range(0, n, 2048)]).astype(np.uint64)
    rshift = 52 - int(np.ceil(np.log2(B * 2048)))
    st = dict(cdf=cdf, A=ls["A"].astype(np.uint64), mb=ls["mb"], rshift=rshift)
    want_start, alive = fr.start_draw(oracle, st, n, 2048, SEED, 0, T)
    assert alive
    y, x, start, prop = g.sim_future_obs(H, spy[T - 1], states=True, start=True, prop=True)
    assert y.shape == (1, H, n) and x.shape == y.shape
    assert np.array_equal(start[0], want_start)
    a = (3.0 * LW_DELTA - 1.0) / (2.0 * LW_DELTA)
    L = np.zeros((4, 4))
    L[np.tril_indices(4)] = prop[0, 4:14]
    bad = mr.check_proposal(prop[0, :4], L, so["theta"][:, start[0].astype(np.int64)], a, B, name=f"forecast form {form} n {n}")
    assert not bad, bad
    wx, wy = fr.forecast_lw(oracle, so, start[0], prop[0], tr, LW_DELTA, n, SEED, 0, T, H, spy[T - 1])
    same_bits(x[0], wx, "x")
    same_bits(y[0], wy, "y")
    assert np.isfinite(y).all()
    g.close()


def test_liu_west_forecasts_leave_the_filter_alone(sa, spy):
    def series(with_forecasts):
        g = _lw(sa, 0, 2049, 1, LW_DEFAULT, r=2, first=3)
        ll, fc = [], {}
        for t in range(12):
            g.filter(spy[t], spy[t - 1] if t else 0.0)
            ll.append(np.array(g.getLogCondLike()))
            if with_forecasts and t + 1 in (3, 7):
                a = g.sim_future_obs(4, spy[t], states=True, start=True, prop=True)
                b = g.sim_future_obs(4, spy[t], states=True, start=True, prop=True)
                for u, v in zip(a, b):
                    assert np.array_equal(u, v)
                fc[t + 1] = a
        out = (np.array(ll), [g.state(f) for f in range(2)], g.expectations(list(range(8))), g.param_means(), fc)
        g.close()
        return out
    ll0, st0, ex0, pm0, _ = series(False)
    ll1, st1, ex1, pm1, fc = series(True)
    assert np.array_equal(ll0, ll1) and np.array_equal(ex0, ex1) and np.array_equal(pm0, pm1)
    for a, b in zip(st0, st1):
        for k in ("x", "theta", "thetabar", "L"):
            assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(fc[3][0], fc[7][0]) and not np.array_equal(fc[3][2], fc[7][2])
    assert not np.array_equal(fc[3][0][0], fc[3][0][1])                  # the two filters have streams of their own


def test_liu_west_status_codes(sa):
    from ssme_amd import _capi
    g = _lw(sa, 0, 100, 1, LW_DEFAULT)
    with pytest.raises(sa.SsmeError) as e:
        g.sim_future_obs(2, 0.0)
    assert e.value.status == _capi.ERR_STATE
    g.filter(0.01, 0.0)
    with pytest.raises(sa.SsmeError) as e:
        g.sim_future_obs(65536, 0.0)
    assert e.value.status == _capi.ERR_INVALID_ARG
    assert g.sim_future_obs(2, 0.0).shape == (1, 2, 100)
    g.close()


# ---- the Python wrappers around the bank --------------------------------------------------------------------------------------------
def test_model_objects_return_the_banks_forecast(sa, spy):
    """_SingleFilter.sim_future_obs (svol_bs, svol_leverage, lin_gauss_bs) strips the filter axis of the bank's result, whatever
    combination of outputs is asked for."""
    mods = [(sa.svol_bs(0.95, 1.0, 0.25, nparts=500, seed=SEED), False), (sa.svol_leverage(0.95, 0.01, 0.2, -0.3, nparts=500, seed=SEED), True),
            (sa.lin_gauss_bs(0.9, 0.4, 0.7, nparts=500, seed=SEED), False)]
    for m, cov in mods:
        for t in range(3):
            m.filter(spy[t], (spy[t - 1] if t else 0.0) if cov else None)
        by, bx, bs = m.bank.sim_future_obs(4, spy[2], states=True, start=True)
        y = m.sim_future_obs(4, spy[2])
        assert isinstance(y, np.ndarray) and y.shape == (4, 500) and np.array_equal(y, by[0])
        y2, x2, s2 = m.sim_future_obs(4, spy[2], states=True, start=True)
        assert np.array_equal(y2, by[0]) and np.array_equal(x2, bx[0]) and np.array_equal(s2, bs[0]) and s2.shape == (500,)
        y3, s3 = m.sim_future_obs(4, spy[2], start=True)
        assert np.array_equal(y3, by[0]) and np.array_equal(s3, bs[0])
        if cov:
            assert not np.array_equal(m.sim_future_obs(4, 0.0), y)       # last_obs reaches the leverage model
        m.bank.close()


def test_swarms_return_the_banks_forecast(sa, spy):
    """SwarmWithCovs.simFutureObs / Swarm.simFutureObs: one bank call for all members, [member, time, particle]."""
    sw = sa.svol_swarm_1([0], 0.8, 0.99, -0.1, 0.1, 0.05, 0.3, -0.5, -0.01, nstateparts=300, nparamparts=4, prior_seed=3, seed=SEED)
    for t in range(3):
        sw.update(spy[t], spy[t - 1] if t else 0.0)
    y = sw.simFutureObs(2, spy[2])
    want = sw._bank.sim_future_obs(2, spy[2], states=True, start=True)
    assert y.shape == (4, 2, 300) and np.array_equal(y, want[0]) and not np.array_equal(y[0], y[1])
    for got, w in zip(sw.simFutureObs(2, spy[2], states=True, start=True), want):
        assert np.array_equal(got, w)
    assert not np.array_equal(sw.simFutureObs(2, 0.0), y)
    sw.close()

    class bs_swarm(sa.Swarm):
        k = 0

        def samp_untrans_params(self):
            self.k += 1
            return [0.8 + 0.1 * self.k, 0.9 + 0.01 * self.k, 0.2 + 0.02 * self.k]      # beta, phi, sigma

    sn = bs_swarm([0], 300, 3, seed=SEED)
    for t in range(3):
        sn.update(spy[t])
    yn = sn.simFutureObs(2)
    assert yn.shape == (3, 2, 300) and np.array_equal(yn, sn._bank.sim_future_obs(2)) and not np.array_equal(yn[0], yn[1])
    sn.close()
