"""Backward-simulation smoothing (ssme_pf_sample_trajectories_backward, ssme_pf_download_series_logweights) on the device.

The reference of every parity test is a twin handle of the same configuration stepped with step() under set_debug(record_ancestors,
keep_logw) and downloaded after every step; tests/backward_ref.py restates the backward pass from those downloads with the oracle's
exp, quantiser and Philox, and indices and states are compared bit for bit (tests/backward_cases.py).  The last test is what the
feature is for: against the exact Rauch-Tung-Striebel smoother of a linear Gaussian model.
Every test here fails without the feature: the entry points do not exist there."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import backward_cases as bc
import backward_ref as br
import series_expect_cases as sc
from backward_cases import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
G = br.G
THETAS = {sc.MODEL_SVOL: sc.TH_SVOL3, sc.MODEL_SVOL_LEVERAGE: sc.TH_LEV3, sc.MODEL_LIN_GAUSS: sc.TH_LG3}
# (N, tile_particles): one and two particles, the wave edges, the flagship size, the edge between the 2- and the 8-candidate kernel
# (512 | 513), one chunk of 2048 at its largest and the first size that walks two chunks, three chunks with a ragged last one
SHAPES = ((1, 0), (2, 0), (63, 0), (64, 0), (65, 0), (500, 0), (513, 0), (2048, 0), (2049, 0), (4097, 512))
_WORKER = {}


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ssme_amd
    from ssme_amd import _capi
    assert _capi.lib() is not None
    return ssme_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.build()
    return O


def zs_of(z):
    return None if z is None else [float(v) for v in z]


def logf_rows(O, model, theta):
    return lambda f: br.logf_builtin(O, model, theta[f])


# ---- 1. the log-weights of every step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", [1, 3])
@pytest.mark.parametrize("route", [("lane-500", 500, 0, True), ("pair-1030", 1030, 0, True), ("tiled-500-forced", 500, 0, False)], ids=lambda r: r[0])
@pytest.mark.parametrize("model", [sc.MODEL_SVOL, sc.MODEL_SVOL_LEVERAGE, sc.MODEL_LIN_GAUSS], ids=["svol", "leverage", "lin-gauss"])
def test_logweights_equal_the_step_api(sa, model, route, sched):
    """T = 8: with resamp_sched = 3 steps 1, 2, 4, 5 and the LAST one (7) carry their weights over; the leverage model reads z_t = y_{t-1}."""
    name, n, tile, small = route
    y, z = sc.stock_series(model, 8)
    hist = bc.twin_history(sa, model, THETAS[model], n, tile, sched, y, z)
    bank = bc.recorded(sa, model, THETAS[model], n, tile, small, sched, y, z)
    assert bank.series_route()[0] == sc.expected_route(n, tile, small)[0]
    assert bank.backward_bytes(8) == 8 * 8 * bank.r * bank.tile * bank.n_tiles
    bc.check_logweights(bank, hist, f"{name} model={model} sched={sched}")
    if sched == 3:
        assert not np.array_equal(hist["lws"][0][7], hist["lws"][0][6])
    bank.close()


# ---- 2. the backward pass, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}")
def test_backward_equals_the_restatement_at_every_shape(sa, oracle, shape):
    """SVOL.  (T, R) = (7, 3), (2, 1), (1, 1); K in {1, G, G + 1, min(N, 65)}."""
    n, tile = shape
    for steps, R in ((7, 3), (2, 1), (1, 1)):
        theta = sc.TH_SVOL3[:R]
        y, z = sc.stock_series(sc.MODEL_SVOL, steps)
        hist = bc.twin_history(sa, sc.MODEL_SVOL, theta, n, tile, 1, y, z)
        bank = bc.recorded(sa, sc.MODEL_SVOL, theta, n, tile, True, 1, y, z)
        name = f"N={n} tile={tile} T={steps} R={R}"
        bc.check_logweights(bank, hist, name)
        fb = bc.check_backward(oracle, bank, hist, logf_rows(oracle, sc.MODEL_SVOL, theta), 1, bc.ks_of(n), name)
        assert fb == 0, name
        if steps == 7 and n >= 63:
            idx = bank.sample_trajectories_backward(min(n, 65), return_indices=True)[1]
            gen = bank.sample_trajectories(min(n, 65), indices=True)[1]
            assert not np.array_equal(idx, gen), name + ": backward simulation is not the genealogy"
        bank.close()


@pytest.mark.parametrize("sched", [1, 3])
@pytest.mark.parametrize("model", [sc.MODEL_SVOL_LEVERAGE, sc.MODEL_LIN_GAUSS], ids=["leverage", "lin-gauss"])
def test_backward_other_models_and_schedules(sa, oracle, model, sched):
    """The leverage model's density reads the covariate of step t + 1; N = 65 (lane kernel) and 513 on 512-particle tiles (tiled route)."""
    y, z = sc.stock_series(model, 8)
    for n, tile in ((65, 0), (513, 512)):
        hist = bc.twin_history(sa, model, THETAS[model], n, tile, sched, y, z)
        bank = bc.recorded(sa, model, THETAS[model], n, tile, True, sched, y, z)
        bc.check_backward(oracle, bank, hist, logf_rows(oracle, model, THETAS[model]), sched, (1, G + 1), f"model={model} N={n} sched={sched}",
                          zs=zs_of(z))
        bank.close()


# ---- 3. joins ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(500, 0), (1027, 512)], ids=["lane-500", "tiled-1027-t512"])
def test_terminals_join_the_genealogy_and_the_forecast(sa, oracle, shape):
    n, tile = shape
    y, z = sc.stock_series(sc.MODEL_SVOL, 7)
    bank = bc.recorded(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, True, 1, y, z)
    _, start = bank.sim_future_obs(1, start=True)
    K = 9
    xg, ig = bank.sample_trajectories(K, indices=True)
    xb, ib = bank.sample_trajectories_backward(K, return_indices=True)
    np.testing.assert_array_equal(ib[:, :, 6], ig[:, :, 6])
    np.testing.assert_array_equal(ib[:, :, 6], start[:, :K])
    same_bits(xb[:, :, 6], xg[:, :, 6], "the terminal states")
    term = np.tile(np.array([n - 1, 0, 7, 7, n // 2], dtype=np.uint32), (bank.r, 1))
    xt, it = bank.sample_trajectories_backward(5, term, return_indices=True)
    np.testing.assert_array_equal(it[:, :, 6], term)
    assert not np.array_equal(it[:, 2], it[:, 3]), "two trajectories from one terminal particle are different draws"
    same_bits(bank.sample_trajectories_backward(K), xb, "two calls, same bits")
    same_bits(bank.sample_trajectories(K), xg, "the genealogy is untouched by the backward call")
    bank.close()
    # T = 1: exactly the genealogy call's output
    bank = bc.recorded(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, True, 1, y[:1], None)
    for term1 in (None, term):
        K1 = 5
        xg, ig = bank.sample_trajectories(K1, terminal=term1, indices=True)
        xb, ib = bank.sample_trajectories_backward(K1, term1, return_indices=True)
        np.testing.assert_array_equal(ib, ig)
        same_bits(xb, xg, "T = 1")
    bank.close()


# ---- 4. degenerate inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(500, 0), (1027, 512)], ids=["lane-500", "tiled-1027-t512"])
def test_bad_filter_next_to_live_ones(sa, oracle, shape):
    n, tile = shape
    theta = (sc.TH_SVOL3[0], (-1.0, 0.95, 0.25), sc.TH_SVOL3[2])            # beta = -1: log g = -inf, no weight
    y, z = sc.stock_series(sc.MODEL_SVOL, 7)
    hist = bc.twin_history(sa, sc.MODEL_SVOL, theta, n, tile, 1, y, z)
    bank = bc.recorded(sa, sc.MODEL_SVOL, theta, n, tile, True, 1, y, z)
    bc.check_logweights(bank, hist, f"bad row N={n}")
    assert np.isneginf(bank.series_logweights(1, 3)).all()
    fb = bc.check_backward(oracle, bank, hist, logf_rows(oracle, sc.MODEL_SVOL, theta), 1, (G + 1,), f"bad row N={n}")
    assert fb == (G + 1) * 6                                                # every draw of the dead filter takes the genealogy
    x, idx = bank.sample_trajectories_backward(G + 1, return_indices=True)
    assert np.isnan(x[1]).all() and np.isfinite(x[0]).all() and np.isfinite(x[2]).all() and (idx < n).all()
    bank.close()


@pytest.mark.parametrize("shape", [(500, 0), (1027, 512)], ids=["lane-500", "tiled-1027-t512"])
def test_a_step_without_weight_takes_the_genealogy(sa, oracle, shape):
    """y_3 = 1e200: every log-weight of step 3 is -inf in every filter, so the draw of B_3 has nothing to draw from; step 4 resamples
    from zeros and the series ends with weight.  B_3 is then the lineage of B_4, and every other step is drawn."""
    n, tile = shape
    y, z = sc.stock_series(sc.MODEL_SVOL, 7)
    y[3] = 1e200
    hist = bc.twin_history(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, 1, y, z)
    assert all(np.isneginf(hist["lws"][f][3]).all() for f in range(3))
    bank = bc.recorded(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, True, 1, y, z)
    K = G + 1
    fb = bc.check_backward(oracle, bank, hist, logf_rows(oracle, sc.MODEL_SVOL, sc.TH_SVOL3), 1, (K,), f"dead step N={n}")
    assert fb == 3 * K
    x, idx = bank.sample_trajectories_backward(K, return_indices=True)
    assert np.isfinite(x).all()
    for f in range(3):
        np.testing.assert_array_equal(idx[f, :, 3], hist["ancs"][f][4][idx[f, :, 4]])
    bank.close()


def test_refusals_and_life_cycle(sa):
    from ssme_amd import _capi
    from test_backward_cpu import refusals_with_a_handle
    L = _capi.lib()
    n, T = 500, 7
    y, z = sc.stock_series(sc.MODEL_SVOL, T)
    bank = sc.make_bank(sa, sc.MODEL_SVOL, n, sc.TH_SVOL3, 0, 1, 0)
    refusals_with_a_handle(L, bank._h, n=n, r=3)
    bank.record_series_history()
    bank.run_series(y, z)
    buf, lw = np.zeros(bank.r * T * 4), np.zeros(n)
    back = lambda steps=T, K=1: L.ssme_pf_sample_trajectories_backward(bank._h, K, None, _capi.dptr(buf), None, steps)
    row = lambda t=0: L.ssme_pf_download_series_logweights(bank._h, 0, t, _capi.dptr(lw))
    # the argument refusals once a history IS in force
    assert back(K=n + 1) == _capi.ERR_INVALID_ARG and back(T + 1) == _capi.ERR_INVALID_ARG and row(T) == _capi.ERR_INVALID_ARG
    assert back() == _capi.OK and row(T - 1) == _capi.OK
    x1, i1 = bank.sample_trajectories_backward(G + 1, return_indices=True)
    l1 = bank.series_logweights(2, 4)
    for what, move in (("step", lambda: bank.step(y[0], None)), ("reset", bank.reset), ("set_params", lambda: bank.set_params(np.asarray(sc.TH_SVOL3)))):
        assert back() == _capi.OK, what
        move()
        assert back() == _capi.ERR_STATE and row() == _capi.ERR_STATE, what
        bank.run_series(y, z)                              # the setting survived: this run records again
    # a second recording run of ANOTHER series refills the weights buffer: nothing of the first is handed out
    y2 = sc.stock_series(sc.MODEL_SVOL, T, shift=50)[0]
    bank.run_series(y2, None)
    l2 = bank.series_logweights(2, 4)
    assert not np.array_equal(l2, l1)
    hist2 = bc.twin_history(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, 0, 1, y2, None)
    same_bits(l2, hist2["lws"][2][4], "refilled after a second recording run")
    bank.run_series(y, z)
    x3, i3 = bank.sample_trajectories_backward(G + 1, return_indices=True)
    np.testing.assert_array_equal(i3, i1)
    same_bits(x3, x1, "the first series again: the same trajectories")
    same_bits(bank.series_logweights(2, 4), l1, "... and rows")
    kernel_ms, call_ms = bank.smoothing_elapsed_ms()
    assert 0.0 < kernel_ms <= call_ms
    bank.record_series_history(False)
    bank.run_series(y, z)
    assert back() == _capi.ERR_STATE
    bank.close()


def test_f32_handle_rounds_the_states(sa):
    n, tile = 500, 0
    y, z = sc.stock_series(sc.MODEL_SVOL, 7)
    th32 = np.asarray(sc.TH_SVOL3, dtype=np.float32).astype(np.float64)
    y32 = y.astype(np.float32).astype(np.float64)
    b64 = bc.recorded(sa, sc.MODEL_SVOL, th32, n, tile, True, 1, y32, None)
    b32 = bc.recorded(sa, sc.MODEL_SVOL, np.asarray(sc.TH_SVOL3), n, tile, True, 1, y, None, dtype=1)
    x64, i64 = b64.sample_trajectories_backward(G + 1, return_indices=True)
    x32, i32 = b32.sample_trajectories_backward(G + 1, return_indices=True)
    np.testing.assert_array_equal(i32, i64)
    same_bits(x32, x64.astype(np.float32).astype(np.float64), "trajectories rounded to float")
    b64.close()
    b32.close()


# ---- 5. user models -----------------------------------------------------------------------------------------------------------------------
def _worker(tmp_path_factory, header, lib=None):
    if header not in _WORKER:
        try:
            from ssme_amd import build
            env = dict(os.environ)
            src = header if lib is None else lib[0]
            env["SSME_PF_LIB"] = build.build_user_model(os.path.join(ROOT, "tests", "models", src + ".h"), src if lib is None else lib[1])
            out = str(tmp_path_factory.mktemp("backward_" + header) / "res.pkl")
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "backward_worker.py"), out, header], env=env, check=True, timeout=240)
            with open(out, "rb") as f:
                _WORKER[header] = pickle.load(f)
        except Exception as e:          # remembered, not retried
            _WORKER[header] = e
    if isinstance(_WORKER[header], Exception):
        raise RuntimeError(f"the worker failed and is not started again: {_WORKER[header]!r}") from _WORKER[header]
    return _WORKER[header]


@pytest.mark.parametrize("header", ["svol_student_t_f", "svol_two_factor_f", "svol_reg_cov_f"])
def test_user_model_with_a_transition_density(tmp_path_factory, header):
    """A scalar model, a (2, 2) vector model and a dim_cov model with a first step of its own: log-weights and backward simulation
    equal the restatement at N in {65, 513} on the lane kernel, the pair kernel and the tiled route (the worker asserts it)."""
    res = _worker(tmp_path_factory, header)
    assert len(res) == 6
    for name, r in res.items():
        assert r["fallbacks"] == 0 and r["dx"] == (2 if header == "svol_two_factor_f" else 1), name
    assert {r["route"][0] for r in res.values()} == {sc.ROUTE_SERIES_LANE, sc.ROUTE_SERIES_PAIR, sc.ROUTE_TILED}


def test_user_model_without_a_transition_density_is_unsupported(tmp_path_factory):
    res = _worker(tmp_path_factory, "no_logf", lib=("svol_student_t", "student_t"))
    assert res["backward"] == res["unsupported"] and res["logweights"] == res["unsupported"]
    assert res["genealogy"] == 0                            # ... and the header behaves as before


# ---- 6. what the feature is for -----------------------------------------------------------------------------------------------------------
def _rts(phi, sigma, tau, y):
    """Exact smoothed means and variances of x_t = phi x_{t-1} + sigma e_t, y_t = x_t + tau v_t, x_0 ~ N(0, sigma^2 / (1 - phi^2)):
    the Kalman filter and the Rauch-Tung-Striebel backward recursion."""
    T = len(y)
    P0 = sigma ** 2 / (1.0 - phi ** 2)
    m, P, mp, Pp = np.empty(T), np.empty(T), np.empty(T), np.empty(T)
    for t in range(T):
        mp[t] = 0.0 if t == 0 else phi * m[t - 1]
        Pp[t] = P0 if t == 0 else phi ** 2 * P[t - 1] + sigma ** 2
        k = Pp[t] / (Pp[t] + tau ** 2)
        m[t] = mp[t] + k * (y[t] - mp[t])
        P[t] = (1.0 - k) * Pp[t]
    ms, Ps = m.copy(), P.copy()
    for t in range(T - 2, -1, -1):
        g = P[t] * phi / Pp[t + 1]
        ms[t] = m[t] + g * (ms[t + 1] - mp[t + 1])
        Ps[t] = P[t] + g * g * (Ps[t + 1] - Pp[t + 1])
    return ms, Ps


def test_backward_simulation_undoes_path_degeneracy(sa):
    """Linear Gaussian model (phi, sigma, tau) = (0.9, 0.5, 0.7), N = 256, T = 64, K = 256, one filter, a series simulated from the model.

    The K genealogical paths of the filter share their ancestor at t = 0 (one distinct index); backward simulation draws x_0 again from
    all N particles, and the moments of its K draws are compared with the EXACT smoothed law N(mu, V) of x_0 (Rauch-Tung-Striebel).

    Margins (5 standard errors of each of the two independent errors, added):
      * K draws: given the filter they are iid, so their mean has standard error sqrt(V / K) and their variance V sqrt(2 / (K - 1));
      * the filter's own Monte-Carlo error at t = 0: the particles x_0[i] are N iid draws from the prior p = N(0, P0), and the smoothed
        law pi is approximated by reweighting them -- self-normalised importance sampling, whose asymptotic variance for a function h
        is  int pi(x)^2 / p(x) (h(x) - E_pi h)^2 dx / N,  evaluated by quadrature for h = x and h = (x - mu)^2.
    With this series: mu = -0.4345, V = 0.2310, margin of the mean 0.3050, of the variance 0.1924.  A plain numpy bootstrap filter with
    numpy backward simulation, 200 seeds at this shape: worst |error| / margin 0.41 (mean) and 0.45 (variance), about 110 distinct
    indices at t = 0.
    Measured on the device (MI355X): 116 distinct x_0 indices against the genealogy's 4, mean error +0.0915 (margin 0.3050),
    variance error -0.0036 (margin 0.1924)."""
    phi, sigma, tau = 0.9, 0.5, 0.7
    n, T, K = 256, 64, 256
    P0 = sigma ** 2 / (1.0 - phi ** 2)
    rng = np.random.default_rng(20240229)
    xs = np.empty(T)
    xs[0] = rng.normal() * np.sqrt(P0)
    for t in range(1, T):
        xs[t] = phi * xs[t - 1] + sigma * rng.normal()
    y = xs + tau * rng.normal(size=T)
    ms, Ps = _rts(phi, sigma, tau, y)
    mu, V = float(ms[0]), float(Ps[0])
    g = np.linspace(-12.0, 12.0, 200001) * np.sqrt(P0)
    dg = g[1] - g[0]
    pi = np.exp(-0.5 * (g - mu) ** 2 / V) / np.sqrt(2.0 * np.pi * V)
    p = np.exp(-0.5 * g * g / P0) / np.sqrt(2.0 * np.pi * P0)
    w = pi * pi / p
    is_mean = np.sqrt(np.sum(w * (g - mu) ** 2) * dg / n)
    is_var = np.sqrt(np.sum(w * ((g - mu) ** 2 - V) ** 2) * dg / n)
    margin_mean = 5.0 * (np.sqrt(V / K) + is_mean)
    margin_var = 5.0 * (V * np.sqrt(2.0 / (K - 1)) + is_var)
    assert abs(mu + 0.4345) < 1e-3 and abs(V - 0.2310) < 1e-3 and abs(margin_mean - 0.3050) < 1e-3 and abs(margin_var - 0.1924) < 1e-3
    bank = bc.recorded(sa, sc.MODEL_LIN_GAUSS, ((phi, sigma, tau),), n, 0, True, 1, y, None)
    xg, ig = bank.sample_trajectories(K, indices=True)
    xb, ib = bank.sample_trajectories_backward(K, return_indices=True)
    means = bank.backward_smoothed_means(K, (0, 1))
    bank.close()
    d_gen, d_back = len(np.unique(ig[0, :, 0])), len(np.unique(ib[0, :, 0]))
    x0 = xb[0, :, 0, 0]
    err_mean, err_var = float(x0.mean() - mu), float(x0.var(ddof=1) - V)
    print(f"distinct x_0 indices: genealogy {d_gen}, backward {d_back}; mean error {err_mean:+.4f} (margin {margin_mean:.4f}), "
          f"variance error {err_var:+.4f} (margin {margin_var:.4f})")
    assert d_back > d_gen, (d_back, d_gen)
    assert abs(err_mean) <= margin_mean, (err_mean, margin_mean)
    assert abs(err_var) <= margin_var, (err_var, margin_var)
    # backward_smoothed_means is the plain mean of the same K draws
    assert means.shape == (T, 2, 1)
    np.testing.assert_allclose(means[:, 0, 0], xb[0, :, :, 0].mean(axis=0), rtol=0, atol=1e-15)
    np.testing.assert_allclose(means[:, 1, 0], (xb[0, :, :, 0] ** 2).mean(axis=0), rtol=0, atol=1e-15)
