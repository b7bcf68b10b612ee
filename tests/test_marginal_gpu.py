"""Marginal smoothing weights (ssme_pf_download_smoothing_weights, ssme_pf_get_marginal_smoothed_expectations) on the device.

The reference of every parity test is a twin handle of the same configuration stepped with step() under set_debug(record_ancestors,
keep_logw) and downloaded after every step; tests/marginal_ref.py restates the recursion from those downloads, column by column with
backward_ref.backward_weights -- the weights backward simulation draws from -- and sums in float64 in its own order.  The tolerance is
derived, not tuned: all terms are non-negative and a step adds at most N + 1 roundings per row entry on each side, so with u = 2^-53

    |device - ref| <= 2.2 (T - 1 - t) (N + 1) u ref     at row t        (marginal_ref.bound)

exact zeros coincide, and row T - 1 has the bits of ssme_pf_download_weights.  The last test is what the feature is for: against the
exact Rauch-Tung-Striebel smoother of a linear Gaussian model.
Every test here fails without the feature: the entry points do not exist there."""
import ctypes as C
import math
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import backward_cases as bc
import backward_ref as br
import marginal_cases as mc
import series_expect_cases as sc
from backward_cases import same_bits
from test_backward_gpu import SHAPES as BACKWARD_SHAPES, _rts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
THETAS = {sc.MODEL_SVOL: sc.TH_SVOL3, sc.MODEL_SVOL_LEVERAGE: sc.TH_LEV3, sc.MODEL_LIN_GAUSS: sc.TH_LG3}
# (N, tile_particles): the shapes of backward simulation -- among them the edges of the 64 rows of a workgroup of k_msm_rows and of
# the 64 columns one of its waves stages at a time (63 | 64 | 65), of one chunk per wave (8 x 64 = 512 | 513), which is also the edge of
# the 512 columns of a workgroup of k_msm_columns -- and the edges of the 256 rows k_msm_columns stages at a time (255 | 256 | 257)
SHAPES = tuple(sorted(set(BACKWARD_SHAPES + ((255, 0), (256, 0), (257, 0), (512, 0)))))
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


def all_rows(bank, T):
    return np.stack([mc.device_rows(bank, f, T)[0] for f in range(bank.r)])


# ---- 1. every row against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}")
def test_rows_equal_the_restatement_at_every_shape(sa, oracle, shape):
    """SVOL.  (T, R) = (7, 3), (2, 1), (1, 1) up to N = 513, (3, 1) above.  The longest case is also formed from a history recorded on
    the tiled route (small-series route off), which must agree to the bit."""
    n, tile = shape
    cases = ((7, 3), (2, 1), (1, 1)) if n <= 513 else ((3, 1),)
    for steps, R in cases:
        theta = sc.TH_SVOL3[:R]
        y, z = sc.stock_series(sc.MODEL_SVOL, steps)
        hist = bc.twin_history(sa, sc.MODEL_SVOL, theta, n, tile, 1, y, z)
        bank = bc.recorded(sa, sc.MODEL_SVOL, theta, n, tile, True, 1, y, z)
        name = f"N={n} tile={tile} T={steps} R={R}"
        assert bank.marginal_smoothing_bytes(steps) == 32 * steps * bank.r * bank.tile * bank.n_tiles == 4 * bank.backward_bytes(steps)
        degenerate, worst = mc.check_rows(oracle, bank, hist, logf_rows(oracle, sc.MODEL_SVOL, theta), 1, name)
        print(f"{name}: worst |device - ref| / bound = {worst:.4f}")
        assert degenerate == 0, name
        if steps == cases[0][0]:
            rows = all_rows(bank, steps)
            if n >= 63:
                assert len(np.unique(rows[0, 0])) > 1, name + ": the weights of step 0 have spread"
            other = bc.recorded(sa, sc.MODEL_SVOL, theta, n, tile, False, 1, y, z)
            same_bits(all_rows(other, steps), rows, name + ": from a history recorded on the tiled route")
            other.close()
        bank.close()


@pytest.mark.parametrize("sched", [1, 3])
@pytest.mark.parametrize("model", [sc.MODEL_SVOL_LEVERAGE, sc.MODEL_LIN_GAUSS], ids=["leverage", "lin-gauss"])
def test_rows_other_models_and_schedules(sa, oracle, model, sched):
    """The leverage model's density reads the covariate of step t + 1; with resamp_sched = 3 most steps carry their weights over and a
    degenerate column would stay where it is.  N = 65 and 513 on 512-particle tiles (the tiled route)."""
    y, z = sc.stock_series(model, 8)
    for n, tile in ((65, 0), (513, 512)):
        hist = bc.twin_history(sa, model, THETAS[model], n, tile, sched, y, z)
        bank = bc.recorded(sa, model, THETAS[model], n, tile, True, sched, y, z)
        name = f"model={model} N={n} sched={sched}"
        _, worst = mc.check_rows(oracle, bank, hist, logf_rows(oracle, model, THETAS[model]), sched, name, zs=zs_of(z))
        print(f"{name}: worst |device - ref| / bound = {worst:.4f}")
        mc.check_means(bank, 8, name)
        bank.close()


# ---- 2. exact anchors -------------------------------------------------------------------------------------------------------------------
def test_one_particle_rows_are_the_final_weight(sa):
    """N = 1: q = D = 2^sh, so c q = w_0 exactly at every step."""
    y, z = sc.stock_series(sc.MODEL_SVOL, 7)
    bank = bc.recorded(sa, sc.MODEL_SVOL, sc.TH_SVOL3, 1, 0, True, 1, y, z)
    for f in range(3):
        w = bank.weights(f)[1]
        for t in range(7):
            same_bits(bank.smoothing_weights(f, t)[1], w, f"N = 1, filter {f}, step {t}")
    bank.close()


@pytest.mark.parametrize("shape", [(500, 0), (1027, 512)], ids=["lane-500", "tiled-1027-t512"])
def test_calls_repeat_and_leave_the_other_smoothers_alone(sa, shape):
    n, tile = shape
    y, z = sc.stock_series(sc.MODEL_SVOL, 7)
    # T = 1: the row is the final weights
    bank = bc.recorded(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, True, 1, y[:1], None)
    for f in range(3):
        same_bits(bank.smoothing_weights(f, 0)[1], bank.weights(f)[1], "T = 1")
    bank.close()
    bank = bc.recorded(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, True, 1, y, z)
    K = 9
    before = (bank.sample_trajectories(K, indices=True), bank.sample_trajectories_backward(K, return_indices=True), bank.smoothed_expectations((0, 1, 2, 3)))
    rows = all_rows(bank, 7)
    means = bank.marginal_smoothed_expectations((0, 2))
    same_bits(all_rows(bank, 7), rows, "two calls, same bits")
    same_bits(bank.marginal_smoothed_expectations((0, 2)), means, "two calls, same means")
    after = (bank.sample_trajectories(K, indices=True), bank.sample_trajectories_backward(K, return_indices=True), bank.smoothed_expectations((0, 1, 2, 3)))
    for a, b, what in zip(before, after, ("the genealogy", "backward simulation", "the genealogical means")):
        if isinstance(a, tuple):
            same_bits(a[0], b[0], what)
            np.testing.assert_array_equal(a[1], b[1], err_msg=what)
        else:
            same_bits(a, b, what)
    # a fresh handle that asks for the means FIRST fills the same rows
    fresh = bc.recorded(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, True, 1, y, z)
    same_bits(fresh.marginal_smoothed_expectations((0, 2)), means, "means first")
    same_bits(all_rows(fresh, 7), rows, "means first, then the rows")
    fresh.close()
    bank.close()


# ---- 3. degenerate inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(500, 0), (1027, 512)], ids=["lane-500", "tiled-1027-t512"])
def test_bad_filter_next_to_live_ones(sa, oracle, shape):
    n, tile = shape
    theta = (sc.TH_SVOL3[0], (-1.0, 0.95, 0.25), sc.TH_SVOL3[2])            # beta = -1: log g = -inf, no weight
    y, z = sc.stock_series(sc.MODEL_SVOL, 7)
    hist = bc.twin_history(sa, sc.MODEL_SVOL, theta, n, tile, 1, y, z)
    bank = bc.recorded(sa, sc.MODEL_SVOL, theta, n, tile, True, 1, y, z)
    assert not mc.final_weights(bank, 1)[1] and mc.final_weights(bank, 0)[1] and mc.final_weights(bank, 2)[1]
    mc.check_rows(oracle, bank, hist, logf_rows(oracle, sc.MODEL_SVOL, theta), 1, f"bad row N={n}")       # zero rows of filter 1 asserted there
    out = mc.check_means(bank, 7, f"bad row N={n}")
    assert np.isnan(out[:, :, 1]).all() and np.isfinite(out[:, :, 0]).all() and np.isfinite(out[:, :, 2]).all()
    bank.close()


@pytest.mark.parametrize("shape", [(500, 0), (1027, 512)], ids=["lane-500", "tiled-1027-t512"])
def test_a_step_without_weight_takes_the_genealogy(sa, oracle, shape):
    """y_3 = 1e200: every log-weight of step 3 is -inf in every filter, so every column of step 4 is degenerate and row 3 is the
    genealogical push of row 4, exactly: om_3[i] = the sum of om_4[j] over anc_4[j] = i in the kernel's order (marginal_cases.device_order_push)."""
    n, tile = shape
    y, z = sc.stock_series(sc.MODEL_SVOL, 7)
    y[3] = 1e200
    hist = bc.twin_history(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, 1, y, z)
    assert all(np.isneginf(hist["lws"][f][3]).all() for f in range(3))
    bank = bc.recorded(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, True, 1, y, z)
    degenerate, _ = mc.check_rows(oracle, bank, hist, logf_rows(oracle, sc.MODEL_SVOL, sc.TH_SVOL3), 1, f"dead step N={n}")
    assert degenerate == 3 * n
    for f in range(3):
        row4, row3 = bank.smoothing_weights(f, 4)[1], bank.smoothing_weights(f, 3)[1]
        push = mc.device_order_push(row4, np.minimum(hist["ancs"][f][4], n - 1), n)
        same_bits(row3, push, f"dead step N={n}, filter {f}: row 3 is the push of row 4")
    mc.check_means(bank, 7, f"dead step N={n}")
    bank.close()


# ---- 4. means, rounding, life cycle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 0), (257, 0), (500, 0), (2049, 0)], ids=lambda s: f"N{s[0]}")
def test_means_equal_the_rows(sa, shape):
    n, tile = shape
    T = 5
    y, z = sc.stock_series(sc.MODEL_SVOL, T)
    bank = bc.recorded(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, True, 1, y, z)
    out = mc.check_means(bank, T, f"means N={n}")
    one = mc.check_means(bank, T, f"means N={n}, one functional", functionals=(2,))
    same_bits(one[:, 0], out[:, 2], "a functional alone == the same functional among four")
    # row T - 1: the filtered expectations, formed from the same weights by another tree
    filt = bank.expectations_multi((0, 1, 2, 3))
    for f in range(bank.r):
        x, w = bank.smoothing_weights(f, T - 1)
        for i in range(4):
            h = mc.HS[i](np.atleast_2d(x)[0])
            tol = (n + 3) * mc.U * math.fsum(np.abs(h) * w) / math.fsum(w)
            assert abs(out[T - 1, i, f] - filt[i, f]) <= tol, (n, f, i, out[T - 1, i, f], filt[i, f], tol)
    bank.close()


def test_f32_handle_rounds_weights_and_means(sa):
    n, tile = 500, 0
    y, z = sc.stock_series(sc.MODEL_SVOL, 7)
    th32 = np.asarray(sc.TH_SVOL3, dtype=np.float32).astype(np.float64)
    y32 = y.astype(np.float32).astype(np.float64)
    b64 = bc.recorded(sa, sc.MODEL_SVOL, th32, n, tile, True, 1, y32, None)
    b32 = bc.recorded(sa, sc.MODEL_SVOL, np.asarray(sc.TH_SVOL3), n, tile, True, 1, y, None, dtype=1)
    r32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    for t in (0, 6):
        x64, w64 = b64.smoothing_weights(2, t)
        x32, w32 = b32.smoothing_weights(2, t)
        same_bits(w32, r32(w64), "weights rounded to float")
        same_bits(x32, r32(x64), "states rounded to float")
    same_bits(b32.marginal_smoothed_expectations((0, 2)), r32(b64.marginal_smoothed_expectations((0, 2))), "means rounded to float")
    b64.close()
    b32.close()


def test_refusals_and_life_cycle(sa, oracle):
    from ssme_amd import _capi
    from test_marginal_cpu import refusals_with_a_handle
    L = _capi.lib()
    n, T = 500, 7
    y, z = sc.stock_series(sc.MODEL_SVOL, T)
    bank = sc.make_bank(sa, sc.MODEL_SVOL, n, sc.TH_SVOL3, 0, 1, 0)
    refusals_with_a_handle(L, bank._h, n=n, r=3)
    bank.record_series_history()
    bank.run_series(y, z)
    buf, w = np.zeros(T * 4 * bank.r), np.zeros(n)
    ids = (C.c_int32 * 4)(0, 1, 2, 3)
    means = lambda steps=T, k=1: L.ssme_pf_get_marginal_smoothed_expectations(bank._h, ids, k, _capi.dptr(buf), steps)
    row = lambda t=0, f=0: L.ssme_pf_download_smoothing_weights(bank._h, f, t, None, _capi.dptr(w))
    # the argument refusals once a history IS in force
    assert means(T + 1) == _capi.ERR_INVALID_ARG and means(T - 1) == _capi.ERR_INVALID_ARG and row(T) == _capi.ERR_INVALID_ARG
    assert row(0, 3) == _capi.ERR_INVALID_ARG and means(k=5) == _capi.ERR_INVALID_ARG
    assert means() == _capi.OK and row(T - 1) == _capi.OK
    kernel_ms, call_ms = bank.smoothing_elapsed_ms()
    assert 0.0 <= kernel_ms <= call_ms
    rows1 = all_rows(bank, T)
    m1 = bank.marginal_smoothed_expectations((0, 2))
    for what, move in (("step", lambda: bank.step(y[0], None)), ("reset", bank.reset), ("set_params", lambda: bank.set_params(np.asarray(sc.TH_SVOL3))),
                       ("set_seed", lambda: bank.set_seed(sc.SEED))):
        assert means() == _capi.OK and row() == _capi.OK, what
        move()
        assert means() == _capi.ERR_STATE and row() == _capi.ERR_STATE, what
        bank.run_series(y, z)                              # the setting survived: this run records again
    # a second recording run of ANOTHER series of the same length refills the rows: nothing of the first is handed out, whether or not
    # backward simulation filled the log-weights first
    y2 = sc.stock_series(sc.MODEL_SVOL, T, shift=50)[0]
    bank.run_series(y2, None)
    bank.sample_trajectories_backward(1)
    rows2 = all_rows(bank, T)
    assert not np.array_equal(rows2[:, 0], rows1[:, 0])
    hist2 = bc.twin_history(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, 0, 1, y2, None)
    mc.check_rows(oracle, bank, hist2, logf_rows(oracle, sc.MODEL_SVOL, sc.TH_SVOL3), 1, "refilled after a second recording run")
    bank.run_series(y, z)
    same_bits(all_rows(bank, T), rows1, "the first series again: the same rows")
    same_bits(bank.marginal_smoothed_expectations((0, 2)), m1, "... and means")
    # a shorter series in the same buffers, then the longer one again
    bank.run_series(y[:4], None if z is None else z[:4])
    assert means(4) == _capi.OK and means(T) == _capi.ERR_INVALID_ARG and row(4) == _capi.ERR_INVALID_ARG and row(3) == _capi.OK
    bank.run_series(y, z)
    same_bits(all_rows(bank, T), rows1, "after a shorter series: the same rows")
    bank.record_series_history(False)
    bank.run_series(y, z)
    assert means() == _capi.ERR_STATE and row() == _capi.ERR_STATE
    bank.close()


# ---- 5. user models ---------------------------------------------------------------------------------------------------------------------
def _worker(tmp_path_factory, header, lib=None):
    if header not in _WORKER:
        try:
            from ssme_amd import build
            env = dict(os.environ)
            src = header if lib is None else lib[0]
            env["SSME_PF_LIB"] = build.build_user_model(os.path.join(ROOT, "tests", "models", src + ".h"), src if lib is None else lib[1])
            out = str(tmp_path_factory.mktemp("marginal_" + header) / "res.pkl")
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "marginal_worker.py"), out, header], env=env, check=True, timeout=240)
            with open(out, "rb") as f:
                _WORKER[header] = pickle.load(f)
        except Exception as e:          # remembered, not retried
            _WORKER[header] = e
    if isinstance(_WORKER[header], Exception):
        raise RuntimeError(f"the worker failed and is not started again: {_WORKER[header]!r}") from _WORKER[header]
    return _WORKER[header]


@pytest.mark.parametrize("header", ["svol_student_t_f", "svol_two_factor_f", "svol_reg_cov_f"])
def test_user_model_with_a_transition_density(tmp_path_factory, header):
    """A scalar model, a (2, 2) vector model and a dim_cov model with a first step of its own: every row within the bound of the
    restatement at N in {65, 513} on the lane kernel, the pair kernel and the tiled route (the worker asserts it)."""
    res = _worker(tmp_path_factory, header)
    assert len(res) == 6
    for name, r in res.items():
        assert r["degenerate"] == 0 and r["dx"] == (2 if header == "svol_two_factor_f" else 1) and 0.0 <= r["worst"] <= 1.0, name
    assert {r["route"][0] for r in res.values()} == {sc.ROUTE_SERIES_LANE, sc.ROUTE_SERIES_PAIR, sc.ROUTE_TILED}


def test_user_model_without_a_transition_density_is_unsupported(tmp_path_factory):
    res = _worker(tmp_path_factory, "no_logf", lib=("svol_student_t", "student_t"))
    assert res["weights"] == res["unsupported"] and res["means"] == res["unsupported"]
    assert res["bytes"] == 0 and res["genealogy"] == 0     # ... and the header behaves as before


# ---- 6. what the feature is for ---------------------------------------------------------------------------------------------------------
def test_marginal_weights_undo_path_degeneracy(sa):
    """The linear Gaussian series of test_backward_simulation_undoes_path_degeneracy: (phi, sigma, tau) = (0.9, 0.5, 0.7), N = 256, T = 64,
    one filter, the same seed.

    The genealogy of the filter reaches x_0 through a handful of distinct indices; under om_0 far more particles carry weight, and the
    mean and variance of x_0 under om_0 are compared with the EXACT smoothed law N(mu, V) of x_0 (Rauch-Tung-Striebel).  There are no K
    draws here, so the margins are 5 standard errors of the filter's part alone: the particles x_0[i] are N iid draws from the prior and
    the smoothed law is approximated by reweighting them -- self-normalised importance sampling, whose asymptotic variance that test
    derives by quadrature.  With this series: mu = -0.4345, V = 0.2310, margin of the mean 0.1548, of the variance 0.0901.  A plain
    numpy bootstrap filter with this recursion, 200 seeds at this shape: worst |error| / margin 0.72 (mean) and 0.62 (variance).
    Measured on the device (MI355X): the genealogy reaches x_0 through 4 distinct indices, all 256 particles carry weight under om_0
    (effective sample size 128.9), mean error +0.0520 (margin 0.1548), variance error -0.0021 (margin 0.0901)."""
    phi, sigma, tau = 0.9, 0.5, 0.7
    n, T = 256, 64
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
    margin_mean = 5.0 * np.sqrt(np.sum(w * (g - mu) ** 2) * dg / n)
    margin_var = 5.0 * np.sqrt(np.sum(w * ((g - mu) ** 2 - V) ** 2) * dg / n)
    assert abs(mu + 0.4345) < 1e-3 and abs(V - 0.2310) < 1e-3 and abs(margin_mean - 0.1548) < 1e-3 and abs(margin_var - 0.0901) < 1e-3
    bank = bc.recorded(sa, sc.MODEL_LIN_GAUSS, ((phi, sigma, tau),), n, 0, True, 1, y, None)
    ig = bank.sample_trajectories(n, terminal=np.arange(n, dtype=np.uint32)[None, :], indices=True)[1]
    x0, om0 = bank.smoothing_weights(0, 0)
    means = bank.marginal_smoothed_expectations((0, 1))
    bank.close()
    d_gen, d_marg = len(np.unique(ig[0, :, 0])), int(np.count_nonzero(om0 > 0.0))
    W = om0 / math.fsum(om0)
    ess = 1.0 / float(np.sum(W * W))
    m0 = float(np.sum(W * x0))
    err_mean, err_var = m0 - mu, float(np.sum(W * (x0 - m0) ** 2)) - V
    print(f"x_0: genealogy {d_gen} distinct indices, {d_marg} particles with weight under om_0 (effective sample size {ess:.1f}); "
          f"mean error {err_mean:+.4f} (margin {margin_mean:.4f}), variance error {err_var:+.4f} (margin {margin_var:.4f})")
    assert d_marg > d_gen, (d_marg, d_gen)
    assert abs(err_mean) <= margin_mean, (err_mean, margin_mean)
    assert abs(err_var) <= margin_var, (err_var, margin_var)
    # the device's means are the same moments
    assert abs(means[0, 0, 0] - m0) <= (n + 3) * mc.U * float(np.sum(W * np.abs(x0)))
    assert abs(means[0, 1, 0] - float(np.sum(W * x0 * x0))) <= (n + 3) * mc.U * float(np.sum(W * x0 * x0))
