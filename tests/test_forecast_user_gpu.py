"""GPU suite for forecasts of user models that declare their observation draw (ssme_amd/csrc/model_api.h: gsamp / gsamp_vec; kernels
k_fc_start_vec and k_fc_horizon_user of ssme_amd/csrc/forecast.h).  Every model's library runs in a process
of its own (tests/forecast_user_model_worker.py with SSME_PF_LIB), one at a time, each with its own timeout.

  * twin: in ONE library a scalar user model that restates the built-in leverage model returns the built-in model's bits;
  * parity: (2, 2), (3, 1) and (4, 4) against tests/forecast_user_ref.py from the device's own downloaded state, bit for bit;
  * analytic anchors of the (4, 4) linear Gaussian model with libm only, |z| <= 5 each: the particles of a forecast are independent
    given the filtered cloud (iid ancestors, counters of their own), so every standard error is that of an iid sample;
  * determinism, non-interference, the contract of the entry point, and the C++ adaptor."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fc_user_cases as cases
import forecast_user_ref as fur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "tests", "models")
LIBS = {"svol_leverage_user": "leverage_user", "svol_two_factor_g": "two_factor_g", "svol_two_factor_lev_g": "two_factor_lev_g", "lin_gauss_3d_g": "lin_gauss_3d_g", "lin_gauss_4d_g": "lin_gauss_4d_g"}
DIMS = {"svol_two_factor_g": (2, 2), "svol_two_factor_lev_g": (2, 2), "lin_gauss_3d_g": (3, 1), "lin_gauss_4d_g": (4, 4)}


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a HIP device"
    import ssme_amd
    return ssme_amd


def _lib(model):
    from ssme_amd import build
    return build.build_user_model(os.path.join(MODELS, model + ".h"), LIBS[model])


def _worker(model, mode, tmp_path, timeout=300):
    out = str(tmp_path / (model + "_" + mode + ".npz"))
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "forecast_user_model_worker.py"), mode, out, model],
                   env=dict(os.environ, SSME_PF_LIB=_lib(model)), check=True, timeout=timeout)
    return np.load(out)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def test_scalar_user_model_is_the_built_in_leverage_model_bit_for_bit(sa, tmp_path):
    """SSME_MODEL_USER0 (svol_leverage_user.h) and SSME_MODEL_SVOL_LEVERAGE handles of one library: same seed, ids, theta, last_obs != 0,
    after 4 steps.  Particles, cdf, start, x and y are identical bits at every shape."""
    r = _worker("svol_leverage_user", "twin", tmp_path)
    for n, tile, H, R in cases.TWIN_SHAPES:
        u, b = f"u_{n}_{H}_{R}", f"b_{n}_{H}_{R}"
        assert int(r["tile_" + u][0]) == int(r["tile_" + b][0]) and (tile == 0 or int(r["tile_" + u][0]) == tile)
        assert _same_bits(r["ll_" + u], r["ll_" + b]) and np.isfinite(r["ll_" + u]).all(), (n, H, R)
        for f in range(R):
            assert _same_bits(r[f"x{f}_" + u], r[f"x{f}_" + b]), (n, H, R, f)
            assert np.array_equal(r[f"cdf{f}_" + u], r[f"cdf{f}_" + b]), (n, H, R, f)
        assert r["y_" + u].shape == (R, H, n) and r["xs_" + u].shape == (R, H, n) and r["start_" + u].shape == (R, n)
        assert np.array_equal(r["start_" + u], r["start_" + b]), (n, H, R)
        assert _same_bits(r["xs_" + u], r["xs_" + b]), (n, H, R)
        assert _same_bits(r["y_" + u], r["y_" + b]), (n, H, R)
        assert np.isfinite(r["y_" + u]).all()
        if R > 1:                                                    # per-filter theta and ids: the filters differ
            assert not np.array_equal(r["y_" + u][0], r["y_" + u][1])


@pytest.mark.parametrize("model", ["svol_two_factor_g", "svol_two_factor_lev_g", "lin_gauss_3d_g", "lin_gauss_4d_g"])
def test_vector_models_equal_the_reference_bit_for_bit(sa, oracle, tmp_path, model):
    """start, x and y of every filter against forecast_user_ref from the device's own downloaded state: N = 1, odd N (the pad column),
    one tile, several tiles with a ragged 7-particle last one (where the draw must cross tiles).  svol_two_factor_lev_g's prop_vec reads
    the covariate: component 0 of the previous simulated observation, last_obs at the first horizon."""
    r = _worker(model, "parity", tmp_path)
    dx, dy = DIMS[model]
    for n, tile, H, R in cases.PARITY_SHAPES:
        key = f"{n}_{H}_{R}"
        tl = int(r["tile_" + key][0])
        assert tile == 0 or tl == tile
        y, x, start = r["y_" + key], r["xs_" + key], r["start_" + key]
        assert y.shape == ((R, H, n) if dy == 1 else (R, H, dy, n)) and x.shape == (R, H, dx, n) and start.shape == (R, n)
        th = cases.thetas(model, R)
        lo = cases.last_obs(R)
        for f in range(R):
            st = dict(x=r[f"x{f}_" + key], cdf=r[f"cdf{f}_" + key], A=r[f"A{f}_" + key], mb=r[f"mb{f}_" + key], rshift=int(r[f"rshift{f}_" + key][0]))
            rep = (cases.FIRST_ID if R > 1 else 0) + f
            s_ref, x_ref, y_ref = fur.forecast_user(oracle, model, th[f], st, n, tl, cases.SEED, rep, cases.T_STEPS, H, last_obs=lo[f])
            assert np.isfinite(y_ref).all()
            assert np.array_equal(start[f], s_ref), (key, f)
            assert _same_bits(x[f], x_ref), (key, f)
            assert _same_bits(y[f].reshape(H, dy, n), y_ref), (key, f)
        if n == 3 * 2048 + 7:
            assert tl == 512 and all(np.unique(start[f] // tl).size > 1 for f in range(R)), "the draw must cross tiles"


def _z_corr(a, b):
    return float(np.corrcoef(a, b)[0, 1] * np.sqrt(a.size))


def test_linear_gaussian_4d_moments(sa, tmp_path):
    """(4, 4), N = 65536, H = 3, libm only.  Per component d and horizon k: Var(y_d) - Var(x_d) = tau_d^2 (standard error as
    forecast_ref.moment_anchors: sqrt((2 tau^4 + 4 tau^2 s_x^2) / n)); x_d(k) - phi x_d(k-1) has variance sigma^2; sqrt(n) corr of the
    observation noises y_d - x_d of every pair d != d'; sqrt(n) corr of the state innovation and the observation noise of one
    component.  The last two fail if two components share a normal or zs and zo alias."""
    r = _worker("lin_gauss_4d_g", "anchors", tmp_path)
    phi, sigma = cases.BASE_THETA["lin_gauss_4d_g"][:2]
    tau = cases.BASE_THETA["lin_gauss_4d_g"][2:]
    n, H = cases.ANCHOR_N, cases.ANCHOR_H
    x, y, start = r["xs_a"][0], r["y_a"][0], r["start_a"][0]
    assert x.shape == (H, 4, n) and y.shape == (H, 4, n)
    prev = r["x"][:, start]
    zs = []
    for k in range(H):
        for d in range(4):
            sx2 = np.var(x[k, d], ddof=1)
            se = np.sqrt((2.0 * tau[d] ** 4 + 4.0 * tau[d] ** 2 * sx2) / n)
            zs.append((f"var(y)-var(x) k={k} d={d}", float((np.var(y[k, d], ddof=1) - sx2 - tau[d] ** 2) / se)))
            innov = x[k, d] - phi * prev[d]
            zs.append((f"var(x'-phi x) k={k} d={d}", float((np.var(innov, ddof=1) - sigma ** 2) / (sigma ** 2 * np.sqrt(2.0 / (n - 1))))))
            zs.append((f"corr(innov, noise) k={k} d={d}", _z_corr(innov, y[k, d] - x[k, d])))
            for e in range(d + 1, 4):
                zs.append((f"corr(noise {d}, noise {e}) k={k}", _z_corr(y[k, d] - x[k, d], y[k, e] - x[k, e])))
                zs.append((f"corr(innov {d}, innov {e}) k={k}", _z_corr(innov, x[k, e] - phi * prev[e])))
        prev = x[k]
    for name, z in zs:
        print(f"{name}: z = {z:+.3f}")
    assert len(zs) == H * (4 * 3 + 6 * 2)
    worst = max(zs, key=lambda t: abs(t[1]))
    assert abs(worst[1]) <= 5.0, worst


def test_forecasts_are_reproducible_and_change_nothing(sa, tmp_path):
    """Two forecasts from one origin: the same bits.  Filter r of a bank and a one-filter handle with first_filter_id = r and
    n_filters_total = R: the same bits.  A 12-step series with a forecast after every step: the per-step log-likelihood bits and the
    final particles of one without."""
    r = _worker("svol_two_factor_g", "determinism", tmp_path)
    assert np.isfinite(r["y_a"]).all() and r["y_a"].shape == (3, 3, 2, 2049)
    for k in ("y", "x"):
        assert _same_bits(r[k + "_a"], r[k + "_b"])
    assert np.array_equal(r["s_a"], r["s_b"])
    for f in range(3):
        assert np.array_equal(r["s_a"][f], r[f"s_one{f}"][0]), f
        assert _same_bits(r["x_a"][f], r[f"x_one{f}"][0]) and _same_bits(r["y_a"][f], r[f"y_one{f}"][0]), f
    assert r["lls_with"].shape == (12, 3) and np.isfinite(r["lls_with"]).all()
    assert _same_bits(r["lls_with"], r["lls_without"]) and _same_bits(r["final_with"], r["final_without"])


def test_contract(sa, tmp_path):
    """SSME_ERR_STATE before the first step; num_steps 0 and 65536: SSME_ERR_INVALID_ARG; a `bad` parameter row: NaN y for that filter
    only, status OK; Python shapes [R, H, dim_y, N] / [R, H, dim_x, N]; an SSME_F32 scalar user handle returns floats."""
    from ssme_amd import _capi
    r = _worker("svol_two_factor_g", "contract", tmp_path)
    assert r["before_step"].tolist() == [_capi.ERR_STATE]
    assert r["num_steps"].tolist() == [_capi.ERR_INVALID_ARG, _capi.ERR_INVALID_ARG]
    assert r["bad_status"].tolist() == [_capi.OK]
    y, x, start = r["y_bad"], r["xs_bad"], r["start_bad"]
    assert y.shape == (3, 2, 2, 300) and x.shape == (3, 2, 2, 300) and start.shape == (3, 300)
    assert np.isnan(y[1]).all() and np.isnan(x[1]).all()
    assert np.isfinite(y[[0, 2]]).all() and np.isfinite(x[[0, 2]]).all()
    r = _worker("svol_leverage_user", "f32", tmp_path)
    for k in ("y", "xs"):
        v32, v64 = r[k + "_f32"], r[k + "_f64"]
        assert v32.shape == (2, 3, 700) and np.isfinite(v32).all()
        assert np.array_equal(v32, v32.astype(np.float32).astype(np.float64))            # every value is a float
        assert not np.array_equal(v64, v64.astype(np.float32).astype(np.float64))         # the fp64 handle's are not


def test_cpp_adaptor_returns_the_banks_bits(sa, spy, tmp_path):
    """tests/cpp/test_user_forecast.cpp (user_bs_gpu<3001, 2, 2>::sim_future_obs) against ParticleFilterBank.sim_future_obs of the same
    seed and filter id: six values and the 64-bit sum of all bit patterns."""
    from test_forecast_user_cpu import build_adaptor_program
    exe = build_adaptor_program()
    res = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "spy_returns.csv")], stdout=subprocess.PIPE, text=True, check=True, timeout=120)
    got = dict(line.split() for line in res.stdout.strip().splitlines())
    y = _worker("svol_two_factor_g", "adaptor", tmp_path)["y"]
    assert y.shape == (1, 3, 2, 3001) and np.isfinite(y).all()
    flat = y.ravel()
    assert got["has_gsamp"] == "1" and int(got["size"]) == flat.size and got["repeat"] == "same"
    assert int(got["bitsum"]) == int(np.sum(_bits(flat), dtype=np.uint64))
    probes = [k for k in got if k.startswith("y_")]
    assert len(probes) == 6
    for k in probes:
        assert float(got[k]) == flat[int(k[2:])], k
