"""Runs a library whose user model declares its observation draw (ssme_amd/csrc/model_api.h: gsamp / gsamp_vec) in a process of its
own (SSME_PF_LIB: one of tests/models/svol_leverage_user.h, svol_two_factor_g.h, lin_gauss_3d_g.h, lin_gauss_4d_g.h) and writes what
tests/test_forecast_user_gpu.py compares.      python tests/forecast_user_model_worker.py MODE OUT.npz [MODEL]
MODEL names the header where the dimensions do not (svol_two_factor_lev_g.h is (2, 2), as svol_two_factor_g.h)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssme_amd  # noqa: E402
from ssme_amd import _capi  # noqa: E402
import fc_user_cases as cases  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
L = _capi.lib()
assert L.ssme_pf_user_model_has_gsamp() == 1 and ssme_amd.user_model_has_gsamp()
dx, dy = C.c_int32(), C.c_int32()
assert L.ssme_pf_user_model_dims(C.byref(dx), C.byref(dy)) == _capi.OK
name = {(1, 1): "svol_leverage_user", (2, 2): "svol_two_factor_g", (3, 1): "lin_gauss_3d_g", (4, 4): "lin_gauss_4d_g"}[(dx.value, dy.value)]
if len(sys.argv) > 3:
    assert cases.DIM_Y[sys.argv[3]] == dy.value
    name = sys.argv[3]
spy = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
res = {}


def status_of(fn):
    try:
        fn()
    except _capi.SsmeError as e:
        return e.status
    return _capi.OK


def obs(t):
    return cases.observation(spy, name, t)


def make_bank(n, tile, R, model=_capi.MODEL_USER0, thetas=None, **kw):
    first = cases.FIRST_ID if R > 1 else 0
    bank = ssme_amd.ParticleFilterBank(model, n, R, cases.SEED, tile=tile, first_filter_id=kw.pop("first", first), **kw)
    bank.set_params(cases.thetas(name, R) if thetas is None else thetas)
    return bank


def filter_steps(bank, T=cases.T_STEPS):
    """T steps; the covariate of step t is the previous observation's component 0 (0 at t = 0).  Returns the log conditional likelihoods."""
    lls = []
    for t in range(T):
        lls.append(bank.step(obs(t), 0.0 if t == 0 else float(np.ravel(obs(t - 1))[0])))
    return np.stack(lls)


def save_state(bank, key, R):
    for r in range(R):
        st = bank.state(r, logw=False)
        for k in ("x", "cdf", "A", "mb"):
            res[f"{k}{r}_{key}"] = st[k]
        res[f"rshift{r}_{key}"] = np.array([st["rshift"]])
    res["tile_" + key] = np.array([bank.tile])


def save_forecast(bank, key, H, last_obs):
    y, x, start = bank.sim_future_obs(H, last_obs, states=True, start=True)
    res["y_" + key], res["xs_" + key], res["start_" + key] = y, x, start


if mode == "twin":
    assert name == "svol_leverage_user"
    for n, tile, H, R in cases.TWIN_SHAPES:
        for tag, model in (("u", _capi.MODEL_USER0), ("b", _capi.MODEL_SVOL_LEVERAGE)):
            key = f"{tag}_{n}_{H}_{R}"
            bank = make_bank(n, tile, R, model)
            res["ll_" + key] = filter_steps(bank)
            save_state(bank, key, R)
            save_forecast(bank, key, H, cases.last_obs(R))
            bank.close()
elif mode == "parity":
    for n, tile, H, R in cases.PARITY_SHAPES:
        key = f"{n}_{H}_{R}"
        bank = make_bank(n, tile, R)
        filter_steps(bank)
        save_state(bank, key, R)
        save_forecast(bank, key, H, cases.last_obs(R))
        bank.close()
elif mode == "anchors":
    assert name == "lin_gauss_4d_g"
    bank = make_bank(cases.ANCHOR_N, 0, 1)
    filter_steps(bank)
    res["x"] = bank.state(0, logw=False)["x"]
    save_forecast(bank, "a", cases.ANCHOR_H, None)
    bank.close()
elif mode == "determinism":
    n, H, R = 2049, 3, 3
    bank = make_bank(n, 0, R)
    filter_steps(bank)
    res["y_a"], res["x_a"], res["s_a"] = bank.sim_future_obs(H, cases.last_obs(R), states=True, start=True)
    res["y_b"], res["x_b"], res["s_b"] = bank.sim_future_obs(H, cases.last_obs(R), states=True, start=True)
    bank.close()
    for r in range(R):
        one = make_bank(n, 0, 1, thetas=cases.thetas(name, R)[r], first=cases.FIRST_ID + r, n_filters_total=R)
        filter_steps(one)
        res[f"y_one{r}"], res[f"x_one{r}"], res[f"s_one{r}"] = one.sim_future_obs(H, float(cases.last_obs(R)[r]), states=True, start=True)
        one.close()
    # a 12-step series with a forecast after every step against one without
    for tag, fc in (("with", True), ("without", False)):
        bank = make_bank(n, 0, R)
        lls = []
        for t in range(12):
            lls.append(bank.step(obs(t), 0.0 if t == 0 else float(np.ravel(obs(t - 1))[0])))
            if fc:
                bank.sim_future_obs(2, float(np.ravel(obs(t))[0]), states=(t % 2 == 0))
        res["lls_" + tag] = np.stack(lls)
        res["final_" + tag] = np.stack([bank.state(r, logw=False)["x"] for r in range(R)])
        bank.close()
elif mode == "contract":
    n, R = 300, 3
    th = cases.thetas(name, R)
    bank = make_bank(n, 0, R, thetas=th)
    res["before_step"] = np.array([status_of(lambda: bank.sim_future_obs(2))])
    filter_steps(bank, 2)
    y = np.empty((R, 1, dy.value, n))
    res["num_steps"] = np.array([L.ssme_pf_sim_future_obs(bank._h, hh, None, _capi.dptr(y), None, None) for hh in (0, 65536)])
    bank.close()
    # a `bad` parameter row (filter 1): NaN samples for that filter only
    thb = th.copy()
    thb[1] = cases.bad_theta(name)
    bank = make_bank(n, 0, R, thetas=thb)
    filter_steps(bank, 2)
    res["bad_status"] = np.array([status_of(lambda: save_forecast(bank, "bad", 2, 0.1))])
    bank.close()
elif mode == "f32":
    assert name == "svol_leverage_user"
    for tag, dtype in (("f32", _capi.F32), ("f64", _capi.F64)):
        bank = make_bank(700, 0, 2, dtype=dtype)
        filter_steps(bank)
        save_forecast(bank, tag, 3, 0.3)
        bank.close()
elif mode == "adaptor":
    # the bank's forecast for the seed, filter id, parameters and series of tests/cpp/test_user_forecast.cpp
    assert name == "svol_two_factor_g"
    bank = ssme_amd.ParticleFilterBank(_capi.MODEL_USER0, 3001, 1, 21, first_filter_id=1)
    bank.set_params([1.1, 0.95, 0.9, 0.2, 0.15, -0.4])
    for t in range(4):
        bank.step(np.array([spy[t], spy[100 + t]]))
    res["y"] = bank.sim_future_obs(3, 0.25)
    bank.close()
else:
    raise SystemExit("unknown mode " + mode)
np.savez(out, **res)
