"""Runs a library whose user model declares covariates (ssme_amd/csrc/model_api.h: dim_cov; SSME_PF_LIB = a build of one of the
headers of tests/user_cov_ref.py, or of tests/models/svol_leverage_user.h for the "leverage_plain" mode) in a process of its own -- a
process binds ONE libssme_pf.so -- and writes what tests/test_user_cov_gpu.py compares.
    python tests/user_cov_worker.py NAME OUT.npz"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssme_amd  # noqa: E402
from ssme_amd import _capi  # noqa: E402
import user_cov_ref as ucr  # noqa: E402

name, out = sys.argv[1], sys.argv[2]
L = _capi.lib()
spy = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
T = ucr.T_STEPS
res = {}


def status_of(fn):
    try:
        fn()
    except _capi.SsmeError as e:
        return e.status
    return _capi.OK


def put(key, st):
    for k in ("x", "logw", "cdf", "anc", "A", "mb"):
        if st.get(k) is not None:
            res[f"{key}_{k}"] = st[k]
    res[f"{key}_m"] = np.array([st["m"]])
    res[f"{key}_rshift"] = np.array([st["rshift"]])


def make(n, tile, sched=1, rs=0, R=2, th=None, **kw):
    bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, n, R, ucr.SEED, rs, sched, tile=tile, **kw)
    bank.set_debug(True, True)
    bank.set_params(th)
    return bank


if name == "leverage_plain":
    # tests/models/svol_leverage_user.h: the scalar-covariate grammar, for the bits svol_leverage_cov1.h must reproduce
    assert L.ssme_pf_user_model_dim_cov() == 0 and L.ssme_pf_user_model_has_first() == 0
    y, Z = ucr.observations(spy, 1), ucr.covariates(1)
    for n, tile in ucr.SHAPES:
        bank = make(n, tile, th=ucr.TH_LEV)
        res[f"{n}_{tile}_lls"] = np.array([bank.step(y[t], Z[t, 0])[1] for t in range(T)])
        put(f"{n}_{tile}_step", bank.state(1, ancestors=True))
        res[f"{n}_{tile}_series"] = bank.run_series(y, Z[:, 0])
        res[f"{n}_{tile}_per"] = bank.per_step()
        put(f"{n}_{tile}_ser", bank.state(1, ancestors=True))
        if n == 500:
            # a user model without dim_cov has no covariate forecast
            yb = np.empty((2, 2, n))
            res["fc_cov_status"] = np.array([L.ssme_pf_sim_future_obs_cov(bank._h, 2, _capi.dptr(np.zeros(2)), _capi.dptr(yb), None, None)])
        bank.close()
    np.savez(out, **res)
    raise SystemExit(0)

if name == "svol_reg_cov_nodraw":
    # a dim_cov header without the observation draw: it filters, and its covariate forecast is unsupported
    assert L.ssme_pf_user_model_dim_cov() == 3 and L.ssme_pf_user_model_has_gsamp() == 0
    y, Z = ucr.observations(spy, 1), ucr.covariates(3)
    bank = make(500, 0, th=ucr.TH_REG)
    res["lls"] = np.array([bank.step(y[t], Z[t])[1] for t in range(T)])
    yb = np.empty((2, 2, 500))
    res["fc_cov_status"] = np.array([L.ssme_pf_sim_future_obs_cov(bank._h, 2, _capi.dptr(np.zeros((2, 3))), _capi.dptr(yb), None, None)])
    bank.close()
    np.savez(out, **res)
    raise SystemExit(0)

m = ucr.MODELS[name]
K, dx, dy, TH = m["K"], m["dx"], m["dy"], m["theta"]
assert L.ssme_pf_user_model_dim_cov() == K and ssme_amd.filters.user_model_dim_cov() == K
y, Z = ucr.observations(spy, dy), ucr.covariates(K)

# ---- parity: the step API (covariates by value) and run_series (covariates from the table), every shape / schedule / resampler ----
for n, tile in ucr.SHAPES:
    for sched in (1, 2):
        for rs in (0, 1):
            key = f"{n}_{tile}_{sched}_{rs}"
            bank = make(n, tile, sched, rs, th=TH)
            res[key + "_lls"] = np.array([bank.step(y[t], Z[t])[1] for t in range(T)])
            put(key + "_step", bank.state(1, ancestors=True))
            if m["n_h"] and sched == 1 and rs == 0:
                res[key + "_ue_step"] = bank.user_expectations()
            for small in ((True, False) if n <= 2048 and dx == 1 and dy == 1 else (False,)):
                bank.set_small_series(small)
                tag = key + ("_small" if small else "_ser")
                res[tag + "_ll"] = bank.run_series(y, Z)
                res[tag + "_per"] = bank.per_step()
                put(tag, bank.state(1, ancestors=True))
            if m["n_h"] and sched == 1 and rs == 0:
                res[key + "_ue_series"] = bank.user_expectations()
            if sched == 1 and rs == 0:
                # z = NULL against z = zeros: by value and from the table
                bank.set_small_series(False)
                for zk, zs, zrow in (("null", None, None), ("zeros", np.zeros((T, K)), np.zeros(K))):
                    res[f"{key}_{zk}_ser_ll"] = bank.run_series(y, zs)
                    put(f"{key}_{zk}_ser", bank.state(1, ancestors=True))
                    if m["n_h"] and zk == "null":
                        res[key + "_ue_series_null"] = bank.user_expectations()
                    bank.reset()
                    res[f"{key}_{zk}_lls"] = np.array([bank.step(y[t], zrow)[1] for t in range(T)])
                    put(f"{key}_{zk}_step", bank.state(1, ancestors=True))
            bank.close()

# ---- forecast with exogenous covariates ------------------------------------------------------------------------------------------------
if m["gsamp"] is not None and name in ("svol_reg_cov", "svol_two_factor_cov", "svol_leverage_cov1"):
    H = 3
    Zf = np.random.default_rng(11).standard_normal((H, 4))[:, :K].copy()
    res["Zf"] = Zf
    for n, tile in ((500, 2048), (2500, 512)):
        key = f"fc_{n}"
        bank = make(n, tile, th=TH)
        for t in range(4):
            bank.step(y[t], Z[t])
        put(key + "_state", bank.state(1, ancestors=True))
        ys, xs, st = bank.sim_future_obs(H, states=True, start=True, z_future=Zf)
        ys2, xs2, st2 = bank.sim_future_obs(H, states=True, start=True, z_future=Zf)
        res[key + "_y"], res[key + "_x"], res[key + "_start"] = ys, xs, st
        res[key + "_y2"], res[key + "_x2"], res[key + "_start2"] = ys2, xs2, st2
        res[key + "_next_after"] = bank.step(y[4], Z[4])
        put(key + "_next_after_state", bank.state(1))
        bank.close()
        bank = make(n, tile, th=TH)
        for t in range(4):
            bank.step(y[t], Z[t])
        res[key + "_next_plain"] = bank.step(y[4], Z[4])
        put(key + "_next_plain_state", bank.state(1))
        bank.close()

# ---- contract ---------------------------------------------------------------------------------------------------------------------------
if name == "svol_reg_cov":
    Zf = np.zeros((3, K))
    bank = make(500, 0, th=TH)
    yb = np.empty((2, 3, 500))
    res["fc_before_step"] = np.array([L.ssme_pf_sim_future_obs_cov(bank._h, 3, _capi.dptr(Zf), _capi.dptr(yb), None, None)])
    bank.step(y[0], Z[0])
    res["fc_null_z"] = np.array([L.ssme_pf_sim_future_obs_cov(bank._h, 3, None, _capi.dptr(yb), None, None)])
    res["fc_num_steps"] = np.array([L.ssme_pf_sim_future_obs_cov(bank._h, hh, _capi.dptr(Zf), _capi.dptr(yb), None, None) for hh in (0, 65536)])
    res["fc_plain_on_cov"] = np.array([L.ssme_pf_sim_future_obs(bank._h, 3, None, _capi.dptr(yb), None, None)])
    bank.close()
    # a built-in model of the same library has no dim_cov
    sv = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_SVOL, 500, 2, 4)
    sv.set_params([1.0, 0.95, 0.25])
    sv.step(spy[0])
    res["fc_builtin"] = np.array([L.ssme_pf_sim_future_obs_cov(sv._h, 3, _capi.dptr(Zf), _capi.dptr(yb), None, None)])
    sv.close()
    # sharded handles
    cfg = _capi.Config(model=_capi.MODEL_USER0, n_particles=4 * 2048, n_filters=1, dtype=0, resampler=0, resamp_sched=1, seed=1, device=0)
    hs = C.c_void_p()
    res["shard_create"] = np.array([L.ssme_pf_shard_create(C.byref(cfg), 0, 2, C.byref(hs))])
    # a `bad` filter (sigma < 0 in row 0): NaN samples and SSME_OK; the healthy row is untouched
    thb = TH.copy()
    thb[0, 2] = -0.25
    bank = make(500, 0, th=thb)
    for t in range(3):
        bank.step(y[t], Z[t])
    res["fc_bad_status"] = np.array([status_of(lambda: res.__setitem__("fc_bad_y", bank.sim_future_obs(3, z_future=np.ones((3, K)))))])
    bank.close()
    # float at the boundary: an SSME_F32 handle against the double handle run on float-rounded y, z and theta
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
    for tag, dt, yy, zz, th in (("f32", _capi.F32, y, Z, TH), ("f64r", _capi.F64, f32(y), f32(Z), f32(TH))):
        bank = make(2500, 512, th=th, dtype=dt)
        res[tag + "_lls"] = np.array([bank.step(yy[t], zz[t]) for t in range(T)])
        res[tag + "_ue"] = bank.user_expectations()
        res[tag + "_series"] = bank.run_series(yy, zz)
        res[tag + "_fc"] = bank.sim_future_obs(2, z_future=(Z[:2] if dt == _capi.F32 else f32(Z[:2])))
        bank.close()

np.savez(out, **res)
