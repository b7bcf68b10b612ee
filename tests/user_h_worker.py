"""Runs a library whose user model declares functionals of its own (ssme_amd/csrc/model_api.h: n_h, h) in a process of its own
(SSME_PF_LIB: tests/models/svol_student_t_h.h or tests/models/svol_two_factor_h.h) and writes what tests/test_user_functionals_gpu.py
compares.      python tests/user_h_worker.py MODE OUT.npz"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssme_amd  # noqa: E402
from ssme_amd import _capi  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
L = _capi.lib()
spy = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
TH_T = [1.1, 0.95, 0.25, 7.0]                          # svol_student_t: beta, phi, sigma, nu
TH_2F = [1.1, 0.95, 0.9, 0.2, 0.15, -0.4]              # svol_two_factor: beta, phi1, phi2, sigma1, sigma2, rho
res = {}


def status_of(fn):
    try:
        fn()
    except _capi.SsmeError as e:
        return e.status
    return _capi.OK


def y2(t):
    return np.array([spy[t], spy[100 + t]])


def two_factor_thetas(R):
    rng = np.random.default_rng(5)
    return np.stack([rng.uniform(.9, 1.2, R), rng.uniform(.9, .97, R), rng.uniform(.8, .95, R), rng.uniform(.15, .25, R),
                     rng.uniform(.1, .2, R), rng.uniform(-.5, -.2, R)], axis=1)


if mode == "scalar":
    assert L.ssme_pf_user_model_n_h() == 4
    for n in (700, 5000):
        for rs in (0, 1, 2, 3):
            for sched in (1, 3):
                bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, n, 3, 11, rs, sched)
                bank.set_params(TH_T)
                for t in range(5):
                    bank.step(spy[t])
                key = f"{n}_{rs}_{sched}"
                res["ue_" + key] = bank.user_expectations()
                res["em_" + key] = bank.expectations_multi([0, 1, 2, 3])
                bank.close()
elif mode == "vector":
    assert L.ssme_pf_user_model_n_h() == 7
    for n in (1000, 40000):
        for tile in (512, 1024, 2048):
            bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, n, 2, 21, 0, 1, tile=tile)
            bank.set_params(TH_2F)
            for t in range(4):
                bank.step(y2(t), 0.37 + t)
            key = f"{n}_{tile}"
            res["ue_" + key] = bank.user_expectations()
            res["ex0_" + key] = bank.expectations(_capi.H_X)
            for r in range(2):
                x, w = bank.weights(r)
                res[f"x{r}_" + key], res[f"w{r}_" + key] = x, w
            res["z_" + key] = np.array([0.37 + 3])
            # a series leaves the covariate of its last time index behind; without covariates that is 0
            T = 3
            ys = np.stack([y2(t) for t in range(T)])
            bank.run_series(ys, np.array([0.5, -1.25, 2.5]))
            res["ue_series_z_" + key] = bank.user_expectations()
            bank.run_series(ys)
            res["ue_series_noz_" + key] = bank.user_expectations()
            bank.close()
elif mode == "exact":
    # every case of expect_cases.USER_CASES: state and expectations for tests/test_expectations_gpu.py (no debug mode)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import expect_cases as ec
    assert L.ssme_pf_user_model_n_h() == 7
    for case in ec.USER_CASES:
        y, zs = ec.user_observations(case)
        bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, case["n"], 1, 21, 0, case["sched"], tile=case["tile"])
        bank.set_params(TH_2F)
        res["lls_" + case["name"]] = np.array([bank.step(y[t], zs[t])[0] for t in range(case["T"])])
        res["ue_" + case["name"]] = bank.user_expectations()
        g = bank.state(0, logw=False)
        for k in ("x", "cdf", "A", "mb"):
            res[k + "_" + case["name"]] = g[k]
        bank.close()
elif mode == "swarm_big":
    # more members than k_swarm_means has threads: R = 300 and 513, every num_threads the bootstrap test uses
    for R in (300, 513):
        bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, 600, R, 3)
        bank.set_params(two_factor_thetas(R))
        for t in range(3):
            lcl = bank.step(y2(t), 0.1 * (t + 1))
        res[f"lcl_{R}"], res[f"ue_{R}"] = lcl, bank.user_expectations()
        for nt in (0, 7, 256, 299, R, R + 5):
            ll, ex = bank.swarm_aggregate_user(nt)
            res[f"ll_{R}_{nt}"], res[f"ex_{R}_{nt}"] = np.array([ll]), ex
        bank.close()
elif mode == "determinism":
    n, R = 40000, 3
    th = two_factor_thetas(R)

    def run(nt, first=0, nf=R, total=0, rows=None):
        bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, n, nf, 21, 1, 1, tile=2048, first_filter_id=first, n_filters_total=total)
        bank.set_tuning(nt)
        bank.set_params(th if rows is None else th[rows])
        for t in range(3):
            bank.step(y2(t), 0.25 * t)
        a, b = bank.user_expectations(), bank.user_expectations()
        bank.close()
        return a, b
    for nt in (256, 512, 1024):
        res[f"a_{nt}"], res[f"b_{nt}"] = run(nt)
    for r in range(R):
        res[f"single_{r}"] = run(512, first=r, nf=1, total=R, rows=[r])[0]
elif mode == "swarm":
    R = 7
    bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, 700, R, 3)
    bank.set_params(two_factor_thetas(R))
    for t in range(4):
        lcl = bank.step(y2(t), 0.1 * (t + 1))
    res["lcl"] = lcl
    res["ue"] = bank.user_expectations()
    for nt in (0, 3, 7):
        ll, ex = bank.swarm_aggregate_user(nt)
        res[f"ll_{nt}"], res[f"ex_{nt}"] = np.array([ll]), ex
    bank.close()
elif mode == "contract":
    assert L.ssme_pf_user_model_n_h() == 4
    bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, 3000, 2, 4)
    bank.set_params(TH_T)
    res["before_step"] = np.array([status_of(bank.user_expectations), status_of(bank.swarm_aggregate_user)])
    bank.close()
    # a sharded handle of the same model (rank 0 of 2; it is never stepped here)
    cfg = _capi.Config(model=_capi.MODEL_USER0, n_particles=4 * 2048, n_filters=1, dtype=0, resampler=0, resamp_sched=1, seed=1, device=0)
    hs = C.c_void_p()
    assert L.ssme_pf_shard_create(C.byref(cfg), 0, 2, C.byref(hs)) == _capi.OK
    buf, one = np.zeros(4), np.zeros(1)
    res["sharded"] = np.array([L.ssme_pf_get_user_expectations(hs, _capi.dptr(buf)), L.ssme_pf_swarm_aggregate_user(hs, 0, _capi.dptr(one), _capi.dptr(buf))])
    L.ssme_pf_destroy(hs)
    # a built-in model of the same library
    sv = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_SVOL, 3000, 2, 4)
    sv.set_params([1.0, 0.95, 0.25])
    sv.step(spy[0])
    res["builtin_model"] = np.array([status_of(sv.user_expectations), status_of(sv.swarm_aggregate_user)])
    sv.close()
    # degenerate parameters (beta < 0; phi > 1): the log conditional likelihood is NaN, and so is every expectation
    for i, th in enumerate(([-1.0, 0.5, 0.1, 7.0], [1.0, 1.5, 0.1, 7.0])):
        bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, 300, 1, 1)
        bank.set_params(th)
        res[f"nan_ll_{i}"] = bank.step(0.3)
        res[f"nan_ue_{i}"] = bank.user_expectations()
        bank.close()
    # float at the boundary
    b32 = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, 5000, 2, 4, dtype=_capi.F32)
    b32.set_params(TH_T)
    for t in range(3):
        b32.step(spy[t])
    res["f32_ue"] = b32.user_expectations()
    res["f32_agg"] = b32.swarm_aggregate_user()[1]
    b32.close()
    # a queued step (logcondlike_out = NULL) against the synchronous order
    for name, queued in (("sync", False), ("queued", True)):
        bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, 5000, 2, 4)
        bank.set_params(TH_T)
        for t in range(3):
            if queued:
                yv = np.array([spy[t]])
                assert L.ssme_pf_step(bank._h, _capi.dptr(yv), None, None) == _capi.OK
            else:
                bank.step(spy[t])
        res["ue_" + name] = bank.user_expectations()
        bank.close()
        bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, 5000, 2, 4)
        bank.set_params(TH_T)
        for t in range(3):
            if queued:
                yv = np.array([spy[t]])
                assert L.ssme_pf_step(bank._h, _capi.dptr(yv), None, None) == _capi.OK
            else:
                bank.step(spy[t])
        ll, ex = bank.swarm_aggregate_user()
        res["agg_" + name] = np.concatenate([[ll], ex])
        bank.close()
else:
    raise SystemExit("unknown mode " + mode)
np.savez(out, **res)
