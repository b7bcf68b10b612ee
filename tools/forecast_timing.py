"""Times the forecast (ssme_pf_sim_future_obs / ssme_lw_sim_future_obs, csrc/forecast.h) against the filter's own step at the same shape:
    bootstrap SVOL       1 filter    x 2^20 particles, H = 16
    SVOL with leverage   512 filters x 2^14 particles, H = 16
    Liu-West (form 0)    1 filter    x 2^20 particles, H = 16
Per configuration: the HIP-event time of the horizon kernel alone and of the whole call without the download (events recorded by the
library on the handle's stream: ssme_*_forecast_elapsed_ms), medians of REPS calls after WARM warm-up calls; and the filter's own
time per step from the unchanged step kernels, ssme_*_last_elapsed_ms / T of a T-step run_series (median of FILTER_REPS series).
The condition (no margin): horizon-kernel time per horizon step <= filter time per step.  A forecast step is a subset of a filter
step's work -- no search, no scan, no cdf; 8 bytes written per particle and nothing read.
    python tools/forecast_timing.py [> profiles/forecast_timing.txt]
User models that declare their observation draw (csrc/model_api.h: gsamp_vec; k_fc_horizon_user), the same measurement and condition:
    svol_two_factor_g (2, 2)   1 filter x 2^20 particles, H = 16
    lin_gauss_4d_g    (4, 4)   1 filter x 2^20 particles, H = 16
each in a process of its own (a process binds one library: SSME_PF_LIB), one after the other; the built-in legs are not run.
    python tools/forecast_timing.py --user [> profiles/forecast_user_timing.txt]"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssme_amd as sa  # noqa: E402

H, WARM, REPS, T, FILTER_REPS = 16, 3, 21, 64, 7
LEG_TIMEOUT_S = 180                # per child process of --user
spy = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
y = spy[:T]
z = np.concatenate([[0.0], y[:-1]])


def med(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def report(name, n, r, filt_ms, hor, call):
    per_h = med(hor) * 1e3 / H
    per_t = med(filt_ms) * 1e3 / T
    ok = per_h <= per_t
    print(f"{name}: R = {r}, N = {n}, H = {H}", flush=True)
    print(f"  horizon kernel      {med(hor) * 1e3:9.1f} us per call (min {min(hor) * 1e3:.1f}, max {max(hor) * 1e3:.1f}; {REPS} calls) = {per_h:.2f} us per horizon step", flush=True)
    print(f"  whole call, no copy {med(call) * 1e3:9.1f} us per call (level-2, start draw, horizon kernel; min {min(call) * 1e3:.1f}, max {max(call) * 1e3:.1f})", flush=True)
    print(f"  filter step         {per_t:9.2f} us per step (run_series of T = {T}, median of {FILTER_REPS}; min {min(filt_ms) * 1e3 / T:.2f}, max {max(filt_ms) * 1e3 / T:.2f})", flush=True)
    print(f"  horizon step / filter step = {per_h / per_t:.3f}   condition (<= 1): {'met' if ok else 'NOT MET'}", flush=True)
    return ok


def bootstrap(name, model, theta, n, r, cov, series=y):
    bank = sa.ParticleFilterBank(model, n, r, seed=20260101)
    bank.set_params(theta)
    filt = []
    for _ in range(FILTER_REPS + 1):
        bank.run_series(series, z if cov else None)
        filt.append(bank.last_elapsed_ms())
    hor, call = [], []
    for i in range(WARM + REPS):
        bank.sim_future_obs(H, y[-1])
        if i >= WARM:
            a, b = bank.forecast_elapsed_ms()
            hor.append(a)
            call.append(b)
    bank.close()
    return report(name, n, r, filt[1:], hor, call)


def liu_west(n):
    g = sa.svol_lw_1_par(0.99, 0.8, 0.99, -0.1, 0.1, 0.01, 0.1, -0.5, -0.01, nparts=n, seed=20260101)
    filt = []
    for _ in range(FILTER_REPS + 1):
        g.run_series(y, z)
        filt.append(g.last_elapsed_ms())
    hor, call = [], []
    for i in range(WARM + REPS):
        g.sim_future_obs(H, y[-1])
        if i >= WARM:
            a, b = g.forecast_elapsed_ms()
            hor.append(a)
            call.append(b)
    g.close()
    return report("Liu-West, auxiliary form", n, 1, filt[1:], hor, call)


# header, library name, theta, dim_y of the user-model legs
USER_LEGS = {"svol_two_factor_g": ("two_factor_g", [1.1, 0.95, 0.9, 0.2, 0.15, -0.4], 2),
             "lin_gauss_4d_g": ("lin_gauss_4d_g", [0.9, 0.5, 0.7, 0.4, 1.1, 0.25], 4)}
if "--user-leg" in sys.argv:                       # the child: SSME_PF_LIB names this model's library
    model = sys.argv[sys.argv.index("--user-leg") + 1]
    _, theta, dy = USER_LEGS[model]
    series = np.column_stack([spy[100 * j:100 * j + T] for j in range(dy)])
    try:
        assert sa.user_model_has_gsamp()
        met = bootstrap("user model " + model, sa.MODEL_USER0, theta, 1 << 20, 1, False, series)
    except Exception:                              # a HIP error among them: not "condition not met" (1); the parent stops at it
        import traceback
        traceback.print_exc()
        sys.exit(4)
    sys.exit(0 if met else 1)
if "--user" in sys.argv:
    from ssme_amd import build
    ok = True
    for model, (lib, _, _) in USER_LEGS.items():
        so = build.build_user_model(os.path.join(ROOT, "tests", "models", model + ".h"), lib)
        # one child per leg, each under a time limit of its own (a leg takes about 15 s).  0: condition met, 1: not met; anything else
        # (a signal, an abort, a HIP error) or a leg that does not end is fatal: nothing more is started on the device
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--user-leg", model], env=dict(os.environ, SSME_PF_LIB=so),
                                timeout=LEG_TIMEOUT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"user model {model}: no result within {LEG_TIMEOUT_S} s; stopping", flush=True)
            sys.exit(3)
        if rc not in (0, 1):
            print(f"user model {model}: the leg ended with status {rc}; stopping", flush=True)
            sys.exit(3)
        ok = rc == 0 and ok
    print("all conditions met" if ok else "CONDITION NOT MET", flush=True)
    sys.exit(0 if ok else 1)
ok = bootstrap("bootstrap SVOL", sa.MODEL_SVOL, [1.0, 0.95, 0.25], 1 << 20, 1, False)
rng = np.random.default_rng(1)
th = np.column_stack([rng.uniform(0.8, 0.99, 512), rng.uniform(-0.1, 0.1, 512), rng.uniform(0.05, 0.3, 512), rng.uniform(-0.5, -0.01, 512)])
ok = bootstrap("SVOL with leverage", sa.MODEL_SVOL_LEVERAGE, th, 1 << 14, 512, True) and ok
ok = liu_west(1 << 20) and ok
print("all conditions met" if ok else "CONDITION NOT MET", flush=True)
sys.exit(0 if ok else 1)
