"""Times the forecast (ssme_pf_sim_future_obs / ssme_lw_sim_future_obs, csrc/forecast.h) against the filter's own step at the same shape:
    bootstrap SVOL       1 filter    x 2^20 particles, H = 16
    SVOL with leverage   512 filters x 2^14 particles, H = 16
    Liu-West (form 0)    1 filter    x 2^20 particles, H = 16
Per configuration: the HIP-event time of the horizon kernel alone and of the whole call without the download (events recorded by the
library on the handle's stream: ssme_*_forecast_elapsed_ms), medians of REPS calls after WARM warm-up calls; and the filter's own
time per step from the unchanged step kernels, ssme_*_last_elapsed_ms / T of a T-step run_series (median of FILTER_REPS series).
The condition (no margin): horizon-kernel time per horizon step <= filter time per step.  A forecast step is a subset of a filter
step's work -- no search, no scan, no cdf; 8 bytes written per particle and nothing read.
    python tools/forecast_timing.py [> profiles/forecast_timing.txt]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssme_amd as sa  # noqa: E402

H, WARM, REPS, T, FILTER_REPS = 16, 3, 21, 64, 7
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


def bootstrap(name, model, theta, n, r, cov):
    bank = sa.ParticleFilterBank(model, n, r, seed=20260101)
    bank.set_params(theta)
    filt = []
    for _ in range(FILTER_REPS + 1):
        bank.run_series(y, z if cov else None)
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


ok = bootstrap("bootstrap SVOL", sa.MODEL_SVOL, [1.0, 0.95, 0.25], 1 << 20, 1, False)
rng = np.random.default_rng(1)
th = np.column_stack([rng.uniform(0.8, 0.99, 512), rng.uniform(-0.1, 0.1, 512), rng.uniform(0.05, 0.3, 512), rng.uniform(-0.5, -0.01, 512)])
ok = bootstrap("SVOL with leverage", sa.MODEL_SVOL_LEVERAGE, th, 1 << 14, 512, True) and ok
ok = liu_west(1 << 20) and ok
print("all conditions met" if ok else "CONDITION NOT MET", flush=True)
sys.exit(0 if ok else 1)
