"""us per step of the two run_series routes of a VECTOR user model at N <= 2048: the whole-series kernels (pf_small.h) against the
tiled step kernel (set_small_series(False): the code path such a model had before it got a whole-series form), ON THE SAME HANDLE,
the two routes alternating.  Run once per library:
    SSME_PF_LIB=build/user/libssme_pf_two_factor.so python tools/vector_series_timing.py [passes]
Libraries: two_factor (2, 2), lin_gauss_3d (3, 1), lin_gauss_4d_h (4, 4), svol_two_factor_cov (2, 2, dim_cov = 4).
Shapes: N in {100, 500, 1000, 2000}, R in {1, 100} replicate filters, T = 3084 rows of spy_returns.csv (component d: the series rolled
by 100 d rows), multinomial resampling every step.  Timing source: last_elapsed_ms (HIP events around the launches of one series).
Reported: the median of the passes of each route after two warm-up passes of each, and the spread (max - min) of the baseline's
own passes; "gain" is baseline - series, to be read against twice that spread (the rule of the default)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssme_amd as sa  # noqa: E402
from ssme_amd import _capi  # noqa: E402

THETA = {(2, 2): [1.1, 0.95, 0.9, 0.2, 0.15, -0.4], (3, 1): [0.9, 0.5, 0.3, 0.2, 0.7], (4, 4): [0.9, 0.5, 0.7, 0.4, 1.1, 0.25]}
passes = int(sys.argv[1]) if len(sys.argv) > 1 else 21
spy = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
T = 3084
assert spy.size >= T
b0 = sa.ParticleFilterBank(sa.MODEL_USER0, 8, 1)
dx, dy = b0._dims()
K = sa.user_model_dim_cov()
b0.close()
y = np.stack([np.roll(spy[:T], -100 * d) for d in range(dy)], axis=1)
Z = np.random.default_rng(7).standard_normal((T, K)) if K else None
name = os.path.basename(os.environ.get("SSME_PF_LIB", "stock"))
print(f"# {name}: (dim_x, dim_y, dim_cov) = ({dx}, {dy}, {K}); T = {T}; {passes} passes per route after 2 warm-up passes; us per step")
print("#    N    R  route(threads)   series med   tiled med  tiled min..max (spread)    gain  2*spread  same bits")
for n in (100, 500, 1000, 2000):
    for R in (1, 100):
        b = sa.ParticleFilterBank(sa.MODEL_USER0, n, R, 20260101)
        b.set_params(THETA[(dx, dy)])
        ms = {True: [], False: []}
        ll = {}
        b.set_small_series(True)
        route = b.series_route()
        for i in range(passes + 2):
            for small in (False, True):                      # the two routes alternate
                b.set_small_series(small)
                ll[small] = b.run_series(y, Z)
                if i >= 2:
                    ms[small].append(b.last_elapsed_ms())
        us = {k: np.array(v) * 1e3 / T for k, v in ms.items()}
        med_s, med_t = float(np.median(us[True])), float(np.median(us[False]))
        spread = float(us[False].max() - us[False].min())
        same = bool((ll[True].view(np.uint64) == ll[False].view(np.uint64)).all())
        print(f"  {n:5d} {R:4d}  {('lane', 'pair')[route[0] - 1] if route[0] else 'tiled':>5s}({route[1]:4d})  {med_s:10.3f}  {med_t:10.3f}  "
              f"{us[False].min():7.3f}..{us[False].max():7.3f} ({spread:6.3f})  {med_t - med_s:6.3f}  {2 * spread:8.3f}  {same}", flush=True)
        b.close()
