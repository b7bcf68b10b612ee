"""us per step of the two routes of ssme_lw_run_series for Liu-West filters of one tile (N <= 2048): the whole-series kernel
(csrc/lw_small.h, set_small_series(True)) against the tiled stage launches (set_small_series(False): k_lw_stage1 + k_lw_stage2 per
step, the only route before the series kernel existed and untouched by it), ON THE SAME HANDLE, the two routes alternating.
    python tools/lw_series_timing.py [passes] > profiles/lw_series_timing.txt
Shapes: both forms (svol_lw_1_par auxiliary, svol_lw_2_par SISR), N in {10, 100, 500, 1000, 2048} at R = 1 and N = 500 at R = 100,
T = 3084 rows of spy_returns.csv with z its lag, resampling every step.  Timing source: last_elapsed_ms (HIP events around the
launches of one series: Gamma tables, k_lw_init and the steps, on both routes).  Reported: the median of the passes of each route
after two warm-up passes of each, and the spread (max - min) of the tiled route's own passes; "gain" is tiled - series.
The rule of the default (the one series_route records for the bootstrap kernels): the series route is the default of a new handle
only if the gain exceeds twice that spread at EVERY measured shape, for both forms; the last line says which way it went."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssme_amd as sa  # noqa: E402

passes = int(sys.argv[1]) if len(sys.argv) > 1 else 21
spy = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
T = 3084
assert spy.size >= T
y = spy[:T].copy()
z = np.concatenate([[0.0], y[:-1]])
print(f"# Liu-West run_series, T = {T}; {passes} passes per route after 2 warm-up passes; us per step")
print("# form     N    R   series med   tiled med  tiled min..max (spread)    gain  2*spread  gain > 2*spread  same bits")
wins = []
for form, cls in ((0, sa.svol_lw_1_par), (1, sa.svol_lw_2_par)):
    for n, R in ((10, 1), (100, 1), (500, 1), (1000, 1), (2048, 1), (500, 100)):
        g = cls(0.99, 0.8, 0.99, -0.1, 0.1, 0.01, 0.1, -0.5, -0.01, nparts=n, n_filters=R, seed=20260101)
        g.set_small_series(True)
        assert g.series_route() == (sa.ROUTE_LW_SERIES, 512)
        ms = {True: [], False: []}
        ll = {}
        for i in range(passes + 2):
            for small in (False, True):                      # the two routes alternate
                g.set_small_series(small)
                ll[small] = g.run_series(y, z)
                if i >= 2:
                    ms[small].append(g.last_elapsed_ms())
        us = {k: np.array(v) * 1e3 / T for k, v in ms.items()}
        med_s, med_t = float(np.median(us[True])), float(np.median(us[False]))
        spread = float(us[False].max() - us[False].min())
        same = bool((ll[True].view(np.uint64) == ll[False].view(np.uint64)).all())
        win = (med_t - med_s) > 2 * spread
        wins.append(win and same)
        print(f"  {form:4d} {n:5d} {R:4d}  {med_s:10.3f}  {med_t:10.3f}  {us[False].min():7.3f}..{us[False].max():7.3f} ({spread:6.3f})  "
              f"{med_t - med_s:6.3f}  {2 * spread:8.3f}  {str(win):>15s}  {same}", flush=True)
        g.close()
print("# default route by the rule: " + ("SERIES (a gain of more than twice the spread at every shape, both forms)" if all(wins)
                                          else "TILED (the rule fails at the shapes marked False; the series route stays opt-in)"))
