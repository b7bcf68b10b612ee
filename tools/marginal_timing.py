"""Timings of marginal smoothing on the GPU (profiles/marginal_smoothing_timing.txt).

    python tools/marginal_timing.py [--reps 5] [--out FILE] [--stats-dir DIR [--stats-only]]
    python tools/marginal_timing.py --trace            the marginal calls alone, two passes per shape: what a kernel trace is taken of

SVOL, multinomial resampling every step, T = 256.  Shapes: N = 500 x R = 100, N = 2048 x 1 and N = 2^14 x 1.  Per shape, `reps` passes
after a warm-up pass (the largest shape: at most 3); a pass is
    run_series (recording) -> marginal_smoothed_expectations -> marginal_smoothed_expectations -> smoothing_weights
                           -> sample_trajectories_backward(K = N) + the host mean -> smoothed_expectations
so the calls alternate and see the same history.  Device times are the HIP events of ssme_pf_smoothing_elapsed_ms (kernels alone):
the first marginal call after a recording run fills the log-weight rows, the column tables and the weight rows and forms the means;
the second forms the means alone, so
    repeated call  = k_msm_expect,
    fill           = first - second  (k_bsim_logw, k_msm_start, k_msm_columns, k_msm_rows), 3 N^2 (T - 1) R density evaluations.
The split of the fill between k_msm_columns and k_msm_rows is not visible to events: --stats-dir names the output directory of a
kernel trace of `--trace` (a run of its own), whose times are appended per kernel and grid, that is per shape.  SSME_PF_LIB selects another build of the library
(an A/B of the number of partial sums of k_msm_rows: ssme_amd.build.build(force=True, extra=("-DSSME_MSM_SEG=16",), out=...)).
Medians and min .. max of the passes.  Needs a GPU: without one the first create fails (there is no CPU path)."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T = 256
CASES = ((500, 100), (2048, 1), (1 << 14, 1))          # (N, R)
TH = (1.0, 0.95, 0.25)
SEED = 11
IDS = (0, 1)
TRACE_PASSES = 2


def stats(v):
    return "median %10.3f  min %10.3f  max %10.3f" % (statistics.median(v), min(v), max(v))


def make_bank(sa, n, r):
    bank = sa.ParticleFilterBank(sa.MODEL_SVOL, n, r, seed=SEED)
    bank.set_params(TH)
    bank.record_series_history()
    return bank


def trace(sa, y):
    for n, r in CASES:
        bank = make_bank(sa, n, r)
        for _ in range(TRACE_PASSES):
            bank.run_series(y)
            bank.marginal_smoothed_expectations(IDS)
            bank.marginal_smoothed_expectations(IDS)
        bank.close()


def kernel_stats(stats_dir, emit):
    """Per kernel and grid (= per shape) of the newest kernel_trace.csv under stats_dir: launches, total and median / min / max ms."""
    files = sorted(glob.glob(os.path.join(stats_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        emit("no kernel_trace.csv under %s" % stats_dir)
        return
    emit("\n== kernel trace of `--trace` (%d passes per shape; per kernel and grid, ms) ==" % TRACE_PASSES)
    agg = {}
    for row in csv.DictReader(open(files[-1])):
        name = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("ssme::", "")
        if "k_msm" in name or "k_bsim_logw" in name:
            wg = int(row["Workgroup_Size_X"])
            key = (name, "%d x %s x %s workgroups of %d" % (int(row["Grid_Size_X"]) // wg, row["Grid_Size_Y"], row["Grid_Size_Z"], wg))
            agg.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    for (name, grid), v in agg.items():
        emit("%-22s %-38s launches %4d  total %9.3f  median %8.4f  min %8.4f  max %8.4f" % (name, grid, len(v), sum(v), statistics.median(v), min(v), max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--stats-dir")
    ap.add_argument("--stats-only", action="store_true", help="with --stats-dir: print the report of a trace and stop (needs no GPU)")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    if a.stats_dir and a.stats_only:
        kernel_stats(a.stats_dir, emit)
        return
    import ssme_amd as sa
    y = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))[:T].copy()
    if a.trace:
        trace(sa, y)
        return
    emit("tools/marginal_timing.py: SVOL, multinomial resampling every step, T = %d, timed passes after a warm-up pass; kernel times are HIP events, ms%s"
         % (T, "; library " + os.path.basename(os.environ["SSME_PF_LIB"]) if os.environ.get("SSME_PF_LIB") else ""))
    for n, r in CASES:
        reps = min(a.reps, 3) if n > 4096 else a.reps
        evals = float(n) * n * (T - 1) * r
        bank = make_bank(sa, n, r)
        emit("\n== N = %d, R = %d, T = %d, %d passes: history %.1f MiB, marginal smoothing %.1f MiB (%.1f MiB of it shared with backward simulation) =="
             % (n, r, T, reps, bank.series_history_bytes(T) / 2.0 ** 20, bank.marginal_smoothing_bytes(T) / 2.0 ** 20, bank.backward_bytes(T) / 2.0 ** 20))
        first, second, call1, call2, wall1, wall2, row, back, back_wall, gen = [], [], [], [], [], [], [], [], [], []
        for i in range(reps + 1):
            bank.run_series(y)
            t0 = time.perf_counter()
            m1 = bank.marginal_smoothed_expectations(IDS)
            w1 = (time.perf_counter() - t0) * 1e3
            k1, c1 = bank.smoothing_elapsed_ms()
            t0 = time.perf_counter()
            m2 = bank.marginal_smoothed_expectations(IDS)
            w2 = (time.perf_counter() - t0) * 1e3
            k2, c2 = bank.smoothing_elapsed_ms()
            assert np.array_equal(m1, m2)
            t0 = time.perf_counter()
            bank.smoothing_weights(0, 0)
            w3 = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            mb = bank.backward_smoothed_means(n, IDS)
            w4 = (time.perf_counter() - t0) * 1e3
            k4 = bank.smoothing_elapsed_ms()[0]
            mg = bank.smoothed_expectations(IDS)
            k5 = bank.smoothing_elapsed_ms()[0]
            if i:
                first.append(k1), second.append(k2), call1.append(c1), call2.append(c2), wall1.append(w1), wall2.append(w2), row.append(w3)
                back.append(k4), back_wall.append(w4), gen.append(k5)
        fill = [f - s for f, s in zip(first, second)]
        emit("first call: kernels                         %s" % stats(first))
        emit("  fill (first - second)                     %s   %.1f G density evaluations/s (3 N^2 (T - 1) R = %.3g)"
             % (stats(fill), 3.0 * evals / statistics.median(fill) / 1e6, 3.0 * evals))
        emit("  call without the download / host wall     %s  |  %s" % (stats(call1), stats(wall1)))
        emit("repeated call: kernels (k_msm_expect)       %s" % stats(second))
        emit("  call without the download / host wall     %s  |  %s" % (stats(call2), stats(wall2)))
        emit("smoothing_weights(0, 0), rows filled, wall  %s" % stats(row))
        emit("sample_trajectories_backward(K = N) kernels %s   %.1f G density evaluations/s (N^2 (T - 1) R = %.3g)"
             % (stats(back), evals / statistics.median(back) / 1e6, evals))
        emit("  backward_smoothed_means(K = N), host wall %s" % stats(back_wall))
        emit("smoothed_expectations (genealogy) kernels   %s" % stats(gen))
        t0 = int(np.argmax(np.abs(mb[:, 0, 0] - m1[:, 0, 0])))
        emit("  E[x_0] of filter 0: marginal %+.6f, backward simulation (K = N draws) %+.6f, genealogy %+.6f; largest |backward - marginal| of E[x_t]: %.4f at t = %d"
             % (m1[0, 0, 0], mb[0, 0, 0], mg[0, 0, 0], abs(mb[t0, 0, 0] - m1[t0, 0, 0]), t0))
        bank.close()
    if a.stats_dir:
        kernel_stats(a.stats_dir, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
