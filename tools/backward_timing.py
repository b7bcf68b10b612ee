"""Timings of backward-simulation smoothing on the GPU (profiles/backward_sim_timing.txt).

    python tools/backward_timing.py [--reps 7] [--out FILE]

SVOL, multinomial resampling every step, T = 256.  Shapes: N = 500 x R = 100 with K = 1, 16, 500 and N = 2^16 (R = 1) with K = 16.
Per (shape, K), `reps` passes after a warm-up pass; a pass is
    run_series (recording)  ->  sample_trajectories_backward  ->  sample_trajectories_backward  ->  sample_trajectories
so the three calls alternate and see the same history.  Device times are the HIP events of ssme_pf_smoothing_elapsed_ms (kernels alone):
the first backward call after a recording run also fills the log-weight rows, the second reuses them, so
    k_bsim       = the second call's kernel time,
    k_bsim_logw  = first - second  (per pass),
    genealogy    = ssme_pf_sample_trajectories at the same K: the cost of what backward simulation replaces.
Medians and min .. max of the passes.  Last: the restatement's numpy arithmetic (tests/backward_ref.py) for ONE trajectory of one filter
of N = 500 on the host, from per-step downloads -- what a user would otherwise do.
Needs a GPU: without one the first create fails (there is no CPU path)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T = 256
CASES = ((500, 100, (1, 16, 500)), (1 << 16, 1, (16,)))
TH = (1.0, 0.95, 0.25)
SEED = 11


def stats(v):
    return "median %9.3f  min %9.3f  max %9.3f" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    import ssme_amd as sa
    y = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))[:T].copy()
    emit("tools/backward_timing.py: SVOL, multinomial resampling every step, T = %d, %d timed passes after a warm-up pass; kernel times are HIP events, ms" % (T, a.reps))
    for n, r, Ks in CASES:
        bank = sa.ParticleFilterBank(sa.MODEL_SVOL, n, r, seed=SEED)
        bank.set_params(TH)
        bank.record_series_history()
        emit("\n== N = %d, R = %d, T = %d: history %.1f MiB, log-weight rows %.1f MiB ==" % (n, r, T, bank.series_history_bytes(T) / 2.0 ** 20, bank.backward_bytes(T) / 2.0 ** 20))
        for K in Ks:
            first, second, gen, wall = [], [], [], []
            for i in range(a.reps + 1):
                bank.run_series(y)
                bank.sample_trajectories_backward(K)
                k1 = bank.smoothing_elapsed_ms()[0]
                t0 = time.perf_counter()
                xb, ib = bank.sample_trajectories_backward(K, return_indices=True)
                w = (time.perf_counter() - t0) * 1e3
                k2 = bank.smoothing_elapsed_ms()[0]
                xg, ig = bank.sample_trajectories(K, indices=True)
                k3 = bank.smoothing_elapsed_ms()[0]
                if i:
                    first.append(k1), second.append(k2), gen.append(k3), wall.append(w)
            emit("K = %4d  k_bsim                        %s" % (K, stats(second)))
            emit("          k_bsim_logw (first - second)  %s" % stats([f - s for f, s in zip(first, second)]))
            emit("          sample_trajectories (genealogy) %s" % stats(gen))
            emit("          backward call, host wall        %s   distinct indices at t = 0, filter 0: backward %d, genealogy %d"
                 % (stats(wall), len(np.unique(ib[0, :, 0])), len(np.unique(ig[0, :, 0]))))
        bank.close()
    # the host route for one trajectory
    import backward_ref as br
    from oracle import oracle as O
    O.build()
    twin = sa.ParticleFilterBank(sa.MODEL_SVOL, 500, 1, seed=SEED)
    twin.set_params(TH)
    t0 = time.perf_counter()
    hist = br.stepped_history(twin, y)
    t_hist = (time.perf_counter() - t0) * 1e3
    twin.close()
    logf = br.logf_builtin(O, br.MODEL_SVOL, TH)
    w = []
    for _ in range(3):
        t0 = time.perf_counter()
        br.backward_filter(O, logf, hist["xs"][0], hist["lws"][0], hist["ancs"][0], 1, [0], SEED, 0)
        w.append((time.perf_counter() - t0) * 1e3)
    emit("\nhost route, N = 500, ONE filter, ONE trajectory: step API with per-step downloads %.1f ms, then the restatement's numpy arithmetic %s" % (t_hist, stats(w)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
