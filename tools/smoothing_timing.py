"""Timings of the series history and the smoothing calls on the GPU (profiles/series_history_timing.txt).

    python tools/smoothing_timing.py [--parent-lib /path/to/parent/libssme_pf.so] [--reps 9] [--out FILE]

Shapes: N = 500 x R = 100 (the one-tile route), N = 2^16 and N = 2^20 (R = 1), T = 256 each, SVOL, multinomial resampling every step.
Per shape:
  run_series, history off    device time per step (ssme_pf_last_elapsed_ms / T: HIP events around the series), this library and, with
                             --parent-lib, the parent commit's library in the SAME process, alternating, `reps` passes each after a
                             warm-up; median and min .. max of both (the spread).  Both are driven through the same few ctypes calls.
  run_series, history on     the same for this library with ssme_pf_set_series_history(1)
  backward sweep             ssme_pf_get_smoothed_expectations with 4 functionals: kernels (HIP events), call without download, host wall
  sample_trajectories        K = 1 and K = N: the same three
  the route this replaces    ssme_pf_step under set_debug(record_ancestors) with a download of (x, ancestors) of every filter after
                             every step, host wall per step (N = 500 and 2^16; at 2^20 the bytes per step are stated instead)
Needs a GPU: without one the first create fails (there is no CPU path)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ssme_amd import _capi  # noqa: E402

T = 256
SHAPES = ((500, 100), (1 << 16, 1), (1 << 20, 1))
TH = (1.0, 0.95, 0.25)
SEED = 11


class RawBank:
    """The few calls a non-recording series needs, on any build of the library (the parent's has no smoothing symbols)."""

    def __init__(self, L, n, r):
        self.L, self.h = L, C.c_void_p()
        cfg = _capi.Config(model=0, n_particles=n, n_filters=r, dtype=0, resampler=0, resamp_sched=1, seed=SEED, device=0)
        L.ssme_pf_create.argtypes = [C.POINTER(_capi.Config), C.POINTER(C.c_void_p)]
        dp = C.POINTER(C.c_double)
        L.ssme_pf_set_params.argtypes = [C.c_void_p, dp, C.c_int32, C.c_int32]
        L.ssme_pf_run_series.argtypes = [C.c_void_p, dp, dp, C.c_int32, dp]
        L.ssme_pf_last_elapsed_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.ssme_pf_destroy.argtypes = [C.c_void_p]
        _capi.check(L.ssme_pf_create(C.byref(cfg), C.byref(self.h)))
        th = np.asarray(TH, dtype=np.float64)
        _capi.check(L.ssme_pf_set_params(self.h, _capi.dptr(th), 3, 1))
        self.ll = np.empty(r)

    def run_us_per_step(self, y):
        _capi.check(self.L.ssme_pf_run_series(self.h, _capi.dptr(y), None, len(y), _capi.dptr(self.ll)))
        ms = C.c_float()
        self.L.ssme_pf_last_elapsed_ms(self.h, C.byref(ms))
        return ms.value * 1000.0 / len(y)

    def close(self):
        self.L.ssme_pf_destroy(self.h)


def stats(v):
    return "median %8.3f  min %8.3f  max %8.3f" % (statistics.median(v), min(v), max(v))


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def measure(n, r, y, reps, parent, emit):
    import ssme_amd as sa
    L = _capi.lib()
    emit(f"\n== N = {n}, R = {r}, T = {T} ==")
    new = RawBank(L, n, r)
    old = RawBank(parent, n, r) if parent is not None else None
    for b in (new, old):
        if b is not None:
            b.run_us_per_step(y), b.run_us_per_step(y)                      # warm-up: code objects, graph capture
    t_new, t_old = [], []
    for _ in range(reps):                                                    # alternating
        if old is not None:
            t_old.append(old.run_us_per_step(y))
        t_new.append(new.run_us_per_step(y))
    if old is not None:
        emit("run_series, history off, parent commit   us/step: " + stats(t_old))
        same = np.array_equal(old.ll, new.ll)
        emit("run_series, history off, this commit     us/step: " + stats(t_new) + ("   log-likelihoods equal the parent's bits: %s" % same))
        old.close()
    else:
        emit("run_series, history off, this commit     us/step: " + stats(t_new))
    ll_off = new.ll.copy()
    new.close()

    bank = sa.ParticleFilterBank(sa.MODEL_SVOL, n, r, seed=SEED)
    bank.set_params(TH)
    bank.record_series_history()
    emit("history: %.1f MiB" % (bank.series_history_bytes(T) / 2.0 ** 20))
    t_on = []
    for i in range(reps + 2):
        ll = bank.run_series(y)
        if i >= 2:
            t_on.append(bank.last_elapsed_ms() * 1000.0 / T)
    emit("run_series, history on,  this commit     us/step: " + stats(t_on) + ("   log-likelihoods equal history off: %s" % np.array_equal(ll, ll_off)))

    def timed(label, fn):
        fn()                                                                 # warm-up (buffers, code objects)
        k, c, w = [], [], []
        for _ in range(reps):
            _, ms = wall(fn)
            km, cm = bank.smoothing_elapsed_ms()
            k.append(km), c.append(cm), w.append(ms)
        emit("%-40s ms: kernels %s | call without download median %8.3f | host wall median %9.3f" % (label, stats(k), statistics.median(c), statistics.median(w)))

    timed("backward sweep, 4 functionals", lambda: bank.smoothed_expectations((0, 1, 2, 3)))
    timed("sample_trajectories(K = 1)", lambda: bank.sample_trajectories(1))
    timed("sample_trajectories(K = N = %d)" % n, lambda: bank.sample_trajectories(n))
    bank.close()

    if n <= (1 << 16):
        step = sa.ParticleFilterBank(sa.MODEL_SVOL, n, r, seed=SEED)
        step.set_params(TH)
        step.set_debug(record_ancestors=True, keep_logw=False)
        x, anc = np.empty(n), np.empty(n, dtype=np.uint32)

        def stepping():
            step.reset()
            for t in range(T):
                step.step(y[t])
                for f in range(r):
                    _capi.check(L.ssme_pf_download_state(step._h, f, _capi.dptr(x), None, None, _capi.u32ptr(anc)))
        stepping()
        w = [wall(stepping)[1] * 1000.0 / T for _ in range(3)]
        emit("step API + download of (x, ancestors) of every filter after every step, host wall us/step: " + stats(w))
        step.close()
    else:
        emit("step API + per-step download of (x, ancestors): not measured at this size; it moves 12 x %d = %d bytes over PCIe per step" % (n, 12 * n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    y = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))[:T].copy()
    _capi.lib()                                            # this library (and torch's HIP runtime, if torch is there) first: one runtime serves both
    parent = C.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    emit("tools/smoothing_timing.py: SVOL, multinomial resampling every step, T = %d, %d timed passes after warm-up; device times are HIP events" % (T, a.reps))
    for n, r in SHAPES:
        measure(n, r, y, a.reps, parent, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
