"""Recorded Liu-West series (ssme_lw_set_series_expectations): what recording costs and which route a recording handle takes.
    python tools/lw_series_expect_timing.py PARENT_LIB [passes] > profiles/lw_series_expectations_timing.txt
PARENT_LIB: libssme_pf.so built from the parent commit.  T = 3084 rows of spy_returns.csv with z its lag, both forms (svol_lw_1_par
auxiliary, svol_lw_2_par SISR), (N, R) = (500, 1), (2048, 1), (500, 100), resampling every step.  Every library runs in a process of
its own (`--worker LIB PART passes`), through ctypes alone: the parent's library has no recording entry points.
  (i)  non-recording run_series, HIP-event time (ssme_lw_last_elapsed_ms): parent, this commit, parent again.  The margin is the
       parent's own spread between its two runs.
  (ii) recording, wall time including the download of the trajectory: the whole-series route, the tiled route, and a step loop of
       ssme_lw_step + ssme_lw_get_expectations (all eight ids), the only way before this change.
The rule (profiles/lw_series_timing.txt): a recording handle of one tile keeps the whole-series route only if its gain over the
recording tiled route exceeds twice the tiled route's own pass-to-pass spread at every measured shape, for both forms."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 3084
SHAPES = ((500, 1), (2048, 1), (500, 100))
WARMUP = 2


class LwConfig(C.Structure):
    _fields_ = [("n_particles", C.c_int32), ("n_filters", C.c_int32), ("seed", C.c_uint64), ("device", C.c_int32),
                ("first_filter_id", C.c_uint32), ("delta", C.c_double), ("transforms", C.c_int32 * 4),
                ("prior_lo", C.c_double * 4), ("prior_hi", C.c_double * 4), ("form", C.c_int32), ("resamp_sched", C.c_int32)]


def series():
    spy = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
    assert spy.size >= T
    y = spy[:T].copy()
    return y, np.concatenate([[0.0], y[:-1]])


def worker(path, part, passes):
    L = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    H = C.c_void_p
    L.ssme_lw_create.argtypes = [C.POINTER(LwConfig), C.POINTER(H)]
    L.ssme_lw_destroy.argtypes = [H]
    L.ssme_lw_reset.argtypes = [H]
    L.ssme_lw_step.argtypes = [H, dp, dp, dp]
    L.ssme_lw_run_series.argtypes = [H, dp, dp, C.c_int32, dp]
    L.ssme_lw_get_expectations.argtypes = [H, ip, C.c_int32, dp]
    L.ssme_lw_set_small_series.argtypes = [H, C.c_int32]
    L.ssme_lw_last_elapsed_ms.argtypes = [H, C.POINTER(C.c_float)]
    if part == "ii":
        L.ssme_lw_set_series_expectations.argtypes = [H, C.c_int32]
        L.ssme_lw_get_series_expectations.argtypes = [H, ip, C.c_int32, dp, C.c_int32]

    def ok(rc):
        assert rc == 0, rc

    y, z = series()
    yp, zp = y.ctypes.data_as(dp), z.ctypes.data_as(dp)
    ids = np.arange(8, dtype=np.int32)
    idp = ids.ctypes.data_as(ip)
    for form in (0, 1):
        for n, R in SHAPES:
            cfg = LwConfig(n_particles=n, n_filters=R, seed=20260101, device=0, first_filter_id=0, delta=0.99, form=form, resamp_sched=1)
            cfg.transforms[:] = [2, 0, 3, 1]
            cfg.prior_lo[:] = [0.8, -0.1, 0.01, -0.5]
            cfg.prior_hi[:] = [0.99, 0.1, 0.1, -0.01]
            h = H()
            ok(L.ssme_lw_create(C.byref(cfg), C.byref(h)))
            tot = np.empty(R)
            totp = tot.ctypes.data_as(dp)
            if part == "i":
                us = []
                for i in range(passes + WARMUP):
                    ok(L.ssme_lw_run_series(h, yp, zp, T, totp))
                    ms = C.c_float()
                    ok(L.ssme_lw_last_elapsed_ms(h, C.byref(ms)))
                    if i >= WARMUP:
                        us.append(ms.value * 1e3 / T)
                print(f"DATA {form} {n} {R} plain {np.median(us):.3f} {min(us):.3f} {max(us):.3f}", flush=True)
            else:
                rows = {}
                ok(L.ssme_lw_set_series_expectations(h, 1))
                traj = np.empty((T, 8, R))
                for key, small in (("series", 1), ("tiled", 0)):
                    ok(L.ssme_lw_set_small_series(h, small))
                    us = []
                    for i in range(passes + WARMUP):
                        t0 = time.perf_counter()
                        ok(L.ssme_lw_run_series(h, yp, zp, T, totp))
                        ok(L.ssme_lw_get_series_expectations(h, idp, 8, traj.ctypes.data_as(dp), T))
                        dt = time.perf_counter() - t0
                        if i >= WARMUP:
                            us.append(dt * 1e6 / T)
                    rows[key] = traj.copy()
                    print(f"DATA {form} {n} {R} {key} {np.median(us):.3f} {min(us):.3f} {max(us):.3f}", flush=True)
                us = []
                loop = np.empty((T, 8, R))
                out = np.empty(R)
                outp = out.ctypes.data_as(dp)
                ys = [C.cast(C.c_void_p(y.ctypes.data + 8 * t), dp) for t in range(T)]
                zs = [C.cast(C.c_void_p(z.ctypes.data + 8 * t), dp) for t in range(T)]
                rows_t = [loop[t].ctypes.data_as(dp) for t in range(T)]
                for i in range(passes + WARMUP):
                    t0 = time.perf_counter()
                    ok(L.ssme_lw_reset(h))
                    for t in range(T):
                        ok(L.ssme_lw_step(h, ys[t], zs[t], outp))
                        ok(L.ssme_lw_get_expectations(h, idp, 8, rows_t[t]))
                    dt = time.perf_counter() - t0
                    if i >= WARMUP:
                        us.append(dt * 1e6 / T)
                rows["loop"] = loop
                print(f"DATA {form} {n} {R} loop {np.median(us):.3f} {min(us):.3f} {max(us):.3f}", flush=True)
                same = all(np.array_equal(rows["series"].view(np.uint64), rows[k].view(np.uint64)) for k in ("tiled", "loop"))
                print(f"DATA {form} {n} {R} samebits {int(same)} 0 0", flush=True)
            ok(L.ssme_lw_destroy(h))


def run_worker(path, part, passes):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", path, part, str(passes)], stdout=subprocess.PIPE, text=True,
                       check=True, timeout=900)
    out = {}
    for line in p.stdout.splitlines():
        if line.startswith("DATA "):
            _, form, n, R, key, med, lo, hi = line.split()
            out[(int(form), int(n), int(R), key)] = (float(med), float(lo), float(hi))
    return out


def cell(v):
    return f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"


def main(parent, passes):
    from ssme_amd import build
    this = build.build()
    p1 = run_worker(parent, "i", passes)
    t1 = run_worker(this, "i", passes)
    p2 = run_worker(parent, "i", passes)
    t2 = run_worker(this, "ii", passes)
    print("Recorded Liu-West series (ssme_lw_set_series_expectations): timings on one MI355X")
    print("=================================================================================")
    print(f"spy_returns.csv (T = {T}, z its lag), resampling every step, seed 20260101.  {WARMUP} warm-up passes, then {passes} passes; all figures")
    print("are us per step: median (min .. max) of the passes.  The parent commit's library and this commit's ran in one job on one")
    print("machine: parent, this commit, parent again, each in a process of its own (tools/lw_series_expect_timing.py).")
    print()
    print("(i) Non-recording run_series on the default route: this commit against the parent (HIP-event time, ssme_lw_last_elapsed_ms)")
    print("-" * 125)
    print(f"{'form  N     R':<16s}{'parent, first run':<30s}{'this commit':<30s}{'parent, second run':<30s}this - slower parent   parent's own spread")
    worst = []
    for form in (0, 1):
        for n, R in SHAPES:
            a, b, c = p1[(form, n, R, "plain")], t1[(form, n, R, "plain")], p2[(form, n, R, "plain")]
            over = b[0] - max(a[0], c[0])
            own = abs(a[0] - c[0])
            worst.append((over, own))
            print(f"{form:<6d}{n:<6d}{R:<4d}{cell(a):<30s}{cell(b):<30s}{cell(c):<30s}{over:+.3f}                 {own:.3f}")
    inside = all(o <= s for o, s in worst)
    print("This commit's median is " + ("at or below the slower of the parent's two medians, or above it by no more than the parent's two runs differ, at every shape."
                                       if inside else "ABOVE the slower of the parent's two medians by more than the parent's two runs differ at the shapes with over > spread."))
    print()
    print("(ii) Recording runs, wall time of ssme_lw_run_series + ssme_lw_get_series_expectations (all eight ids; the download is part of")
    print("     what the caller pays); the step loop is ssme_lw_reset + T x (ssme_lw_step + ssme_lw_get_expectations of the eight ids)")
    print("-" * 125)
    print(f"{'form  N     R':<16s}{'whole-series route':<30s}{'tiled route':<30s}{'step loop':<32s}gain    2 x tiled spread  gain > 2 x spread  same bits")
    wins = []
    for form in (0, 1):
        for n, R in SHAPES:
            s, t, lp = t2[(form, n, R, "series")], t2[(form, n, R, "tiled")], t2[(form, n, R, "loop")]
            same = bool(t2[(form, n, R, "samebits")][0])
            gain, spread = t[0] - s[0], t[2] - t[1]
            win = gain > 2 * spread
            wins.append(win and same)
            print(f"{form:<6d}{n:<6d}{R:<4d}{cell(s):<30s}{cell(t):<30s}{cell(lp):<32s}{gain:<8.3f}{2 * spread:<18.3f}{str(win):<19s}{same}")
    print()
    print("Recording on the whole-series route against not recording (event time of (i), this commit; wall time of (ii)):")
    for form in (0, 1):
        for n, R in SHAPES:
            print(f"  form {form}, N = {n}, R = {R}: {t1[(form, n, R, 'plain')][0]:.3f} -> {t2[(form, n, R, 'series')][0]:.3f}")
    print()
    print("Decision by the rule (the gain over the recording tiled route must exceed twice that route's own pass-to-pass spread at every")
    print("shape, for both forms): " + ("a recording handle of one tile KEEPS the whole-series route; ssme_lw_get_series_route of a recording handle is that of a non-recording one."
                                        if all(wins) else "recording handles take the TILED route (the rule fails at the shapes marked False)."))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        sys.path.insert(0, ROOT)
        main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 7)
