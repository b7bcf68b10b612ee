"""Times the device pass over a user model's own functionals against the download-and-sum route it replaces, at the two-factor test
model (tests/models/svol_two_factor_h.h: dim_x = 2, n_h = 7), R = 512 filters of N = 2^14 particles.  Per call:
  (a) ParticleFilterBank.user_expectations(): two kernels and ONE download of 7 * R doubles
  (b) the host route: ssme_pf_download_weights per member (3 * 8 * N * R bytes to the host) and the seven weighted sums in numpy
  (c) expectations_multi with the four built-in functionals: the yardstick for a pass over one plane
Wall-clock times are host clocks around calls that end in a stream synchronise; HIP-event times are the elapsed time between two events
recorded on the handle's stream right before and right after a call (kernels, copy, and the host's return).  Kernel durations alone:
run this script with --kernels-only under `rocprofv3 --kernel-trace --stats`.
    SSME_PF_LIB=build/user/libssme_pf_two_factor_h.so python tools/user_expect_timing.py [--kernels-only]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ssme_amd as sa  # noqa: E402
from ssme_amd import _capi  # noqa: E402

R, N = 512, 1 << 14
kernels_only = "--kernels-only" in sys.argv
assert _capi.lib().ssme_pf_user_model_n_h() == 7, "run with SSME_PF_LIB = the library built from tests/models/svol_two_factor_h.h"
spy = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
bank = sa.ParticleFilterBank(sa.MODEL_USER0, N, R, 20260101)
stream = torch.cuda.Stream()
bank._chk(_capi.lib().ssme_pf_set_stream(bank._h, stream.cuda_stream))
bank.set_params([1.1, 0.95, 0.9, 0.2, 0.15, -0.4])
z = 0.5
for t in range(8):
    bank.step(np.array([spy[t], spy[100 + t]]), z)


def host_route():
    out = np.empty((7, R))
    for r in range(R):
        x, w = bank.weights(r)
        x1, x2 = x[0], x[1]
        s = w.sum()
        for k, hv in enumerate((x1, x2, x1 * x1, x1 * x2, x2 * x2, np.exp(0.5 * (x1 + x2)), np.full(N, z + 1.0))):
            out[k, r] = np.dot(hv, w) / s
    return out


def timed(fn, warm, reps):
    """(median wall-clock us, median HIP-event us) per call"""
    for _ in range(warm):
        fn()
    wall, evt = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record(stream)
        e1.synchronize()
        wall.append((t1 - t0) * 1e6)
        evt.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(wall)), float(np.median(evt)), float(np.min(wall)), float(np.max(wall))


if kernels_only:
    for _ in range(50):
        bank.user_expectations()
        bank.expectations_multi([0, 1, 2, 3])
    print("kernels-only run: 50 calls each of user_expectations and expectations_multi", flush=True)
else:
    dev = bank.user_expectations()
    host = host_route()
    print(f"two-factor model, R = {R}, N = {N}; largest |device - host| over the 7 x R expectations: {np.max(np.abs(dev - host)):.3e}", flush=True)
    a = timed(bank.user_expectations, 50, 500)
    print(f"(a) user_expectations, 7 functionals, one download of {7 * R * 8} bytes: wall-clock {a[0]:.1f} us per call (min {a[2]:.1f}, max {a[3]:.1f}), HIP events {a[1]:.1f} us", flush=True)
    c = timed(lambda: bank.expectations_multi([0, 1, 2, 3]), 50, 500)
    print(f"(c) expectations_multi, 4 built-in functionals of component 0: wall-clock {c[0]:.1f} us per call (min {c[2]:.1f}, max {c[3]:.1f}), HIP events {c[1]:.1f} us", flush=True)
    b = timed(host_route, 1, 5)
    print(f"(b) download_weights per member + host sums, {3 * 8 * N * R / 1e6:.0f} MB to the host: wall-clock {b[0] / 1e3:.1f} ms per call (min {b[2] / 1e3:.1f}, max {b[3] / 1e3:.1f}), HIP events {b[1] / 1e3:.1f} ms", flush=True)
    only_dl = timed(lambda: [bank.weights(r) for r in range(R)], 1, 5)
    print(f"    of which the {R} downloads alone: wall-clock {only_dl[0] / 1e3:.1f} ms per call", flush=True)
    print(f"(b) / (a) = {b[0] / a[0]:.0f}x; bytes read by (a): {(2 + 1) * 8 * N * R / 1e6:.0f} MB from device memory per call", flush=True)
bank.close()
