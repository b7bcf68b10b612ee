"""What tests/test_marginal_gpu.py and tests/marginal_worker.py share: the comparison of the device's marginal smoothing weights with
tests/marginal_ref.py on a recorded handle and its stepped twin (tests/backward_cases.py makes both)."""
import math

import numpy as np

import marginal_ref as mr
from backward_cases import same_bits

U = 2.0 ** -53
SEG, CHUNK = 8, 64                         # kMsmSeg and the columns a wave of k_msm_rows stages at a time: the device's order of summation


def device_order_push(row_next, parents, n):
    """sum of row_next[j] over parents[j] = i in the order k_msm_rows adds: chunk j // 64 belongs to segment (j // 64) % 8, a segment is
    summed in ascending j, the 8 segment sums in ascending order."""
    parts = np.zeros((SEG, n))
    for j in range(n):
        parts[(j // CHUNK) % SEG, parents[j]] += row_next[j]
    w = parts[0].copy()
    for q in range(1, SEG):
        w = w + parts[q]
    return w


def final_weights(bank, f):
    """(w of ssme_pf_download_weights, alive): a filter without final weight hands out NaN there and has all-zero rows here."""
    w = np.asarray(bank.weights(f)[1], dtype=np.float64)
    alive = bool(np.isfinite(w).all() and math.fsum(w) > 0.0)
    return w, alive


def device_rows(bank, f, T):
    """(om [T, N], x [T][dim_x, N]) of filter f."""
    rows = [bank.smoothing_weights(f, t) for t in range(T)]
    return np.stack([w for _, w in rows]), [np.atleast_2d(x) for x, _ in rows]


def check_rows(O, bank, hist, logf_of_filter, sched, name, zs=None):
    """Every om row of every filter against the restatement within marginal_ref.bound, zeros coinciding, row T - 1 with the bits of
    download_weights, x_t with the bits of the twin, and the mass of every row.  Returns (degenerate columns of the restatement, the
    worst |device - ref| / (bound ref) seen)."""
    T = len(hist["xs"][0])
    n = bank.n
    degenerate, worst = 0, 0.0
    for f in range(bank.r):
        w, alive = final_weights(bank, f)
        dev, xs = device_rows(bank, f, T)
        for t in range(T):
            same_bits(xs[t], hist["xs"][f][t], f"{name}: x_{t} of filter {f}")
        if not alive:
            assert (dev == 0.0).all() and not np.signbit(dev).any(), f"{name}: filter {f} has no final weight: all-zero rows"
            continue
        same_bits(dev[T - 1], w, f"{name}: row T - 1 of filter {f} is the final weights")
        ref, d = mr.filter_rows(O, logf_of_filter(f), hist["xs"][f], hist["lws"][f], hist["ancs"][f], sched, w, zs)
        degenerate += d
        total = math.fsum(w)
        for t in range(T):
            b = mr.bound(T, n, t)
            assert np.array_equal(dev[t] == 0.0, ref[t] == 0.0), f"{name}: zeros of row {t}, filter {f}"
            assert np.isfinite(dev[t]).all() and (dev[t] >= 0.0).all(), f"{name}: row {t}, filter {f}"
            err = np.abs(dev[t] - ref[t])
            lim = b * ref[t]
            bad = np.flatnonzero(err > lim)
            assert bad.size == 0, (name, f, t, bad[:4], dev[t][bad[:4]], ref[t][bad[:4]], b)
            if t < T - 1:
                nz = ref[t] > 0.0
                if nz.any():
                    worst = max(worst, float(np.max(err[nz] / lim[nz])))
                mass = math.fsum(dev[t])
                assert abs(mass - total) <= b * total, (name, f, t, mass, total, b)
    return degenerate, worst


HS = {0: lambda v: v, 1: lambda v: v * v, 2: lambda v: np.exp(0.5 * v), 3: lambda v: np.full_like(v, 42.0)}


def check_means(bank, T, name, functionals=(0, 1, 2, 3)):
    """marginal_smoothed_expectations against sum h om / sum om formed with fsum from the downloaded rows, within
    (N + 3) u sum |h| om / sum om: the product, at most N - 1 additions of either sum, the division and an ulp of h itself.
    NaN rows for a filter without final weight."""
    n = bank.n
    out = bank.marginal_smoothed_expectations(functionals)
    assert out.shape == (T, len(functionals), bank.r)
    for f in range(bank.r):
        _, alive = final_weights(bank, f)
        dev, xs = device_rows(bank, f, T)
        for t in range(T):
            den = math.fsum(dev[t])
            for i, fid in enumerate(functionals):
                if not alive or not den > 0.0:
                    assert np.isnan(out[t, i, f]), (name, f, t, fid)
                    continue
                h = HS[fid](xs[t][0])
                want = math.fsum(h * dev[t]) / den
                tol = (n + 3) * U * math.fsum(np.abs(h) * dev[t]) / den
                assert abs(out[t, i, f] - want) <= tol, (name, f, t, fid, out[t, i, f], want, tol)
    return out
