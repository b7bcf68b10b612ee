"""An exact reference of the log conditional likelihood of the bootstrap filter, and the budget of the device's fixed-point value.
Plain numpy / Python, no device code: test_bs_edges_cpu.py (oracle) and test_bootstrap_edges_gpu.py (device) share it, as
expect_ref.py is shared by the expectation tests.

Definition.  With logw_i the log-weights of step t (log g alone after a resampling step, carried sums otherwise),
    lse_t = log sum_i exp(logw_i),       l_t = lse_t - prev_t,
    prev_t = log N if step t starts from resampled (equal) weights, i.e. t = 0 or t % sched == 0, else lse_{t-1}.
exact_series evaluates it as M + log sum_i exp(logw_i - M), M = max logw: the exponentials in 80-bit long double (each within
2^-63 relative), their sum EXACTLY in rational arithmetic up to FRACTION_MAX_N particles and by 80-bit pairwise sums above (depth
<= 23: 2^-59 relative), the logarithm and the two additions in long double.  The reference's own error is below 2^-58 (1 + |l_t|).
A step whose log-weights hold a NaN, or no value above -inf, has no positive finite weight left: the value is NaN (the reference
library's log-sum-exp gives -inf + log(NaN) there), and NaN is carried through prev_t while the weights are not reset.

Budget of |device - exact|, derived from the code (csrc/pf_kernels.h; oracle/ssme_oracle.cpp restates the same sequence):
    q_i  = rne(exp_t(fl(logw_i - m_b)) 2^41)            tile maximum m_b, kTileShift = 41
    A_b  = sum_{i in b} q_i                              exact integers
    A'_b = rint(fl(A_b * e_b) 2^(rg - 41)),  e_b = exp_t(fl(m_b - m)),  rg = 52 - ceil(log2 Npad)
    S    = sum_b A'_b                                    exact;  lse_dev = fl(m + dlog(S 2^-rg)),  l_dev = fl(lse_dev - prev_dev)
Write W = sum_i exp(logw_i - m) >= 1 (the largest weight is exp(0)) and s_b = exp(m_b - m) <= 1.  Then |S 2^-rg - W| <= E_W with
    per particle   s_b 2^-42                             the rne of q_i: half a unit of 2^-41, scaled by s_b
                 + w_i (2^-51 + u |logw_i - m_b|)       exp_t within 2 ulp (test_oracle_cpu.py pins it), the rounded subtraction
    per tile       2^-rg / 2                             the one rint of the rescaling
                 + W_b (2^-51 + u |m_b - m| + u)         e_b within 2 ulp, its rounded argument, the rounded product A_b * e_b
                 + A_b 2^-41 2^-1074                     a subnormal e_b: one unit of the subnormal grid, absolute
and where e_b has underflowed to zero the tile's whole W_b is the error.  Through the logarithm (W >= 1, |log(1 + x)| <= |x| / (1 - |x|)):
    |lse_dev - lse| <= r / (1 - r), r = E_W / W          the sum
                     + 2^-51 |log W|                     dlog within 2 ulp of its result
                     + u |lse|                           the addition m + log
    |l_dev - l|     <= that + err(prev) + u |l|          the final subtraction; err(log N) = 2^-51 log N (dlog), err(lse_{t-1}) as above
plus the reference's own 2^-58 (1 + |l|).  Every rounding is taken at its maximum and with one sign, so observed errors are a small
fraction of it (profiles/bs_edge_budgets.txt): the quantisation errors of N particles do not all point one way."""
import numpy as np

from expect_ref import FRACTION_MAX_N, LD, TILE_SHIFT, U, pairwise_sum

NAN = float("nan")


def _exact_sum(w):
    """Sum of non-negative long doubles: exactly (every term is an integer multiple of a power of two: the rational sum is one big
    integer over the smallest unit, rounded once to 64 bits at the end) up to FRACTION_MAX_N terms, pairwise above."""
    if w.size > FRACTION_MAX_N:
        return pairwise_sum(w)
    w = w[w > 0]
    if w.size == 0:
        return LD(0)
    mant, ex = np.frexp(w)                                        # w = mant 2^ex, mant in [0.5, 1): mant 2^64 is an integer
    hi = np.floor(mant * LD(2.0 ** 32))
    lo = (mant * LD(2.0 ** 32) - hi) * LD(2.0 ** 32)
    emin = int(ex.min())
    total = 0
    for h, l, e in zip(hi.astype(np.float64), lo.astype(np.float64), ex):
        total += ((int(h) << 32) | int(l)) << (int(e) - emin)
    sh = max(total.bit_length() - 64, 0)
    top = (total + ((1 << sh) >> 1)) >> sh                       # 64 significant bits, rounded to nearest
    return np.ldexp(LD(float(top >> 32)) * LD(2.0 ** 32) + LD(float(top & 0xFFFFFFFF)), sh + emin - 64)          # total 2^(emin - 64)


def rg_of(n, tile):
    """rshift of the handle: 52 - ceil(log2 Npad), Npad = N rounded up to whole tiles."""
    npad = -(-int(n) // tile) * tile
    return 52 - (npad - 1).bit_length()


def lse_exact(logw, tile):
    """(lse, err): the exact log-sum-exp of one step's log-weights as a long double and the budget of the device's lse against it;
    (NaN, NaN) where no positive finite weight is left."""
    lw = np.asarray(logw, dtype=np.float64)
    n = lw.size
    if np.isnan(lw).any() or not (lw > -np.inf).any():
        return LD(NAN), NAN
    assert not np.isposinf(lw).any()
    M = float(lw.max())
    with np.errstate(all="ignore"):
        w = np.exp(lw.astype(LD) - LD(M))
        W = _exact_sum(w)
        lse = LD(M) + np.log(W)
        starts = np.arange(0, n, tile)
        mb = np.maximum.reduceat(lw, starts)
        tix = np.arange(n) // tile
        live = np.isfinite(mb)                                    # a tile of -inf only: q = 0, A = 0, nothing to rescale
        d2 = np.where(live, np.abs(mb - M), 0.0)
        s = np.where(live, np.exp((mb - M).astype(LD)), LD(0))
        d1 = np.where(np.isfinite(lw), np.abs(lw - mb[tix]), 0.0)
        Wb = np.array([pairwise_sum(w[a:a + tile]) for a in starts], dtype=LD)
        cnt = np.minimum(tile, n - starts).astype(LD)
        e_part = pairwise_sum(s * cnt) * LD(2.0) ** -(TILE_SHIFT + 1) + pairwise_sum(w * (LD(2.0 ** -51) + LD(U) * d1.astype(LD)))
        e_tile = LD(starts.size) * LD(2.0) ** -(rg_of(n, tile) + 1) + pairwise_sum(Wb * (LD(2.0 ** -51) + LD(U) * d2.astype(LD) + LD(U)))
        sd = np.exp(-d2).astype(np.float64)                       # the double scale: subnormal or zero where the tile lies far below
        sub = live & (sd < 2.0 ** -1022)
        if sub.any():
            e_tile = e_tile + pairwise_sum(np.where(sd == 0.0, Wb, cnt * LD(2.0) ** -1074)[sub])
        r = float((e_part + e_tile) / W)
    assert r < 0.5, r
    err = r / (1.0 - r) + 2.0 ** -51 * abs(float(np.log(W))) + U * abs(float(lse)) + 2.0 ** -58 * (1.0 + abs(float(lse)))
    return lse, err


def exact_series(logws, n, tile, sched=1):
    """logws: the log-weights after every step t = 0 .. T-1.  Returns [(l_t as a double, budget of |device - l_t|)]; (NaN, NaN)
    where the exact value is NaN."""
    out, prev, prev_err = [], None, None
    logn, logn_err = np.log(LD(n)), 2.0 ** -51 * float(np.log(n))
    for t, lw in enumerate(logws):
        if t == 0 or t % sched == 0:
            prev, prev_err = logn, logn_err
        lse, err = lse_exact(lw, tile)
        ell = lse - prev
        if np.isnan(ell):
            out.append((NAN, NAN))
        else:
            out.append((float(ell), err + prev_err + U * abs(float(ell)) + 2.0 ** -58 * (1.0 + abs(float(ell)))))
        prev, prev_err = lse, err
    return out


def check(name, got, want, log=None):
    """got: per-step values of the oracle or the device; want: exact_series().  NaN for NaN, infinities equal, finite values within
    the budget.  Returns the list of failures; log(name, t, err, budget) records every finite step."""
    bad = []
    for t, (g, (w, b)) in enumerate(zip(got, want)):
        if np.isnan(w):
            if not np.isnan(g):
                bad.append(f"{name} t={t}: {g!r}, the exact value is NaN")
        elif np.isinf(w):
            if g != w:
                bad.append(f"{name} t={t}: {g!r} != {w!r}")
        else:
            err = abs(float(g) - w) if np.isfinite(g) else float("inf")
            if log is not None:
                log(name, t, err, b)
            if not err <= b:
                bad.append(f"{name} t={t}: |{g!r} - {w!r}| = {err:.3e} > budget {b:.3e}")
    return bad
