"""An exact reference for the expectation kernels, and derived error budgets.  Plain numpy / Python, no device code: the CPU tests
(test_expect_ref_cpu.py) and the GPU tests (test_expectations_gpu.py) share it.

What the device computes (csrc/pf_kernels.h, user_expect.h, lw_kernels.h) is the ratio

    E_q[h] = sum_j h_j q_j s_b(j)  /  sum_b A_b s_b,     q_j = cdf_j - cdf_{j-1} (tile-local integers), A_b = sum_{j in b} q_j,
                                                          s_b = the DOUBLE exp(m_b - m) of the libm-free exp (oracle.exp == dexp)

Given the doubles h_j and s_b that ratio is a rational number: expect_fixed_point evaluates it exactly (fractions.Fraction) or in
80-bit long double with pairwise sums.  expect_exact_weights is the same ratio with w_j = exp(logw_j - m), what the reference
library's formula means.  The budgets bound |device - E_q| (the kernel's summation tree) and |E_q - E_exact| (the fixed point).

A `state` is what make_state() builds from an oracle filter's state(): x, q, A, s, tile index of every particle, logw, mb, m.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                      # unit roundoff of fp64
TILE_SHIFT = 41                     # kTileShift (csrc/pf_kernels.h) == TILE_SHIFT (oracle/ssme_oracle.cpp): q_j = rne(exp(logw_j - m_b) 2^41)
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "expect_ref needs an 80-bit long double"
FRACTION_MAX_N = 10000              # above this the exact rational evaluation takes too long; long double then


# ---- the state ------------------------------------------------------------------------------------------------------------------
def q_from_cdf(cdf, tile):
    """Tile-local integer weights from the tile-local inclusive cdf."""
    c = np.asarray(cdf).astype(np.int64)
    q = np.diff(c, prepend=0)
    first = np.arange(0, c.size, tile)
    q[first] = c[first]
    return q


def make_state(oracle, st, tile, n=None):
    """st: Filter.state() / UserVectorModelFilter.state() of the oracle (or the device's own download, same keys)."""
    n = int(np.asarray(st["cdf"]).size if n is None else n)
    mb = np.asarray(st["mb"], dtype=np.float64)
    m = float(st["m"])
    q = q_from_cdf(st["cdf"], tile)
    A = np.asarray(st["A"]).astype(np.int64)
    tix = np.arange(n) // tile
    assert np.array_equal(np.bincount(tix, weights=None, minlength=A.size) > 0, np.ones(A.size, bool))
    assert np.array_equal(np.add.reduceat(q, np.arange(0, n, tile)), A), "tile sums are the sums of the tile's integer weights"
    return dict(x=np.asarray(st["x"]), q=q, A=A, s=oracle.exp(mb - m), tix=tix, mb=mb, m=m, tile=int(tile), n=n,
                logw=None if st.get("logw") is None else np.asarray(st["logw"], dtype=np.float64))


def lw_state(oracle, st, tile=2048):
    """The same for the oracle's Liu-West filter, whose state() carries the second-stage log-weights but no cdf: the tile maxima and
    q_j = oracle.quantize(logw_j - m_b, 41) are rebuilt exactly as the oracle's own step builds them (Filter::build_cdf)."""
    logw = np.asarray(st["logw"], dtype=np.float64)
    n = logw.size
    starts = np.arange(0, n, tile)
    mb = np.maximum.reduceat(logw, starts)
    tix = np.arange(n) // tile
    q = oracle.quantize(logw - mb[tix], TILE_SHIFT).astype(np.int64)
    A = np.add.reduceat(q, starts)
    m = float(mb.max())
    return dict(x=np.asarray(st["x"]), q=q, A=A, s=oracle.exp(mb - m), tix=tix, mb=mb, m=m, tile=int(tile), n=n, logw=logw)


def builtin_h(oracle, kind, x):
    """The built-in functionals in the device's own operation sequence (builtin_h of pf_kernels.h): x, x * x, dexp(0.5 x), 42."""
    x = np.asarray(x, dtype=np.float64)
    return x if kind == 0 else x * x if kind == 1 else oracle.exp(0.5 * x) if kind == 2 else np.full_like(x, 42.0)


# ---- evaluation -----------------------------------------------------------------------------------------------------------------
def pairwise_sum(a):
    """Balanced pairwise sum of a long-double vector: depth ceil(log2 n), so a relative error <= log2(n) 2^-64 of sum |a|."""
    a = np.asarray(a, dtype=LD)
    if a.size == 0:
        return LD(0)
    while a.size > 1:
        if a.size & 1:
            a = np.concatenate([a, np.zeros(1, dtype=LD)])
        a = a[0::2] + a[1::2]
    return a[0]


def _rows(h_vals, n):
    h = np.asarray(h_vals, dtype=np.float64)
    h = h[None, :] if h.ndim == 1 else h
    assert h.shape[1] == n
    return h


def exact_dot(v, q):
    """sum_j v_j q_j of finite doubles v and integers q as a Fraction, exactly: v_j = m_j 2^(e_j) with an integer m_j of at most 53
    bits (frexp), the products m_j q_j and their sums per exponent are Python integers, and the exponents are applied once per
    distinct value.  The same number as sum(Fraction(v_j) * q_j), two orders of magnitude sooner."""
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return Fraction(0)
    if not np.isfinite(v).all():
        raise ValueError("exact_dot: a value that is not finite")
    m, e = np.frexp(v)
    mi = np.ldexp(m, 53).astype(np.int64)                       # |m| < 1: an integer below 2^53, exactly
    e = e.astype(np.int64) - 53
    prod = mi.astype(object) * np.asarray(q).astype(np.int64).astype(object)
    lo = int(e.min())
    tot = 0
    for ue in np.unique(e):
        tot += int(prod[e == ue].sum()) << (int(ue) - lo)
    return Fraction(tot) * Fraction(2) ** lo


def _ratio_fraction(h, st):
    tix, q, s = st["tix"], st["q"], st["s"]
    sf = [Fraction(float(v)) for v in s]
    den = sum((int(a) * f for a, f in zip(st["A"], sf)), Fraction(0))
    starts = np.flatnonzero(np.diff(tix, prepend=-1))              # tix is sorted: tile b is a contiguous run
    assert (np.diff(tix) >= 0).all() and len(starts) == len(sf)
    ends = np.append(starts[1:], len(tix))
    out = []
    for row in h:
        num = Fraction(0)
        for b in range(len(sf)):
            num += exact_dot(row[starts[b]:ends[b]], q[starts[b]:ends[b]]) * sf[b]
        out.append(num / den)
    return out


def _ratio_longdouble(h, w):
    """sum_j h_j w_j / sum_j w_j in long double with pairwise sums; w: long double weights."""
    den = pairwise_sum(w)
    return [pairwise_sum(row.astype(LD) * w) / den for row in h]


def fixed_point_weights(st):
    """w~_j = q_j s_b in long double (q < 2^42 and s a double: the product is exact in 64 bits of mantissa up to one rounding)."""
    if "_wq" not in st:
        st["_wq"] = st["q"].astype(LD) * st["s"].astype(LD)[st["tix"]]
    return st["_wq"]


def exact_weights(st):
    """w_j = exp(logw_j - m) in long double, scaled by 2^41 so that it is on the scale of fixed_point_weights."""
    if "_wx" not in st:
        st["_wx"] = np.exp(st["logw"].astype(LD) - LD(st["m"])) * LD(2.0 ** TILE_SHIFT)
    return st["_wx"]


def expect_fixed_point(h_vals, st, method=None):
    """E_q[h] for every row of h_vals ([K, N] or [N]).  method: "fraction" (exact; returns Fractions), "longdouble", or None = exact
    up to FRACTION_MAX_N particles and long double above (relative error <= 2^-59 of sum |h| w / sum w: two pairwise sums of depth
    <= 23 and one division, each rounding 2^-64)."""
    h = _rows(h_vals, st["n"])
    if method is None:
        method = "fraction" if st["n"] <= FRACTION_MAX_N else "longdouble"
    if method == "fraction":
        return _ratio_fraction(h, st)
    return _ratio_longdouble(h, fixed_point_weights(st))


def expect_exact_weights(h_vals, st):
    """sum_j h_j w_j / sum_j w_j with w_j = exp(logw_j - m) in long double: the reference library's formula, unquantised."""
    return _ratio_longdouble(_rows(h_vals, st["n"]), exact_weights(st))


def s_abs(h_vals, st, exact=False):
    """sum |h_j| w_j / sum w_j under the fixed-point (default) or the exact weights; as doubles."""
    h = np.abs(_rows(h_vals, st["n"]))
    return np.array([float(v) for v in _ratio_longdouble(h, exact_weights(st) if exact else fixed_point_weights(st))])


# ---- budgets --------------------------------------------------------------------------------------------------------------------
def k_sum(tile, B, kernel):
    """Number of rounded operations that bound the relative error (in units of 2^-53 times S_abs) of one device expectation.

    kernel "expect" (k_expect_partials / k_expect_final) and "user" (k_user_expect_partials / k_user_expect_final): counted from
    the trees in the header comments of pf_kernels.h and user_expect.h.  Longest path from one particle to the NUMERATOR:
        1              the product h_j * q_j                       (-ffp-contract=off: product and sum round separately)
        tile / 256     chained adds of the thread                  ("expect": particles t, t + 256, ...; "user": 2t, 2t + 1, 2t + 512, ...:
                                                                    the same count, tile / 512 iterations of two adds)
        6 + 3          xor butterfly 32 .. 1, then ((w0 + w1) + w2) + w3
        1              the product part_b * s_b in the final kernel
        ceil(B / 256)  chained adds of the final kernel's thread   (tiles t, t + 256, ...)
        6 + 3          butterfly and waves again
    so k_num = tile / 256 + ceil(B / 256) + 20.  The DENOMINATOR takes the exact integers A_b: 1 + ceil(B / 256) + 9 operations.
    The division is one more.  |E_dev - E_q| <= (k_num + k_den + 1) u S_abs to first order, because a relative error of the
    denominator moves the ratio by that fraction of |E_q| <= S_abs.  k = k_num + k_den + 1 = tile / 256 + 2 ceil(B / 256) + 31.

    kernel "lw" (k_lw_param_partials / k_lw_param_means): the weight is formed per particle, w = q_j * scale (1 rounding), then
    w * h (1; for x^2 the square is part of h), tile / 256 chained adds, 9 tree adds, and k_lw_param_means adds the B tile partials in
    tile order: B adds.  k_num = 2 + tile / 256 + 9 + B; k_den = 1 + tile / 256 + 9 + B; one division:
    k = 2 tile / 256 + 2 B + 22.

    kernel "weights" (k_weights / k_lw_weights): one product (c_j - c_{j-1}) * sc of exact integers with the double sc; the reference
    forms sc as exp(m_b - m) 2^-41, the device as one scaled exp: equal unless the result is subnormal.  k = 2, relative to w_j."""
    chains = tile // 256
    wraps = -(-B // 256)
    if kernel in ("expect", "user"):
        return (chains + wraps + 20) + (wraps + 10) + 1
    if kernel == "lw":
        return (2 + chains + 9 + B) + (1 + chains + 9 + B) + 1
    if kernel == "weights":
        return 2
    raise ValueError(kernel)


def budget_sum(tile, B, kernel, sabs):
    """Forward error bound of the device's summation tree: gamma_k S_abs with gamma_k = k u / (1 - k u) (Higham, Accuracy and
    Stability, lemma 3.1) and k = k_sum(tile, B, kernel); plus the reference's own 2^-59.  FMA contraction would only lower it.
    It is a worst-case bound: every rounding at its maximum and with one sign.  Observed errors are a few per cent of it
    (profiles/expectation_budgets.txt), so a defect of under about an ulp of S_abs passes; a dropped, doubled or misindexed term does not."""
    k = k_sum(tile, B, kernel)
    return (k * U / (1.0 - k * U) + 2.0 ** -59) * np.asarray(sabs, dtype=np.float64)


def budget_fixed_point(h_vals, st, e_exact=None):
    """A bound of |E_q - E_exact| from the definition of the quantisation (Filter::build_cdf of the oracle, the step kernel of the
    device): q_j = rne(exp_t(fl(logw_j - m_b)) 2^41), w~_j = q_j s_b 2^-41, s_b = exp(fl(m_b - m)), against w_j = exp(logw_j - m).
        |w~_j - w_j| <= eps_j = s_b 2^-41 / 2                         round to nearest: half a unit of the tile's fixed point
                              + w~_j (u |logw_j - m_b| + u |m_b - m|   the two rounded subtractions, through exp
                                      + 2^-51 + 2^-51)                 exp_t and exp: within 2 ulp (test_oracle_cpu.py pins 1 ulp of libm)
                              + q_j 2^-41 2^-1074                      s_b subnormal: an absolute error of one subnormal unit
    and where s_b has underflowed to zero the whole w_j is the error.  Because sum_j (h_j - E_exact) w_j = 0,
        E_q - E_exact = sum_j (h_j - E_exact) (w~_j - w_j) / sum_j w~_j      exactly, so
        |E_q - E_exact| <= sum_j (|h_j| + |E_exact|) eps_j / sum_j w~_j.
    Returned per row of h_vals, in long double arithmetic (weights on the 2^41 scale of fixed_point_weights)."""
    h = _rows(h_vals, st["n"])
    tix = st["tix"]
    wq = fixed_point_weights(st)
    s = st["s"].astype(LD)[tix]
    d1 = np.abs(st["logw"] - st["mb"][tix]).astype(LD)
    d2 = np.abs(st["mb"] - st["m"]).astype(LD)[tix]
    eps = s * LD(0.5) + wq * (LD(U) * (d1 + d2) + LD(2.0 ** -50)) + st["q"].astype(LD) * LD(2.0) ** -1074
    under = st["s"][tix] == 0.0
    if under.any():
        eps = np.where(under, exact_weights(st), eps)
    den = pairwise_sum(wq)
    e_exact = expect_exact_weights(h, st) if e_exact is None else e_exact
    return np.array([float(pairwise_sum((np.abs(row).astype(LD) + abs(e)) * eps) / den) for row, e in zip(h, e_exact)])


def weights_ref(oracle, st):
    """What weights() hands out: q_j exp(m_b - m) 2^-41, as doubles (the product rounds once)."""
    return st["q"].astype(np.float64) * (st["s"] * 2.0 ** -TILE_SHIFT)[st["tix"]]


# ---- swarm means ----------------------------------------------------------------------------------------------------------------
def effective_threads(R, num_threads):
    """k_swarm_means: num_threads <= 0 is the plain mean (0); more threads than members leaves the surplus threads without a member,
    and the reference pool averages over the threads that have one: T = R."""
    return 0 if num_threads <= 0 else min(int(num_threads), int(R))


def swarm_means_ref(rows, num_threads):
    """rows: [n, R] per-member values.  Returns (plain mean, the reference pool's mean of per-thread means) per row in long double:
    member i runs on thread i % T, every thread averages its members, the thread averages are averaged."""
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows[None, :] if rows.ndim == 1 else rows
    R = rows.shape[1]
    T = effective_threads(R, num_threads)
    plain = np.array([pairwise_sum(r) / LD(R) for r in rows], dtype=LD)
    if T == 0:
        return plain, plain
    pooled = np.array([pairwise_sum(np.array([pairwise_sum(r[j::T]) / LD(len(r[j::T])) for j in range(T)], dtype=LD)) / LD(T) for r in rows], dtype=LD)
    return plain, pooled


def budget_swarm(R, rows):
    """k_swarm_means' tree: each member's value is divided by its thread's member count (1 rounding; pooled form only), added in a
    chain of ceil(R / 256) adds, 6 butterfly levels and 3 wave adds, and the total divided once: k = ceil(R / 256) + 11.  Bound:
    gamma_k mean |v| (every weight is <= 1 / T / members, so the absolute sum is at most max over the weightings <= max_t mean_t |v|,
    bounded here by max |v|)."""
    k = -(-R // 256) + 11
    rows = np.abs(np.asarray(rows, dtype=np.float64))
    rows = rows[None, :] if rows.ndim == 1 else rows
    return (k * U / (1.0 - k * U)) * rows.max(axis=1)
