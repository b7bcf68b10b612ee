"""A numpy restatement of the forecast (include/ssme_pf.h: ssme_pf_sim_future_obs, ssme_lw_sim_future_obs),
written from its definition: the start draw from the integer weight cdf, then per horizon "propagate, then observe"
(include/ssme/liu_west_filter.h:1330-1360 of the reference).  No device code; the CPU tests (test_forecast_cpu.py) and the GPU
tests (test_forecast_gpu.py) share it.

Independent of that restatement (and of each other): start_interval_check, an exact reference of the start draw that never forms the
two-level quantities, and moment_anchors, analytic moments of the outputs with libm only (tests/fc_edge_cases.py lists where they run).

Only the oracle's exported primitives are used: philox, log_u, sincos_k24, exp_t, exp, rescale, quantize.  u01_mid40 and the
inverse parameter transforms are restated here in a few lines of numpy.  Every function takes the oracle module as `O`.

Counters: (particle, t0, filter id, stream + (k << 8)) with t0 = steps done so far, k = horizon; streams 160 (start draw),
161 (bootstrap horizons: words 0-1 -> (z_state, z_obs)), 162 / 163 (Liu-West horizons: the four jitter normals / (z_state, z_obs)).
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from expect_ref import FRACTION_MAX_N, LD, U

TILE_SHIFT = 41
REF_EPS = 2.0 ** -60                 # start_interval_check: the long-double evaluation of F above FRACTION_MAX_N particles
STREAM_START, STREAM_SIM, STREAM_LW_JIT, STREAM_LW_SIM = 160, 161, 162, 163
MODEL_SVOL, MODEL_SVOL_LEVERAGE, MODEL_LIN_GAUSS = 0, 1, 2
TR_NULL, TR_TWICE_FISHER, TR_LOGIT, TR_LOG = 0, 1, 2, 3


# ---- random numbers ---------------------------------------------------------------------------------------------------------------
def philox_rows_oracle(O, c0, c1, c2, c3, seed):
    """Philox4x32-10 of the counters (c0[i], c1, c2, c3) under the key (seed lo, seed hi): [n, 4] uint32, one oracle call each.
    Kept to pin philox4x32_10 below (test_fc_edges_cpu.py); everything else uses the numpy form."""
    c0 = np.asarray(c0, dtype=np.uint32)
    fn = O.lib().orc_philox4x32_10
    ctr = (C.c_uint32 * 4)(0, int(c1) & 0xffffffff, int(c2) & 0xffffffff, int(c3) & 0xffffffff)
    key = (C.c_uint32 * 2)(int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff)
    out = (C.c_uint32 * 4)()
    res = np.empty((c0.size, 4), dtype=np.uint32)
    for i, v in enumerate(c0.tolist()):
        ctr[0] = v
        fn(ctr, key, out)
        res[i] = out[:]
    return res


_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_LO32, _SH32 = np.uint64(0xffffffff), np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC 2011) over arrays of counters: [n, 4] uint32.  Every counter word may be an array or a
    scalar; the key is one pair.  Words are held in uint64 so that the 32 x 32 products are exact."""
    c = [np.array(v, dtype=np.uint64).ravel() & _LO32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    for _ in range(10):
        p0, p1 = c[0] * _PHILOX_M0, c[2] * _PHILOX_M1
        c = [(p1 >> _SH32) ^ c[1] ^ np.uint64(k0), p1 & _LO32, (p0 >> _SH32) ^ c[3] ^ np.uint64(k1), p0 & _LO32]
        k0, k1 = (k0 + _PHILOX_W0) & 0xffffffff, (k1 + _PHILOX_W1) & 0xffffffff
    return np.stack(c, axis=1).astype(np.uint32)


def philox_rows(O, c0, c1, c2, c3, seed):
    """Philox4x32-10 of the counters (c0[i], c1, c2, c3) under the key (seed lo, seed hi): [n, 4] uint32.  Vectorised; O is unused
    and kept for the callers' signature (test_fc_edges_cpu.py pins philox4x32_10 to the oracle's)."""
    return philox4x32_10(np.asarray(c0, dtype=np.uint64), int(c1) & 0xffffffff, int(c2) & 0xffffffff, int(c3) & 0xffffffff,
                         int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff)


def u01_mid40(w0, w1):
    """Midpoints of the 2^-40 grid, strictly inside (0, 1): the 32 bits of w0 and the top 8 bits of w1."""
    k = (np.asarray(w0, dtype=np.uint64) << np.uint64(8)) | (np.asarray(w1, dtype=np.uint64) >> np.uint64(24))
    return 1.0 - (k.astype(np.float64) * 2.0 + 1.0) * 2.0 ** -41         # = 2 - (1 + k 2^-40 + 2^-41), every step exact


def pair_normals(O, w0, w1):
    """Box-Muller pair of the hot loops: radius from the 40-bit uniform (table log), angle 2 pi k / 2^24 from the low 24 bits of w1."""
    rad = np.sqrt(-2.0 * O.log_u(u01_mid40(w0, w1)))
    sn, cs = O.sincos_k24((np.asarray(w1, dtype=np.uint32) & np.uint32(0x00ffffff)).astype(np.float64))
    return rad * cs, rad * sn


# ---- the start draw ---------------------------------------------------------------------------------------------------------------
def level2(O, A, mb, rshift):
    """The resampler's level-2 quantities: rescaled tile sums A'_b = rint(A_b exp(m_b - m) 2^(rshift - 41)), their inclusive sums
    T_b, S = T_{B-1} and ratio_b = A_b / A'_b.  m = the maximum of the tile maxima (NaN propagating)."""
    A = np.asarray(A, dtype=np.uint64)
    mb = np.asarray(mb, dtype=np.float64)
    m = np.max(mb)
    with np.errstate(invalid="ignore", divide="ignore"):
        Ap = O.rescale(A, mb - m, int(rshift) - TILE_SHIFT)
        T = np.cumsum(Ap.astype(np.float64))                       # exact: integers below 2^53
        ratio = A.astype(np.float64) / Ap.astype(np.float64)
    return Ap, T, float(T[-1]), ratio


def tile_of_target(T, target):
    """b = min(#{j < B : T_j < target}, B - 1)."""
    return np.minimum(np.searchsorted(T, target, side="left"), T.size - 1)


def start_from_uniforms(u, cdf, T, S, ratio, n, tile):
    """Ancestors of the uniforms u (the two-level search of the step kernel's general path).  cdf: tile-local inclusive integer
    sums of the n particles."""
    cdf = np.asarray(cdf).astype(np.float64)
    if not S > 0:
        return np.zeros(u.size, dtype=np.uint32)
    target = np.ceil(u * S)
    b = tile_of_target(T, target)
    Pb = np.where(b > 0, T[np.maximum(b - 1, 0)], 0.0)
    tloc = np.ceil((target - Pb) * ratio[b])
    anc = np.empty(u.size, dtype=np.int64)
    order = np.argsort(b, kind="stable")                               # one slice per chosen tile (a mask per tile is B passes over u)
    bs = b[order]
    tiles, first = np.unique(bs, return_index=True)
    for bb, lo, hi in zip(tiles.tolist(), first.tolist(), first.tolist()[1:] + [bs.size]):
        sel = order[lo:hi]
        c = cdf[bb * tile:min((bb + 1) * tile, n)]
        j = np.minimum(np.searchsorted(c, tloc[sel], side="left"), tile - 1)     # #{q : cdf_b[q] < tloc}; the search stops at tile - 1
        anc[sel] = bb * tile + j
    return np.minimum(anc, n - 1).astype(np.uint32)


def start_draw(O, st, n, tile, seed, rep, t0):
    """(ancestors[n], alive) of one filter from its downloaded state: cdf (tile-local integer sums), A (tile sums), mb (tile
    maxima), rshift.  alive = S > 0; a filter without weight gets ancestors 0 and NaN samples."""
    _, T, S, ratio = level2(O, st["A"], st["mb"], st["rshift"])
    w = philox_rows(O, np.arange(n), t0, rep, STREAM_START, seed)
    return start_from_uniforms(u01_mid40(w[:, 0], w[:, 1]), st["cdf"], T, S, ratio, n, tile), bool(S > 0)


# ---- bootstrap models -------------------------------------------------------------------------------------------------------------
def bs_prop(O, model, th, x, zs, y_prev):
    """fSamp in the filter's operation order.  th: untransformed parameters as the C ABI takes them."""
    if model == MODEL_SVOL_LEVERAGE:                                # test/test_pswarm.cpp:90-97
        phi, mu, sigma, rho = th
        sd = sigma * np.sqrt(1.0 - phi * phi)
        e = O.exp_t(-0.5 * x)
        mean = (mu + phi * (x - mu)) + ((rho * sigma) * y_prev) * e
        return mean + zs * sd
    phi, sigma = (th[1], th[2]) if model == MODEL_SVOL else (th[0], th[1])
    return phi * x + zs * sigma


def bs_gsamp(O, model, th, x, zo):
    if model == MODEL_LIN_GAUSS:
        return x + th[2] * zo
    e = O.exp_t(0.5 * x)
    return (th[0] * e) * zo if model == MODEL_SVOL else e * zo     # leverage: test/test_pswarm.cpp:112-116


def forecast_bs(O, model, theta, st, n, tile, seed, rep, t0, H, last_obs=0.0, f32=False):
    """(start[n], x[H, n], y[H, n]) of one bootstrap filter.  st: the device's own download of the filter (state())."""
    th = np.asarray(theta, dtype=np.float64)
    if f32:
        th = th.astype(np.float32).astype(np.float64)
        last_obs = float(np.float32(last_obs))
    start, alive = start_draw(O, st, n, tile, seed, rep, t0)
    xs, ys = np.full((H, n), np.nan), np.full((H, n), np.nan)
    if alive:
        with np.errstate(invalid="ignore", over="ignore"):
            x = np.asarray(st["x"], dtype=np.float64)[start]
            yp = np.full(n, float(last_obs))
            for k in range(H):
                w = philox_rows(O, np.arange(n), t0, rep, STREAM_SIM + (k << 8), seed)
                zs, zo = pair_normals(O, w[:, 0], w[:, 1])
                x = bs_prop(O, model, th, x, zs, yp)
                yp = bs_gsamp(O, model, th, x, zo)
                xs[k], ys[k] = x, yp
    if f32:
        xs, ys = xs.astype(np.float32).astype(np.float64), ys.astype(np.float32).astype(np.float64)
    return start, xs, ys


# ---- Liu-West ---------------------------------------------------------------------------------------------------------------------
def tr_inv(O, kind, tp):
    """Inverse parameter transforms (include/ssme/parameters.h: null, twice_fisher, logit, log) in the filter's form: one
    exp(-|tp|) serves both signs -- logit: (tp >= 0 ? 1 : t) / (1 + t); twice_fisher: q = 2 / (1 + t), tp >= 0 ? q - 1 : 1 - q."""
    tp = np.asarray(tp, dtype=np.float64)
    if kind == TR_NULL:
        return tp
    if kind == TR_LOG:
        return O.exp_t(tp)
    pos = tp >= 0.0
    t = O.exp_t(np.where(pos, -tp, tp))
    den = 1.0 + t
    if kind == TR_LOGIT:
        return np.where(pos, 1.0, t) / den
    q = 2.0 / den
    return np.where(pos, q - 1.0, 1.0 - q)


def forecast_lw(O, st, start, prop, transforms, delta, n, seed, rep, t0, H, last_obs, alive=True):
    """(x[H, n], y[H, n]) of one Liu-West filter given its start population `start` and prop = (theta-bar[4], L[10]: the lower
    triangle by rows) as the device used them.  st: x[n], theta[4, n] (transformed) of the last step.  Per horizon, in the order
    of the filter's second stage (liu_west_filter.h:1024-1027, fSamp of test/test_liu_west.cpp:114-121)."""
    a = (3.0 * delta - 1.0) / (2.0 * delta)
    tb = np.asarray(prop[:4], dtype=np.float64)
    L = np.zeros((4, 4))
    L[np.tril_indices(4)] = np.asarray(prop[4:14], dtype=np.float64)
    start = np.asarray(start).astype(np.int64)
    x = np.asarray(st["x"], dtype=np.float64)[start] if alive else np.full(n, np.nan)       # a filter without weight: NaN states
    th = np.asarray(st["theta"], dtype=np.float64)[:, start].copy()
    yp = np.full(n, float(last_obs))
    xs, ys = np.empty((H, n)), np.empty((H, n))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(H):
            wj = philox_rows(O, np.arange(n), t0, rep, STREAM_LW_JIT + (k << 8), seed)
            e = pair_normals(O, wj[:, 0], wj[:, 1]) + pair_normals(O, wj[:, 2], wj[:, 3])
            tu = []
            for d in range(4):
                m = a * th[d] + (1.0 - a) * tb[d]
                acc = np.zeros(n)
                for c in range(d + 1):
                    acc = acc + L[d, c] * e[c]
                th[d] = m + acc
                tu.append(tr_inv(O, transforms[d], th[d]))
            ws = philox_rows(O, np.arange(n), t0, rep, STREAM_LW_SIM + (k << 8), seed)
            zs, zo = pair_normals(O, ws[:, 0], ws[:, 1])
            mean = (tu[1] + tu[0] * (x - tu[1])) + ((yp * tu[3]) * tu[2]) * O.exp_t(-0.5 * x)
            x = mean + zs * (tu[2] * np.sqrt(1.0 - tu[3] * tu[3]))
            yp = zo * O.exp_t(0.5 * x) if alive else np.full(n, np.nan)
            xs[k], ys[k] = x, yp
    return xs, ys


# ---- an exact reference of the start draw ----------------------------------------------------------------------------------------
def _fraction_of_ld(v):
    """A long double as the rational it is."""
    m, e = np.frexp(LD(v))
    t = m * LD(2.0 ** 32)
    hi = np.floor(t)
    lo = (t - hi) * LD(2.0 ** 32)
    return Fraction((int(hi) << 32) | int(lo)) * Fraction(2) ** (int(e) - 64)


def _ld_of_fraction(f):
    hi = float(f)
    return LD(hi) + LD(float(f - Fraction(hi)))


def start_interval_check(q, mb, rshift, tile, u, anc):
    """Is `anc` a draw from the weights by the uniforms u?  Independent of the two-level search: no A', T', S' or ratio is formed.

    Weights.  w_j = q_j s_b with s_b = exp(m_b - m), m = max_b m_b, b = the tile of j; W_b = A_b s_b the tile sums, W their sum,
    F(a) = sum_{j <= a} w_j / W the normalised inclusive cdf.  s_b is taken in 80-bit long double (relative error below 2^-62
    with the rounded difference); the tile sums, their prefixes and W are then EXACT rationals; F(a) = (prefix_b + C_a s_b) / W,
    C_a the tile-local integer cdf, is evaluated exactly (Fraction) up to expect_ref.FRACTION_MAX_N particles and in long
    double above (three roundings of 2^-64: REF_EPS = 2^-60 covers them).

    The claim, for every particle i with ancestor a:   F(a - 1) - beta  <  u_i  <=  F(a) + beta,   no exceptions.

    beta, from the code (fc_draw_ancestor of csrc/forecast.h, k_level2_plan of csrc/pf_kernels.h).  With K = 2^(rshift - 41):
        A'_b = rint(fl(A_b e_b) K),  e_b = exp_t(fl(m_b - m))           so  |A'_b - K W_b| <= 1/2 + K W_b eta_b,
        eta_b = 2^-51 (exp_t within 2 ulp, as loglik_ref.py states it) + u |m_b - m| (the rounded argument) + u (the product)
                + 2^-62 + 2^-64 |m_b - m| (the reference's own s_b);
        a tile with K W_b < 1/4 has A'_b = 0 whatever its eta_b (a subnormal or zero e_b included): its whole K W_b is inside the 1/2.
        eta = the largest eta_b of the other tiles.
    Hence P_b = T'_{b-1} = K prefix_b (1 +- eta) +- b / 2 and S' = K W (1 +- eta) +- B / 2: one rint per tile, at most B / 2
    units; write d = eta + B / (2 K W), so that K W (1 - d) <= S' <= K W (1 + d).
        target = ceil(fl(u S')):    u S' (1 - u) <= target < u S' (1 + u) + 1                      (the first ceil: one unit)
        tile b:  P_b < target <= P_b + A'_b, tau = target - P_b exact (integers below 2^53)
        tloc = ceil(v), v = fl(tau fl(A_b / A'_b)) = tau A_b / A'_b (1 + e2), |e2| <= 2u + u^2    (the division and the product)
        j = #{cdf_b < tloc}:  C_{a-1} < tloc <= C_a; the C are integers, so C_{a-1} < v <= C_a       (the second ceil costs nothing;
              where the count stops at tile - 1 or the index at N - 1, tau <= A'_b gives tau A_b / A'_b <= A_b = C_a exactly)
    Upper side: tau <= C_a A'_b / A_b (1 + e2'), so
        u S' (1 - u) <= P_b + (C_a / A_b) A'_b (1 + e2') <= K W F(a) (1 + eta + e2') + B / 2 (1 + e2')
        u - F(a) <= ((eta + e2' + u) + d) / (1 - d) + (B / 2) / (K W (1 - d)).
    Lower side: tau > C_{a-1} A'_b / A_b (1 - e2'), u S' (1 + u) > target - 1, the same terms with one more unit:
        F(a - 1) - u < ((eta + e2' + u) + d) / (1 - d) + (B / 2 + 1) / (K W (1 - d)).
    beta = ((eta + 4u) + d) / (1 - d) + (B / 2 + 1) (1 + 4u) / (K W (1 - d)) + REF_EPS.

    Teeth, from the reference alone: a* = the exact inverse of F at u_i.  Replacing a* by the nearest index of positive weight
    below it is rejected iff u_i - F(a* - 1) > beta, above it iff F(a*) - u_i >= beta; `teeth` = the share of particles for
    which both replacements (where such an index exists) are rejected.

    Returns dict(beta, ratio = the largest violation / beta (<= 0: none is near its edge), bad = particles outside, teeth)."""
    q = np.asarray(q).astype(np.int64)
    mb = np.asarray(mb, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    anc = np.asarray(anc).astype(np.int64)
    n, B = q.size, mb.size
    assert B == -(-n // tile) and u.size == n and anc.size == n and (q >= 0).all()
    m = float(np.max(mb))
    assert np.isfinite(m), "no weight: there is no draw to check"
    starts = np.arange(0, n, tile)
    tix = np.arange(n) // tile
    A = np.add.reduceat(q, starts)
    Cg = np.cumsum(q)
    C = Cg - np.concatenate([[0], Cg[starts[1:] - 1]])[tix]             # tile-local inclusive integer cdf
    with np.errstate(all="ignore"):
        dm = mb.astype(LD) - LD(m)
        s = np.where(np.isfinite(mb), np.exp(dm), LD(0))
    sf = [_fraction_of_ld(v) for v in s]
    Wb = [int(a) * f for a, f in zip(A, sf)]
    pre, acc = [], Fraction(0)
    for w in Wb:
        pre.append(acc)
        acc += w
    W = acc
    assert W > 0
    K = Fraction(2) ** (int(rshift) - TILE_SHIFT)
    KW = float(K * W)
    live = np.array([K * w >= Fraction(1, 4) for w in Wb])
    adm = np.abs(mb[live] - m)
    eta = float(np.max(2.0 ** -51 + U * (adm + 1.0) + 2.0 ** -62 + 2.0 ** -64 * adm))
    d = eta + B / (2.0 * KW)
    assert d < 0.25, d
    beta = ((eta + 4.0 * U) + d) / (1.0 - d) + (B / 2.0 + 1.0) * (1.0 + 4.0 * U) / (KW * (1.0 - d)) + REF_EPS
    preW = np.array([_ld_of_fraction(p / W) for p in pre], dtype=LD)
    sW = np.array([_ld_of_fraction(f / W) for f in sf], dtype=LD)
    Fhi_all = preW[tix] + C.astype(LD) * sW[tix]                         # F(j) of every particle, long double
    Flo_all = preW[tix] + (C - q).astype(LD) * sW[tix]                   # F(j - 1): the zero-weight run below j adds nothing
    uL = u.astype(LD)
    if n <= FRACTION_MAX_N:
        bf = Fraction(beta)
        viol = Fraction(-1)
        bad = 0
        for ui, a in zip(u.tolist(), anc.tolist()):
            b = a // tile
            lo = (pre[b] + int(C[a] - q[a]) * sf[b]) / W
            hi = (pre[b] + int(C[a]) * sf[b]) / W
            uf = Fraction(ui)
            v = max(lo - uf, uf - hi)
            viol = max(viol, v)
            bad += not (lo - bf < uf <= hi + bf)
        ratio = float(viol / bf)
    else:
        v = np.maximum(Flo_all[anc] - uL, uL - Fhi_all[anc])
        ratio = float(v.max() / LD(beta))
        bad = int(np.count_nonzero(~((Flo_all[anc] - LD(beta) < uL) & (uL <= Fhi_all[anc] + LD(beta)))))
    # teeth
    pos = np.flatnonzero(q > 0)
    Fp = Fhi_all[pos]
    by_u = np.argsort(u)                                                 # sorted needles: the search walks the array once
    k = np.empty(n, dtype=np.int64)
    k[by_u] = np.minimum(np.searchsorted(Fp.astype(np.float64), u[by_u], side="left"), pos.size - 1)   # a* = pos[k]: the first F >= u.  The
    for _ in range(64):                                                  # double search is a step or two off at most; settle in long double
        down = (k > 0) & (Fp[np.maximum(k - 1, 0)] >= uL)
        up = (k < pos.size - 1) & (Fp[k] < uL) & ~down
        if not (down.any() or up.any()):
            break
        k = k - down + up
    else:
        raise AssertionError("the inverse of F did not settle")
    below = (k == 0) | (uL - Flo_all[pos[k]] > LD(beta))
    above = (k == pos.size - 1) | (Fhi_all[pos[k]] - uL >= LD(beta))
    return dict(beta=beta, ratio=ratio, bad=bad, teeth=float(np.mean(below & above)))


def start_uniforms(n, seed, rep, t0):
    w = philox_rows(None, np.arange(n), t0, rep, STREAM_START, seed)
    return u01_mid40(w[:, 0], w[:, 1])


# ---- analytic moment anchors of the outputs (libm only) ---------------------------------------------------------------------------
def _z_var(v, var):
    """z-score of the sample variance of iid normals against `var`: its standard error is var sqrt(2 / (n - 1))."""
    return float((np.var(v, ddof=1) - var) / (var * np.sqrt(2.0 / (v.size - 1))))


def _z_mean(v, want=0.0):
    return float((np.mean(v) - want) / (np.std(v, ddof=1) / np.sqrt(v.size)))


def moment_anchors(model, theta, x, y, x_start=None, last_obs=0.0, w=None, xw=None):
    """[(name, z)]: every z is a statistic of the forecast's outputs x[H, n], y[H, n] (and, where given, the start states
    x_start[n] = state()["x"][start] and the filtered cloud (xw, w) = weights()) minus its analytic value, in standard errors;
    |z| <= 5 is required of each.  The particles of a forecast are independent draws given the filtered cloud (iid ancestors,
    a counter of its own per particle), so the standard errors are those of iid samples.
      linear Gaussian (phi, sigma, tau):  Var(y_k) - Var(x_k) = tau^2 (given x: variance 2 tau^4 / n + 4 tau^2 s_x^2 / n);
                                          x_{k+1} - phi x_k has variance sigma^2 (k = -1: from x_start);
      SVOL (beta, phi, sigma):            E[y_k^2] = beta^2 sum_i w_i exp(phi^(k+1) x_i + sigma^2 (1 - phi^(2(k+1))) / (2 (1 - phi^2)));
                                          y_k exp(-x_k / 2) / beta has mean 0 and variance 1;
      leverage (phi, mu, sigma, rho):     zo_k = y_k exp(-x_k / 2), r_k = x_{k+1} - mu - phi (x_k - mu) - rho sigma zo_k has mean 0,
                                          variance sigma^2 (1 - phi^2) and no correlation with zo_k (sqrt(n) corr ~ N(0, 1));
                                          k = -1: zo = last_obs exp(-x_start / 2)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    H, n = x.shape
    out = []
    if model == MODEL_LIN_GAUSS:
        phi, sigma, tau = theta
        for k in range(H):
            sx2 = np.var(x[k], ddof=1)
            se = np.sqrt((2.0 * tau ** 4 + 4.0 * tau * tau * sx2) / n)
            out.append((f"lg var(y)-var(x) k={k}", float((np.var(y[k], ddof=1) - sx2 - tau * tau) / se)))
        prev = x_start
        for k in range(H):
            if prev is not None:
                out.append((f"lg sd(x'-phi x) k={k}", _z_var(x[k] - phi * prev, sigma * sigma)))
            prev = x[k]
    elif model == MODEL_SVOL:
        beta, phi, sigma = theta
        for k in range(H):
            if w is not None:
                wn = np.asarray(w, dtype=np.float64) / np.sum(w)
                p = phi ** (k + 1)
                want = beta * beta * np.sum(wn * np.exp(p * np.asarray(xw) + 0.5 * sigma * sigma * (1.0 - p * p) / (1.0 - phi * phi)))
                out.append((f"svol E[y^2] k={k}", _z_mean(y[k] * y[k], want)))
            zo = y[k] * np.exp(-0.5 * x[k]) / beta
            out.append((f"svol sd(zo) k={k}", _z_var(zo, 1.0)))
            out.append((f"svol mean(zo) k={k}", _z_mean(zo)))
    else:
        phi, mu, sigma, rho = theta
        prev, zo = x_start, None if x_start is None else float(last_obs) * np.exp(-0.5 * x_start)
        for k in range(H):
            if prev is not None:
                r = x[k] - mu - phi * (prev - mu) - (rho * sigma) * zo
                out.append((f"lev mean(r) k={k}", _z_mean(r)))
                out.append((f"lev sd(r) k={k}", _z_var(r, sigma * sigma * (1.0 - phi * phi))))
                if np.std(zo) > 0:
                    out.append((f"lev corr(r,zo) k={k}", float(np.corrcoef(r, zo)[0, 1] * np.sqrt(n))))
            prev, zo = x[k], y[k] * np.exp(-0.5 * x[k])
    return out


def horizon_normals(O, i, t0, rep, k, seed, stream=STREAM_SIM):
    """(z_state, z_obs) of particles i at horizon k."""
    w = philox_rows(O, i, t0, rep, stream + (k << 8), seed)
    return pair_normals(O, w[:, 0], w[:, 1])
