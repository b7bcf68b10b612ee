"""A numpy restatement of the forecast (include/ssme_pf.h: ssme_pf_sim_future_obs, ssme_lw_sim_future_obs),
written from its definition: the start draw from the integer weight cdf, then per horizon "propagate, then observe"
(include/ssme/liu_west_filter.h:1330-1360 of the reference).  No device code; the CPU tests (test_forecast_cpu.py) and the GPU
tests (test_forecast_gpu.py) share it.

Only the oracle's exported primitives are used: philox, log_u, sincos_k24, exp_t, exp, rescale, quantize.  u01_mid40 and the
inverse parameter transforms are restated here in a few lines of numpy.  Every function takes the oracle module as `O`.

Counters: (particle, t0, filter id, stream + (k << 8)) with t0 = steps done so far, k = horizon; streams 160 (start draw),
161 (bootstrap horizons: words 0-1 -> (z_state, z_obs)), 162 / 163 (Liu-West horizons: the four jitter normals / (z_state, z_obs)).
"""
import ctypes as C

import numpy as np

TILE_SHIFT = 41
STREAM_START, STREAM_SIM, STREAM_LW_JIT, STREAM_LW_SIM = 160, 161, 162, 163
MODEL_SVOL, MODEL_SVOL_LEVERAGE, MODEL_LIN_GAUSS = 0, 1, 2
TR_NULL, TR_TWICE_FISHER, TR_LOGIT, TR_LOG = 0, 1, 2, 3


# ---- random numbers ---------------------------------------------------------------------------------------------------------------
def philox_rows(O, c0, c1, c2, c3, seed):
    """Philox4x32-10 of the counters (c0[i], c1, c2, c3) under the key (seed lo, seed hi): [n, 4] uint32 (one oracle call each)."""
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
    for bb in np.unique(b):
        sel = b == bb
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


def forecast_lw(O, st, start, prop, transforms, delta, n, seed, rep, t0, H, last_obs):
    """(x[H, n], y[H, n]) of one Liu-West filter given its start population `start` and prop = (theta-bar[4], L[10]: the lower
    triangle by rows) as the device used them.  st: x[n], theta[4, n] (transformed) of the last step.  Per horizon, in the order
    of the filter's second stage (liu_west_filter.h:1024-1027, fSamp of test/test_liu_west.cpp:114-121)."""
    a = (3.0 * delta - 1.0) / (2.0 * delta)
    tb = np.asarray(prop[:4], dtype=np.float64)
    L = np.zeros((4, 4))
    L[np.tril_indices(4)] = np.asarray(prop[4:14], dtype=np.float64)
    start = np.asarray(start).astype(np.int64)
    x = np.asarray(st["x"], dtype=np.float64)[start]
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
            yp = zo * O.exp_t(0.5 * x)
            xs[k], ys[k] = x, yp
    return xs, ys
