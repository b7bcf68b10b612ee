"""A Python restatement of backward-simulation smoothing (include/ssme_pf.h: ssme_pf_sample_trajectories_backward; DESIGN.md section
12.1; ssme_amd/csrc/backward.h), written from its definition.  It works from what the STEP API exposes: a twin handle stepped under
set_debug(record_ancestors, keep_logw) is downloaded after every step -- the pre-resampling population x_t, its log-weights lw_t and
the ancestors of the step's draw (stepped_history) -- and the backward pass is restated here:

    B_{T-1} given;  for t = T-2 .. 0, x~ = x_{t+1}[B_{t+1}]:
        a_i = lw_t[i] + logf(x~ | x_t[i], z_{t+1})   (NaN -> -inf),   m = max a_i,
        q_i = quantize(a_i - m, sh),  sh = min(41, 52 - ceil(log2 N)),   S = sum q_i,  C_i = q_0 + .. + q_i   (integers: exact),
        u = u01_mid40(words 0-1 of Philox(k, t, filter id, 165)),  target = ceil(u S),  B_t = the first i with C_i >= target;
        m not finite or S not > 0:  B_t = anc_{t+1}[B_{t+1}] where step t + 1 resampled, B_{t+1} otherwise.

Device bits come from the oracle alone (exp_t for the leverage model's mean, quantize for the weights, philox for the uniform); the
sums are integers (numpy uint64, or Python ints in brute_force).  brute_force() evaluates one draw with Fractions and shares only the
quantised weights with the restatement.  Every function takes the oracle module as `O`."""
from fractions import Fraction
import math

import numpy as np

from forecast_ref import philox_rows, u01_mid40
from smooth_ref import resampled

STREAM_BSIM = 165
TILE_SHIFT = 41
MODEL_SVOL, MODEL_SVOL_LEVERAGE, MODEL_LIN_GAUSS = 0, 1, 2
G = 4                                      # trajectories per workgroup of k_bsim (kBsimG): where the tests put their K edges


def shift_of(n):
    """sh = min(41, 52 - ceil(log2 N)): N weights of at most 2^sh sum to less than 2^53."""
    return min(TILE_SHIFT, 52 - (int(n) - 1).bit_length())


# ---- transition log-densities, in the operation order of the device functions ------------------------------------------------------
def logf_builtin(O, model, th):
    """logf(xn[1], x[1, N], z) of a built-in model with untransformed parameters th (model_logf of csrc/pf_kernels.h)."""
    th = [float(v) for v in th]
    if model == MODEL_SVOL_LEVERAGE:
        phi, mu, sigma, rho = th
        sd = sigma * np.sqrt(1.0 - phi * phi)
        a4 = rho * sigma

        def f(xn, x, z):
            e = O.exp_t(-0.5 * x[0])
            mean = (mu + phi * (x[0] - mu)) + (a4 * float(z)) * e
            d = (xn[0] - mean) / sd
            return -0.5 * (d * d)
        return f
    phi, sigma = (th[1], th[2]) if model == MODEL_SVOL else (th[0], th[1])

    def f(xn, x, z):
        d = (xn[0] - phi * x[0]) / sigma
        return -0.5 * (d * d)
    return f


def logf_student_t_f(O, th):
    """tests/models/svol_student_t_f.h: theta = (beta, phi, sigma, nu)."""
    return logf_builtin(O, MODEL_SVOL, th[:3])


def logf_two_factor_f(O, th):
    """tests/models/svol_two_factor_f.h: theta = (beta, phi1, phi2, sigma1, sigma2, rho)."""
    _, phi1, phi2, s1, s2, rho = [float(v) for v in th]
    a3, a4 = s2 * rho, s2 * np.sqrt(1.0 - rho * rho)

    def f(xn, x, z):
        e1 = (xn[0] - phi1 * x[0]) / s1
        e2 = ((xn[1] - phi2 * x[1]) - a3 * e1) / a4
        return -0.5 * (e1 * e1 + e2 * e2)
    return f


def logf_reg_cov_f(O, th):
    """tests/models/svol_reg_cov_f.h: theta = (phi, mu, sigma, b0, b2, g); z = the three covariates of the step that made xn."""
    phi, mu, sigma, _, _, g = [float(v) for v in th]

    def f(xn, x, z):
        mean = (mu + phi * (x[0] - mu)) + g * float(z[1])
        d = (xn[0] - mean) / sigma
        return -0.5 * (d * d)
    return f


# ---- the history of a stepped twin -------------------------------------------------------------------------------------------------
def stepped_history(bank, y, z=None):
    """Steps `bank` (parameters set, fresh) through the series under set_debug(record_ancestors, keep_logw) and downloads every filter
    after every step: dict(xs=[R][T] populations [dim_x, N], lws=[R][T] log-weights, ancs=[R][T] ancestors)."""
    R, T = bank.r, len(y)
    bank.set_debug(record_ancestors=True, keep_logw=True)
    xs = [[None] * T for _ in range(R)]
    lws = [[None] * T for _ in range(R)]
    ancs = [[None] * T for _ in range(R)]
    for t in range(T):
        bank.step(y[t], None if z is None else z[t])
        for f in range(R):
            st = bank.state(f, ancestors=True)
            xs[f][t] = np.atleast_2d(np.asarray(st["x"], dtype=np.float64)).copy()
            lws[f][t] = np.asarray(st["logw"], dtype=np.float64).copy()
            ancs[f][t] = np.asarray(st["anc"]).astype(np.int64).copy()
    return dict(xs=xs, lws=lws, ancs=ancs)


# ---- the backward pass -------------------------------------------------------------------------------------------------------------
def backward_weights(O, logf, xn, x_t, lw_t, z_next, sh):
    """(q[N] uint64, m) of one draw; q is None where the transition is degenerate (m not finite)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = np.asarray(lw_t, dtype=np.float64) + logf(xn, x_t, z_next)
        a = np.where(np.isnan(a), -np.inf, a)
        m = float(np.max(a))
        if not np.isfinite(m):
            return None, m
        return O.quantize(a - m, sh), m


def draw_uniform(k, t, rep, seed):
    w = philox_rows(None, np.array([k]), t, rep, STREAM_BSIM, seed)
    return float(u01_mid40(w[:, 0], w[:, 1])[0])


def select(q, u):
    """The first i with C_i >= ceil(u S), or None where S is not > 0.  uint64 sums: exact."""
    C = np.cumsum(np.asarray(q, dtype=np.uint64))
    S = int(C[-1])
    if not S > 0:
        return None
    target = int(np.ceil(u * float(S)))
    return int(np.searchsorted(C, np.uint64(target), side="left"))


def backward_filter(O, logf, xs, lws, ancs, sched, terminal, seed, rep, zs=None, k0=0):
    """One filter: (B [K, T] int64, X [K, T, dim_x], fallbacks).  xs / lws / ancs: [T] downloads; terminal: [K] final indices;
    zs: [T] covariates (a float or an array per step) or None: zeros; trajectory k uses counter k0 + k."""
    T, n = len(xs), xs[0].shape[1]
    sh = shift_of(n)
    K = len(terminal)
    B = np.empty((K, T), dtype=np.int64)
    fallbacks = 0
    for k in range(K):
        b = min(int(terminal[k]), n - 1)
        B[k, T - 1] = b
        for t in range(T - 2, -1, -1):
            zn = 0.0 if zs is None else zs[t + 1]
            q, _ = backward_weights(O, logf, xs[t + 1][:, b], xs[t], lws[t], zn, sh)
            nb = None if q is None else select(q, draw_uniform(k0 + k, t, rep, seed))
            if nb is None:
                fallbacks += 1
                nb = int(ancs[t + 1][b]) if resampled(t + 1, sched) else b
            b = min(nb, n - 1)
            B[k, t] = b
    X = np.stack([np.stack([xs[t][:, B[k, t]] for t in range(T)]) for k in range(K)])
    return B, X, fallbacks


def reference(O, logf_of_filter, hist, sched, terminal, seed, first_filter=0, zs=None):
    """All filters of a stepped_history(): (X [R, K, T, dim_x], B [R, K, T] uint32, fallbacks).  terminal: [R, K]."""
    Xs, Bs, fb = [], [], 0
    for f in range(len(hist["xs"])):
        B, X, n = backward_filter(O, logf_of_filter(f), hist["xs"][f], hist["lws"][f], hist["ancs"][f], sched, terminal[f], seed,
                                  first_filter + f, zs)
        Xs.append(X); Bs.append(B); fb += n
    return np.stack(Xs), np.stack(Bs).astype(np.uint32), fb


# ---- one draw, exactly -------------------------------------------------------------------------------------------------------------
def brute_force(q, u, a=None, sh=None):
    """The index of one draw by rational arithmetic alone: target = ceil of the correctly rounded double of the exact product u S,
    then the first i whose exact inclusive sum reaches it.  With a (the a_i) and sh: also asserts that every q_i is the quantised
    weight, |q_i 2^-sh - exp(a_i - m)| <= 2^-(sh+1) + 2^-50 (the rounding to an integer plus the exponential's own error)."""
    q = [int(v) for v in q]
    S = sum(q)
    if not S > 0:
        return None
    target = math.ceil(float(Fraction(u) * S))
    acc = Fraction(0)
    pick = None
    for i, v in enumerate(q):
        acc += v
        if pick is None and acc >= target:
            pick = i
    assert pick is not None
    if a is not None:
        m = max(a)
        for v, ai in zip(q, a):
            w = 0.0 if ai == -math.inf else math.exp(ai - m)
            assert abs(v * 2.0 ** -sh - w) <= 2.0 ** -(sh + 1) + 2.0 ** -50, (v, ai, m)
    return pick
