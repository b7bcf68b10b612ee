"""An exact reference of the Liu-West parameter proposal, written from the reference library's definition
(update_parameter_proposal_components, liu_west_filter.h:1184-1198): theta-bar = sum_i theta_i / N,
V = sum_i theta_i theta_i^T / N - theta-bar theta-bar^T over the TRANSFORMED parameters, covariance (1 - a^2) V with
a = (3 delta - 1) / (2 delta) (:960), of which the filters take a square root (here: the Cholesky factor L).

Which population.  filter() calls update_parameter_proposal_components() first thing at every step t > 0 (:979), on
m_param_particles as the previous call left them: after its resampling when (t - 1 + 1) % m_rs == 0 (:1152-1153), untouched
otherwise.  Both implementations resample lazily at the start of step t, so with theta_{t-1} the parameters downloaded after step
t - 1 and anc_t the ancestors downloaded after step t, the population is theta_{t-1}[:, anc_t]; on a step of an m_rs > 1 schedule
that does not resample, anc_t is the identity and the population is theta_{t-1} itself.  population() is that one line.

Exact side.  Up to FRACTION_MAX_N particles every sum is exact: a double is an integer multiple of 2^-1074, so the 14 sums are
taken over Python integers and only the final quotients are Fractions.  Above, numpy.longdouble pairwise sums of the two-pass
(centred) covariance: depth <= 22 at 2^21 particles, 2^-64 per level plus the centring, products and quotient, below
REF_EPS = 2^-58 of sum |c_d c_e| / N <= S2_de + A_d A_e -- added to the budget.

Budget of the device's one-pass value, counted from the summation trees as they stand in csrc/lw_kernels.h (u = 2^-53,
gamma_k = k u / (1 - k u)):
  k_lw_stage1, one tile of 2048 particles: fold of the two tile halves (1 addition), of the pair (1), lw_row_tree14 (4 levels),
      the four DPP rows of a wave (2), the eight waves in order onto 0.0 (8)                                       = 16 additions
  the tile partials: lane l adds its ceil(B / 64) contiguous tiles in order onto 0.0, then wave_incl_scan_f64 (6 levels)
                                                                                                     = ceil(B / 64) + 6 additions
  All three moment paths add the partials in this one order -- the fused path in k_lw_stage2 (B <= 585: at most 10 + 6),
  k_lw_mom_totals before k_lw_mid<false> (586..1024 tiles: at most 16 + 6) and before k_lw_mid<true> (split level-2, up to
  16384 tiles: at most 256 + 6) -- so k_add(B) = 22 + ceil(B / 64) on the longest path of each: 32, 38 and 278 at most.
  A second moment has one more rounding (the product), then both are multiplied by invN = fl(1 / N) (2 roundings):
      |tb^_d - tb_d|   <= gamma_{k+2} A_d                          A_d = sum |theta_d| / N
      |M^_de - M_de|   <= gamma_{k+3} S2_de                        S2_de = sum |theta_d theta_e| / N
      |fl(tb^_d tb^_e) - tb_d tb_e| <= gamma_{2k+5} A_d A_e
  and the subtraction rounds once more, u (S2_de + A_d A_e)(1 + gamma): the cancellation term.  Together
      |V^_de - V_de| <= gamma_{2k+6} (S2_de + A_d A_e).
  (A_d A_e >= |tb_d| |tb_e| with equality for a parameter of one sign; it is what the rounding errors of the two means scale with.)
  h^ = fl(1 - fl(a a)) has |h^ - h2| <= u a^2 + u (h2 + u a^2) <= u (1 + u) because a^2 + h2 = 1, and the product h^ V^ rounds once:
      |S^_de - h2 V_de| <= (S2_de + A_d A_e) ((h2 + 2u) gamma_{2k+7} + 2u)  =: budget_S[d][e]
Factorisation.  Entry (i, j), j <= i, of the 4 x 4 Cholesky loop is S^_ij minus at most 3 products (3 multiplications, 3
subtractions), then one division by L_jj or one square root: 7 rounded operations, 8 with a square root allowed 1 ulp.  By the
standard argument (Higham, Accuracy and Stability, lemma 8.4) |S^_ij - sum_k L_ik L_jk| <= gamma_8 sum_k |L_ik| |L_jk| =: fact[i][j]:
a backward error, which needs no condition number."""
from fractions import Fraction

import numpy as np

import expect_ref as er

U = er.U
LD = er.LD
FRACTION_MAX_N = er.FRACTION_MAX_N
REF_EPS = 2.0 ** -58
FACT_OPS = 8
_SCALE = 1074                                  # every finite double times 2^1074 is an integer
_UP = 1.0 + 2.0 ** -40                         # the budgets themselves are evaluated in doubles: a few roundings, upwards


def gamma(k):
    return k * U / (1.0 - k * U)


def k_add(B):
    """Additions on the longest path of a moment total (module docstring): the same for the three paths."""
    return 16 + -(-int(B) // 64) + 6


def population(theta_prev, anc):
    """The population the moments of step t run over (module docstring): theta of step t - 1 indexed by step t's ancestors."""
    return np.asarray(theta_prev)[:, np.asarray(anc).astype(np.int64)]


def _ints(row):
    return [int(Fraction(float(v)) * (1 << _SCALE)) for v in row]


def exact_moments(pop, a):
    """pop: [4, N] doubles.  Returns dict(tb[4], S[4][4] = (1 - a^2) V, A[4], S2[4][4], exact) with tb and S exact Fractions when
    N <= FRACTION_MAX_N and long doubles above; A and S2 as doubles (rounded, used only inside budgets)."""
    pop = np.asarray(pop, dtype=np.float64)
    D, N = pop.shape
    A = np.abs(pop).astype(LD).sum(axis=1) / N
    S2 = np.array([[(np.abs(pop[d]).astype(LD) * np.abs(pop[e]).astype(LD)).sum() / N for e in range(D)] for d in range(D)])
    out = dict(A=A.astype(np.float64), S2=S2.astype(np.float64), exact=N <= FRACTION_MAX_N)
    if N <= FRACTION_MAX_N:
        rows = [_ints(pop[d]) for d in range(D)]
        one, two = 1 << _SCALE, 1 << (2 * _SCALE)
        tb = [Fraction(sum(r), one * N) for r in rows]
        h2 = 1 - Fraction(float(a)) ** 2
        S = [[None] * D for _ in range(D)]
        for d in range(D):
            for e in range(d + 1):
                m2 = Fraction(sum(p * q for p, q in zip(rows[d], rows[e])), two * N)
                S[d][e] = S[e][d] = h2 * (m2 - tb[d] * tb[e])
        out.update(tb=tb, S=S)
    else:
        x = pop.astype(LD)
        tb = np.array([er.pairwise_sum(x[d]) / N for d in range(D)], dtype=LD)
        c = x - tb[:, None]
        r = np.array([er.pairwise_sum(c[d]) / N for d in range(D)], dtype=LD)       # what the rounded mean left: second pass
        h2 = LD(1) - LD(float(a)) * LD(float(a))
        S = np.zeros((D, D), dtype=LD)
        for d in range(D):
            for e in range(d + 1):
                S[d, e] = S[e, d] = h2 * (er.pairwise_sum(c[d] * c[e]) / N - r[d] * r[e])
        out.update(tb=list(tb + r), S=[[S[d, e] for e in range(D)] for d in range(D)])
    return out


def budget_thetabar(mom, B):
    return (gamma(k_add(B) + 2) + REF_EPS) * mom["A"] * _UP


def budget_S(mom, B, a):
    """[4, 4] doubles: the bound of |S^_de - (1 - a^2) V_de| derived in the module docstring, plus the reference's own REF_EPS."""
    k = k_add(B)
    h2 = abs(1.0 - float(a) * float(a)) + 2.0 * U
    scale = mom["S2"] + np.outer(mom["A"], mom["A"])
    return scale * ((h2 * gamma(2 * k + 7) + 2.0 * U) + REF_EPS) * _UP


def _num(v, exact):
    return Fraction(float(v)) if exact else LD(v)


def check_proposal(thetabar, L, pop, a, B, name="", log=None):
    """thetabar[4], L[4, 4] (the lower triangle is read) of either implementation against the exact moments of pop.  Returns a list
    of failures (empty: all within budget); log(name, error, budget) is called for every entry.

    theta-bar: |tb^_d - tb_d| <= budget_thetabar.
    L by backward error, entry (i, j), j <= i, with R_ij = S_ij - sum_{k <= j} L_ik L_jk evaluated exactly:
      L_jj > 0: |R_ij| <= budget_S[i][j] + fact[i][j].
      L_jj == 0 (the guard `sdiag > 0.0` zeroed the column): the loop saw a reduced diagonal <= 0, so the exact reduced diagonal
        R_jj must itself lie within bd_j = budget_S[j][j] + fact[j][j] of it: |R_jj| <= bd_j.  The off-diagonals of that column
        were never divided; the exactly reduced matrix is positive semi-definite up to these budgets, so its 2 x 2 minor gives
        (|R_ij| - b_ij)^2 <= (R_jj + bd_j)(R_ii' + b_ii) <= 2 bd_j (S_ii + b_ii) -- Cauchy-Schwarz:
        |R_ij| <= b_ij + sqrt(2 bd_j (S_ii + b_ii)), b = budget_S + fact."""
    mom = exact_moments(pop, a)
    ex = mom["exact"]
    bad = []
    log = log or (lambda *_: None)
    btb = budget_thetabar(mom, B)
    for d in range(4):
        err = abs(float(_num(thetabar[d], ex) - mom["tb"][d]))
        log(f"{name} thetabar[{d}]", err, btb[d])
        if not err <= btb[d]:
            bad.append(("thetabar", d, float(thetabar[d]), err, btb[d]))
    bS = budget_S(mom, B, a)
    Lf = np.tril(np.asarray(L, dtype=np.float64))
    fact = gamma(FACT_OPS) * (np.abs(Lf) @ np.abs(Lf).T) * _UP
    b = bS + fact
    Ln = [[_num(Lf[i, j], ex) for j in range(4)] for i in range(4)]
    for j in range(4):
        for i in range(j, 4):
            R = mom["S"][i][j] - sum((Ln[i][k] * Ln[j][k] for k in range(j + 1)), _num(0.0, ex))
            err = abs(float(R))
            if Lf[j, j] > 0.0:
                tol = b[i, j]
            elif i == j:
                tol = b[j, j]
            else:
                tol = b[i, j] + float(np.sqrt(2.0 * b[j, j] * (float(mom["S"][i][i]) + b[i, i]))) * _UP
                if Lf[i, j] != 0.0:
                    bad.append(("L below a zeroed diagonal is not zero", i, j, Lf[i, j], 0.0, 0.0))
            log(f"{name} L[{i}][{j}]" + ("" if Lf[j, j] > 0.0 else " (guard)"), err, tol)
            if not err <= tol:
                bad.append(("L", i, j, Lf[i, j], err, tol))
    return bad
