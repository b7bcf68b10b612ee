"""A Python restatement of marginal smoothing (include/ssme_pf.h: ssme_pf_download_smoothing_weights; DESIGN.md section 12.2;
ssme_amd/csrc/marginal.h), written from its definition.  It works from the downloads of a stepped twin (backward_ref.stepped_history)
and the final weights w of the recorded handle:

    om_{T-1} = w;   for t = T-2 .. 0, column j of step t + 1:
        (q_.j, m_j) = backward_ref.backward_weights(O, logf, x_{t+1}[:, j], x_t, lw_t, z_{t+1}, sh)     -- the weights backward simulation
        D_j = sum_i q_ij (integers: exact);  live when m_j is finite and D_j > 0:  c_j = om_{t+1}[j] / D_j      draws B_t from, per column
        degenerate otherwise:  g(j) = min(anc_{t+1}[j], N - 1) where step t + 1 resampled, j otherwise
        om_t[i] = sum_{j live} c_j q_ij  +  sum_{j degenerate, g(j) = i} om_{t+1}[j]

The sums over j are float64 sums in numpy's own (pairwise, per chunk of columns) order -- not the device's.  Columns are processed in
chunks, so no N x N array of Python objects is ever built.  brute_force() does the same with Fractions for tiny N and shares only the
quantised weights q.  Every function takes the oracle module as `O`."""
from fractions import Fraction

import numpy as np

import backward_ref as br
from smooth_ref import resampled

CHUNK = 256                                # columns per block of q (N x CHUNK doubles)


def parent(ancs, t, j, n, sched):
    """g(j): where the mass of a degenerate column j of step t + 1 goes."""
    return min(int(ancs[t + 1][j]), n - 1) if resampled(t + 1, sched) else j


def step_back(O, logf, x_next, x_t, lw_t, anc_parent, om_next, z_next, sh):
    """om_t from om_{t+1}.  anc_parent(j) = g(j).  Returns (om_t, degenerate columns)."""
    n = x_t.shape[1]
    om = np.zeros(n, dtype=np.float64)
    degenerate = 0
    for j0 in range(0, n, CHUNK):
        js = range(j0, min(n, j0 + CHUNK))
        Q = np.zeros((n, len(js)), dtype=np.float64)
        c = np.zeros(len(js), dtype=np.float64)
        push = np.zeros(n, dtype=np.float64)
        for k, j in enumerate(js):
            q, m = br.backward_weights(O, logf, x_next[:, j], x_t, lw_t, z_next, sh)
            D = 0 if q is None else int(np.sum(np.asarray(q, dtype=np.uint64)))
            if q is not None and np.isfinite(m) and D > 0:
                Q[:, k] = np.asarray(q, dtype=np.uint64).astype(np.float64)       # q <= 2^41: exact
                c[k] = om_next[j] / float(D)                                      # D < 2^53: exact
            else:
                degenerate += 1
                push[anc_parent(j)] += om_next[j]
        om = om + (Q * c[None, :]).sum(axis=1) + push
    return om, degenerate


def filter_rows(O, logf, xs, lws, ancs, sched, w_final, zs=None):
    """One filter: (om [T, N], degenerate columns).  xs / lws / ancs: [T] downloads; w_final: the final weights; zs as in backward_ref."""
    T, n = len(xs), xs[0].shape[1]
    sh = br.shift_of(n)
    om = np.zeros((T, n), dtype=np.float64)
    om[T - 1] = np.asarray(w_final, dtype=np.float64)
    degenerate = 0
    for t in range(T - 2, -1, -1):
        zn = 0.0 if zs is None else zs[t + 1]
        om[t], d = step_back(O, logf, xs[t + 1], xs[t], lws[t], lambda j: parent(ancs, t, j, n, sched), om[t + 1], zn, sh)
        degenerate += d
    return om, degenerate


def brute_force(O, logf, xs, lws, ancs, sched, w_final, zs=None):
    """The same rows by rational arithmetic (tiny N): every om_t[i] is the exact rational sum, returned as Fractions [T][N].  Only the
    quantised weights are shared with the restatement; c_j is the exact quotient here, so the two differ by roundings alone."""
    T, n = len(xs), xs[0].shape[1]
    sh = br.shift_of(n)
    om = [[Fraction(0)] * n for _ in range(T)]
    om[T - 1] = [Fraction(float(v)) for v in w_final]
    for t in range(T - 2, -1, -1):
        zn = 0.0 if zs is None else zs[t + 1]
        row = [Fraction(0)] * n
        for j in range(n):
            q, m = br.backward_weights(O, logf, xs[t + 1][:, j], xs[t], lws[t], zn, sh)
            D = 0 if q is None else sum(int(v) for v in q)
            if q is not None and np.isfinite(m) and D > 0:
                for i in range(n):
                    row[i] += om[t + 1][j] * int(q[i]) / D
            else:
                row[parent(ancs, t, j, n, sched)] += om[t + 1][j]
        om[t] = row
    return om


def bound(T, n, t):
    """|device - restatement| <= bound * restatement at row t: all terms are non-negative and a step adds at most N + 1 roundings per
    entry on each side (the division, the product, N - 1 additions), u = 2^-53."""
    return 2.2 * (T - 1 - t) * (n + 1) * 2.0 ** -53
