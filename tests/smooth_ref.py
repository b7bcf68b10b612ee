"""Host reference of the smoothing calls (ssme_pf_sample_trajectories, ssme_pf_get_smoothed_expectations): the genealogy of a series
built in numpy from what the STEP API already exposes.  A handle stepped with step() under set_debug(record_ancestors) is downloaded
after every step -- the pre-resampling population x_t and the ancestors the step's draw used -- and the lineages are chased here:

    B_{T-1}(j) = j,   B_{t-1}(j) = anc_t[B_t(j)]  where step t resampled (t >= 1 and t % resamp_sched == 0),  B_t(j) otherwise.

The ancestors of a step are taken ONLY where the step resampled: the debug buffer is stale on every other step (it keeps the last
draw's indices).  Plain numpy, no device code in genealogy() / lineage_states(): the CPU test pins them to a hand-written case."""
import numpy as np


def resampled(t, sched):
    return t >= 1 and t % sched == 0


def genealogy(ancs, sched, n=None):
    """ancs: [T] arrays of N ancestor indices (entry t is read only where step t resampled; entry 0 never).  Returns B [T, N]:
    B[t, j] = index in the population of step t of the ancestor of final particle j."""
    T = len(ancs)
    n = int(len(ancs[-1]) if n is None else n)
    B = np.empty((T, n), dtype=np.int64)
    B[T - 1] = np.arange(n)
    for t in range(T - 1, 0, -1):
        B[t - 1] = np.asarray(ancs[t], dtype=np.int64)[B[t]] if resampled(t, sched) else B[t]
    return B


def lineage_states(xs, B):
    """xs: [T] populations, each [N] or [dim_x, N].  Returns [N, T, dim_x]: the state trajectory that ends at every final particle."""
    T, n = B.shape
    planes = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in xs]
    out = np.empty((n, T, planes[0].shape[0]))
    for t in range(T):
        out[:, t, :] = planes[t][:, B[t]].T
    return out


def stepped_history(bank, y, z=None):
    """Steps `bank` (parameters set, fresh) through the series under set_debug(record_ancestors, keep_logw) and downloads every
    filter after every step.  Returns dict(xs=[R][T] populations, ancs=[R][T] ancestors, final=[R] state() after the last step,
    ll=[T, R] log conditional likelihoods)."""
    R, T = bank.r, len(y)
    bank.set_debug(record_ancestors=True, keep_logw=True)
    xs = [[None] * T for _ in range(R)]
    ancs = [[None] * T for _ in range(R)]
    ll = np.empty((T, R))
    final = None
    for t in range(T):
        ll[t] = bank.step(y[t], None if z is None else z[t])
        sts = [bank.state(f, ancestors=True) for f in range(R)]
        for f, st in enumerate(sts):
            xs[f][t], ancs[f][t] = st["x"].copy(), st["anc"].copy()
        final = sts
    return dict(xs=xs, ancs=ancs, final=final, ll=ll)


def reference(hist, sched):
    """From stepped_history(): (states [R, N, T, dim_x], indices [R, N, T]) of the lineages of ALL final particles."""
    xs, idx = [], []
    for f in range(len(hist["xs"])):
        B = genealogy(hist["ancs"][f], sched)
        xs.append(lineage_states(hist["xs"][f], B))
        idx.append(B.T.copy())
    return np.stack(xs), np.stack(idx).astype(np.uint32)
