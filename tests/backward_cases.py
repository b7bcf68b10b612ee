"""What tests/test_backward_gpu.py and tests/backward_worker.py share: a recorded handle and its stepped twin of one configuration,
and the comparison of the device's backward simulation with tests/backward_ref.py, bit for bit."""
import numpy as np

import backward_ref as br
import series_expect_cases as sc

G = br.G


def same_bits(a, b, name):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    bad = np.flatnonzero(a.view(np.uint64).ravel() != b.view(np.uint64).ravel())
    assert bad.size == 0, (name, bad[:8], a.ravel()[bad[:8]], b.ravel()[bad[:8]])


def ks_of(n):
    """K in {1, G, G + 1, N}, N capped at 65, those that a filter of n particles allows."""
    return sorted({k for k in (1, G, G + 1, min(n, 65)) if k <= n})


def recorded(sa, model, theta, n, tile, small, sched, y, z, rs=0, dtype=0):
    bank = sc.make_bank(sa, model, n, theta, rs, sched, tile, dtype=dtype)
    bank.set_small_series(small)
    bank.record_series_history()
    bank.run_series(y, z)
    return bank


def twin_history(sa, model, theta, n, tile, sched, y, z, rs=0):
    bank = sc.make_bank(sa, model, n, theta, rs, sched, tile)
    hist = br.stepped_history(bank, y, z)
    bank.close()
    return hist


def check_logweights(bank, hist, name):
    """Every row of ssme_pf_download_series_logweights == the twin's step-API logw."""
    T = len(hist["lws"][0])
    for f in range(bank.r):
        for t in range(T):
            same_bits(bank.series_logweights(f, t), hist["lws"][f][t], f"{name}: log-weights of filter {f}, step {t}")


def check_backward(O, bank, hist, logf_of_filter, sched, Ks, name, zs=None, seed=sc.SEED, given=None):
    """index_out and x_out of the device for every K of Ks against the restatement; drawn terminals are taken from
    sample_trajectories (the join is asserted), `given`: [R, K] terminals to pass instead.  Returns the restatement's fallbacks."""
    T = len(hist["xs"][0])
    Kmax = max(Ks)
    if given is None:
        term = bank.sample_trajectories(Kmax, indices=True)[1][:, :, T - 1]
    else:
        term = np.asarray(given, dtype=np.uint32)
    X, B, fb = br.reference(O, logf_of_filter, hist, sched, term, seed, 0, zs)
    for K in Ks:
        x, idx = bank.sample_trajectories_backward(K, None if given is None else term[:, :K].copy(), return_indices=True)
        assert x.shape == (bank.r, K, T, X.shape[-1]) and idx.shape == (bank.r, K, T)
        np.testing.assert_array_equal(idx[:, :, T - 1], term[:, :K], err_msg=f"{name} K={K}: terminal indices")
        np.testing.assert_array_equal(idx, B[:, :K], err_msg=f"{name} K={K}: backward indices")
        assert (idx < bank.n).all()
        alive = ~np.isnan(x).reshape(bank.r, -1).all(axis=1)
        for f in range(bank.r):
            if alive[f]:
                same_bits(x[f], X[f, :K], f"{name} K={K} filter {f}: states")
    return fb
