"""The Liu-West kernels (csrc/lw_kernels.h, lw_enqueue_step) at the degenerate inputs of tests/lw_edge_cases.py: NaN and extreme
observations, a NaN covariate, collapsed parameter clouds, N = 1, 2, 3, delta = 1, point priors, the first shapes of the
k_lw_mom_totals and split level-2 paths -- where the guards written into the kernels are taken and where theta-bar and L depend on
the exact order of every addition.  For every case and both forms the device must return the oracle's bits at every step (states,
parameters, ancestors, k indices, theta-bar, the lower triangle of L including which entries are exactly 0, the log conditional
likelihood with NaN where the oracle has NaN), through the step API in debug mode and through run_series; the read-outs
(expectations, param_means, weights) are held to the budgets of expect_ref.py, and theta-bar and L of the DEVICE to the exact
reference of lw_moments_ref.py -- redundant while the bits equal the oracle's, kept so that a failure says whether device and oracle
disagree with each other or with the definition.  test_lw_edges_cpu.py proves without a GPU that each case reaches its path.

Why no search can hang or leave its arrays on a cdf of zeros or on NaN tile maxima (read before the first run):
  * every search is a descent with a fixed number of probes: count_less_pow2 halves a power-of-two step down to 1, lds_count_search
    and staged_search are unrolled at compile time; count_from of k_level2_plan doubles `sz` only while p + sz - 1 < Bpow2 and then
    halves it.  No loop waits for a condition on the data.  A comparison with NaN is false, so a NaN target counts nothing.
  * level2_scan: block_max_nanprop returns NaN if any tile maximum is NaN; dexp_scaled_t clamps a NaN argument to 0, so every
    rescaled tile sum A' = rint(A * 0) = 0 and S = 0: never NaN, never negative.  With S = 0 the targets are t_scale = 0 / G = 0
    (G, a sum of Gamma draws, is positive), t_lo = 0 and t_hi = 2: no T' is below 0 and every T' = 0 is below 2, so lo = 0 and
    hi = B, clamped to B - 1; hi >= lo always because both count the same monotone T' against t_lo <= t_hi.
  * span = hi - lo + 1 <= 3 stages tiles lo .. hi <= B - 1 (the loads are guarded by span >= 2, >= 3); a longer span takes the
    global path, whose tile index is clamped to B - 1 and whose in-tile count is at most 2047.  A / A' = 0 / 0 = NaN there makes
    the in-tile target NaN: count 0.  Every resulting index is clamped to N - 1 before it is used as a gather address.
  * the accounting writes Sd = (S > 0) ? ... : NaN, so a step without weight is NaN in per_step and in the sum; the next step
    resamples every particle from index 0 (S = 0) or, after finite weights return, as usual.
The NaN cases run first when this module is run alone in two invocations (-k "nan or inf" / -k "not (nan or inf)")."""
import numpy as np
import pytest

import expect_cases as ec
import expect_ref as er
import lw_edge_cases as lc
import lw_moments_ref as mr
import test_expectations_gpu as teg

pytestmark = pytest.mark.gpu
CASES = lc.cases()
sa = teg.sa


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    """Bit for bit, NaN for NaN (a NaN's payload is not part of the contract)."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=what + ": NaN pattern")
    np.testing.assert_array_equal(_bits(got)[~gn], _bits(want)[~wn], err_msg=what)


def make(sa, oracle, case, split=None):
    tr, lo, hi = lc.prior(case, oracle)
    cls = sa.svol_lw_2_par if case["form"] else sa.svol_lw_1_par
    g = cls(case["delta"], lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], nparts=case["n"], n_filters=case["R"], seed=lc.SEED,
            transforms=tuple(tr), rs=case["rs"])
    g.set_debug(True, split_level2=split)
    return g


def budget_log(name, err, budget):
    teg.record(name, err, budget if budget else 1.0, 0)


def check_readouts(g, oracle, case, r, so, name):
    """expectations([0..7]), param_means() and weights() of filter r against the oracle state `so` (expect_ref.py's budgets)."""
    ex = g.expectations(list(range(8)))[:, r]
    pm = g.param_means()[r]
    x, thu, w = g.weights(r)
    same_bits(x, so["x"], name + ": weights() particles")
    with np.errstate(all="ignore"):
        st = er.lw_state(oracle, so)
        # the fixed-point weights q_j exp(m_b - m) 2^-41 formed from the oracle's log-weights: a NaN log-weight makes its tile's
        # maximum and with it the filter's maximum m NaN (both maxima propagate NaN), and then every weight is NaN; log-weights that
        # are all -inf (form 1 after y = 1e200) have q_j = 0 exactly and a maximum that is not NaN: weights of 0, not NaN
        want_nan = np.full(so["x"].shape, bool(np.isnan(st["m"])))
        assert np.isnan(st["mb"]).any() == np.isnan(st["m"]) == np.isnan(so["logw"]).any()
    if lc.zero_denominator(so):
        # no weight left: every expectation is 0 / 0, E[42] included (k_lw_param_means writes 42 * (den / den))
        assert np.isnan(ex).all(), (name, ex)
        assert np.isnan(pm).all(), (name, pm)
        np.testing.assert_array_equal(np.isnan(w), want_nan, err_msg=name + ": NaN pattern of weights()")
        return ex, w
    h = ec.lw_h_rows(oracle, so["x"], thu)
    teg.check_rows(name, ex, h, st, "lw")
    assert ex[3] == 42.0
    np.testing.assert_array_equal(_bits(pm), _bits(ex[4:]), err_msg=name + ": param_means() == expectations([4..7])")
    np.testing.assert_array_equal(np.isnan(w), want_nan, err_msg=name + ": NaN pattern of weights()")
    teg.check_weights(name, w, oracle, st)
    return ex, w


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_liu_west_edge_case(sa, oracle, case):
    run = lc.oracle_run(oracle, case)
    T, n, R = case["T"], case["n"], case["R"]
    B, a = lc.tiles(n), lc.a_shrink(case["delta"])
    y, z = lc.series(case)
    g = make(sa, oracle, case, split=True if case["split"] else None)
    twin = make(sa, oracle, case) if case["split"] else None             # the default level-2 policy on the same case
    dev_ll = np.empty((R, T))
    prev_theta, last_read = [None] * R, [None] * R
    for t in range(T):
        g.filter(y[t], z[t])
        dev_ll[:, t] = np.atleast_1d(g.getLogCondLike())
        same_bits(dev_ll[:, t], run[t][0], f"{case['name']} t={t}: getLogCondLike()")
        if twin is not None:
            twin.filter(y[t], z[t])
            same_bits(np.atleast_1d(twin.getLogCondLike()), dev_ll[:, t], f"t={t}: forced split == default path, log conditional likelihood")
        for r in range(R):
            name = f"{case['name']} t={t} r={r}"
            gs, so = g.state(r, indices=True), run[t][1][r]
            if twin is not None:
                ts = twin.state(r, indices=True)
                for k in ("x", "theta", "thetabar", "L"):
                    same_bits(ts[k], gs[k], f"{name}: forced split == default path, {k}")
                for k in ("anc", "kidx"):
                    np.testing.assert_array_equal(ts[k], gs[k], err_msg=f"{name}: forced split == default path, {k}")
            if t >= 1:
                same_bits(gs["thetabar"], so["thetabar"], name + ": theta-bar")
                same_bits(np.tril(gs["L"]), np.tril(so["L"]), name + ": L")
                np.testing.assert_array_equal(np.tril(gs["L"]) == 0.0, np.tril(so["L"]) == 0.0, err_msg=name + ": which entries of L are 0")
            if so["x"] is not None:
                same_bits(gs["x"], so["x"], name + ": particles")
                same_bits(gs["theta"], so["theta"], name + ": parameters")
                if t >= 1:
                    np.testing.assert_array_equal(gs["anc"], so["anc"], err_msg=name + ": ancestors")
                    np.testing.assert_array_equal(gs["kidx"], so["kidx"], err_msg=name + ": k indices")
            if t >= 1 and prev_theta[r] is not None and (n <= 100000 or t == T - 1):
                # the device's own theta-bar and L against the definition, over the device's own population
                pop = mr.population(prev_theta[r], gs["anc"])
                bad = mr.check_proposal(gs["thetabar"], gs["L"], pop, a, B, name, budget_log)
                assert not bad, bad
                if case["expect"].get("identity") == "delta1":
                    want = pop[:, gs["kidx"].astype(np.int64)] if case["form"] == 0 else pop
                    same_bits(gs["theta"], want, name + ": a = 1 leaves every parameter where it was")
            if case["expect"].get("identity") == "point":
                same_bits(gs["theta"], np.repeat(run[0][1][r]["theta"][:, :1], n, axis=1), name + ": the transformed prior point")
            prev_theta[r] = gs["theta"]
            if t == case["probe"] or t == T - 1:
                last_read[r] = check_readouts(g, oracle, case, r, so, name)
    g.close()
    if twin is not None:
        twin.close()
    # the series API on a fresh handle, and a second pass on it
    s = make(sa, oracle, case, split=True if case["split"] else None)
    for again in (False, True):
        tot = s.run_series(y, z)
        per = s.per_step()
        same_bits(per, dev_ll, f"{case['name']}: per_step() == the step API" + (" (second pass)" if again else ""))
        for r in range(R):
            assert np.isnan(tot[r]) == np.isnan(dev_ll[r]).any(), (case["name"], r, tot[r])
            want = 0.0
            for t in range(T):
                want = want + run[t][0][r]
            same_bits([tot[r]], [want], f"{case['name']} r={r}: the returned sum")
    for r in range(R):
        so = run[T - 1][1][r]
        gs = s.state(r)
        if so["x"] is not None:
            same_bits(gs["x"], so["x"], "after run_series: particles")
            same_bits(gs["theta"], so["theta"], "after run_series: parameters")
        if n <= 100000:
            check_readouts(s, oracle, case, r, so, f"{case['name']} series r={r}")
        else:                                   # the large shapes: the same bits as the step API's read-outs, checked above
            same_bits(s.expectations(list(range(8)))[:, r], last_read[r][0], "after run_series: expectations")
            same_bits(s.weights(r)[2], last_read[r][1], "after run_series: weights()")
    s.close()
