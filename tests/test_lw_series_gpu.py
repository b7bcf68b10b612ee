"""The whole-series Liu-West kernel (ssme_amd/csrc/lw_small.h, k_lw_series) against the tiled route and the oracle, bit for bit.

Three parties per case: a handle on the series route (set_small_series(1)), a second handle with the same seed on the tiled route
(set_small_series(0)) and oracle.LWFilter stepped on the CPU.  After the series:
  series == tiled   per-step log conditional likelihoods, their sum, x, transformed theta, the last step's k indices and ancestors,
                    theta-bar, the Cholesky factor, param_means(), expectations(range(8)), weights() -- every bit, NaN for NaN
  series == oracle  the same list up to the Cholesky factor (the three read-outs are sums in the device's own order, which the
                    oracle does not reproduce to the bit; they are held to the tiled route's bits, and the tiled route to the
                    budgets of expect_ref.py by test_liu_west_edges_gpu.py)
The case list is tests/lw_series_cases.py (what each case reaches: test_lw_series_cpu.py)."""
import os

import numpy as np
import pytest

import lw_edge_cases as lc
import lw_series_cases as sc
import test_expectations_gpu as teg
from test_liu_west_edges_gpu import same_bits

pytestmark = pytest.mark.gpu
sa = teg.sa
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(sa, oracle, case, series, n=None, R=None):
    tr, lo, hi = lc.prior(case, oracle)
    cls = sa.svol_lw_2_par if case["form"] else sa.svol_lw_1_par
    g = cls(case["delta"], lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], nparts=case["n"] if n is None else n,
            n_filters=case["R"] if R is None else R, seed=lc.SEED, transforms=tuple(tr), rs=case["rs"])
    g.set_debug(True)
    g.set_small_series(series)
    return g


def same_handles(s, t, R, T, what):
    """Everything a caller can read after a series: handle s against handle t."""
    same_bits(s.per_step(), t.per_step(), what + ": per_step()")
    same_bits(s.param_means(), t.param_means(), what + ": param_means()")
    same_bits(s.expectations(list(range(8))), t.expectations(list(range(8))), what + ": expectations(range(8))")
    for r in range(R):
        a, b = s.state(r, indices=True), t.state(r, indices=True)
        for k in ("x", "theta"):
            same_bits(a[k], b[k], f"{what} r={r}: {k}")
        if T >= 2:                               # step 0 has no draws, theta-bar or factor
            for k in ("thetabar", "L"):
                same_bits(a[k], b[k], f"{what} r={r}: {k}")
            np.testing.assert_array_equal(np.signbit(a["L"]), np.signbit(b["L"]), err_msg=f"{what} r={r}: signed zeros of L")
            for k in ("anc", "kidx"):
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what} r={r}: {k}")
        for u, v, k in zip(s.weights(r), t.weights(r), ("x", "untransformed theta", "w")):
            same_bits(u, v, f"{what} r={r}: weights() {k}")


def same_as_oracle(g, lls, states, tot, what, reps=None):
    """lls: [T][R] oracle log conditional likelihoods, states: the R oracle states after the last step."""
    T = len(lls)
    per = g.per_step()
    reps = range(len(states)) if reps is None else reps
    for j, r in enumerate(reps):
        want = np.array([lls[t][j] for t in range(T)])
        same_bits(per[r], want, f"{what} r={r}: per_step() == oracle")
        acc = 0.0
        for t in range(T):
            acc = acc + want[t]
        same_bits([tot[r]], [acc], f"{what} r={r}: the returned sum")
        gs, so = g.state(r, indices=True), states[j]
        same_bits(gs["x"], so["x"], f"{what} r={r}: particles == oracle")
        same_bits(gs["theta"], so["theta"], f"{what} r={r}: parameters == oracle")
        if T >= 2:
            same_bits(gs["thetabar"], so["thetabar"], f"{what} r={r}: theta-bar == oracle")
            same_bits(np.tril(gs["L"]), np.tril(so["L"]), f"{what} r={r}: L == oracle")
            np.testing.assert_array_equal(np.tril(gs["L"]) == 0.0, np.tril(so["L"]) == 0.0, err_msg=f"{what} r={r}: which entries of L are 0")
            np.testing.assert_array_equal(gs["anc"], so["anc"], err_msg=f"{what} r={r}: ancestors == oracle")
            np.testing.assert_array_equal(gs["kidx"], so["kidx"], err_msg=f"{what} r={r}: k indices == oracle")


def three_ways(sa, oracle, case):
    y, z = lc.series(case)
    run = lc.oracle_run(oracle, case)
    s, t = make(sa, oracle, case, True), make(sa, oracle, case, False)
    assert s.series_route() == (sa.ROUTE_LW_SERIES, 512)
    assert t.series_route() == (sa.ROUTE_TILED, 512)
    tot_s, tot_t = s.run_series(y, z), t.run_series(y, z)
    assert s.series_route() == (sa.ROUTE_LW_SERIES, 512)                   # the setting survives run_series
    same_bits(tot_s, tot_t, case["name"] + ": the returned sums")
    same_handles(s, t, case["R"], case["T"], case["name"] + ": series == tiled")
    same_as_oracle(s, [lls for lls, _ in run], run[-1][1], tot_s, case["name"])
    s.close()
    t.close()


@pytest.mark.parametrize("case", sc.size_cases(), ids=lambda c: c["name"])
def test_sizes(sa, oracle, case):
    three_ways(sa, oracle, case)


@pytest.mark.parametrize("form", (0, 1))
def test_route_query(sa, oracle, form):
    case = dict(sc.size_cases()[0], form=form)
    g = make(sa, oracle, case, True, n=sc.TILED_ONLY)
    assert g.series_route() == (sa.ROUTE_TILED, 512)                        # two tiles: tiled whatever the setting
    g.close()
    g = make(sa, oracle, case, True, n=sc.ONE_TILE)
    assert g.series_route() == (sa.ROUTE_LW_SERIES, 512)
    g.set_small_series(False)
    assert g.series_route() == (sa.ROUTE_TILED, 512)
    g.set_small_series(True)
    g.reset()
    assert g.series_route() == (sa.ROUTE_LW_SERIES, 512)                   # the setting survives reset
    g.close()


@pytest.mark.parametrize("case", sc.schedule_cases(), ids=lambda c: c["name"])
def test_schedules(sa, oracle, case):
    three_ways(sa, oracle, case)


@pytest.mark.parametrize("case", sc.degenerate_cases(), ids=lambda c: c["name"])
def test_degenerate_inputs(sa, oracle, case):
    three_ways(sa, oracle, case)


@pytest.mark.parametrize("case", sc.handover_cases(), ids=lambda c: c["name"])
def test_handover_to_the_step_api(sa, oracle, case):
    """run_series of 5 steps followed by 3 filter() calls equals 8 oracle steps, and the tiled route handed over the same."""
    y, z = lc.series(case)
    run = lc.oracle_run(oracle, case)
    s, t = make(sa, oracle, case, True), make(sa, oracle, case, False)
    s.run_series(y[:5], z[:5])
    t.run_series(y[:5], z[:5])
    for k in range(5, 8):
        s.filter(y[k], z[k])
        t.filter(y[k], z[k])
        same_bits(np.atleast_1d(s.getLogCondLike()), run[k][0], f"{case['name']} t={k}: getLogCondLike() == oracle")
        same_bits(np.atleast_1d(s.getLogCondLike()), np.atleast_1d(t.getLogCondLike()), f"{case['name']} t={k}: series == tiled")
        gs, so = s.state(0, indices=True), run[k][1][0]
        for key in ("x", "theta", "thetabar"):
            same_bits(gs[key], so[key], f"{case['name']} t={k}: {key} == oracle")
        same_bits(np.tril(gs["L"]), np.tril(so["L"]), f"{case['name']} t={k}: L == oracle")
        for key in ("anc", "kidx"):
            np.testing.assert_array_equal(gs[key], so[key], err_msg=f"{case['name']} t={k}: {key} == oracle")
    for r in range(case["R"]):
        a, b = s.state(r, indices=True), t.state(r, indices=True)
        for key in ("x", "theta", "thetabar", "L"):
            same_bits(a[key], b[key], f"{case['name']}: after the steps, {key}, series == tiled")
    same_bits(s.expectations(list(range(8))), t.expectations(list(range(8))), case["name"] + ": expectations after the steps")
    s.close()
    t.close()


@pytest.mark.parametrize("case", sc.handover_cases(), ids=lambda c: c["name"])
def test_any_order_on_one_handle(sa, oracle, case):
    """Two run_series calls on one handle return the same bits; run_series after three filter() calls equals a fresh handle."""
    y, z = lc.series(case)
    fresh = make(sa, oracle, case, True)
    tot = fresh.run_series(y, z)
    again = make(sa, oracle, case, True)
    again.run_series(y[:6], z[:6])
    same_bits(again.run_series(y, z), tot, case["name"] + ": second run_series, the sums")
    same_handles(again, fresh, case["R"], case["T"], case["name"] + ": second run_series == fresh handle")
    stepped = make(sa, oracle, case, True)
    for k in range(3):
        stepped.filter(y[k], z[k])
    same_bits(stepped.run_series(y, z), tot, case["name"] + ": run_series after three steps, the sums")
    same_handles(stepped, fresh, case["R"], case["T"], case["name"] + ": run_series after three steps == fresh handle")
    for g in (fresh, again, stepped):
        g.close()


@pytest.mark.parametrize("case", sc.handover_cases(), ids=lambda c: c["name"])
def test_forecast_after_the_series(sa, oracle, case):
    y, z = lc.series(case)
    s, t = make(sa, oracle, case, True), make(sa, oracle, case, False)
    s.run_series(y, z)
    t.run_series(y, z)
    a = s.sim_future_obs(4, y[-1], states=True, start=True, prop=True)
    b = t.sim_future_obs(4, y[-1], states=True, start=True, prop=True)
    same_bits(a[0], b[0], case["name"] + ": forecast observations")
    same_bits(a[1], b[1], case["name"] + ": forecast states")
    np.testing.assert_array_equal(a[2], b[2], err_msg=case["name"] + ": start draw")
    same_bits(a[3][:, :14], b[3][:, :14], case["name"] + ": forecast proposal")
    s.close()
    t.close()


def _spy_rows(T):
    y = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))[:T]
    return y, np.concatenate([[0.0], y[:-1]])


@pytest.mark.parametrize("form", (0, 1))
def test_a_longer_series(sa, oracle, form):
    case = lc._c("series-long", n=sc.LONG_N, T=sc.LONG_T, form=form)
    y, z = _spy_rows(sc.LONG_T)
    of = lc.oracle_filters(oracle, case)[0]
    lls = [[of.step(y[k], z[k])] for k in range(sc.LONG_T)]
    s, t = make(sa, oracle, case, True), make(sa, oracle, case, False)
    tot_s, tot_t = s.run_series(y, z), t.run_series(y, z)
    same_bits(tot_s, tot_t, "long series: the returned sums")
    same_handles(s, t, 1, sc.LONG_T, "long series: series == tiled")
    same_as_oracle(s, lls, [of.state()], tot_s, "long series")
    s.close()
    t.close()


@pytest.mark.parametrize("form", (0, 1))
def test_a_bank(sa, oracle, form):
    case = lc._c("series-bank", n=sc.BANK_N, T=sc.BANK_T, R=sc.BANK_R, form=form)
    y, z = _spy_rows(sc.BANK_T)
    s, t = make(sa, oracle, case, True), make(sa, oracle, case, False)
    tot_s, tot_t = s.run_series(y, z), t.run_series(y, z)
    same_bits(tot_s, tot_t, "bank: the returned sums")
    same_handles(s, t, sc.BANK_R, sc.BANK_T, "bank: series == tiled")
    tr, lo, hi = lc.prior(case, oracle)
    ofs = [oracle.LWFilter(sc.BANK_N, lc.SEED, rep=r, delta=case["delta"], transforms=tr, lo=lo, hi=hi, form=form, resamp_sched=1)
           for r in sc.BANK_ORACLE_REPS]
    lls = [[of.step(y[k], z[k]) for of in ofs] for k in range(sc.BANK_T)]
    same_as_oracle(s, lls, [of.state() for of in ofs], tot_s, "bank", reps=sc.BANK_ORACLE_REPS)
    s.close()
    t.close()
