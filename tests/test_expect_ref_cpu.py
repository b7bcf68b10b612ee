"""The exact expectation reference (tests/expect_ref.py) checked against itself and against the oracle, without a GPU; and the proof,
from the oracle's state alone, that every scenario of tests/expect_cases.py reaches the path it is there for."""
import os
from fractions import Fraction

import numpy as np
import pytest

import expect_cases as ec
import expect_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _state_after(oracle, n, tile, T=3, model=ec.MODEL_SVOL, theta=ec.TH_SVOL, seed=7):
    case = ec._case("x", n, tile, model=model, theta=theta, T=T, seed=seed)
    for t, tile, ofs, _ in ec.walk_oracle(oracle, case):
        pass
    return er.make_state(oracle, ofs[0].state(), tile), ofs[0]


@pytest.mark.parametrize("n,tile", [(1, 2048), (2, 2048), (513, 2048), (2049, 2048), (5000, 512)])
def test_fraction_and_long_double_evaluations_agree(oracle, n, tile):
    st, _ = _state_after(oracle, n, tile)
    h = ec.builtin_rows(oracle, st["x"])
    fr = er.expect_fixed_point(h, st, "fraction")
    ld = er.expect_fixed_point(h, st, "longdouble")
    sabs = er.s_abs(h, st)
    for k in range(4):
        err = abs(Fraction(float(ld[k])) + Fraction(float(ld[k] - np.longdouble(float(ld[k])))) - fr[k])
        print(n, tile, "h", k, "rel", float(err) / sabs[k])
        assert err <= Fraction(2) ** -60 * Fraction(sabs[k]), (n, tile, k)
    assert fr[3] == 42                                           # the constant's expectation is exactly 42 in rational arithmetic


def test_constant_is_exact_where_tiles_are_empty(oracle):
    st, _ = _state_after(oracle, 20000, 512, T=4, model=ec.MODEL_LIN_GAUSS, theta=ec.TH_DEGENERATE, seed=5)
    assert er.expect_fixed_point(np.full(st["n"], 42.0), st, "fraction")[0] == 42


def _check_against_oracle(oracle, st, of, what):
    h = ec.builtin_rows(oracle, st["x"])
    den = er.pairwise_sum(er.fixed_point_weights(st))
    assert den > 0, what + ": denominator"
    eq = er.expect_fixed_point(h, st, "longdouble")
    ex = er.expect_exact_weights(h, st)
    bfp = er.budget_fixed_point(h, st)
    sabs = er.s_abs(h, st, exact=True)
    for k in range(4):
        own = st["n"] * er.U * sabs[k]                          # the oracle's sequential sums
        d_or = abs(float(eq[k]) - of.expectation(k))
        d_ex = abs(float(eq[k] - ex[k]))
        print(what, "h", k, "|E_q - oracle|", d_or, "|E_q - E_exact|", d_ex, "budget_fixed_point", bfp[k], "oracle sum", own)
        assert d_ex <= bfp[k], (what, k, d_ex, bfp[k])
        assert d_or <= bfp[k] + own, (what, k, d_or, bfp[k], own)


@pytest.mark.parametrize("case", ec.bootstrap_cases() + ec.series_cases(), ids=lambda c: c["name"])
def test_scenarios_from_the_oracle_alone(oracle, case):
    """|E_q - oracle.expectation| <= budget_fixed_point + N u S_abs at every shape of the GPU module; the degenerate scenarios contain
    tiles whose integer weights are all zero but the maximum's and tile scales down to subnormal, the underflow scenarios tiles whose scale
    exp(m_b - m) is exactly 0; the wrapped shapes have more than 256 tiles and a one-particle tail;
    a schedule-3 walk visits steps that resample and steps that do not."""
    for t, tile, ofs, _ in ec.walk_oracle(oracle, case):
        for r, of in enumerate(ofs):
            st = er.make_state(oracle, of.state(), tile)
            _check_against_oracle(oracle, st, of, f"{case['name']} t={t} r={r}")
            B = st["A"].size
            if case.get("degenerate") and t == case["T"] - 1:
                # A_b = 0 cannot occur: the tile's own maximum always has q = 2^41.  What does occur: tiles in which EVERY other
                # integer weight is zero, and tile scales far below the 2^-41 resolution of the weights (subnormal at the wrapped shape)
                assert (st["A"] >= 2 ** 41).all() and (st["A"] == 2 ** 41).any() and (st["q"] == 0).mean() > 0.99
                assert st["s"].min() < 1e-20 and (st["s"] == 1.0).any()
            if case.get("underflow") and t == case["T"] - 1:
                assert (st["s"] == 0.0).sum() > 30 and (st["s"] == 1.0).any(), "tile scales that underflow to zero"
            if case["n"] == ec.WRAP:
                assert B == 258 and st["n"] - (B - 1) * tile == 1
            if case["name"] == "split-level2":
                assert B > 2048
    if case["sched"] == 3:
        assert [(t + 1) % 3 == 0 for t in range(case["T"])].count(True) == 2 and case["every_step"]


def test_outlier_scenario_spreads_the_weights(oracle):
    """The outliers put the weights hundreds of units of log-weight apart; at those steps at least a quarter of the integer weights are zero."""
    case = [c for c in ec.bootstrap_cases() if c["name"] == "outliers"][0]
    spread = []
    for t, tile, ofs, _ in ec.walk_oracle(oracle, case):
        st = er.make_state(oracle, ofs[0].state(), tile)
        spread.append(float(st["logw"].max() - st["logw"].min()))
        zero = float((st["q"] == 0).mean())
        if spread[-1] > 100.0:
            assert zero > 0.25, (t, zero)
    assert max(spread) > 100.0, spread


@pytest.mark.parametrize("case", [c for c in ec.lw_cases() if c["n"] <= 2049], ids=lambda c: c["name"])
def test_liu_west_state_rebuilt_from_log_weights(oracle, case):
    """The q_j rebuilt from the second-stage log-weights give the oracle's own expectations within the same bound."""
    tr, lo, hi = ec.lw_prior(case, oracle)
    of = oracle.LWFilter(case["n"], 11, transforms=tr, lo=lo, hi=hi, form=case["form"], resamp_sched=case["rs"])
    y, z = ec.lw_series(case["T"])
    for t in range(case["T"]):
        of.step(y[t], z[t])
        so = of.state()
        st = er.lw_state(oracle, so)
        h = ec.lw_h_rows(oracle, so["x"], ec.lw_untransform(oracle, tr, so["theta"]))
        eq, bfp, sabs = er.expect_fixed_point(h, st, "longdouble"), er.budget_fixed_point(h, st), er.s_abs(h, st, exact=True)
        for k in range(8):
            d = abs(float(eq[k]) - of.expectation(k))
            assert d <= bfp[k] + st["n"] * er.U * sabs[k], (case["name"], t, k, d, bfp[k])
        np.testing.assert_allclose(of.param_means(), [float(v) for v in eq[4:]], rtol=0, atol=float(np.max(bfp[4:] + st["n"] * er.U * sabs[4:])))


def test_swarm_reference_and_budgets():
    rng = np.random.default_rng(3)
    rows = rng.normal(size=(2, 300))
    plain, pooled = er.swarm_means_ref(rows, 7)
    groups = [np.arange(300)[np.arange(300) % 7 == j] for j in range(7)]
    want = [np.mean([rows[f][g].mean() for g in groups]) for f in range(2)]
    np.testing.assert_allclose(pooled.astype(float), want, rtol=1e-14)
    np.testing.assert_allclose(plain.astype(float), rows.mean(axis=1), rtol=1e-13)
    assert np.array_equal(er.swarm_means_ref(rows, 305)[1], er.swarm_means_ref(rows, 300)[1])     # more threads than members: T = R
    # one member per thread is the plain mean: both are pairwise long-double sums of the same 300 values, within 10 roundings of 2^-64
    one_each = er.swarm_means_ref(rows, 300)[1]
    assert (np.abs(one_each - plain) <= 10 * 2.0 ** -64 * np.abs(rows).max(axis=1)).all()
    assert er.k_sum(512, 258, "expect") == 2 + 2 * 2 + 31 and er.k_sum(2048, 1, "user") == 8 + 2 + 31
    assert er.k_sum(2048, 3, "lw") == 16 + 6 + 22 and er.k_sum(512, 1, "weights") == 2


@pytest.mark.parametrize("case", [c for c in ec.lw_cases() if c["n"] > 2049 and c["form"] == 0], ids=lambda c: c["name"])
def test_liu_west_large_shapes_reach_their_paths(oracle, case):
    """257 * 2048 + 1 has more than 256 tiles (k_lw_weights' maximum loop wraps, k_lw_param_means runs 17 batches of 16) and a one-particle
    tail; 2049 * 2048 + 5 has more than 2048 tiles.  The smaller one is also walked: the state rebuilt from the log-weights meets the
    oracle's expectations there (the larger costs 10 s of oracle and long-double time and is walked by the GPU test)."""
    n = case["n"]
    B = -(-n // 2048)
    assert (B > 2048 and n - (B - 1) * 2048 == 5) if n > 4000000 else (B == 258 and n - (B - 1) * 2048 == 1)
    if n > 4000000:
        return
    of = oracle.LWFilter(n, 11, form=0)
    y, z = ec.lw_series(case["T"])
    for t in range(case["T"]):
        of.step(y[t], z[t])
    so = of.state()
    st = er.lw_state(oracle, so)
    assert st["A"].size == B
    h = ec.builtin_rows(oracle, so["x"])
    eq, bfp, sabs = er.expect_fixed_point(h, st), er.budget_fixed_point(h, st), er.s_abs(h, st, exact=True)
    for k in range(4):
        assert abs(float(eq[k]) - of.expectation(k)) <= bfp[k] + n * er.U * sabs[k], (k,)
