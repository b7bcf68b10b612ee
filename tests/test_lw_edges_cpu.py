"""The case list of tests/lw_edge_cases.py through the oracle alone (no GPU): every case reaches the path it is listed for, the exact
reference of tests/lw_moments_ref.py agrees with the oracle's theta-bar and L within the derived budget at every step, and the
identities of the delta = 1 and point-prior cases hold on the oracle.  test_liu_west_edges_gpu.py then asks the device for the
oracle's bits on the same list."""
import numpy as np
import pytest

import bs_edge_cases as bc
import lw_edge_cases as lc
import lw_moments_ref as mr

CASES = lc.cases()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _diag_zero(st):
    return np.diag(st["L"]) == 0.0


def test_the_two_large_shapes_lie_in_their_tile_ranges():
    by = {c["name"]: c for c in lc.base_cases()}
    B = lc.tiles(by["mid-path"]["n"])
    assert lc.FUSED_MAX_TILES < B <= lc.SPLIT_ABOVE_TILES and B == 587 and lc.moment_path(by["mid-path"]) == "mid"
    assert lc.tiles(586 * lc.TILE) == 586 and lc.moment_path(dict(by["mid-path"], n=585 * lc.TILE)) == "fused"
    B = lc.tiles(by["split-path"]["n"])
    assert B > lc.SPLIT_ABOVE_TILES and B == 1026 and lc.moment_path(by["split-path"]) == "split"
    # the window area of stage 2 that decides fused / not: three staged tiles, T' and A / A' (2 x Bpow2 doubles)
    for Bt, fused in ((585, True), (586, False)):
        bpow2 = 1 << (Bt - 1).bit_length()
        assert (Bt * 14 * 8 <= (3 * lc.TILE + 2 * bpow2) * 8) == fused
    for name in ("nan-y", "huge-y", "point-prior", "n3", "wide-span"):
        assert lc.moment_path(by[name]) == "fused" and lc.moment_path(by[name + "-forced-split"]) == "split"
    lo, hi = lc.POINT, lc.POINT
    assert 0.0 < lo[0] < 1.0 and lo[2] > 0.0 and -1.0 < lo[3] < 1.0 and lo == hi         # inside logit, log and twice-Fisher supports


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_case_reaches_its_path_and_the_exact_reference_agrees(oracle, case):
    run = lc.oracle_run(oracle, case)
    exp, T, n = case["expect"], case["T"], case["n"]
    B, a = lc.tiles(n), lc.a_shrink(case["delta"])
    ll = np.array([lls for lls, _ in run])                                              # [T, R]
    if "nan_steps" in exp:
        for r in range(case["R"]):
            assert tuple(np.flatnonzero(np.isnan(ll[:, r]))) == tuple(exp["nan_steps"]), (case["name"], ll[:, r])
    if "big_step" in exp:
        assert ll[exp["big_step"], 0] < -1e5 and np.isfinite(ll).all()
    for t in range(1, T):
        for r, st in enumerate(run[t][1]):
            dz = _diag_zero(st)
            if exp.get("L_zero") == "all":
                assert not np.tril(st["L"]).any(), (t, st["L"])
            if exp.get("L_zero") == "none":
                assert not dz.any(), (t, st["L"])
            if "L_zero_diag" in exp:
                assert tuple(np.flatnonzero(dz)) == tuple(exp["L_zero_diag"]), (t, st["L"])
                for j in exp["L_zero_diag"]:                                             # row and column j: the division guard
                    assert not st["L"][j, :].any() and not st["L"][:, j].any()
            prev = run[t - 1][1][r]
            if prev["theta"] is None or st["anc"] is None:
                continue                                                                 # the large shapes keep their last two states
            pop = mr.population(prev["theta"], st["anc"])
            bad = mr.check_proposal(st["thetabar"], st["L"], pop, a, B, f"{case['name']} t={t} r={r}")
            assert not bad, bad
            if exp.get("identity") == "delta1":
                want = pop[:, st["kidx"].astype(np.int64)] if case["form"] == 0 else pop
                np.testing.assert_array_equal(_bits(st["theta"]), _bits(want), err_msg="a = 1: a theta + (1 - a) theta-bar + L z is theta")
    last = run[-1][1][0]
    if "distinct_last" in exp:
        assert np.unique(last["anc"]).size == exp["distinct_last"]
    if exp.get("L_zero_last") == "all":
        assert not np.tril(last["L"]).any()
    if exp.get("x_nan_last"):
        assert np.isnan(last["x"]).all() and np.isfinite(last["theta"]).all() and lc.zero_denominator(last)
    if "collapsed_after" in exp:
        st = run[exp["collapsed_after"] + 1][1][0]
        assert np.unique(st["anc"]).size == 1 and lc.zero_denominator(run[exp["collapsed_after"]][1][0])
    if "wide_span" in exp:
        key, t = exp["wide_span"][case["form"]]
        assert bc.source_span(run[t][1][0][key], lc.TILE).max() > bc.STAGE_TILES, (key, t)      # the kernel's own span is at least this
    if "distinct_at" in exp:
        t, lo, hi = exp["distinct_at"]
        assert lo <= np.unique(run[t][1][0]["anc"]).size <= hi
    if exp.get("identity") == "point":
        tr, plo, _ = lc.prior(case, oracle)
        for t in range(T):
            th = run[t][1][0]["theta"]
            assert (_bits(th) == _bits(th[:, :1])).all() and (_bits(th[:, 0]) == _bits(run[0][1][0]["theta"][:, 0])).all()
        # the transformed prior point: what the t = 0 draw lo + u (hi - lo) = lo gives through the forward transform
        pt = run[0][1][0]["theta"][:, 0]
        back = [oracle.inv_transform(int(tr[d]), float(pt[d])) for d in range(4)]
        assert np.allclose(back, plo, rtol=0, atol=8 * 2.0 ** -52)
        assert pt[1] == plo[1]                                                            # the null transform is the identity
    if case["rs"] > 1:
        for t in range(1, T):
            ident = np.array_equal(run[t][1][0]["anc"], np.arange(n))
            assert ident == (t % case["rs"] != 0), t                                     # steps that do not resample: the population stays


@pytest.mark.parametrize("base", ["n3", "nan-y", "huge-y"])
def test_the_noise_regime_really_occurs(oracle, base):
    """At least one non-zero diagonal of L below 1e-6: rounding noise of the collapsed cloud decided it (over both forms: the
    auxiliary form of huge-y happens to round every diagonal to a non-positive value)."""
    seen = []
    for case in CASES:
        if case["base"] == base:
            for _, sts in lc.oracle_run(oracle, case)[1:]:
                d = np.diag(sts[0]["L"])
                seen += [v for v in d if 0.0 < v < 1e-6]
    assert seen, base


def test_budget_counts():
    assert mr.k_add(1) == 23 and mr.k_add(585) == 32 and mr.k_add(1024) == 38 and mr.k_add(16384) == 278
