"""The case and route lists of tests/bs_edge_cases.py through the oracle alone (no GPU): every (case, route) pair reaches the path it is
listed for, route_of() selects the instantiations written out below, the exact log conditional likelihood of tests/loglik_ref.py agrees
with the oracle within the derived budget at every finite step and is NaN exactly where the oracle is, and the Kalman filter's
log-likelihood is consistent with it for the linear Gaussian case.  test_bootstrap_edges_gpu.py then asks the device for the oracle's
bits on the same lists.  Largest observed error / budget per case and step: profiles/bs_edge_budgets.txt (every comparison is printed here, `BUDGET oracle ...`)."""
import numpy as np
import pytest

import bs_edge_cases as bc
import loglik_ref as lr

PAIRS = bc.pairs()
CASES = {c["name"]: c for c in bc.cases()}
ROUTES = {r["name"]: r for r in bc.routes()}

# the first live tile of zero-tile lies at index >= 3 on every multi-tile route but these two (their tile of the dominant particle is
# 1 and 2); there the global search path is reached by resampler 3, which never stages
ZERO_TILE_NARROW = ("wl2-1024", "wl2-2048")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# (route, form, resampler) -> (kernel, NT, BIG, TILE, RS, WL2, level-2): written out from csrc/pf_api.hip by hand, not by route_of()
TABLE = {
    ("small-1", "hot", 0): ("k_filter_series_lane<64>", 64, False, 2048, None, None, "in the loop"),
    ("small-64", "hot", 1): ("k_filter_series_lane<64>", 64, False, 2048, None, None, "in the loop"),
    ("small-100", "hot", 0): ("k_filter_series_lane<128>", 128, False, 2048, None, None, "in the loop"),
    ("small-200", "hot", 0): ("k_filter_series_lane<256>", 256, False, 2048, None, None, "in the loop"),
    ("small-300", "hot", 0): ("k_filter_series_lane<512>", 512, False, 2048, None, None, "in the loop"),
    ("small-1000", "hot", 0): ("k_filter_series_small<512,1>", 512, False, 2048, None, None, "in the loop"),
    ("small-2000", "hot", 1): ("k_filter_series_small<512,2>", 512, False, 2048, None, None, "in the loop"),
    # the step API never takes the one-launch kernel: one tile of 2048, 512 threads, the wave-by-wave level-2
    ("small-300", "general", 0): ("k_filter_step", 512, False, 2048, -1, True, "wave-by-wave in k_filter_step + fused accounting (ticket)"),
    ("edge-n1", "hot", 0): ("k_filter_step", 512, False, 2048, 0, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("edge-n2049", "hot", 1): ("k_filter_step", 512, False, 2048, 1, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("wl2-512", "hot", 0): ("k_filter_step", 256, False, 512, 0, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("wl2-512", "hot", 2): ("k_filter_step", 256, False, 512, -1, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("wl2-1024", "hot", 1): ("k_filter_step", 512, False, 1024, 1, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("wl2-2048", "hot", 0): ("k_filter_step", 512, False, 2048, 0, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("wl2-2048", "general", 3): ("k_filter_step", 512, False, 2048, -1, True, "wave-by-wave in k_filter_step + fused accounting (ticket)"),
    ("inkernel-129", "hot", 0): ("k_filter_step", 256, False, 512, 0, False, "level2_scan in k_filter_step + kf_finalize"),
    ("inkernel-129", "general", 1): ("k_filter_step", 256, False, 512, -1, False, "level2_scan in k_filter_step + fused accounting (ticket)"),
    ("inkernel-forced-1025", "hot", 1): ("k_filter_step", 256, False, 512, 1, False, "level2_scan in k_filter_step + kf_finalize"),
    ("split-forced-5", "hot", 0): ("k_filter_step", 256, True, 512, 0, False, "k_l2_scan_blocks x1 (l2_inkernel), ranges in k_filter_step"),
    ("split-forced-5", "general", 2): ("k_filter_step", 256, True, 512, -1, False, "k_l2_scan_blocks x1 (l2_inkernel), ranges in k_filter_step"),
    ("split-1025", "hot", 0): ("k_filter_step", 256, True, 512, 0, False, "k_l2_scan_blocks x2 (l2_inkernel), ranges in k_filter_step"),
    ("split-2049", "hot", 1): ("k_filter_step", 256, True, 512, 1, False, "k_l2_scan_blocks x3 (l2_inkernel), ranges in k_filter_step"),
    ("tables-5", "hot", 0): ("k_filter_step", 256, True, 512, 0, False, "k_level2_plan"),
    ("tables-5", "general", 0): ("k_filter_step", 256, True, 512, -1, False, "k_level2_plan"),
    ("tables-1025", "hot", 1): ("k_filter_step", 256, True, 512, 1, False, "k_l2_scan_blocks + k_l2_ranges"),
}


def test_route_of_selects_the_listed_instantiations():
    plain = CASES["nan-y"]
    for (route, form, rs), want in TABLE.items():
        assert bc.route_of(plain, ROUTES[route], form, rs) == want, (route, form, rs)
    # step 0 and a schedule other than 1 run the general kernel whatever the flags (hot_config)
    assert bc.route_of(plain, ROUTES["wl2-512"], "hot", 0, t=0)[4] == -1
    assert bc.route_of(CASES["nan-sched3-carried"], ROUTES["wl2-512"], "hot", 0)[4] == -1
    # every branch of launch_small_m, every tile size, both sides of the WL2, split and kMaxTilesPerFilter thresholds are on the list
    hot = {bc.route_of(plain, r, "hot", 0)[0] for r in bc.routes()}
    assert {f"k_filter_series_lane<{k}>" for k in (64, 128, 256, 512)} | {"k_filter_series_small<512,1>", "k_filter_series_small<512,2>"} <= hot
    tiled = [bc.route_of(plain, r, "hot", rs) for r in bc.routes() if r["kind"] != "small" for rs in (0, 1)]
    assert {t[3] for t in tiled} == {512, 1024, 2048} and {t[4] for t in tiled} == {0, 1}
    assert {(t[2], t[5]) for t in tiled} == {(False, True), (False, False), (True, False)}
    B = {r["name"]: bc.shape(plain, r)[2] for r in bc.routes()}
    assert B["wl2-512"] == B["wl2-1024"] == B["wl2-2048"] == 4 and B["inkernel-129"] == 129 == bc.WL2_MAX_TILES + 1
    assert B["split-1025"] == B["inkernel-forced-1025"] == B["tables-1025"] == 1025 == bc.SPLIT_ABOVE_TILES + 1
    assert B["split-2049"] == 2049 == bc.MAX_TILES_PER_FILTER + 1 and B["split-forced-5"] == B["tables-5"] == 5
    for r in bc.routes():
        assert bc.shape(plain, r)[1] == (r["tile"] or 2048)


def test_the_chosen_pairs_cover_the_minimum():
    ids = {bc.pair_id(p) for p in PAIRS}
    for r in bc.routes():
        if r["kind"] != "edge":
            assert {f"{c}@{r['name']}" for c in bc.EVERY_ROUTE} <= ids
    for c in CASES:
        assert {f"{c}@{r}" for r in bc.THREE_ROUTES} <= ids
    assert {f"nan-y@edge-n{n}" for n in (1, 2, 3, 2047, 2049)} <= ids
    y, _ = bc.series(CASES["zeros-y"])
    assert np.signbit(y[1]) and y[1] == 0.0 and not np.signbit(y[0]) and 13.56 in y and -10.36 in y


def _nan_steps(case, T, r):
    e = case["expect"]
    steps = e["nan_steps_r"][r] if "nan_steps_r" in e else e["nan_steps"]
    return tuple(t for t in steps if t < T)


@pytest.mark.parametrize("rs", [0, 1])
@pytest.mark.parametrize("pair", PAIRS, ids=bc.pair_id)
def test_pair_reaches_its_path_and_the_exact_reference_agrees(oracle, pair, rs):
    case, route = pair
    run = bc.oracle_run(oracle, case, route, rs)
    n, tile, B, T = bc.shape(case, route)
    exp = case["expect"]
    ll = np.array([lls for lls, _ in run])                                               # [T, R]
    finite = 0
    for r in range(case["R"]):
        assert tuple(np.flatnonzero(np.isnan(ll[:, r]))) == _nan_steps(case, T, r), (bc.pair_id(pair), r, ll[:, r])
        finite += int(np.isfinite(ll[:, r]).sum())
    if "nan_steps_r" in exp:
        # a bad theta row leaves its neighbours alone: every valid filter is the single-filter oracle at its rep
        th = bc.theta_rows(case)
        y, z = bc.series(case, T)
        for r in [r for r in range(case["R"]) if not exp["nan_steps_r"][r]]:
            solo = oracle.Filter(case["model"], n, th[r], bc.SEED, rep=r, resampler=rs, tile=tile)
            np.testing.assert_array_equal(_bits(solo.run_series(y, z)[1]), _bits(ll[:, r]), err_msg=f"filter {r} alone")
    assert finite >= 1, "every case has a finite step"
    sts = [run[t][1][0] for t in range(T)]
    for t in exp.get("S0_at", ()):
        if t < T:
            assert sts[t]["S"] == 0 and (sts[t]["logw"] is None or bc.no_weight_left(sts[t])), t
    for t in exp.get("m_neg_inf_at", ()):
        if t < T:
            assert sts[t]["m"] == -np.inf, (t, sts[t]["m"])
    for t in exp.get("collapsed_at", ()):
        if t < T and sts[t]["anc"] is not None:
            # a cdf of zeros: every target counts nothing, every ancestor is particle 0
            assert not sts[t]["anc"].any(), (t, np.unique(sts[t]["anc"]))
    if "big_step" in exp and exp["big_step"] < T:
        assert ll[exp["big_step"], 0] < -1e4 and np.isfinite(ll).all()
    if "distinct_at" in exp:
        t, lo, hi = exp["distinct_at"]
        if t < T:
            assert lo <= np.unique(sts[t]["anc"]).size <= hi
    if "one_source_tile_at" in exp and exp["one_source_tile_at"] < T:
        assert (bc.source_span(sts[exp["one_source_tile_at"]]["anc"], tile) == 1).all()
    if "x_nan_from" in exp:
        for t in range(T):
            assert np.isnan(sts[t]["x"]).all() == (t >= exp["x_nan_from"]), t
    if exp.get("x_all_zero"):
        assert all(not st["x"].any() for st in sts) and np.isfinite(ll).all()
    if exp.get("zero_scale") and B > 1:
        st = sts[1]
        with np.errstate(all="ignore"):
            scale = np.exp(st["mb"] - st["m"])
        Ap = bc.rescaled_sums(oracle, st)
        assert ((scale < 2.0 ** -1022)).any() and (Ap == 0).any(), "a tile whose scale is zero or subnormal, a tile sum of zero"
        first_live = int(np.flatnonzero(Ap > 0)[0])
        if route["name"] not in ZERO_TILE_NARROW:
            # T'_j = 0 below the first live tile and the multinomial / stratified bounds of output tile 0 start at t_lo = 0: its source
            # range is [0, first_live], more than kStageTiles tiles -- the global search path, with A / A' = x / 0 on the way
            assert first_live >= bc.STAGE_TILES, first_live
    if case["sched"] > 1:
        for t in range(1, T):
            if sts[t]["anc"] is not None and t % case["sched"] == 0:
                assert sts[t]["anc"].max() < n
    # the exact reference against the oracle, every step of every filter whose log-weights are held
    for r in range(case["R"]):
        held = [t for t in range(T) if run[t][1][r]["logw"] is not None]
        if len(held) < T and case["sched"] == 1:
            # the large shapes keep two states: with a schedule of 1 every step stands alone (prev = log N)
            want = {t: lr.exact_series([run[t][1][r]["logw"]], n, tile)[0] for t in held}
        else:
            want = dict(enumerate(lr.exact_series([run[t][1][r]["logw"] for t in range(T)], n, tile, case["sched"])))

        def log(name, t, err, budget, _held=held):
            print(f"BUDGET oracle {name} t={_held[t]} error {err:.3e} budget {budget:.3e} ratio {err / budget:.4f}")

        bad = lr.check(f"{bc.pair_id(pair)} rs={rs} r={r}", [ll[t, r] for t in held], [want[t] for t in held], log)
        assert not bad, bad


def test_kalman_loglik_is_consistent_with_the_exact_reference(oracle):
    """The linear Gaussian case has an exact likelihood.  STATISTICAL, in distribution only, one loose bound: exp(l_0) of the exact
    reference is the mean of N iid values g(y_0 | x_i), x_i from the stationary law N(0, s^2), so it is unbiased for the Kalman
    filter's p_0 = N(y_0; 0, s^2 + tau^2) with relative variance (E g^2 / (E g)^2 - 1) / N, E g^2 = N(y_0; 0, s^2 + tau^2 / 2) / (2 tau
    sqrt(pi)).  The mean over 30 replicates must lie within five standard errors of 1.  After the 300-sigma observation y_1 = 3.0 a
    filter sits on a handful of particles, so the later steps are only required to stay below the maximum of the observation density,
    log(1 / (tau sqrt(2 pi))), which no weighted mean of it can exceed."""
    case, route = CASES["zero-tile"], ROUTES["split-forced-5"]
    n, tile, _, T = bc.shape(case, route)
    y, _ = bc.series(case)
    phi, sig, tau = bc.TH_LG
    _, kal = oracle.kalman_loglik(phi, sig, tau, y)
    s2 = sig * sig / (1.0 - phi * phi)
    norm = lambda v, var: np.exp(-0.5 * v * v / var) / np.sqrt(2.0 * np.pi * var)
    p0 = norm(y[0], s2 + tau * tau)
    assert abs(np.log(p0) - kal[0]) < 1e-12
    reps = 30
    rel_var = (norm(y[0], s2 + tau * tau / 2.0) / (2.0 * tau * np.sqrt(np.pi)) / p0 ** 2 - 1.0) / n
    l0 = []
    for rep in range(reps):
        f = oracle.Filter(case["model"], n, bc.TH_LG, bc.SEED, rep=rep, tile=tile)
        lls, lws = [], []
        for t in range(T):
            lls.append(f.step(y[t]))
            lws.append(f.state()["logw"])
        ex = lr.exact_series(lws, n, tile)
        assert not lr.check(f"rep {rep}", lls, ex)
        assert max(e for e, _ in ex) <= np.log(1.0 / (tau * np.sqrt(2.0 * np.pi))) + 1e-12
        l0.append(ex[0][0])
    ratio = np.mean(np.exp(np.array(l0) - kal[0]))
    print("kalman: mean exp(l_0) / p_0 =", ratio, "standard error", np.sqrt(rel_var / reps))
    assert abs(ratio - 1.0) <= 5.0 * np.sqrt(rel_var / reps), ratio


def test_exact_sum_is_exact():
    """The rational sum against a hand-made case that long-double addition gets wrong in any order."""
    w = np.array([1.0, 2.0 ** -64, 2.0 ** -70, 2.0 ** -70], dtype=lr.LD)
    assert lr._exact_sum(w) == lr.LD(1.0) + lr.LD(2.0) ** -63                          # 2^-64 + 2^-69: above the tie, one unit of 2^-63; added in this order in long double it is 1
    assert np.isnan(lr.lse_exact([np.nan, 0.0], 2048)[0]) and np.isnan(lr.lse_exact([-np.inf, -np.inf], 2048)[0])
    lse, err = lr.lse_exact([0.0, 0.0, -np.inf], 2048)
    assert abs(float(lse) - np.log(2.0)) < 1e-18 and 0 < err < 1e-11
    assert lr.rg_of(300, 2048) == 41 and lr.rg_of(2049, 2048) == 40 and lr.rg_of(1024 * 512 + 1, 512) == 32
