"""The bootstrap step kernels (csrc/pf_kernels.h: k_filter_step, kf_finalize, k_level2_plan, k_l2_scan_blocks, k_l2_ranges; csrc/pf_small.h:
k_filter_series_lane, k_filter_series_small) at the degenerate inputs of tests/bs_edge_cases.py, on every route through the code that
file lists: NaN, 1e200, -1e160 and 1e3 observations, a NaN covariate, theta rows that are invalid from step 0, tile scales that underflow
to zero, schedules that carry NaN log-weights, N = 1, 2, 3, 2047, 2049.  For every chosen (case, route) the device must return the
oracle's bits: through the step API in debug mode (the GENERAL kernel, RS = -1, resamplers 0-3: particles, log-weights, integer cdf, tile
sums and maxima, m, S, ancestors and the log conditional likelihood, NaN for NaN, at every step) and through run_series without debug
flags (the HOT instantiations RS = 0 / 1 and the one-launch kernels: per_step(), the sum, final particles, cdf, m and S; a second pass on
the same handle; captured graph and eager launches).  The read-outs (expectations, expectations_multi, weights()) after a degenerate step
are held to the budgets of expect_ref.py, all NaN -- E[42] included -- where no weight is left; the log conditional likelihood of the
DEVICE'S OWN log-weights to the exact reference of loglik_ref.py -- redundant while the bits equal the oracle's, kept so that a failure
says whether device and oracle disagree with each other or with the definition.  test_bs_edges_cpu.py proves without a GPU that each
pair reaches its path and that route_of() names the instantiation below.

    route                  N        tile  B     hot form (run_series, no flags)                        level-2 of the hot form
    small-1 / -64          1, 64    2048  1     k_filter_series_lane<64>                               in the time loop
    small-100              100      2048  1     k_filter_series_lane<128>                              "
    small-200              200      2048  1     k_filter_series_lane<256>                              "
    small-300              300      2048  1     k_filter_series_lane<512>                              "
    small-1000             1000     2048  1     k_filter_series_small<512, 1>                          "
    small-2000             2000     2048  1     k_filter_series_small<512, 2>                          "
    edge-n1 .. edge-n2049  1..2049  2048  1, 2  k_filter_step<512, BIG=0, 2048, RS, WL2=1>             wave by wave + kf_finalize
    wl2-512                1613     512   4     k_filter_step<256, BIG=0, 512, RS, WL2=1>              wave by wave + kf_finalize
    wl2-1024               3149     1024  4     k_filter_step<512, BIG=0, 1024, RS, WL2=1>             "
    wl2-2048               6221     2048  4     k_filter_step<512, BIG=0, 2048, RS, WL2=1>             "
    inkernel-129           65537    512   129   k_filter_step<256, BIG=0, 512, RS, WL2=0>              level2_scan + kf_finalize
    inkernel-forced-1025   524289   512   1025  k_filter_step<256, BIG=0, 512, RS, WL2=0>              level2_scan (two entries per thread)
    split-forced-5         2125     512   5     k_filter_step<256, BIG=1, 512, RS, WL2=0>              k_l2_scan_blocks x 1, one launch
    split-1025             524289   512   1025  "                                                       k_l2_scan_blocks x 2, one launch
    split-2049             1048577  512   2049  "                                                       k_l2_scan_blocks x 3, one launch
    tables-5               2125     512   5     "                                                       k_level2_plan
    tables-1025            524289   512   1025  "                                                       k_l2_scan_blocks + k_l2_ranges
RS = 0 / 1 for resamplers 0 / 1 from step 1 on (step 0 and every step of a schedule other than 1 run RS = -1); the general form runs
the same row with RS = -1 and, where the level-2 is in the kernel, the fused accounting of the step API's ticket; on the small routes
the general form is k_filter_step<512, BIG=0, 2048, -1, WL2=1> (the step API never takes the one-launch kernels).

Why no search can hang, and none leaves its arrays, on NaN tile maxima or a cdf of zeros (read from the code before the first run):
  * every loop has a trip count fixed by the shape, never by the data: count_less_pow2 halves a power-of-two step down to 1;
    lds_count_search and count_less_radix8<P, NQ> are unrolled at compile time; the 64-ary descent of the one-launch split is three rounds
    (strides 256, 4, 1); count_from of k_level2_plan doubles `sz` only while p + sz - 1 < Bpow2 (at most log2 Bpow2 times) and then
    halves it; k_l2_ranges halves Bpow2 down to 1; series_accounting and the time loops run T times.  No loop waits for a value;
    the two tickets (step API, l2_ticket) are counted once per workgroup and reset by the last arriver whatever the data are.
    A comparison with NaN is false, so a NaN target or a NaN element counts nothing.
  * level-2 (level2_scan, the wave-by-wave form, k_level2_plan, k_l2_scan_blocks, the one-tile form of pf_small.h): the maximum is NaN
    if any tile maximum is (block_max_nanprop / the ballot), dexp_scaled_t clamps a NaN argument -- m_b - m with either NaN, or
    -inf - -inf -- to 0, so A'_b = rint(A_b * 0) = 0 and S = 0: never NaN, never negative.  Every accounting site (k_filter_step
    ~849 and ~1255, kf_finalize, k_level2_plan, k_l2_scan_blocks, k_l2_ranges, series_accounting) writes (S > 0) ? ... : NaN.
  * tile_target_bounds with S = 0: t_scale = 0 / G (G > 0, a sum of Gamma draws) or 0 / N = 0, t_lo = 0 and t_hi = 0 or 2: no T'
    is below 0, every T' = 0 is below 2, so lo = 0 and hi <= B; both are clamped to B - 1 where they are read (k_filter_step ~877,
    the tables of k_level2_plan / k_l2_ranges when written) and hi >= lo because both count the same nondecreasing T' against
    t_lo <= t_hi.  count_from(prev, t_lo) assumes t_lo(b) >= t_lo(b - 1): pgam is a prefix sum of positive draws and t_scale >= 0, so
    the bounds are monotone for every S >= 0; a wrong lower bound could only move a count, not an address (clamped as above).
  * the window of the one-launch split (l2w0 .. l2w0 + 63, clamped to [0, B - 64]) is read under `l2w0 + tid < B`; its descent reads
    l2Tg(j) under `j < B` and its counts are clamped to B - 1 afterwards.
  * span = hi - lo + 1 <= 3 stages tiles lo .. hi <= B - 1 of the padded cdf (the loads of tiles 2 and 3 are guarded by span); inside
    staged_search the tile select is clamped to span - 1, a count is at most TILE - 1 (the sum of the unrolled steps), the window start
    is clamped to [tile start, tile start + TILE - W]: every LDS address lies in the three staged tiles.  A longer span takes the
    global path: the tile index is clamped to B - 1, the in-tile count is at most TILE - 1, and A / A' = x / 0 = inf or 0 / 0 = NaN makes
    the in-tile target NaN or (0 * inf) NaN: count 0.  Every resulting index is clamped to N - 1 before it is a gather address
    (k_filter_step ~1052, ~1074; pf_small.h ~213, ~455).
  * NaN particles or log-weights are only ever VALUES: no index is computed from x, y, z or logw.
The reading found no unclamped index and no unbounded loop.  The NaN and inf cases run first when this module is run in two
invocations (-k "nan or inf or bad" / -k "not (nan or inf or bad)")."""
import numpy as np
import pytest

import bs_edge_cases as bc
import expect_cases as ec
import expect_ref as er
import loglik_ref as lr
import test_expectations_gpu as teg
from test_liu_west_edges_gpu import same_bits

pytestmark = pytest.mark.gpu
sa = teg.sa
CASES = {c["name"]: c for c in bc.cases()}
ROUTES = {r["name"]: r for r in bc.routes()}


def _shape_major(items):
    """Tests of one shape follow each other, so that the three routes of 1025 tiles share one oracle run per (case, resampler)."""
    return sorted(items, key=lambda it: (bc.shape(it[0][0], it[0][1])[0], it[0][1]["tile"], it[0][0]["name"], it[1], it[0][1]["name"]) + tuple(it[2:]))


GENERAL = _shape_major([(p, rs) for p in bc.pairs() for rs in (0, 1, 2, 3)])
# the one-launch kernels are not captured in a graph: the small routes run eagerly only
HOT = _shape_major([(p, rs, graph) for p in bc.pairs() for rs in (0, 1) for graph in ((False,) if p[1]["kind"] == "small" else (False, True))])


def _gid(it):
    return bc.pair_id(it[0]) + f"-rs{it[1]}" + ("" if len(it) < 3 else ("-graph" if it[2] else "-eager"))


def make(sa, case, route, rs, debug, graph=None, seed=bc.SEED, small=None):
    n = route["n"]
    b = sa.ParticleFilterBank(case["model"], n, case["R"], seed, rs, case["sched"], tile=route["tile"])
    assert (b.tile, b.n_tiles) == bc.shape(case, route)[1:3]
    if not (route["small"] if small is None else small):
        b.set_small_series(False)
    b.set_debug(debug, debug, split_level2=route["split"])
    if graph is not None:
        b.set_graph_mode(graph)
    b.set_params(bc.theta_rows(case))
    return b


def compare_state(g, o, name, anc, logw=True):
    """The device's download against the oracle's state, bit for bit; arrays the oracle run no longer holds are skipped."""
    if o["x"] is not None:
        same_bits(g["x"], o["x"], name + ": particles")
        if logw:
            same_bits(g["logw"], o["logw"], name + ": log-weights")
        np.testing.assert_array_equal(g["cdf"], o["cdf"], err_msg=name + ": integer cdf")
        if anc:
            np.testing.assert_array_equal(g["anc"], o["anc"], err_msg=name + ": ancestors")
    np.testing.assert_array_equal(g["A"], o["A"], err_msg=name + ": tile sums")
    same_bits(g["mb"], o["mb"], name + ": tile maxima")
    same_bits([g["m"]], [o["m"]], name + ": maximum")
    assert g["S"] == o["S"] and g["rshift"] == o["rshift"], (name, g["S"], o["S"])


def check_readouts(bank, oracle, so, tile, r, name):
    """expectations, expectations_multi and weights() of filter r against the oracle state `so` (expect_ref.py's budgets)."""
    em = bank.expectations_multi([0, 1, 2, 3])
    for kind in range(4):
        same_bits(bank.expectations(kind), em[kind], name + ": single == multi")
    x, w = bank.weights(r)
    same_bits(x, so["x"], name + ": weights() particles")
    if bc.no_weight_left(so):
        # no weight left: every expectation is 0 / 0, E[42] included.  A NaN maximum makes every weight NaN (k_weights); log-weights
        # that are all -inf have q = 0 exactly and a maximum that is not NaN: weights of 0
        assert np.isnan(em[:, r]).all(), (name, em[:, r])
        np.testing.assert_array_equal(np.isnan(w), np.full(w.shape, bool(np.isnan(so["m"]))), err_msg=name + ": NaN pattern of weights()")
        if not np.isnan(so["m"]):
            assert not w.any(), name
        return
    st = er.make_state(oracle, so, tile)
    teg.check_rows(name, em[:, r], ec.builtin_rows(oracle, st["x"]), st, "expect")
    teg.check_weights(name, w, oracle, st)


def probes(case, T):
    """The steps after which the read-outs are taken: every step that leaves no weight (the series "stopped at the NaN step"), the step
    of the extreme observation, the step with underflowed tile scales, and the last."""
    e = case["expect"]
    p = set(e.get("S0_at", ())) | {T - 1}
    if "big_step" in e:
        p.add(e["big_step"])
    if e.get("zero_scale"):
        p.add(1)
    if "nan_steps_r" in e:
        p.add(0)
    return {t for t in p if t < T}


def device_budget_log(name, t, err, budget):
    print(f"BUDGET device {name} t={t} error {err:.3e} budget {budget:.3e} ratio {err / budget:.4f}")


@pytest.mark.parametrize("item", GENERAL, ids=_gid)
def test_general_form_step_api(sa, oracle, item):
    (case, route), rs = item
    run = bc.oracle_run(oracle, case, route, rs)
    n, tile, B, T = bc.shape(case, route)
    R, name = case["R"], _gid(item)
    y, z = bc.series(case, T)
    assert bc.route_of(case, route, "general", rs)[4] == -1
    g = make(sa, case, route, rs, True)
    dev_ll = np.empty((R, T))
    dev_lw = [[] for _ in range(R)]
    heavy = n <= bc.BIG_N or rs == 0                       # the long-double references above 10^5 particles: once per pair
    for t in range(T):
        dev_ll[:, t] = g.step(y[t], None if z is None else z[t])
        same_bits(dev_ll[:, t], run[t][0], f"{name} t={t}: log conditional likelihood")
        resampled = t > 0 and t % case["sched"] == 0
        for r in range(R):
            gs, so = g.state(r, ancestors=True), run[t][1][r]
            compare_state(gs, so, f"{name} t={t} r={r}", resampled)
            if resampled:
                assert gs["anc"].max() < n
            if heavy:
                dev_lw[r].append(gs["logw"])
            if heavy and t in probes(case, T) and so["x"] is not None:
                check_readouts(g, oracle, so, tile, r, f"{name} t={t} r={r}")
    same_bits(g.loglik(), np.array([sum((run[t][0][r] for t in range(T)), 0.0) for r in range(R)]), name + ": loglik()")
    g.close()
    if heavy:
        for r in range(R):
            bad = lr.check(f"{name} r={r}", dev_ll[r], lr.exact_series(dev_lw[r], n, tile, case["sched"]), device_budget_log)
            assert not bad, bad


@pytest.mark.parametrize("item", HOT, ids=_gid)
def test_hot_form_run_series(sa, oracle, item):
    (case, route), rs, graph = item
    run = bc.oracle_run(oracle, case, route, rs)
    n, tile, B, T = bc.shape(case, route)
    R, name = case["R"], _gid(item)
    y, z = bc.series(case, T)
    want_ll = np.array([[run[t][0][r] for t in range(T)] for r in range(R)])
    want_sum = np.array([sum((run[t][0][r] for t in range(T)), 0.0) for r in range(R)])
    s = make(sa, case, route, rs, False, graph)
    for again in (False, True):
        tot = s.run_series(y, z)
        tag = name + (" (second pass)" if again else "")
        same_bits(s.per_step(), want_ll, tag + ": per_step()")
        same_bits(tot, want_sum, tag + ": the returned sum")
        assert (np.isnan(tot) == np.isnan(want_ll).any(axis=1)).all()
        for r in range(R):
            compare_state(s.state(r, logw=False), run[T - 1][1][r], f"{tag} r={r}", False, logw=False)
    if n <= bc.BIG_N:
        for r in range(R):
            check_readouts(s, oracle, run[T - 1][1][r], tile, r, f"{name} series r={r}")
    if route["kind"] == "small":
        # path invariance: the one-launch kernel == the tiled kernel on the same handle shape
        t2 = make(sa, case, route, rs, False, small=False)
        same_bits(t2.run_series(y, z), tot, name + ": small-series == tiled, sum")
        same_bits(t2.per_step(), s.per_step(), name + ": small-series == tiled, per_step()")
        for r in range(R):
            a, b = t2.state(r, logw=False), s.state(r, logw=False)
            same_bits(a["x"], b["x"], "small-series == tiled: particles")
            np.testing.assert_array_equal(a["cdf"], b["cdf"], err_msg="small-series == tiled: cdf")
        t2.close()
    s.close()


INVARIANCE = [(c, shape, rs) for shape in ("5", "1025") for c in bc.EVERY_ROUTE for rs in (0, 1)]


@pytest.mark.parametrize("cname,shape,rs", INVARIANCE, ids=lambda v: str(v))
def test_level2_paths_agree(sa, cname, shape, rs):
    """Path invariance at one N and tile: forced one-launch split == table kernels == in-kernel level-2, with and without debug flags."""
    case = CASES[cname]
    trio = [ROUTES[f"split-forced-5"], ROUTES["tables-5"], dict(ROUTES["split-forced-5"], split=False)] if shape == "5" else \
        [ROUTES["split-1025"], ROUTES["tables-1025"], ROUTES["inkernel-forced-1025"]]
    T = bc.shape(case, trio[0])[3]
    y, z = bc.series(case, T)
    for debug in (False, True):
        outs = []
        for route in trio:
            b = make(sa, case, route, rs, debug)
            tot = b.run_series(y, z)
            st = b.state(0, ancestors=debug, logw=debug)
            outs.append((tot, b.per_step(), st))
            b.close()
        for tot, per, st in outs[1:]:
            same_bits(tot, outs[0][0], "sum")
            same_bits(per, outs[0][1], "per_step()")
            same_bits(st["x"], outs[0][2]["x"], "particles")
            np.testing.assert_array_equal(st["cdf"], outs[0][2]["cdf"])
            np.testing.assert_array_equal(st["A"], outs[0][2]["A"])
            same_bits([st["m"]], [outs[0][2]["m"]], "m")
            assert st["S"] == outs[0][2]["S"]
            if debug:
                np.testing.assert_array_equal(st["anc"], outs[0][2]["anc"])
                same_bits(st["logw"], outs[0][2]["logw"], "log-weights")


@pytest.mark.parametrize("reseed", [False, True], ids=["same-seed", "set_seed"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("rname", ["small-300", "wl2-512", "inkernel-129", "split-forced-5", "tables-5"])
def test_handle_recovers_after_a_nan_series(sa, oracle, rname, graph, reseed):
    """run_series(NaN series), then run_series(clean series) on the SAME handle (the captured graph is replayed, l2_ticket and the step
    API's ticket must be zero between launches) equals a fresh handle bit for bit -- also with set_seed between the two -- and the oracle."""
    route = ROUTES[rname]
    bad, clean = CASES["nan-y"], dict(CASES["nan-y"], y_set={})
    yb, _ = bc.series(bad)
    yc, _ = bc.series(clean)
    seed = bc.SEED + 1 if reseed else bc.SEED
    for rs in (0, 1):
        h = make(sa, bad, route, rs, False, graph)
        assert np.isnan(h.run_series(yb)).all() and np.isnan(h.per_step()[0, 2])
        if reseed:
            h.set_seed(seed)
        fresh = make(sa, clean, route, rs, False, graph, seed=seed)
        tot, want = h.run_series(yc), fresh.run_series(yc)
        assert np.isfinite(want).all()
        same_bits(tot, want, f"{rname} rs={rs}: the sum after a NaN series")
        same_bits(h.per_step(), fresh.per_step(), "per_step() after a NaN series")
        a, b = h.state(0, logw=False), fresh.state(0, logw=False)
        same_bits(a["x"], b["x"], "particles after a NaN series")
        np.testing.assert_array_equal(a["cdf"], b["cdf"])
        n, tile, _, _ = bc.shape(clean, route)
        po = oracle.Filter(clean["model"], n, bc.TH_SVOL, seed, resampler=rs, tile=tile).run_series(yc)[1]
        same_bits(h.per_step()[0], po, "the clean series against the oracle")
        # and the step API on the recovered handle: one more NaN step and one clean step, as a fresh handle takes them
        for yv in (float("nan"), 0.01):
            same_bits(h.step(yv), fresh.step(yv), "step API after the series")
        h.close()
        fresh.close()
