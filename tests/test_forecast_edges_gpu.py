"""The forecast kernels (csrc/forecast.h: k_fc_start_vec, k_fc_horizon, k_fc_lw_start, k_fc_lw_prop, k_fc_lw_horizon; the k_level2_plan and
k_lw_mom_totals launches of ssme_pf_sim_future_obs / ssme_lw_sim_future_obs in csrc/pf_api.hip) at the inputs of tests/fc_edge_cases.py,
through the C ABI.  For every pair of that list:
  * start, x and y equal the numpy restatement of tests/forecast_ref.py to the bit (NaN for NaN, -0 != +0).  The bootstrap side starts
    from the device's own state(), whose bits are compared with the oracle's first; the Liu-West side from an oracle.LWFilter in
    lock-step, after a bit comparison of particles and parameters;
  * all NaN with start == 0 exactly where the table says, finite everywhere else, status 0; the healthy filters beside a dead one
    equal a handle of their own;
  * start_interval_check (the exact reference of the start draw, independent of the two-level search) on the DEVICE'S start
    ancestors; every check prints `BUDGET device ...` (profiles/forecast_edge_budgets.txt);
  * Liu-West: lw_moments_ref.check_proposal of the proposal the device used, over the gathered start population; tril(L) exactly 0
    where listed.
Further: the step API with forecasts after every step equals the series without (also run_series followed by the step API); the
level-2 policies of one shape leave the same forecast; one handle called with H = 2, 17, 2, 1 (y only, then with states) equals
fresh handles; 600 horizons at N = 2 and N = 1; set_seed; f32 handles; the analytic moment anchors of forecast_ref.moment_anchors
at N = 2^16 (`ANCHOR device ...`); a large handle beside a small one.

Bounds, read before the first run: k_level2_plan writes l2_T / l2_R under j < B into [R][Bs] tables and its LDS under j < Bpow2
(the dynamic size is Bpow2 doubles: 128 KiB at 8193 tiles, under the 160 KiB of a workgroup); fc_draw_ancestor reads T under j < B,
clamps the tile to B - 1, counts at most tile - 1 inside it (an index below Npad) and clamps the ancestor to N - 1 before the gather;
the horizon kernels index by particle only.  No index is computed from a weight, a state or an observation."""
import numpy as np
import pytest

import bs_edge_cases as bc
import fc_edge_cases as fc
import forecast_ref as fr
import lw_edge_cases as lc
import lw_moments_ref as mr
import test_bootstrap_edges_gpu as tbe
import test_expectations_gpu as teg
from fc_edge_cases import budget_line, check_anchors, check_start
from test_liu_west_edges_gpu import same_bits

pytestmark = pytest.mark.gpu
sa = teg.sa
PAIRS = fc.pairs()
LW_CASES = fc.lw_cases()
ROUTES = {r["name"]: r for r in fc.routes()}


def step(bank, y, z, t):
    return bank.step(y[t], None if z is None else z[t])


def equal_outputs(a, b, what):
    for u, v, k in zip(a, b, ("y", "x", "start")):
        if u.dtype == np.uint32:
            np.testing.assert_array_equal(u, v, err_msg=f"{what}: {k}")
        else:
            same_bits(u, v, f"{what}: {k}")


# ---- the bootstrap list -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=fc.pair_id)
def test_bootstrap_pair(sa, oracle, pair):
    case, route = pair
    run = bc.oracle_run(oracle, case, route, 0)
    n, tile, B, T = bc.shape(case, route)
    R, exp, th = case["R"], fc.expect(case, T), bc.theta_rows(case)
    y, z = bc.series(case, T)
    when = dict(fc.forecast_steps(case, route))
    g = tbe.make(sa, case, route, 0, False)
    last = None
    for t in range(T):
        same_bits(step(g, y, z, t), run[t][0], f"{fc.pair_id(pair)} t={t}: log conditional likelihood")
        if t not in when:
            continue
        H = when[t]
        out = g.sim_future_obs(H, y[t], states=True, start=True)                 # status 0: no exception
        ys, xs, start = out
        assert ys.shape == (R, H, n) and start.shape == (R, n) and start.max() < n
        for r in range(R):
            name = f"{fc.pair_id(pair)} t={t} r={r}"
            gs = g.state(r, logw=False)
            tbe.compare_state(gs, run[t][1][r], name, False, logw=False)
            dead = (t, r) in exp["dead"]
            if not dead:
                # the exact reference first: it shares nothing with the restatement below (a misreading of the two-level search
                # common to kernel and restatement would pass the bit comparison)
                budget_line("device", name, check_start(name, gs, tile, n, start[r], bc.SEED, r, t + 1))
            ws, wx, wy = fr.forecast_bs(oracle, case["model"], th[r], gs, n, tile, bc.SEED, r, t + 1, H, y[t])
            np.testing.assert_array_equal(start[r], ws, err_msg=name + ": start")
            same_bits(xs[r], wx, name + ": x")
            same_bits(ys[r], wy, name + ": y")
            if dead:
                assert np.isnan(ys[r]).all() and np.isnan(xs[r]).all() and not start[r].any(), name
                continue
            assert np.isfinite(ys[r]).all() and np.isfinite(xs[r]).all(), name
            if exp.get("few_start", (None,))[0] == t:
                assert exp["few_start"][1] <= np.unique(start[r]).size <= exp["few_start"][2], name
        last = out
    if exp["dead"] and R > 1:
        # the healthy filters beside a dead one: a handle of their own at the same place in the bank
        for r in [r for r in range(R) if (T - 1, r) not in exp["dead"]]:
            alone = sa.ParticleFilterBank(case["model"], n, 1, bc.SEED, 0, case["sched"], first_filter_id=r, tile=route["tile"], n_filters_total=R)
            alone.set_debug(False, False, split_level2=route["split"])
            alone.set_params(th[r])
            for t in range(T):
                step(alone, y, z, t)
            equal_outputs(alone.sim_future_obs(when[T - 1], y[T - 1], states=True, start=True), [o[r:r + 1] for o in last], f"filter {r} alone")
            alone.close()
    g.close()
    # the same forecast from the state run_series leaves (the one-launch kernels on the small routes, the hot instantiations elsewhere)
    s = tbe.make(sa, case, route, 0, False)
    s.run_series(y, z)
    equal_outputs(s.sim_future_obs(when[T - 1], y[T - 1], states=True, start=True), last, fc.pair_id(pair) + ": after run_series")
    s.close()


@pytest.mark.parametrize("case", fc.LAST_OBS_CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("rname", fc.LAST_OBS_ROUTES)
def test_last_obs_values(sa, oracle, rname, case):
    route = ROUTES[rname]
    n, tile, _, T = bc.shape(case, route)
    y, z = bc.series(case, T)
    th = bc.theta_rows(case)
    g = tbe.make(sa, case, route, 0, False)
    for t in range(T):
        step(g, y, z, t)
    base = g.sim_future_obs(2, None, states=True, start=True)
    sts = [g.state(r, logw=False) for r in range(3)]
    for lo in fc.LAST_OBS:
        ys, xs, start = g.sim_future_obs(2, None if lo is None else np.array(lo, dtype=np.float64), states=True, start=True)
        np.testing.assert_array_equal(start, base[2], err_msg=f"last_obs {lo}: the start draw does not read it")
        for r in range(3):
            v = 0.0 if lo is None else (lo[r] if isinstance(lo, tuple) else lo)
            ws, wx, wy = fr.forecast_bs(oracle, case["model"], th[r], sts[r], n, tile, bc.SEED, r, T, 2, v)
            same_bits(xs[r], wx, f"last_obs {lo} r={r}: x")
            same_bits(ys[r], wy, f"last_obs {lo} r={r}: y")
            kind = fc.last_obs_expect(case["model"], lo, r)
            if kind == "as-none":
                same_bits(xs[r], base[1][r], f"last_obs {lo} r={r}: as None")
                same_bits(ys[r], base[0][r], f"last_obs {lo} r={r}: as None")
            elif kind == "finite":
                assert np.isfinite(xs[r]).all() and np.isfinite(ys[r]).all()
            else:
                assert not (np.isfinite(xs[r]).all() and np.isfinite(ys[r]).all())
    g.close()


# ---- the Liu-West list --------------------------------------------------------------------------------------------------------------
def lw_make(sa, oracle, case, **kw):
    tr, lo, hi = lc.prior(case, oracle)
    cls = sa.svol_lw_2_par if case["form"] else sa.svol_lw_1_par
    args = dict(nparts=case["n"], n_filters=case["R"], seed=lc.SEED, first_filter_id=case.get("first", 0), transforms=tuple(tr), rs=case["rs"])
    args.update(kw)
    g = cls(case["delta"], lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], **args)
    if case["split"]:
        g.set_debug(False, split_level2=True)
    return g


def lw_check(oracle, case, g, so, r, t, H, last_obs, out, name, seed=lc.SEED):
    """One filter's forecast against the restatement started from the oracle state `so`."""
    ys, xs, start, prop = out
    n, tr = case["n"], lc.prior(case, oracle)[0]
    rep = case.get("first", 0) + r
    st = fc.lw_start_state(oracle, so)
    with np.errstate(all="ignore"):
        want_start, alive = fr.start_draw(oracle, st, n, lc.TILE, seed, rep, t + 1)
    np.testing.assert_array_equal(start[r], want_start, err_msg=name + ": start")
    L = np.zeros((4, 4))
    L[np.tril_indices(4)] = prop[r, 4:14]
    pop = so["theta"][:, start[r].astype(np.int64)]
    bad = mr.check_proposal(prop[r, :4], L, pop, lc.a_shrink(case["delta"]), lc.tiles(n), name)
    assert not bad, bad
    wx, wy = fr.forecast_lw(oracle, so, start[r], prop[r], tr, case["delta"], n, seed, rep, t + 1, H, last_obs, alive=alive)
    same_bits(xs[r], wx, name + ": x")
    same_bits(ys[r], wy, name + ": y")
    return alive, L, st


@pytest.mark.parametrize("case", LW_CASES, ids=lambda c: c["name"])
def test_liu_west_case(sa, oracle, case):
    run = fc.lw_walk(oracle, case)
    exp, n, R = fc.lw_expect(case), case["n"], case["R"]
    y, z = lc.series(case)
    when = dict(fc.lw_forecast_steps(case))
    g = lw_make(sa, oracle, case)
    for t in range(case["T"]):
        g.filter(y[t], z[t])
        if t not in when:
            continue
        H = when[t]
        out = g.sim_future_obs(H, y[t], states=True, start=True, prop=True)
        assert out[0].shape == (R, H, n) and out[2].max() < n
        for r in range(R):
            name = f"{case['name']} t={t} r={r}"
            so, gs = run[t][1][r], g.state(r)
            same_bits(gs["x"], so["x"], name + ": lock-step particles")
            same_bits(gs["theta"], so["theta"], name + ": lock-step parameters")
            if (t, r) not in exp["dead"]:                                # the exact reference of the start draw before the restatement
                st = fc.lw_start_state(oracle, so)
                budget_line("device", name, check_start(name, st, lc.TILE, n, out[2][r], lc.SEED, case["first"] + r, t + 1))
            alive, L, st = lw_check(oracle, case, g, so, r, t, H, y[t], out, name)
            assert alive == ((t, r) not in exp["dead"]), name
            if not alive:
                assert np.isnan(out[0][r]).all() and np.isnan(out[1][r]).all() and not out[2][r].any(), name
                continue
            assert np.isfinite(out[0][r]).all() and np.isfinite(out[1][r]).all(), name
            if exp["L_zero"]:
                assert not L.any(), (name, L)
    g.close()


# ---- a forecast leaves the filter alone; the level-2 policies leave the same forecast -----------------------------------------------
@pytest.mark.parametrize("rname", ["small-300", "wl2-1024", "inkernel-129", "split-1025", "tables-5"])
def test_forecasts_leave_the_bootstrap_filter_alone(sa, rname):
    case, route = fc.BENIGN, ROUTES[rname]
    n, _, _, T = bc.shape(case, route)
    y, z = bc.series(case, T)
    H = fc.H_BIG if n > bc.BIG_N else fc.H_SMALL

    def series(with_forecasts, head):
        """head: the first `head` steps through run_series, the rest through the step API."""
        b = tbe.make(sa, case, route, 0, False)
        ll = []
        if head:
            b.run_series(y[:head])
            ll += list(b.per_step()[0])
            if with_forecasts:
                b.sim_future_obs(H, y[head - 1], states=True, start=True)
        for t in range(head, T):
            ll.append(step(b, y, z, t)[0])
            if with_forecasts:
                b.sim_future_obs(H, y[t], states=(t % 2 == 0), start=True)
        st = b.state(0, logw=False)
        ex = b.expectations_multi([0, 1, 2, 3])
        b.close()
        return np.array(ll), st, ex

    for head in (0, T - 2):
        (ll0, st0, ex0), (ll1, st1, ex1) = series(False, head), series(True, head)
        same_bits(ll1, ll0, f"{rname} head={head}: per-step log-likelihoods")
        same_bits(ex1, ex0, "expectations_multi")
        same_bits(st1["x"], st0["x"], "particles")
        np.testing.assert_array_equal(st1["cdf"], st0["cdf"])
        same_bits([st1["m"]], [st0["m"]], "m")
        assert st1["S"] == st0["S"]


def test_forecasts_leave_the_liu_west_filter_alone_mid_path(sa, oracle):
    case = dict(next(c for c in LW_CASES if c["name"] == "mid-path-form0"))
    y, z = lc.series(case)

    def series(with_forecasts):
        g = lw_make(sa, oracle, case)
        ll = []
        for t in range(case["T"]):
            g.filter(y[t], z[t])
            ll.append(np.atleast_1d(g.getLogCondLike())[0])
            if with_forecasts:
                g.sim_future_obs(1, y[t], states=(t == 1), start=True, prop=True)
        out = (np.array(ll), g.state(0), g.expectations(list(range(8))), g.param_means())
        g.close()
        return out

    a, b = series(False), series(True)
    same_bits(b[0], a[0], "per-step log-likelihoods")
    for k in ("x", "theta", "thetabar", "L"):
        same_bits(b[1][k], a[1][k], k)
    same_bits(b[2], a[2], "expectations")
    same_bits(b[3], a[3], "param_means")


@pytest.mark.parametrize("trio", [("split-forced-5", "tables-5"), ("inkernel-forced-1025", "split-1025", "tables-1025")], ids=["5", "1025"])
def test_level2_policies_leave_the_same_forecast(sa, trio):
    case = fc.BENIGN
    outs = []
    for rname in trio:
        route = ROUTES[rname]
        n, _, _, T = bc.shape(case, route)
        y, z = bc.series(case, T)
        b = tbe.make(sa, case, route, 0, False)
        for t in range(T):
            step(b, y, z, t)
        outs.append(b.sim_future_obs(fc.H_BIG if n > bc.BIG_N else fc.H_SMALL, y[T - 1], states=True, start=True))
        b.close()
    for rname, o in zip(trio[1:], outs[1:]):
        equal_outputs(o, outs[0], f"{rname} == {trio[0]}")


# ---- call-level state ---------------------------------------------------------------------------------------------------------------
def _lev_bank(sa, n, seed=bc.SEED, steps=3, dtype=0, model=bc.MODEL_SVOL_LEVERAGE, theta=bc.TH_LEV):
    b = sa.ParticleFilterBank(model, n, 1, seed, dtype=dtype)
    b.set_params(theta)
    y, z = bc.series(dict(fc.BENIGN, model=model), steps)
    for t in range(steps):
        step(b, y, z, t)
    return b, y


def test_output_buffers_regrow_separately(sa):
    """fc_cap_y and fc_cap_x: H = 2 (y only), 17 with states, 2 with states, 1: each call equals the same call on a fresh handle."""
    n = 2049
    one, y = _lev_bank(sa, n)
    for H, states in ((2, False), (17, True), (2, True), (1, False)):
        got = one.sim_future_obs(H, y[2], states=states, start=True)
        fresh, _ = _lev_bank(sa, n)
        want = fresh.sim_future_obs(H, y[2], states=states, start=True)
        fresh.close()
        for u, v in zip(got, want):
            assert u.shape == v.shape and np.array_equal(u, v), (H, states)
    one.close()


def _noise_differs(zo, H):
    """The observation normals of horizons k and k + 256, recovered from the outputs, differ for every particle."""
    assert (np.abs(zo[:H - 256] - zo[256:]) > 1e-9).all()


def test_six_hundred_horizons_bootstrap(sa, oracle):
    H, n = 600, 2
    b = sa.ParticleFilterBank(0, n, 1, bc.SEED)
    b.set_params(bc.TH_SVOL)
    y, _ = bc.series(fc.BENIGN, 2)
    for v in y:
        b.step(v)
    ys, xs, start = b.sim_future_obs(H, states=True, start=True)
    ws, wx, wy = fr.forecast_bs(oracle, 0, bc.TH_SVOL, b.state(0, logw=False), n, b.tile, bc.SEED, 0, 2, H)
    np.testing.assert_array_equal(start[0], ws)
    same_bits(xs[0], wx, "x")
    same_bits(ys[0], wy, "y")
    assert np.isfinite(ys).all()
    _noise_differs(ys[0] * np.exp(-0.5 * xs[0]) / bc.TH_SVOL[0], H)
    b.close()


def test_six_hundred_horizons_liu_west(sa, oracle):
    H = 600
    case = dict(next(c for c in LW_CASES if c["name"] == "n1-form0"))
    y, z = lc.series(case)
    g = lw_make(sa, oracle, case)
    o = fc.lw_oracle_filters(oracle, case)[0]
    for t in range(2):
        g.filter(y[t], z[t])
        o.step(y[t], z[t])
    out = g.sim_future_obs(H, y[1], states=True, start=True, prop=True)
    lw_check(oracle, case, g, o.state(), 0, 1, H, y[1], out, "n1 H=600")
    assert np.isfinite(out[0]).all()
    _noise_differs(out[0][0] * np.exp(-0.5 * out[1][0]), H)
    g.close()


def test_set_seed_changes_the_forecast_and_the_same_seed_restores_it(sa):
    b, y = _lev_bank(sa, 2049)
    first = b.sim_future_obs(3, y[2], states=True, start=True)
    outs = []
    for seed in (bc.SEED + 1, bc.SEED):
        b.set_seed(seed)                                                 # resets the filter: the same three steps again
        _, z = bc.series(dict(fc.BENIGN, model=1), 3)
        for t in range(3):
            step(b, y, z, t)
        outs.append(b.sim_future_obs(3, y[2], states=True, start=True))
    assert not np.array_equal(outs[0][0], first[0]) and not np.array_equal(outs[0][2], first[2])
    equal_outputs(outs[1], first, "the same seed")
    b.close()


@pytest.mark.parametrize("model,theta", [(0, bc.TH_SVOL), (2, fc.TH_LG_PLAN)], ids=["svol", "lin-gauss"])
def test_f32_handles(sa, oracle, model, theta):
    n = 2049
    b = sa.ParticleFilterBank(model, n, 1, bc.SEED, dtype=1)
    b.set_params(theta)
    y, _ = bc.series(fc.BENIGN, 4)
    y32 = y.astype(np.float32).astype(np.float64)
    for v in y32:
        b.step(v)
    ys, xs, start = b.sim_future_obs(3, y[3], states=True, start=True)
    ws, wx, wy = fr.forecast_bs(oracle, model, theta, b.state(0, logw=False), n, b.tile, bc.SEED, 0, 4, 3, y[3], f32=True)
    np.testing.assert_array_equal(start[0], ws)
    same_bits(xs[0], wx, "x")
    same_bits(ys[0], wy, "y")
    assert np.array_equal(ys, ys.astype(np.float32)) and np.array_equal(xs, xs.astype(np.float32)) and np.isfinite(ys).all()
    b.close()


@pytest.mark.parametrize("model,last_obs", [(2, 0.0), (0, 0.0), (1, 0.02), (1, 0.0)])
def test_moment_anchors(sa, model, last_obs):
    y, z = fc.anchor_series(model)
    theta = fc.ANCHOR_THETA[model]
    b = sa.ParticleFilterBank(model, fc.ANCHOR_N, 1, fc.ANCHOR_SEED)
    b.set_params(theta)
    b.run_series(y, z)
    ys, xs, start = b.sim_future_obs(fc.ANCHOR_H, last_obs, states=True, start=True)
    xw, w = b.weights(0)
    zs = fr.moment_anchors(model, theta, xs[0], ys[0], x_start=b.state(0, logw=False)["x"][start[0]], last_obs=last_obs, w=w, xw=xw)
    check_anchors("device", model, last_obs, zs)
    b.close()


def test_a_large_handle_beside_a_small_one(sa):
    """Both creations set the dynamic-LDS attribute of k_level2_plan; the large handle's plan (2049 tiles: 32 KiB) must still launch,
    and give the same bits, after a 64-particle handle has set its own value."""
    case, route = fc.BENIGN, ROUTES["split-2049"]
    n, _, _, T = bc.shape(case, route)
    y, z = bc.series(case, T)

    def run(with_small):
        big = tbe.make(sa, case, route, 0, False)
        small = tbe.make(sa, case, ROUTES["small-64"], 0, False) if with_small else None
        ll = [step(big, y, z, t)[0] for t in range(T)]
        out = big.sim_future_obs(1, y[T - 1], states=True, start=True)
        if small is not None:
            small.step(y[0])
            assert np.isfinite(small.sim_future_obs(1)).all()
            small.close()
        big.close()
        return np.array(ll), out

    (ll0, out0), (ll1, out1) = run(False), run(True)
    same_bits(ll1, ll0, "log-likelihoods")
    equal_outputs(out1, out0, "beside a small handle")
