"""The lists of tests/fc_edge_cases.py through the oracle and the numpy restatement of tests/forecast_ref.py alone (no GPU):
  * the vectorised Philox of forecast_ref.py is the oracle's, on the known-answer counters and on 10^4 random ones;
  * every (case, route) reaches what the table says: S' = 0 (a NaN tile maximum included) gives a dead filter -- start 0, NaN samples;
    a dead tile has a non-finite ratio A / A' and is never chosen; the cloud that kept a handful of weights gives that many start
    ancestors; every other (step, filter) is finite;
  * start_interval_check -- the exact reference of the start draw, independent of the two-level search -- holds for the restatement's
    own draw on the oracle's states, with at least 99 % of the particles rejected when their ancestor is moved to the neighbouring
    particle of positive weight on either side (`teeth`); every shape of the lists satisfies it, none had to be dropped;
  * the analytic moment anchors hold for the restatement at N = 2^16;
  * a restated run of 600 horizons at N = 2 stays finite for SVOL and its normals at horizons k and k + 256 differ.
Every interval check prints `BUDGET restatement ...` (profiles/forecast_edge_budgets.txt); the module prints its wall time."""
import time

import numpy as np
import pytest

import bs_edge_cases as bc
import expect_ref as er
import fc_edge_cases as fc
import forecast_ref as fr
import lw_edge_cases as lc

PAIRS = fc.pairs()
LW_CASES = fc.lw_cases()
TEETH = 0.99


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.time()
    yield
    print(f"\nWALL test_fc_edges_cpu.py {time.time() - t0:.1f} s")


# ---- Philox -------------------------------------------------------------------------------------------------------------------------
def test_numpy_philox_is_the_oracles(oracle):
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        assert fr.philox4x32_10(*ctr, *key)[0].tolist() == want == [int(v) for v in oracle.philox(ctr, key)]
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 2 ** 32, (10000, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, 2, dtype=np.uint64)
    ctr[:4, 0] = (0, 1, 2 ** 32 - 1, 2 ** 31)
    got = fr.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], int(key[0]), int(key[1]))
    want = np.array([oracle.philox(c, key) for c in ctr])
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    # the row form of the forecast's counters, horizon word included
    seed = 0x5eed0000beef
    for c3 in (fr.STREAM_START, fr.STREAM_SIM + (599 << 8), fr.STREAM_LW_JIT + (65534 << 8)):
        assert np.array_equal(fr.philox_rows(oracle, np.arange(300), 7, 5, c3, seed), fr.philox_rows_oracle(oracle, np.arange(300), 7, 5, c3, seed))


# ---- the bootstrap list -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=fc.pair_id)
def test_bootstrap_pair_reaches_what_the_table_says(oracle, pair):
    case, route = pair
    run = bc.oracle_run(oracle, case, route, 0)
    n, tile, B, T = bc.shape(case, route)
    exp = fc.expect(case, T)
    y, _ = bc.series(case, T)
    th = bc.theta_rows(case)
    for t, H in fc.forecast_steps(case, route):
        for r in range(case["R"]):
            st, name = run[t][1][r], f"{fc.pair_id(pair)} t={t} r={r}"
            with np.errstate(all="ignore"):
                Ap, Tp, S, ratio = fr.level2(oracle, st["A"], st["mb"], st["rshift"])
            start, xs, ys = fr.forecast_bs(oracle, case["model"], th[r], st, n, tile, bc.SEED, r, t + 1, H, y[t])
            if (t, r) in exp["dead"]:
                assert not S > 0 and not start.any() and np.isnan(xs).all() and np.isnan(ys).all(), name
                continue
            assert S > 0 and S == st["S"], (name, S, st["S"])
            assert np.isfinite(xs).all() and np.isfinite(ys).all(), name
            q = er.q_from_cdf(st["cdf"], tile)
            assert (q[start] > 0).all() and (Ap[start // tile] > 0).all(), name + ": a particle or tile without weight was drawn"
            if exp.get("few_start", (None,))[0] == t:
                assert exp["few_start"][1] <= np.unique(start).size <= exp["few_start"][2], (name, np.unique(start).size)
            if exp.get("ratio_nonfinite") == t and B > 1:
                assert (Ap == 0).any() and not np.isfinite(ratio[Ap == 0]).any() and np.isfinite(ratio[Ap > 0]).all(), name
                if B >= 4 and route["name"] not in ("wl2-1024", "wl2-2048"):       # as test_bs_edges_cpu.ZERO_TILE_NARROW; edge-n2049 has two tiles
                    assert int(np.flatnonzero(Ap > 0)[0]) >= 3, name
            res = fc.check_start(name, st, tile, n, start, bc.SEED, r, t + 1)
            fc.budget_line("restatement", name, res)
            assert res["teeth"] >= TEETH, (name, res)


def test_the_bootstrap_list_covers_the_issue():
    ids = {fc.pair_id(p) for p in PAIRS}
    for r in bc.routes():
        assert {f"{c}@{r['name']}" for c in fc.EVERY_ROUTE} <= ids
    for c in fc.cases():
        assert {f"{c['name']}@{r}" for r in fc.THREE_ROUTES} <= ids
    assert len(fc.cases()) == 15 and len(bc.routes()) == 22 and "plan-lg@plan-16384" in ids
    n, tile, B, T = bc.shape(fc.PLAN_CASE, fc.PLAN_ROUTE)
    assert (tile, B, T) == (512, 8193, 2) and 1 << (B - 1).bit_length() == 16384
    assert fc.forecast_steps(fc.PLAN_CASE, fc.PLAN_ROUTE) == [(0, 1), (1, 1)]
    assert fc.forecast_steps(fc.BENIGN, bc.routes()[4]) == [(t, 2) for t in range(6)]
    assert [fc.last_obs_expect(1, v, 1) for v in fc.LAST_OBS] == ["as-none", "as-none", "finite", "nonfinite", "nonfinite", "nonfinite", "nonfinite"]
    assert {fc.last_obs_expect(0, v, r) for v in fc.LAST_OBS for r in range(3)} == {"as-none"}
    assert len(LW_CASES) == 2 * 25 + 2 and sum(c["first"] == 5 for c in LW_CASES) == 2


# ---- the Liu-West list --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LW_CASES, ids=lambda c: c["name"])
def test_liu_west_case_reaches_what_the_table_says(oracle, case):
    run = fc.lw_walk(oracle, case)
    exp, n = fc.lw_expect(case), case["n"]
    for t, H in fc.lw_forecast_steps(case):
        for r in range(case["R"]):
            so, name = run[t][1][r], f"{case['name']} t={t} r={r}"
            st = fc.lw_start_state(oracle, so)
            with np.errstate(all="ignore"):
                start, alive = fr.start_draw(oracle, st, n, lc.TILE, lc.SEED, case["first"] + r, t + 1)
            assert alive == ((t, r) not in exp["dead"]) == (not lc.zero_denominator(so)), name
            if not alive:
                assert not start.any(), name
                continue
            assert (st["q"][start] > 0).all(), name
            res = fc.check_start(name, st, lc.TILE, n, start, lc.SEED, case["first"] + r, t + 1)
            fc.budget_line("restatement", name, res)
            assert res["teeth"] >= TEETH, (name, res)
            if exp["L_zero"] and t >= 1:
                th = so["theta"][:, start.astype(np.int64)]
                if case["expect"].get("identity") == "point":
                    assert (th == th[:, :1]).all(), name                      # one point: no spread to factor


# ---- the moment anchors on the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,last_obs", [(2, 0.0), (0, 0.0), (1, 0.02), (1, 0.0)])
def test_moment_anchors_hold_for_the_restatement(oracle, model, last_obs):
    y, z = fc.anchor_series(model)
    f = oracle.Filter(model, fc.ANCHOR_N, fc.ANCHOR_THETA[model], fc.ANCHOR_SEED)
    for t in range(y.size):
        f.step(y[t], 0.0 if z is None else z[t])
    so = f.state()
    tile = f.tile
    start, xs, ys = fr.forecast_bs(oracle, model, fc.ANCHOR_THETA[model], so, fc.ANCHOR_N, tile, fc.ANCHOR_SEED, 0, y.size, fc.ANCHOR_H, last_obs)
    w = er.weights_ref(oracle, er.make_state(oracle, so, tile))
    zs = fr.moment_anchors(model, fc.ANCHOR_THETA[model], xs, ys, x_start=so["x"][start], last_obs=last_obs, w=w, xw=so["x"])
    assert len(zs) >= 2 * fc.ANCHOR_H
    fc.check_anchors("restatement", model, last_obs, zs)
    # the anchors have teeth: a dropped scale, a dropped exp(x / 2) or a wrong y_prev is many standard errors out
    if model == 0:
        assert max(abs(z) for _, z in fr.moment_anchors(0, fc.ANCHOR_THETA[0], xs, ys / fc.ANCHOR_THETA[0][0], w=w, xw=so["x"])) > 20.0
    if model == 2:
        assert max(abs(z) for _, z in fr.moment_anchors(2, fc.ANCHOR_THETA[2], xs, xs + (ys - xs) / fc.ANCHOR_THETA[2][2])) > 20.0
    if model == 1 and last_obs:
        wrong = fr.moment_anchors(1, fc.ANCHOR_THETA[1], xs[:1], ys[:1], x_start=so["x"][start], last_obs=0.0)
        assert max(abs(z) for _, z in wrong) > 8.0, wrong


# ---- the horizon counter -----------------------------------------------------------------------------------------------------------
def test_six_hundred_horizons_at_two_particles(oracle):
    H, n, seed = 600, 2, bc.SEED
    f = oracle.Filter(0, n, bc.TH_SVOL, seed)
    y, _ = bc.series(fc.BENIGN, 2)
    for v in y:
        f.step(v)
    so = f.state()
    start, xs, ys = fr.forecast_bs(oracle, 0, bc.TH_SVOL, so, n, f.tile, seed, 0, 2, H)
    assert np.isfinite(xs).all() and np.isfinite(ys).all()
    zs = np.array([fr.horizon_normals(oracle, np.arange(n), 2, 0, k, seed) for k in range(H)])          # [H, 2, n]
    assert not (zs[:H - 256] == zs[256:]).any()
    assert not np.array_equal(ys[:H - 256], ys[256:])
