"""The inputs at which the forecast kernels (csrc/forecast.h; ssme_pf_sim_future_obs / ssme_lw_sim_future_obs of csrc/pf_api.hip) are
pinned by tests/test_forecast_edges_gpu.py, and what each must show.  test_fc_edges_cpu.py walks the same lists without a GPU, on the
oracle's states and the numpy restatement of tests/forecast_ref.py.  Written before any device ran a case.

Bootstrap.  A forecast always runs the one-workgroup k_level2_plan into tables of its own, whatever level-2 policy the filter uses,
so the ROUTES of bs_edge_cases.py matter here for the state they leave (which of the double buffers is current, who wrote the tile
sums and maxima, the tile size) and for their tile counts: 1, 4, 5, 129, 1025, 2049 -- and one shape of this file's own, plan-16384
(8193 tiles of 512: Bpow2 = 16384, the plan's largest LDS footprint, 2 x 16384 doubles = 128 KiB on top of its scan area).
  * on every route: benign, nan-y, huge-y, zero-tile;  on small-300, wl2-512 and split-forced-5: all 14 cases of bs_edge_cases.cases();
  * plan-16384: one linear Gaussian series of two steps;
  * a forecast after EVERY step, H = 2; above BIG_N particles after the last two steps only (the oracle run keeps two states), H = 1.
The observation handed over as last_obs is the step's own (a NaN observation is a NaN last_obs; its filter is dead anyway).

expect(case): `dead` = the (step, filter) pairs whose forecast must be all NaN with start == 0 (the step's weights leave S' = 0:
a NaN tile maximum, every log-weight -inf, carried NaN weights); every other pair must be finite.  `few_start` = (step, lo, hi):
the number of distinct start ancestors there (the cloud that kept a handful of weights after the 1e3 observation).
`ratio_nonfinite` = the step after which A / A' holds an inf or NaN (zero-tile on routes of more than one tile).

Liu-West.  Every case of lw_edge_cases.cases() (25 x both forms) in lock-step with oracle.LWFilter, a forecast after every step
(H = 2); mid-path and split-path (587 and 1026 tiles: the first shapes at which k_lw_mom_totals sums many tiles of the forecast's
own partials, and the split level-2 policy of the filter) after the last step only, H = 1; and nan-y-R3 again with
first_filter_id = 5.  lw_expect(case): `dead` steps as above; `L_zero` = tril(L) of the forecast's proposal is exactly 0 at every
live step (delta = 1: 1 - a^2 = 0; point priors: a cloud of one point)."""
import numpy as np

import bs_edge_cases as bc
import expect_ref as er
import forecast_ref as fr
import lw_edge_cases as lc

H_SMALL, H_BIG = 2, 1
TH_LG_PLAN = (0.9, 0.4, 0.7)
PLAN_ROUTE = bc._r("plan-16384", "tiled", 8192 * 512 + 1, 512)
PLAN_CASE = bc._c("plan-lg", model=bc.MODEL_LIN_GAUSS, theta=TH_LG_PLAN, T=2, y=(0.3, -0.2), expect=dict(nan_steps=()))
BENIGN = bc._c("benign", expect=dict(nan_steps=()))
EVERY_ROUTE = ("benign", "nan-y", "huge-y", "zero-tile")
THREE_ROUTES = bc.THREE_ROUTES
FEW_START = {"huge-y": (2, 1, 3)}
RATIO_NONFINITE = {"zero-tile": 1}


def cases():
    return [BENIGN] + bc.cases()


def routes():
    return bc.routes() + [PLAN_ROUTE]


def pairs():
    cs, out = cases(), []
    for r in bc.routes():
        for c in cs:
            if c["name"] in EVERY_ROUTE or r["name"] in THREE_ROUTES:
                out.append((c, r))
    out.append((PLAN_CASE, PLAN_ROUTE))
    return sorted(out, key=lambda p: (bc.shape(*p)[0], p[1]["tile"], p[0]["name"], p[1]["name"]))


pair_id = bc.pair_id


def forecast_steps(case, route):
    """[(t, H)]: after which steps a forecast is taken, and its horizon."""
    n, _, _, T = bc.shape(case, route)
    return [(t, H_BIG) for t in range(max(T - 2, 0), T)] if n > bc.BIG_N else [(t, H_SMALL) for t in range(T)]


def expect(case, T):
    e = case["expect"]
    per = e["nan_steps_r"] if "nan_steps_r" in e else (e["nan_steps"],) * case["R"]
    dead = {(t, r) for r in range(case["R"]) for t in per[r] if t < T}
    out = dict(dead=dead)
    if case["name"] in FEW_START and FEW_START[case["name"]][0] < T:
        out["few_start"] = FEW_START[case["name"]]
    if case["name"] in RATIO_NONFINITE:
        out["ratio_nonfinite"] = RATIO_NONFINITE[case["name"]]
    if "x_nan_from" in e:
        assert all((t, r) in dead for r in range(case["R"]) for t in range(e["x_nan_from"], T) if per[r])
    return out


# ---- last_obs -------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
LAST_OBS_ROUTES = ("small-300", "wl2-512")
LAST_OBS = [None, 0.0, -0.0, NAN, INF, 1e200, (0.02, NAN, -0.01)]
# the leverage model reads last_obs (R = 3: the vector has one NaN among three); SVOL must ignore it bit for bit
LAST_OBS_CASES = [bc._c("lev-R3", model=bc.MODEL_SVOL_LEVERAGE, theta=bc.TH_LEV, R=3, T=3), bc._c("svol-R3", R=3, T=3)]


def last_obs_expect(model, lo, r):
    """What filter r must show: "as-none" (the bits of last_obs = None), "finite", or "nonfinite" (some sample is not finite; the
    start draw is that of None either way)."""
    v = 0.0 if lo is None else (lo[r] if isinstance(lo, tuple) else lo)
    if model != bc.MODEL_SVOL_LEVERAGE or (v == 0.0 and not np.signbit(v)):
        return "as-none"
    if v == 0.0:
        return "finite"                        # -0.0: (rho sigma) * -0.0 is a zero of either sign, added to a mean that is not zero
    return "finite" if np.isfinite(v) and abs(v) < 1e100 else "nonfinite"


# ---- Liu-West -------------------------------------------------------------------------------------------------------------------
LW_LAST_ONLY = ("mid-path", "split-path")
LW_FIRST5 = "nan-y-R3"


def lw_cases():
    cs = [dict(c, first=0) for c in lc.cases()]
    cs += [dict(c, name=c["name"] + "-first5", first=5) for c in lc.cases() if c["base"] == LW_FIRST5]
    return cs


def lw_forecast_steps(case):
    T = case["T"]
    return [(T - 1, H_BIG)] if case["base"] in LW_LAST_ONLY else [(t, H_SMALL) for t in range(T)]


def lw_expect(case):
    e = case["expect"]
    return dict(dead={(t, r) for t in e.get("nan_steps", ()) for r in range(case["R"])},
                L_zero=e.get("identity") in ("delta1", "point"))


def lw_oracle_filters(oracle, case):
    tr, lo, hi = lc.prior(case, oracle)
    return [oracle.LWFilter(case["n"], lc.SEED, rep=case["first"] + r, delta=case["delta"], transforms=tr, lo=lo, hi=hi, form=case["form"],
                            resamp_sched=case["rs"]) for r in range(case["R"])]


def lw_start_state(oracle, so):
    """The integer cdf, tile sums, tile maxima and rshift of an oracle Liu-West state, as expect_ref.lw_state rebuilds them from the
    second-stage log-weights (the device's cdf of a Liu-West handle is not downloadable)."""
    n = np.asarray(so["logw"]).size
    with np.errstate(all="ignore"):
        ls = er.lw_state(oracle, so)
    B = lc.tiles(n)
    cdf = np.concatenate([np.cumsum(ls["q"][s:s + lc.TILE]) for s in range(0, n, lc.TILE)]).astype(np.uint64)
    return dict(cdf=cdf, A=ls["A"].astype(np.uint64), mb=ls["mb"], rshift=52 - int(np.ceil(np.log2(B * lc.TILE))), q=ls["q"])


def lw_walk(oracle, case):
    if case["first"] == 0:
        return lc.oracle_run(oracle, case)
    ofs = lw_oracle_filters(oracle, case)
    y, z = lc.series(case)
    return [([of.step(y[t], z[t]) for of in ofs], [of.state() for of in ofs]) for t in range(case["T"])]


# ---- the moment anchors ---------------------------------------------------------------------------------------------------------
ANCHOR_N, ANCHOR_SEED, ANCHOR_H = 1 << 16, 0x5eed0000beef, 4
ANCHOR_THETA = {0: (0.8, 0.95, 0.25), 1: (0.97, 0.01, 0.2, -0.8), 2: (0.9, 0.4, 0.3)}


def anchor_series(model, T=20):
    """A series simulated from the model itself (numpy's generator, seed 7): (y[T], z[T] or None)."""
    rng = np.random.default_rng(7)
    th = ANCHOR_THETA[model]
    x, yp, ys = 0.0, 0.0, []
    for _ in range(T):
        e1, e2 = rng.standard_normal(2)
        if model == 2:
            x = th[0] * x + th[1] * e1
            yp = x + th[2] * e2
        elif model == 0:
            x = th[1] * x + th[2] * e1
            yp = th[0] * np.exp(0.5 * x) * e2
        else:
            x = th[1] + th[0] * (x - th[1]) + th[3] * th[2] * yp * np.exp(-0.5 * x) + th[2] * np.sqrt(1.0 - th[0] ** 2) * e1
            yp = np.exp(0.5 * x) * e2
        ys.append(yp)
    y = np.array(ys)
    return y, (np.concatenate([[0.0], y[:-1]]) if model == 1 else None)


# ---- checks shared by the CPU and the GPU module ---------------------------------------------------------------------------------
def check_start(name, st, tile, n, start, seed, rep, t0):
    """start_interval_check of one live filter's start ancestors; prints the budget line and returns the result."""
    q = er.q_from_cdf(st["cdf"], tile)
    res = fr.start_interval_check(q, st["mb"], st["rshift"], tile, fr.start_uniforms(n, seed, rep, t0), start)
    assert res["bad"] == 0 and res["ratio"] <= 1.0, (name, res)
    return res


def budget_line(who, name, res):
    print(f"BUDGET {who} {name} violation/beta {res['ratio']:.4f} beta {res['beta']:.3e} teeth {res['teeth']:.5f}")


def check_anchors(who, model, last_obs, zs):
    for name, z in zs:
        print(f"ANCHOR {who} model {model} last_obs {last_obs} {name} z {z:+.3f}")
    bad = [(name, z) for name, z in zs if not abs(z) <= 5.0]
    assert not bad, bad
