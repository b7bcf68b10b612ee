"""The degenerate inputs at which the bootstrap step kernels are pinned (tests/test_bootstrap_edges_gpu.py), the routes through the
code on which each is run, and the oracle side of each.  test_bs_edges_cpu.py walks the same lists without a GPU and proves from the
oracle's state that every case reaches the path it is listed for (`expect`: what the oracle must show, written down from a run of the
oracle alone, before any device ran the case).  The bootstrap counterpart of lw_edge_cases.py.

A CASE is an input: model, theta (one row, or one row per filter), R, the resampling schedule and the observations.  The base series
is spy_returns.csv[:T] (z its lag, for the leverage model), seed 7; `y_set` / `z_set` overwrite single observations.
A ROUTE is a way through the code: a shape (N, tile), the level-2 policy forced through set_debug, and whether run_series takes the
one-launch small-series kernel.  route_of() derives the kernel instantiation a (route, form, resampler) selects from launch_step_grid /
launch_rs / hot_config / launch_small_m / ssme_pf_set_debug of csrc/pf_api.hip; test_bs_edges_cpu.py asserts it against a table
written out by hand.  FORMS: "hot" = run_series without debug flags (RS = 0 / 1 for resamplers 0 / 1 from step 1 on), "general" = the
step API with set_debug(True, True) (RS = -1 for every resampler).

Which pairs are run (pairs()) -- the full product is 14 cases x 21 routes x 8 form / resampler / graph-mode combinations:
  * nan-y, inf-y, huge-y, zero-tile on EVERY route: the four inputs that drive the level-2 guards (a NaN tile maximum, a weight sum of
    zero, all mass in one tile, tile scales that underflow to zero) through every instantiation and every level-2 kernel;
  * every other case on one small-series route (small-300, the shape of the two tests that were there before), one WL2 route
    (wl2-512: four tiles, one workgroup wave-by-wave level-2) and the forced one-launch split (split-forced-5): they vary the MODEL
    side (what the particles and log-weights are), which no level-2 kernel looks at, so one route of each kind is enough;
  * nan-y on the five N edges of the tiled kernel (N = 1, 2, 3, 2047, 2049 in tiles of 2048 with the small-series kernel switched off).
Routes above 10^5 particles run T = 4 steps (the NaN at step 2, one more step that resamples from the cdf of zeros)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SVOL, MODEL_SVOL_LEVERAGE, MODEL_LIN_GAUSS = 0, 1, 2
TH_SVOL = (1.0, 0.95, 0.25)                    # beta, phi, sigma
TH_LEV = (0.9, 0.0, 1.0, -0.1)                 # phi, mu, sigma, rho
TH_LG = (0.5, 0.1, 0.01)                       # phi, sigma, tau: tiny observation noise
SEED = 7
NAN = float("nan")
ALL6 = (0, 1, 2, 3, 4, 5)

WL2_MAX_TILES = 128                            # launch_rs: a.B <= 128 takes the wave-by-wave level-2 (WL2)
SPLIT_ABOVE_TILES = 1024                       # kSplitLevel2Above
MAX_TILES_PER_FILTER = 2048                    # kMaxTilesPerFilter: above it the split level-2 is the only one
STAGE_TILES = 3                                # kStageTiles
BIG_N = 100000                                 # above: T = 4 and only the last two oracle states kept


def _c(name, model=MODEL_SVOL, theta=TH_SVOL, R=1, T=6, sched=1, y=None, y_set=None, z_set=None, expect=None, big=True):
    return dict(name=name, model=model, theta=theta, R=R, T=T, sched=sched, y=y, y_set=y_set or {}, z_set=z_set or {},
                expect=expect or {}, big=big)


def cases():
    """`expect`: nan_steps = the steps whose log conditional likelihood is NaN (every filter unless nan_steps_r gives it per filter);
    S0_at = steps after which the integer weight sum S is 0; collapsed_at = steps whose ancestors are ONE particle (a cdf of zeros
    resolves every target to index 0); distinct_at = (t, lo, hi): the number of distinct ancestors at step t; x_nan_from = the
    particles are NaN from that step on; one_source_tile_at = every output tile's ancestors come from one source tile;
    zero_scale = after step 1 some tile's scale exp(m_b - m) is zero or subnormal and the first tile with A' > 0 is at index >= 3
    (asserted where the route has that many tiles: the multinomial targets of output tile 0 start at 0, so it spans > 3 tiles)."""
    c = [
        _c("nan-y", y_set={2: NAN}, expect=dict(nan_steps=(2,), S0_at=(2,), collapsed_at=(3,))),
        _c("inf-y", y_set={2: 1e200}, expect=dict(nan_steps=(2,), S0_at=(2,), collapsed_at=(3,), m_neg_inf_at=(2,))),
        _c("huge-y", y_set={2: 1e3}, expect=dict(nan_steps=(), big_step=2, distinct_at=(3, 1, 3), one_source_tile_at=3)),
        _c("zero-tile", model=MODEL_LIN_GAUSS, theta=TH_LG, y=(0.3, 3.0, 0.31, -0.2, 0.25, 0.1), expect=dict(nan_steps=(), zero_scale=1)),
        _c("neg-huge-y", y_set={3: -1e160}, big=False, expect=dict(nan_steps=(3,), S0_at=(3,), collapsed_at=(4,), m_neg_inf_at=(3,))),
        _c("zeros-y", y=(0.0, -0.0, 13.56, -10.36, 0.0, -0.0), big=False, expect=dict(nan_steps=())),
        _c("nan-z", model=MODEL_SVOL_LEVERAGE, theta=TH_LEV, z_set={2: NAN}, big=False,
           expect=dict(nan_steps=(2, 3, 4, 5), x_nan_from=2, S0_at=(2, 3, 4, 5), collapsed_at=(3, 4, 5))),
        # bad theta from step 0 (derive() of the oracle, model_const of pf_api.hip): phi = 1.5 makes the stationary sd sqrt(negative) = NaN
        # and every particle NaN; sigma = 0 makes every particle exactly 0 (equal weights, nothing degenerate but the cloud);
        # beta = -1 sets mc.bad: log g = -inf
        # beta = -1 sets mc.bad: log g = -inf.  Each is filter 0 of a handle of two whose filter 1 has the valid theta, so that the case
        # has finite steps to compare and the bad row comes FIRST (bad-row has it in the middle)
        _c("bad-theta-phi", theta=((1.0, 1.5, 0.25), TH_SVOL), R=2, big=False, expect=dict(nan_steps_r=(ALL6, ()), x_nan_from=0)),
        _c("bad-theta-sigma0", theta=((1.0, 0.95, 0.0), TH_SVOL), R=2, big=False, expect=dict(nan_steps_r=((), ()), x_all_zero=True)),
        _c("bad-theta-beta", theta=((-1.0, 0.95, 0.25), TH_SVOL), R=2, big=False, expect=dict(nan_steps_r=(ALL6, ()), m_neg_inf_at=ALL6)),
        _c("bad-row", theta=(TH_SVOL, (-1.0, 0.95, 0.25), (1.0, 0.9, 0.3)), R=3, big=False,
           expect=dict(nan_steps_r=((), ALL6, ()))),
        _c("nan-y-R3", R=3, y_set={2: NAN}, big=False, expect=dict(nan_steps=(2,), S0_at=(2,), collapsed_at=(3,))),
        # schedule 3 resamples at t = 3 and 6.  NaN at t = 4: steps 4 and 5 carry NaN log-weights, step 6 resamples from zeros and is
        # finite again.  NaN at t = 3 (a step that resamples): its own weights are NaN, carried through t = 4, 5.
        _c("nan-sched3-carried", sched=3, T=7, y_set={4: NAN}, big=False, expect=dict(nan_steps=(4, 5), collapsed_at=(6,))),
        _c("nan-sched3-resampling", sched=3, T=7, y_set={3: NAN}, big=False, expect=dict(nan_steps=(3, 4, 5), collapsed_at=(6,))),
    ]
    return c


def _r(name, kind, n, tile=0, split=None, small=True):
    return dict(name=name, kind=kind, n=n, tile=tile, split=split, small=small)


def routes():
    r = [_r(f"small-{n}", "small", n) for n in (1, 64, 100, 200, 300, 1000, 2000)]
    r += [_r(f"wl2-{t}", "tiled", 3 * t + 77, t) for t in (512, 1024, 2048)]
    r += [
        _r("inkernel-129", "tiled", 128 * 512 + 1, 512),
        _r("inkernel-forced-1025", "tiled", 1024 * 512 + 1, 512, split=False),
        _r("split-forced-5", "tiled", 4 * 512 + 77, 512, split=True),
        _r("split-1025", "tiled", 1024 * 512 + 1, 512),
        _r("split-2049", "tiled", 2048 * 512 + 1, 512),
        _r("tables-5", "tiled", 4 * 512 + 77, 512, split="tables"),
        _r("tables-1025", "tiled", 1024 * 512 + 1, 512, split="tables"),
    ]
    r += [_r(f"edge-n{n}", "edge", n, 2048, small=False) for n in (1, 2, 3, 2047, 2049)]
    return r


EVERY_ROUTE = ("nan-y", "inf-y", "huge-y", "zero-tile")
THREE_ROUTES = ("small-300", "wl2-512", "split-forced-5")


def pairs():
    """[(case, route)] in route-major order, so that the runs of one shape follow each other."""
    cs, out = cases(), []
    for r in routes():
        for c in cs:
            if r["kind"] == "edge":
                take = c["name"] == "nan-y"
            else:
                take = c["name"] in EVERY_ROUTE or r["name"] in THREE_ROUTES
            if take:
                out.append((c, r))
    return out


def pair_id(p):
    return f"{p[0]['name']}@{p[1]['name']}"


def default_tile(n, R=1):
    if n <= 2048:
        return 2048
    if R * (-(-n // 512)) <= 256:
        return 512
    if R * (-(-n // 1024)) <= 512:
        return 1024
    return 2048


def shape(case, route):
    """(N, tile, B, T)"""
    n = route["n"]
    tile = route["tile"] or default_tile(n, case["R"])
    T = min(case["T"], 4) if n > BIG_N else case["T"]
    return n, tile, -(-n // tile), T


def route_of(case, route, form, resampler, t=1):
    """The kernels a step t of (case, route) runs in the given form, as launch_step_grid / launch_rs / hot_config / launch_small_m and
    ssme_pf_set_debug select them: (kernel, NT, BIG, TILE, RS, WL2, level-2).  form "hot": run_series, no debug flags; "general": the
    step API in debug mode (ancestors and log-weights recorded)."""
    n, tile, B, _ = shape(case, route)
    if form == "hot" and route["small"] and B == 1 and tile == 2048:                 # ssme_pf_run_series: h->B == 1 && kTile && small_series
        for lim in (64, 128, 256, 512):
            if n <= lim:
                return (f"k_filter_series_lane<{lim}>", lim, False, 2048, None, None, "in the loop")
        return (f"k_filter_series_small<512,{1 if n <= 1024 else 2}>", 512, False, 2048, None, None, "in the loop")
    sp = route["split"]
    split = B > MAX_TILES_PER_FILTER or sp is True or sp == "tables" or (sp is None and B > SPLIT_ABOVE_TILES)
    tables = sp == "tables"
    nt = 256 if tile == 512 else 512
    general = form == "general" or case["sched"] != 1 or t <= 0
    rs = -1 if general else {0: 0, 1: 1}.get(resampler, -1)
    wl2 = (not split) and B <= WL2_MAX_TILES
    if not split:
        l2 = "wave-by-wave in k_filter_step" if wl2 else "level2_scan in k_filter_step"
        l2 += " + fused accounting (ticket)" if form == "general" else " + kf_finalize"
    elif not tables:
        l2 = f"k_l2_scan_blocks x{-(-B // 1024)} (l2_inkernel), ranges in k_filter_step"
    else:
        l2 = "k_l2_scan_blocks + k_l2_ranges" if B > 1024 else "k_level2_plan"
    return ("k_filter_step", nt, split, tile, rs, wl2, l2)


# ---- the observations ------------------------------------------------------------------------------------------------------------
_SPY = None


def series(case, T=None):
    """(y[T], z[T] or None)"""
    global _SPY
    if _SPY is None:
        _SPY = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
    T = case["T"] if T is None else T
    y = (np.asarray(case["y"], dtype=np.float64) if case["y"] is not None else _SPY)[:T].copy()
    z = None
    if case["model"] == MODEL_SVOL_LEVERAGE:
        z = np.concatenate([[0.0], y[:-1]])
        for t, v in case["z_set"].items():
            if t < T:
                z[t] = v
    for t, v in case["y_set"].items():
        if t < T:
            y[t] = v
    return y, z


def theta_rows(case):
    th = np.asarray(case["theta"], dtype=np.float64)
    return np.repeat(th[None, :], case["R"], axis=0) if th.ndim == 1 else th


# ---- the oracle side ---------------------------------------------------------------------------------------------------------------
_RUNS = {}


def oracle_run(oracle, case, route, resampler):
    """[(lls[R], states[R])] after every step, computed once per (case, shape, resampler) and shared read-only by the tests that need
    it (the routes of one shape differ only in the level-2 policy, which the oracle does not have).  At most one run above BIG_N is
    held; of those only the last two steps keep their arrays."""
    n, tile, B, T = shape(case, route)
    key = (case["name"], n, tile, resampler)
    if key not in _RUNS:
        th = theta_rows(case)
        ofs = [oracle.Filter(case["model"], n, th[r], SEED, rep=r, resampler=resampler, resamp_sched=case["sched"], tile=tile)
               for r in range(case["R"])]
        y, z = series(case, T)
        steps = []
        for t in range(T):
            lls = [of.step(y[t], 0.0 if z is None else z[t]) for of in ofs]
            if n > BIG_N and len(steps) >= 2:
                for s in steps[-2][1]:
                    for k in ("x", "logw", "cdf", "anc"):
                        s[k] = None
            steps.append((lls, [of.state() for of in ofs]))
        if n > BIG_N:
            for k in [k for k in _RUNS if k[1] > BIG_N]:
                del _RUNS[k]
        _RUNS[key] = steps
    return _RUNS[key]


def no_weight_left(st):
    """A NaN among the log-weights (the maxima propagate it) or none above -inf: S = 0, every read-out is 0 / 0."""
    lw = np.asarray(st["logw"])
    return bool(np.isnan(lw).any() or not (lw > -np.inf).any())


def rescaled_sums(oracle, st):
    """A'_b of the level-2 as the oracle's own rescale() gives it from the state's tile sums and maxima."""
    mb, m = np.asarray(st["mb"], dtype=np.float64), float(st["m"])
    with np.errstate(all="ignore"):
        return oracle.rescale(st["A"], mb - m, st["rshift"] - 41)


def source_span(anc, tile):
    """Per output tile: how many source tiles its ancestors span (max - min + 1).  The kernel's own span is at least this."""
    a = np.asarray(anc).astype(np.int64) // tile
    starts = np.arange(0, a.size, tile)
    return np.maximum.reduceat(a, starts) - np.minimum.reduceat(a, starts) + 1
