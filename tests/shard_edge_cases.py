"""The degenerate inputs and edge layouts at which the particle-sharded drivers are pinned (tests/test_shard_edges_gpu.py), and the
oracle side of each.  test_shard_edges_cpu.py walks the same lists without a GPU and proves from the oracle's ancestors that every
(case, layout) reaches what it is listed for.  The sharded counterpart of bs_edge_cases.py, whose R = 1 cases and oracle runs it uses.

A LAYOUT is (world, N); the tile is 2048 whenever a filter is sharded.  A rank owns Bl = ceil(B / world) consecutive tiles, the last
rank what is left (shares()); the fixed halo holds halo_margin(Bl, world) tiles on each side of a rank's own ones.  Both are restated
here from csrc/handle_core.h (set_layout) and csrc/shard_driver.h (halo_margin); the GPU module asserts them against
ssme_*_shard_layout, the CPU module against ssme_pf_shard_create's refusal of a layout with an empty rank.

What a rank NEEDS at a step that resamples is read from the oracle's ancestors (needed()): the source tiles of its own particles,
and how far they reach beyond its own tiles to the left and right.  A reach above the margin means the fixed halo cannot hold: mode 0
must end on the exact path (path 2), mode 1 must return SSME_ERR_STATE on every rank.  A reach within the margin proves nothing about
the path: the planned window comes from bounds that ignore the random spacings and may be wider (after a collapse the multinomial
bounds are t_lo = 0, t_hi = 2 against T' = 0 everywhere: the planned window is the whole filter, while systematic and stratified plan
[0, 0]) -- there the path is an observation (profiles/shard_edge_paths.txt).

MUST_LEAVE is `expect`: per (case, layout) the (step, rank) pairs whose needed reach exceeds the margin, for EVERY sorted resampler
(0 multinomial, 1 systematic, 2 stratified) unless a resampler is named.  It was written down from a run of the oracle alone, before
any device ran a case; test_shard_edges_cpu.py asserts that the oracle reproduces it exactly (no pair more, no pair less)."""
import numpy as np

import bs_edge_cases as bc

TILE = 2048
SEED = bc.SEED
SORTED = (0, 1, 2)
IID = 3
RESAMPLERS = (0, 1, 2, 3)                      # every resampler ssme_pf_shard_create accepts
NAN = float("nan")


def _l(name, world, n, why):
    return dict(name=name, world=world, n=n, why=why)


def layouts():
    return [
        _l("4x2", 4, 4 * 2 * TILE, "Bl = 2, margin 2: a collapse leaves the halo on the far ranks only"),
        _l("4r-ragged", 4, 7 * TILE - 700, "shares 2 + 2 + 2 + 1, the last tile ragged"),
        _l("3x1", 3, 3 * TILE, "Bl = 1, margin = 1 = the whole share"),
        _l("2r-one-particle", 2, TILE + 1, "rank 1 owns ONE particle"),
        _l("1r", 1, 3 * TILE + 77, "margin 0, halo_exchange is a no-op"),
        _l("2xBl4", 2, 2 * 4 * TILE, "reach 4 = margin 4 after a collapse: the halo must hold"),
        _l("2xBl5", 2, 2 * 5 * TILE, "reach 5 > margin 4: the halo must not hold"),
        _l("split-l2", 2, 1025 * TILE + 1, "split_l2: k_level2_plan + k_shard_window_check, Bl = 513, margin 8"),
    ]


LAYOUTS = {l["name"]: l for l in layouts()}
GUARD_CASES = ("nan-y", "inf-y", "huge-y", "zero-tile")          # on every layout (split-l2: nan-y and huge-y only)
MODEL_LAYOUTS = ("4x2", "4r-ragged")                              # every other case: the model side, two layouts
LW_LAYOUTS = ("4x2", "4r-ragged", "3x1", "2r-one-particle")       # the four small layouts with two or more ranks
PY_LAYOUT = "4x2"


def halo_margin(Bl, world):
    """shard_driver.h: 4 tiles or 1/64 of the share, never more than the share; nothing to exchange with one rank."""
    if world == 1:
        return 0
    m = max(Bl // 64, 4)
    return min(m, Bl)


def py_margin(B, Bl, world):
    """ssme_amd/sharded.py (_ShardedFilter.margin), the rule of the host-planned loops: 2 tiles or half the share, never more than the
    tiles other ranks own.  A different rule from halo_margin; on PY_LAYOUT (Bl = 2, world 2 and 4) both give 2."""
    return min(B - Bl, max(2, Bl // 2)) if world > 1 else 0


def py_layout(world):
    """PY_LAYOUT for `world` ranks of the Python drivers: Bl = 2 tiles per rank (world 4: LAYOUTS["4x2"] itself)."""
    return dict(LAYOUTS[PY_LAYOUT], world=world, n=world * 2 * TILE)


def shares(n, world):
    """(B, Bl, [tiles rank r owns], [particles rank r owns]) or None if a rank would own no tile (set_layout returns false)."""
    B = -(-n // TILE)
    Bl = -(-B // world)
    if (world - 1) * Bl >= B:
        return None
    own = [min(Bl, B - r * Bl) for r in range(world)]
    parts = [min(n - r * Bl * TILE, own[r] * TILE) for r in range(world)]
    return B, Bl, own, parts


def route(layout):
    """The layout as a route of bs_edge_cases (shape(), oracle_run())."""
    return dict(name=layout["name"], kind="tiled", n=layout["n"], tile=TILE, split=None, small=False)


def cases():
    """The R = 1 cases of bs_edge_cases.cases() and single-row versions of its three bad-theta cases: a sharded handle has one filter,
    so every step of those is NaN (sigma = 0: every particle exactly 0) and the bits of that are what is compared."""
    c = [dict(k) for k in bc.cases() if k["R"] == 1]
    c += [
        bc._c("bad-theta-phi-1", theta=(1.0, 1.5, 0.25), big=False, expect=dict(nan_steps=bc.ALL6, x_nan_from=0)),
        bc._c("bad-theta-sigma0-1", theta=(1.0, 0.95, 0.0), big=False, expect=dict(nan_steps=(), x_all_zero=True)),
        bc._c("bad-theta-beta-1", theta=(-1.0, 0.95, 0.25), big=False, expect=dict(nan_steps=bc.ALL6, m_neg_inf_at=bc.ALL6)),
    ]
    return c


CASES = {c["name"]: c for c in cases()}


def pairs():
    """[(case, layout)] in layout-major order: the four guard-driving inputs on every layout, the model-side cases on two."""
    out = []
    for l in layouts():
        for c in cases():
            if l["name"] == "split-l2":
                take = c["name"] in ("nan-y", "huge-y")
            else:
                take = c["name"] in GUARD_CASES or l["name"] in MODEL_LAYOUTS
            if take:
                out.append((c, l))
    return out


def combos(case, layout):
    """The (resampler, mode) runs of a pair.  Every pair: multinomial and systematic on the automatic path (mode 0), systematic on the
    fixed halo only (mode 1), multinomial on the exact path (mode 2).  nan-y, the collapse, additionally: stratified in modes 0 and 1,
    multinomial in mode 1, systematic in mode 2, iid in modes 0 and 2.  The model-side cases (they change what the particles are, which
    no exchange looks at): mode 0 with multinomial and systematic."""
    if case["name"] == "nan-y":
        return [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (3, 2)]
    if case["name"] in GUARD_CASES:
        return [(0, 0), (1, 0), (1, 1), (0, 2)]
    return [(0, 0), (1, 0)]


def runs():
    return [(c, l, rs, mode) for c, l in pairs() for rs, mode in combos(c, l)]


def run_id(r):
    return f"{r[0]['name']}@{r[1]['name']}-rs{r[2]}-mode{r[3]}"


def shape(case, layout):
    """(N, T): above 10^5 particles T = 4, as bs_edge_cases.shape() has it."""
    n, _, _, T = bc.shape(case, route(layout))
    return n, T


def oracle_run(oracle, case, layout, resampler):
    return bc.oracle_run(oracle, case, route(layout), resampler)


def resampled_steps(case, T):
    return [t for t in range(1, T) if t % case["sched"] == 0]


def needed(anc, layout):
    """Per rank: (lo tile, hi tile, reach left, reach right) of the sources its own particles need, from the ancestors of one step."""
    n, world = layout["n"], layout["world"]
    B, Bl, own, parts = shares(n, world)
    a = np.asarray(anc).astype(np.int64) // TILE
    out = []
    for r in range(world):
        first = r * Bl * TILE
        s = a[first:first + parts[r]]
        lo, hi = int(s.min()), int(s.max())
        bF, bL = r * Bl, r * Bl + own[r] - 1
        out.append((lo, hi, max(0, bF - lo), max(0, hi - bL)))
    return out


def must_leave_from_oracle(oracle, case, layout, resampler):
    """[(t, rank)] whose needed reach exceeds the margin, and the widest needed reach (left, right) per rank over the steps whose
    ancestors the oracle run still holds (above 10^5 particles: the last two steps)."""
    n, T = shape(case, layout)
    B, Bl, own, parts = shares(n, layout["world"])
    margin = halo_margin(Bl, layout["world"])
    run = oracle_run(oracle, case, layout, resampler)
    out, widest = [], [[0, 0] for _ in range(layout["world"])]
    for t in resampled_steps(case, T):
        anc = run[t][1][0]["anc"]
        if anc is None:
            continue
        for r, (lo, hi, left, right) in enumerate(needed(anc, layout)):
            widest[r] = [max(widest[r][0], left), max(widest[r][1], right)]
            if left > margin or right > margin:
                out.append((t, r))
    return out, widest


# ---- expect: (step, rank) pairs whose needed reach exceeds the halo margin -------------------------------------------------------
# A collapse (every ancestor is particle 0) needs tile 0 on every rank: rank r leaves the halo iff r * Bl > margin.
_COLLAPSE_4x2 = (2, 3)                          # Bl = 2, margin 2: ranks 2 and 3 (first tiles 4 and 6)
_COLLAPSE_3x1 = (2,)                            # Bl = 1, margin 1: rank 2 (first tile 2)


def _at(steps, ranks):
    return tuple((t, r) for t in steps for r in ranks)


MUST_LEAVE = {
    # nan-y, inf-y: NaN / 1e200 at step 2, step 3 resamples from a cdf of zeros
    ("nan-y", "4x2"): _at((3,), _COLLAPSE_4x2), ("inf-y", "4x2"): _at((3,), _COLLAPSE_4x2),
    ("nan-y", "4r-ragged"): _at((3,), _COLLAPSE_4x2), ("inf-y", "4r-ragged"): _at((3,), _COLLAPSE_4x2),
    ("nan-y", "3x1"): _at((3,), _COLLAPSE_3x1), ("inf-y", "3x1"): _at((3,), _COLLAPSE_3x1),
    ("nan-y", "2r-one-particle"): (), ("inf-y", "2r-one-particle"): (),
    ("nan-y", "1r"): (), ("inf-y", "1r"): (),
    ("nan-y", "2xBl4"): (), ("inf-y", "2xBl4"): (),                       # reach 4 = margin 4
    ("nan-y", "2xBl5"): ((3, 1),), ("inf-y", "2xBl5"): ((3, 1),),         # reach 5 > margin 4
    ("nan-y", "split-l2"): ((3, 1),),                                     # reach 513 > margin 8
    # the model-side collapses: -1e160 at step 3; a NaN covariate from step 2 on (every later step); the schedules draw at 3 and 6
    ("neg-huge-y", "4x2"): _at((4,), _COLLAPSE_4x2), ("neg-huge-y", "4r-ragged"): _at((4,), _COLLAPSE_4x2),
    ("nan-z", "4x2"): _at((3, 4, 5), _COLLAPSE_4x2), ("nan-z", "4r-ragged"): _at((3, 4, 5), _COLLAPSE_4x2),
    ("nan-sched3-carried", "4x2"): _at((6,), _COLLAPSE_4x2), ("nan-sched3-carried", "4r-ragged"): _at((6,), _COLLAPSE_4x2),
    ("nan-sched3-resampling", "4x2"): _at((6,), _COLLAPSE_4x2), ("nan-sched3-resampling", "4r-ragged"): _at((6,), _COLLAPSE_4x2),
    # invalid theta: NaN particles or log g = -inf from step 0, every resampling step draws from zeros
    ("bad-theta-phi-1", "4x2"): _at((1, 2, 3, 4, 5), _COLLAPSE_4x2), ("bad-theta-phi-1", "4r-ragged"): _at((1, 2, 3, 4, 5), _COLLAPSE_4x2),
    ("bad-theta-beta-1", "4x2"): _at((1, 2, 3, 4, 5), _COLLAPSE_4x2), ("bad-theta-beta-1", "4r-ragged"): _at((1, 2, 3, 4, 5), _COLLAPSE_4x2),
}
# The cases whose windows depend on where the weight sits (one heavy particle, one heavy tile), per sorted resampler:
# (case, layout, resampler) -> pairs.  huge-y and zeros-y put the weight of step 2 on a few particles, zero-tile that of steps 1
# and 3 on the tiles next to y; which rank is then too far away depends on where the draws put those particles.
_ALL3 = lambda case, layout, pairs: {(case, layout, rs): pairs for rs in SORTED}
MUST_LEAVE_BY_RESAMPLER = {
    ("huge-y", "4x2", 0): ((3, 0), (3, 1)), ("huge-y", "4x2", 1): ((3, 0),), ("huge-y", "4x2", 2): ((3, 2), (3, 3)),
    **_ALL3("zero-tile", "4x2", ((2, 3), (4, 3))),
    ("zeros-y", "4x2", 0): ((3, 0),), ("zeros-y", "4x2", 1): ((3, 0),), ("zeros-y", "4x2", 2): ((3, 3),),
    **_ALL3("huge-y", "4r-ragged", ((3, 0), (3, 1))),
    **_ALL3("zero-tile", "4r-ragged", ((2, 3),)),
    ("zeros-y", "4r-ragged", 0): (), ("zeros-y", "4r-ragged", 1): ((3, 0), (3, 1)), ("zeros-y", "4r-ragged", 2): ((3, 2), (3, 3)),
    ("huge-y", "3x1", 0): (), ("huge-y", "3x1", 1): (), ("huge-y", "3x1", 2): ((3, 0),),
    # split-l2 (T = 4; the oracle run keeps the ancestors of its last two steps): the heavy particles of step 2 sit in rank 0's tiles
    ("huge-y", "split-l2", 0): ((3, 1),), ("huge-y", "split-l2", 1): ((3, 1),), ("huge-y", "split-l2", 2): ((3, 0),),
    ("zero-tile", "3x1", 0): ((2, 0),), ("zero-tile", "3x1", 1): ((2, 0), (5, 2)), ("zero-tile", "3x1", 2): ((2, 0),),
}


def must_leave(case, layout, resampler):
    """expect for one run, or None where nothing was written down (the iid resampler: always the exact path, window [0, B - 1])."""
    if resampler == IID:
        return None
    key = (case["name"], layout["name"])
    if key + (resampler,) in MUST_LEAVE_BY_RESAMPLER:
        return tuple(MUST_LEAVE_BY_RESAMPLER[key + (resampler,)])
    return tuple(MUST_LEAVE.get(key, ()))


# ---- the harness's arguments -------------------------------------------------------------------------------------------------------
def _fmt(v):
    return "nan" if v != v else repr(float(v))


def overrides(case, T):
    """(YSET, ZSET, THETA) of tests/cpp/test_shard_threads.cpp for a bootstrap case: the harness reads spy_returns.csv[:T] and takes z
    as its lag, exactly bs_edge_cases.series() before its overrides."""
    ys = dict((t, v) for t, v in enumerate(case["y"][:T])) if case["y"] is not None else {}
    ys.update({t: v for t, v in case["y_set"].items() if t < T})
    zs = {t: v for t, v in case["z_set"].items() if t < T} if case["model"] == bc.MODEL_SVOL_LEVERAGE else {}
    lst = lambda d: ",".join(f"{t}:{_fmt(v)}" for t, v in sorted(d.items())) or "-"
    return lst(ys), lst(zs), ",".join(_fmt(v) for v in case["theta"])


# ---- k_shard_window_check on its own (tests/cpp/test_window_check.hip) -----------------------------------------------------------------
def window_check_cases():
    """[(world, Bl, B, margin, [(lo, hi) per rank])]: windows written by hand around the margin.  On the drivers' split level-2 path
    k_filter_step repeats the comparison per tile and raises the same flag, so a wrong comparison in k_shard_window_check cannot be seen
    through a driver; here the kernel is launched alone.  Every layout is valid ((world - 1) Bl < B) and every window inside [0, B - 1]."""
    out = []
    for world, n in ((2, 1025 * TILE + 1), (3, 1300 * TILE + 11), (4, 64 * 4 * 20 * TILE), (2, 8 * TILE), (4, 7 * TILE - 700)):
        B, Bl, own, _ = shares(n, world)
        m = halo_margin(Bl, world)
        first = [r * Bl for r in range(world)]
        last = [r * Bl + own[r] - 1 for r in range(world)]
        base = [(first[r], last[r]) for r in range(world)]                       # nobody reaches anywhere
        out.append((world, Bl, B, m, base))
        for r in range(world):
            for d in (m - 1, m, m + 1, m + 2):
                if d >= 1 and first[r] - d >= 0:                                  # rank r reaches d tiles to the left ...
                    w = list(base); w[r] = (first[r] - d, last[r]); out.append((world, Bl, B, m, w))
                if d >= 1 and last[r] + d <= B - 1:                               # ... to the right
                    w = list(base); w[r] = (first[r], last[r] + d); out.append((world, Bl, B, m, w))
        out.append((world, Bl, B, m, [(0, 0)] * world))                          # a collapse: tile 0 on every rank
        out.append((world, Bl, B, m, [(0, B - 1)] * world))                      # the multinomial bounds after a collapse: the whole filter
        out.append((world, Bl, B, m, [(B - 1, B - 1)] * world))                  # all weight in the last (ragged) tile
    return out


def window_check_expect(case):
    """(flag, widest left, widest right) as shard_driver.h states the rule: a rank's window may reach `margin` tiles beyond its own
    tiles on either side and not one more; the last rank's own tiles end at B - 1."""
    world, Bl, B, margin, wins = case
    flag = left = right = 0
    for r, (lo, hi) in enumerate(wins):
        l, rt = r * Bl - lo, hi - min((r + 1) * Bl - 1, B - 1)
        flag |= int(l > margin or rt > margin)
        left, right = max(left, l), max(right, rt)
    return flag, left, right


def window_check_file(path):
    cs = window_check_cases()
    with open(path, "w") as f:
        for world, Bl, B, margin, wins in cs:
            f.write(" ".join(str(v) for v in (world, Bl, B, margin) + tuple(x for w in wins for x in w)) + "\n")
    return cs


def window_check_verify(cases, stdout):
    """The program's output against window_check_expect, both forms of every case; returns the number of lines compared."""
    rows = [l.split() for l in stdout.strip().splitlines()]
    assert len(rows) == 2 * len(cases), (len(rows), len(cases))
    for row in rows:
        i, form, got = int(row[1]), int(row[3]), (int(row[5]), int(row[7]), int(row[9]))
        assert got == window_check_expect(cases[i]), (cases[i], form, got, window_check_expect(cases[i]))
    assert {int(r[1]) for r in rows} == set(range(len(cases)))
    return len(rows)


def apply_overrides(v, spec):
    """The "t:value,t:value" lists of the harness, for the Python workers (shard_worker*.py): in place, "-" or None changes nothing."""
    if spec and spec != "-":
        for item in spec.split(","):
            t, val = item.split(":")
            if 0 <= int(t) < len(v):
                v[int(t)] = float(val)
    return v


# ---- Liu-West ----------------------------------------------------------------------------------------------------------------------
LW_T, LW_DELTA = 5, 0.99
LW_CASES = {
    "nan-y": dict(name="nan-y", scale=1.0, y_set={2: NAN}, z_set={}),
    "inf-y": dict(name="inf-y", scale=1.0, y_set={2: 1e200}, z_set={}),
    "huge-y": dict(name="huge-y", scale=40.0, y_set={}, z_set={}),       # observations x 40: the particle of highest volatility takes all the weight
    "nan-z": dict(name="nan-z", scale=1.0, y_set={}, z_set={2: NAN}),
}


def lw_series(case):
    """As the harness builds it: spy[:T] x scale, z its lag, then the overrides."""
    y = bc.series(dict(bc.cases()[0], y_set={}), LW_T)[0] * case["scale"]
    z = np.concatenate([[0.0], y[:-1]])
    for t, v in case["z_set"].items():
        z[t] = v
    for t, v in case["y_set"].items():
        y[t] = v
    return y, z


_LW_RUNS = {}


def lw_oracle_run(oracle, case, layout, form):
    """[(log conditional likelihood, state)] per step: the oracle's Liu-West filter with the harness's fixed priors (the oracle's defaults)."""
    key = (case["name"], layout["n"], form)
    if key not in _LW_RUNS:
        f = oracle.LWFilter(layout["n"], SEED, delta=LW_DELTA, form=form)
        y, z = lw_series(case)
        _LW_RUNS[key] = [(f.step(y[t], z[t]), f.state()) for t in range(LW_T)]
    return _LW_RUNS[key]


def lw_must_leave_steps(oracle, case, layout, form):
    """The steps at which the oracle proves that a window of the RESAMPLING draw leaves the halo: every ancestor of that draw lies in
    ONE source tile (so the window is that tile whichever way the indices are recorded) and that tile is further than the margin from
    some rank.  Only the resampling draw (which = 0) is looked at; the k draw of stage 2 (which = 1) is not covered."""
    B, Bl, own, parts = shares(layout["n"], layout["world"])
    margin = halo_margin(Bl, layout["world"])
    out = []
    for t in range(1, LW_T):
        a = np.asarray(lw_oracle_run(oracle, case, layout, form)[t][1]["anc"]).astype(np.int64) // TILE
        if a.min() == a.max():
            b = int(a[0])
            if any(r * Bl - b > margin or b - (r * Bl + own[r] - 1) > margin for r in range(layout["world"])):
                out.append(t)
    return out


def lw_must_leave(oracle, case, layout, form):
    """True where the oracle proves a window leaves the halo at some step."""
    return bool(lw_must_leave_steps(oracle, case, layout, form))
