"""The degenerate inputs at which the Liu-West kernels are pinned (tests/test_liu_west_edges_gpu.py), and the oracle side of each.
test_lw_edges_cpu.py walks the same list without a GPU and proves from the oracle's state that every case reaches the path it is
listed for (`expect`: what the oracle must show, written down from a run of the oracle alone, before any device ran the case).

Every case runs for both forms (0 auxiliary, 1 SISR): cases().  The series is y = default_rng(3).normal(0, 0.02, 8) cut to T steps
with z its lag (expect_cases.lw_series), seed 7, delta 0.99, the reference's transforms and priors unless the case says otherwise.
`y_set` / `z_set` overwrite single observations; `z_lag` = True takes z as the lag of the EDITED y (an outlier that is finite is
also the next step's covariate), False keeps the lag of the original series (a NaN or 1e200 observation stays one step's event)."""
import numpy as np

import expect_cases as ec

TILE = 2048                                    # kTile of lw_kernels.h: the Liu-West kernels have one tile size
FUSED_MAX_TILES = 585                          # lw_enqueue_step: B * 14 * 8 bytes <= the 64 KiB window area of stage 2's LDS
SPLIT_ABOVE_TILES = 1024                       # kSplitLevel2Above
POINT = (0.9, 0.0, 0.05, -0.3)                 # inside the support of every default transform: logit, null, log, twice Fisher
SEED = 7


def _c(name, n=700, T=5, **kw):
    d = dict(name=name, n=n, T=T, delta=0.99, rs=1, transforms=None, lo=None, hi=None, y_set={}, z_set={}, z_lag=False, split=None,
             R=1, probe=None, expect={})
    d.update(kw)
    return d


def base_cases():
    nan, c = float("nan"), []
    for n in (1, 2, 3, 65, 2047, 2049):
        c.append(_c(f"n{n}", n=n, expect=dict(L_zero="all" if n <= 2 else None, noise=(n == 3))))
    # probe: the step at which expectations() and weights() are ALSO read (the series "stopped at the NaN step")
    c.append(_c("nan-y", y_set={2: nan}, probe=2, expect=dict(nan_steps=(2,), noise=True, collapsed_after=2)))
    c.append(_c("inf-weights", y_set={2: 1e200}, probe=2, expect=dict(nan_steps=(2,), collapsed_after=2)))
    c.append(_c("nan-z", z_set={2: nan}, expect=dict(nan_steps=(2, 3, 4), distinct_last=1, L_zero_last="all", x_nan_last=True)))
    c.append(_c("huge-y", y_set={2: 1e3}, z_lag=True, expect=dict(nan_steps=(), noise=True, big_step=2)))
    c.append(_c("outlier", n=5000, y_set={2: 3.0}, z_lag=True, expect=dict(nan_steps=(), L_zero="none", distinct_at=(2, 3100, 3200))))
    c.append(_c("outlier-rs3", n=5000, T=7, rs=3, y_set={2: 3.0}, z_lag=True, expect=dict(nan_steps=(), L_zero="none")))
    c.append(_c("delta1", delta=1.0, expect=dict(nan_steps=(), L_zero="all", identity="delta1")))
    c.append(_c("point-prior", lo=POINT, hi=POINT, expect=dict(nan_steps=(), L_zero="all", identity="point")))
    c.append(_c("one-dim-point", lo_d={1: 0.0}, hi_d={1: 0.0}, expect=dict(nan_steps=(), L_zero_diag=(1,))))
    c.append(_c("mid-path", n=586 * TILE + 1, T=3, y_set={1: 3.0}, z_lag=True, expect=dict(nan_steps=(), path="mid")))
    c.append(_c("split-path", n=1025 * TILE + 1, T=3, y_set={1: 3.0}, z_lag=True, expect=dict(nan_steps=(), path="split")))
    # an output tile whose sources span more than the three staged tiles, so that lw_select takes the probe search (probe_ancestor)
    # instead of the staged one: after y = 10 a few dozen particles carry the weight.  wide_span: per form, the draw (k indices of
    # stage 2 / ancestors of stage 1) and the step at which the oracle's indices prove it
    c.append(_c("wide-span", n=5 * TILE + 1, T=3, y_set={1: 10.0}, z_lag=True,
                expect=dict(nan_steps=(), wide_span={0: ("kidx", 1), 1: ("anc", 2)})))
    by = {k["name"]: k for k in c}
    for name in ("nan-y", "huge-y", "point-prior", "n3", "wide-span"):
        c.append(dict(by[name], name=name + "-forced-split", split=True, same_as=name))
    # per-filter scalars must not leak into each other: the oracle is rep = 0, 1, 2
    c.append(dict(by["nan-y"], name="nan-y-R3", R=3))
    # the run-time transform switch (FT = false) at a degenerate step
    c.append(dict(by["huge-y"], name="huge-y-3030", transforms=(3, 0, 3, 0), lo=ec.LW_LO_3030, hi=ec.LW_HI_3030,
                  expect=dict(nan_steps=(), big_step=2)))
    return c


def cases():
    return [dict(c, name=f"{c['name']}-form{form}", form=form, base=c["name"]) for c in base_cases() for form in (0, 1)]


def series(case):
    y, _ = ec.lw_series(8)
    y = y[:case["T"]].copy()
    z = np.concatenate([[0.0], y[:-1]])
    for t, v in case["y_set"].items():
        y[t] = v
    if case["z_lag"]:
        z = np.concatenate([[0.0], y[:-1]])
    for t, v in case["z_set"].items():
        z[t] = v
    return y, z


def prior(case, oracle):
    tr = tuple(oracle.LW_TRANSFORMS if case["transforms"] is None else case["transforms"])
    lo = list(oracle.LW_PRIOR_LO if case["lo"] is None else case["lo"])
    hi = list(oracle.LW_PRIOR_HI if case["hi"] is None else case["hi"])
    for d, v in case.get("lo_d", {}).items():
        lo[d] = v
    for d, v in case.get("hi_d", {}).items():
        hi[d] = v
    return tr, tuple(lo), tuple(hi)


def tiles(n):
    """B as set_layout / lw_enqueue_step have it."""
    return -(-int(n) // TILE)


def moment_path(case):
    """Which of the three moment paths lw_enqueue_step takes: the level-2 policy first (split above 1024 tiles or forced), then
    whether the tile partials fit stage 2's window area."""
    B = tiles(case["n"])
    if case["split"] or B > SPLIT_ABOVE_TILES:
        return "split"
    return "fused" if B <= FUSED_MAX_TILES else "mid"


def a_shrink(delta):
    """liu_west_filter.h:960 in the operation order of both implementations."""
    return (3.0 * delta - 1.0) / (2.0 * delta)


def oracle_filters(oracle, case):
    tr, lo, hi = prior(case, oracle)
    return [oracle.LWFilter(case["n"], SEED, rep=r, delta=case["delta"], transforms=tr, lo=lo, hi=hi, form=case["form"],
                            resamp_sched=case["rs"]) for r in range(case["R"])]


def walk_oracle(oracle, case):
    """Yields (t, [log conditional likelihood per filter], [state per filter]) after every step."""
    ofs = oracle_filters(oracle, case)
    y, z = series(case)
    for t in range(case["T"]):
        lls = [of.step(y[t], z[t]) for of in ofs]
        yield t, lls, [of.state() for of in ofs]


_RUNS = {}


def oracle_run(oracle, case):
    """The whole walk of a case, computed once per process and shared (read only) by the tests that need it.  At the two large
    shapes only the per-step values, theta-bar, L and the last two states are kept."""
    key = case["name"]
    if key not in _RUNS:
        big = case["n"] > 100000
        steps = []
        for t, lls, sts in walk_oracle(oracle, case):
            if big and len(steps) >= 2:
                for s in steps[-2][1]:
                    for k in ("x", "theta", "logw", "kidx", "anc"):
                        s[k] = None
            steps.append((lls, sts))
        if big:
            _RUNS.clear()                       # at most one large run held at a time
        _RUNS[key] = steps
    return _RUNS[key]


def zero_denominator(st):
    """True when the second-stage weights of an oracle state leave no positive weight sum: a NaN among the log-weights (the device's
    maxima propagate it) or no finite one."""
    lw = np.asarray(st["logw"])
    return bool(np.isnan(lw).any() or not np.isfinite(lw).any())
