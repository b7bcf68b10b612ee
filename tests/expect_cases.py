"""The shapes and scenarios at which the expectation kernels are pinned (tests/test_expectations_gpu.py), and the oracle side of each.
test_expect_ref_cpu.py walks the same list without a GPU and proves from the oracle's state that every scenario reaches the path
it is there for."""
import os

import numpy as np

import expect_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SVOL, MODEL_SVOL_LEVERAGE, MODEL_LIN_GAUSS = 0, 1, 2

TH_SVOL = [1.0, 0.95, 0.25]
TH_LEV = [0.9, 0.0, 1.0, -0.1]
TH_DEGENERATE = [0.5, 0.1, 0.01]                          # linear Gaussian, tiny observation noise: test_degenerate_weights_many_tile_span
Y_DEGENERATE = [0.3, 0.25, 0.31, -0.2]
Y_UNDERFLOW = [0.3, 3.0]
Y_OUTLIERS = [0.01, 0.02, 6.0, 0.01, -8.0, 0.01]         # the search-window scenario
WRAP = 257 * 512 + 1                                      # 258 tiles of 512: the 256-strided loops wrap, the last tile holds one particle


def _spy():
    return np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))


def _case(name, n, tile=0, model=MODEL_SVOL, theta=TH_SVOL, y=None, T=3, rs=0, sched=1, every_step=False, R=1, z=False, seed=7, **kw):
    return dict(name=name, n=n, tile=tile, model=model, theta=theta, y=y, T=T if y is None else len(y), rs=rs, sched=sched,
                every_step=every_step, R=R, z=z, seed=seed, **kw)


def bootstrap_cases():
    c = []
    for n in (1, 2, 511, 512, 513, 2047, 2049):
        c.append(_case(f"ragged-{n}", n))
    for rs in (1, 2, 3):                                                        # every resampler: one small, one wrapped shape
        c.append(_case(f"resampler{rs}-513", 513, rs=rs))
        c.append(_case(f"resampler{rs}-wrap", WRAP, 512, rs=rs))
    c.append(_case("tile512-256tiles", 256 * 512, 512))
    c.append(_case("tile512-wrap", WRAP, 512))
    c.append(_case("tile2048-wrap", 257 * 2048 - 1, 2048))
    c.append(_case("split-level2", 2049 * 512 + 3, 512, T=2))
    c.append(_case("degenerate-20000", 20000, model=MODEL_LIN_GAUSS, theta=TH_DEGENERATE, y=Y_DEGENERATE, seed=5, degenerate=True))
    c.append(_case("degenerate-wrap", WRAP, 512, model=MODEL_LIN_GAUSS, theta=TH_DEGENERATE, y=Y_DEGENERATE, seed=5, degenerate=True))
    # one more, beyond the issue's list: an observation 30 standard deviations out, after which the tile maxima lie hundreds of units of
    # log-weight apart and whole tiles have the scale exp(m_b - m) == 0 (the scenario above stops at subnormal scales)
    c.append(_case("underflow-20000", 20000, model=MODEL_LIN_GAUSS, theta=TH_DEGENERATE, y=Y_UNDERFLOW, seed=5, underflow=True))
    c.append(_case("underflow-wrap", WRAP, 512, model=MODEL_LIN_GAUSS, theta=TH_DEGENERATE, y=Y_UNDERFLOW, seed=5, underflow=True))
    c.append(_case("outliers", 5000, y=Y_OUTLIERS, every_step=True))
    c.append(_case("sched3-5000", 5000, sched=3, T=7, every_step=True))
    c.append(_case("sched3-wrap", WRAP, 512, sched=3, T=7, every_step=True))
    rng = np.random.default_rng(1)
    th3 = np.stack([rng.uniform(.8, .99, 3), rng.uniform(-.1, .1, 3), rng.uniform(.5, 1.0, 3), rng.uniform(-.5, -.01, 3)], axis=1)
    c.append(_case("three-filters-wrap", WRAP, 512, model=MODEL_SVOL_LEVERAGE, theta=th3, R=3, z=True))
    return c


def series_cases():
    """After run_series: both parities of the handle's buffer index, the one-launch small-series kernel (N <= 2048) and the tiled one."""
    return [_case(f"series-T{T}-{n}", n, tile, T=T) for T in (6, 7) for n, tile in ((500, 0), (2048, 0), (5000, 0), (WRAP, 512))]


def observations(case):
    """(y[T], z[T] or None)"""
    spy = _spy()
    y = np.asarray(case["y"], dtype=np.float64) if case["y"] is not None else spy[:case["T"]]
    z = np.concatenate([[0.0], y[:-1]]) if case["z"] else None
    return y, z


def theta_row(case, r):
    th = np.asarray(case["theta"], dtype=np.float64)
    return th if th.ndim == 1 else th[r]


def oracle_filters(oracle, case):
    tile = case["tile"] or oracle.default_tile(case["n"], case["R"])
    return [oracle.Filter(case["model"], case["n"], theta_row(case, r), case["seed"], rep=r, resampler=case["rs"], resamp_sched=case["sched"],
                          tile=tile) for r in range(case["R"])], tile


def walk_oracle(oracle, case):
    """Steps the oracle filters of a case; yields (t, tile, filters) after every step the case checks."""
    ofs, tile = oracle_filters(oracle, case)
    y, z = observations(case)
    for t in range(case["T"]):
        lls = [of.step(y[t], 0.0 if z is None else z[t]) for of in ofs]
        if case["every_step"] or t == case["T"] - 1:
            yield t, tile, ofs, lls


def builtin_rows(oracle, x):
    return np.stack([er.builtin_h(oracle, k, x) for k in range(4)])


# ---- Liu-West ------------------------------------------------------------------------------------------------------------------------
def lw_cases():
    d = dict(form=0, rs=1, transforms=None, T=3)
    c = [dict(d, name=f"lw-form{form}-{n}", n=n, form=form, T=T) for form in (0, 1)
         for n, T in ((100, 3), (2049, 3), (257 * 2048 + 1, 2), (2049 * 2048 + 5, 2))]
    c.append(dict(d, name="lw-m_rs3", n=2049, rs=3, T=7, every_step=True))
    c.append(dict(d, name="lw-transforms-3030", n=2049, transforms=(3, 0, 3, 0)))
    return c


def lw_series(T, seed=3):
    rng = np.random.default_rng(seed)
    y = rng.normal(0.0, 0.02, T)
    return y, np.concatenate([[0.0], y[:-1]])


LW_LO_3030, LW_HI_3030 = (0.8, -0.1, 0.01, 0.01), (0.99, 0.1, 0.1, 0.5)     # log transforms need positive supports


def lw_prior(case, oracle):
    if case["transforms"] is None:
        return oracle.LW_TRANSFORMS, oracle.LW_PRIOR_LO, oracle.LW_PRIOR_HI
    return case["transforms"], LW_LO_3030, LW_HI_3030


def lw_h_rows(oracle, x, theta_untrans):
    """ids 0-3: x, x^2, exp(x/2), 42; 4-7: the untransformed parameters."""
    return np.concatenate([builtin_rows(oracle, x), np.asarray(theta_untrans, dtype=np.float64)])


def lw_untransform(oracle, transforms, theta, idx=None):
    """tr_inv of the oracle, particle by particle (a scalar entry point: use idx to restrict it to a sample at large N)."""
    theta = np.asarray(theta)
    idx = np.arange(theta.shape[1]) if idx is None else idx
    return np.array([[oracle.inv_transform(int(transforms[d]), float(theta[d, i])) for i in idx] for d in range(4)])


# ---- the two-factor user model (tests/models/svol_two_factor_h.h) -------------------------------------------------------------------
USER_CASES = [dict(name=f"n{n}-tile{tile}", n=n, tile=tile, T=3, sched=1, y=None) for tile in (512, 2048) for n in (1, 2, 513, 1025)] + [
    dict(name="wrap", n=WRAP, tile=512, T=2, sched=1, y=None),
    dict(name="outliers", n=4000, tile=512, T=6, sched=1, y=Y_OUTLIERS),
    dict(name="sched3", n=1025, tile=512, T=5, sched=3, y=None)]


def user_observations(case):
    """(y[T, 2], z[T]) of a two-factor case"""
    spy = _spy()
    if case["y"] is not None:
        y = np.stack([np.asarray(case["y"]), np.asarray(case["y"])[::-1]], axis=1)
    else:
        y = np.stack([spy[:case["T"]], spy[100:100 + case["T"]]], axis=1)
    return np.ascontiguousarray(y), 0.37 + np.arange(case["T"])
