"""The lists of the recorded series (ssme_pf_set_series_expectations): which shapes, models, resamplers and schedules
tests/test_series_expectations_gpu.py compares with the step API, and the helpers both it and tests/series_expect_worker.py (one
process per user-model library) use.  Every comparison on these lists is exact: row t of a recorded trajectory against
expectations_multi() / user_expectations() after step t of a FRESH handle of the same configuration and seed that is stepped with
step().  That yardstick is code that exists without the feature; nothing here has a tolerance."""
import os

import numpy as np

import bs_edge_cases as bc
import user_cov_ref as ucr
import user_edge_cases as uc
import vector_series_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SVOL, MODEL_SVOL_LEVERAGE, MODEL_LIN_GAUSS, MODEL_USER0 = 0, 1, 2, 3
ROUTE_TILED, ROUTE_SERIES_LANE, ROUTE_SERIES_PAIR = 0, 1, 2
SEED = 20240229
T = 8
ALL4 = (0, 1, 2, 3)                                  # SSME_H_X, SSME_H_X2, SSME_H_VOL, SSME_H_CONST42

# the edges of the 256-thread summation tree and of every workgroup size of the lane kernel; the pair kernel with one and two pairs
# per lane; the tiled route by size, by the default tile of a mid-size filter and by tile_particles; the split level-2, forced
LANE_SIZES = (1, 2, 63, 64, 65, 128, 129, 255, 256, 257, 500, 511, 512)
PAIR_SIZES = (513, 1000, 1024, 1025, 2047, 2048)
TILED_SHAPES = ((2049, 0, None), (3000, 0, None), (500, 512, None), (4097, 0, None), (4097, 0, True))     # (N, tile_particles, split)
SHAPES = tuple((n, 0, None) for n in LANE_SIZES + PAIR_SIZES) + TILED_SHAPES
RESAMPLERS = (0, 1, 2, 3)
SCHEDULES = (1, 3)

TH_SVOL3 = ((1.0, 0.95, 0.25), (0.9, 0.9, 0.3), (1.1, 0.97, 0.2))                  # one theta row per filter
TH_LEV3 = ((0.9, 0.0, 1.0, -0.1), (0.95, -0.1, 0.2, -0.4), (0.9, 0.05, 0.25, -0.3))
TH_LG3 = ((0.5, 0.1, 0.5), (0.8, 0.3, 0.4), (0.9, 0.5, 0.7))
MODELS = {MODEL_SVOL: TH_SVOL3, MODEL_SVOL_LEVERAGE: TH_LEV3, MODEL_LIN_GAUSS: TH_LG3}
# the other models, R = 1 and one functional alone: one shape per route
OTHER_SHAPES = ((500, 0, None), (1500, 0, None), (3000, 0, None))

# user-model libraries (the names __graft_entry__.build() builds them under) whose headers declare functionals.  edge: the entry of
# user_edge_cases.HEADERS with the same model (its `bad` theta row: derive() sets `bad`, log g = -inf), None where there is none
USER_LIBS = {
    "student_t_h": dict(header="svol_student_t_h", dy=1, K=0, n_h=4, theta=uc.TH_ST, z="scalar", edge="svol_student_t"),
    "two_factor_h": dict(header="svol_two_factor_h", dy=2, K=0, n_h=7, theta=uc.TH_2F, z="scalar", edge="svol_two_factor"),
    "lin_gauss_4d_h": dict(header="lin_gauss_4d_h", dy=4, K=0, n_h=16, theta=vc.TH_LG4[:2], z=None, edge=None),
    "svol_two_factor_cov": dict(header="svol_two_factor_cov", dy=2, K=4, n_h=4, theta=uc.TH_2F, z="cov", edge="svol_two_factor_cov"),
    "svol_reg_cov": dict(header="svol_reg_cov", dy=1, K=3, n_h=3, theta=uc.TH_REG, z="cov", edge="svol_reg_cov"),
}
BAD_ROW_LIBS = tuple(k for k, v in USER_LIBS.items() if v["edge"])
BAD_ROW_SIZES = (300, 1500, 3000)                    # lane kernel, pair kernel, tiled route
# a user-model library whose header declares NO functionals: user != 0 is SSME_ERR_UNSUPPORTED on its SSME_MODEL_USER0 handles
NO_H_LIB = dict(lib="student_t", header="svol_student_t", theta=uc.TH_ST)
USER_SIZES = (100, 512, 513, 2048, 2049)             # lane, lane at its largest, pair, pair at the LDS maximum, tiled
USER_T = 6

_SPY = None


def spy():
    global _SPY
    if _SPY is None:
        _SPY = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
    return _SPY


def expected_route(n, tile=0, small=True):
    """(route, threads) a handle reports, recording or not: the rule of the host's series_route, restated."""
    if not small or tile not in (0, 2048) or n > 2048:
        return ROUTE_TILED, None
    return vc.expected_route(n)


def stock_series(model, T=T, shift=0):
    """(y [T], z [T] or None): the leverage model takes the previous observation as its covariate."""
    y = spy()[shift:shift + T].copy()
    z = np.concatenate([[0.0], y[:-1]]) if model == MODEL_SVOL_LEVERAGE else None
    return y, z


def user_series(lib, T=USER_T, shift=0):
    """(y [T, dy], z [T] / [T, K] / None) of a library; shift: another stretch of the data and other covariates."""
    s = USER_LIBS[lib]
    y = np.stack([spy()[shift + 100 * d:shift + 100 * d + T] for d in range(s["dy"])], axis=1).copy()
    if s["z"] == "cov":
        z = ucr.covariates(s["K"], T, seed=7 + shift)
    elif s["z"] == "scalar":
        z = 0.37 + 0.5 * np.arange(T) + shift
    else:
        z = None
    return y, z


def make_bank(sa, model, n, theta, rs=0, sched=1, tile=0, split=None, dtype=0):
    theta = np.asarray(theta, dtype=np.float64)
    bank = sa.ParticleFilterBank(model, n, 1 if theta.ndim == 1 else theta.shape[0], SEED, rs, sched, tile=tile, dtype=dtype)
    if split is not None:
        bank.set_debug(False, False, split_level2=split)
    bank.set_params(theta)
    return bank


def stepped(sa, model, n, theta, y, z, functionals=ALL4, user=False, **kw):
    """The yardstick: a fresh handle stepped with step(); ([T, n, R] or None, [T, n_h, R] or None)."""
    bank = make_bank(sa, model, n, theta, **kw)
    b, u = [], []
    for t in range(len(y)):
        bank.step(y[t], None if z is None else z[t])
        if len(functionals):
            b.append(bank.expectations_multi(list(functionals)))
        if user:
            u.append(bank.user_expectations())
    bank.close()
    return (np.stack(b) if b else None), (np.stack(u) if u else None)


def recorded(bank, y, z, functionals=ALL4, user=False):
    """record + run_series on `bank`: (log-likelihoods, [T, n, R] or None, [T, n_h, R] or None)."""
    bank.record_series_expectations(functionals, user)
    ll = bank.run_series(y, z)
    return ll, (bank.series_expectations() if len(functionals) else None), (bank.series_user_expectations() if user else None)


def degenerate_rows():
    """[(name, model, theta rows of R = 3 with the degenerate row in the middle, y_set, resamp_sched, T)] from bs_edge_cases.cases(): parameter rows
    that make every weight NaN (phi = 1.5) or zero (beta = -1: log g = -inf, the maximum is -inf), and observations that do the same
    to every filter from one step on (NaN; 1e200: every log-weight -inf).  No built-in model has a row with weights of +inf: a
    maximum of +-inf is what the rows above and the observation 1e200 produce, and the step kernel's own rule makes both NaN rows.
    resamp_sched = 3 (resampling at t = 3 and 6): a NaN observation at t = 4 is carried through steps that do not resample, one at
    t = 3 falls on a step that does; step 6 resamples from zeros and is finite again."""
    by_name = {c["name"]: c for c in bc.cases()}
    rows = []
    for name in ("bad-theta-phi", "bad-theta-beta"):
        bad = by_name[name]["theta"][0]
        rows.append((name, MODEL_SVOL, (TH_SVOL3[0], bad, TH_SVOL3[2]), {}, 1, 6))
    for name in ("nan-y", "inf-y", "neg-huge-y", "nan-sched3-carried", "nan-sched3-resampling"):
        c = by_name[name]
        rows.append((name, MODEL_SVOL, TH_SVOL3, c["y_set"], c["sched"], c["T"]))
    return rows
