"""The lists of the whole-series route of VECTOR user models (dim_x or dim_y > 1, N <= 2048): which libraries, sizes, resamplers and
schedules tests/test_vector_series_gpu.py runs through tests/vector_series_worker.py, which of them are also compared with the oracle,
and the degenerate cases.  tests/test_vector_series_cpu.py walks the same lists with the oracle alone.

The degenerate cases, their series and the oracle's closures are those of user_edge_cases.py (imported, not copied); the closure of
lin_gauss_4d_h.h is oracle_models._lin_gauss_4d_oracle.  Every comparison on these lists is exact, so there is no tolerance here."""
import os

import numpy as np

import user_cov_ref as ucr
import user_edge_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = uc.SEED
ROUTE_TILED, ROUTE_SERIES_LANE, ROUTE_SERIES_PAIR = 0, 1, 2

TH_LG4 = ((0.9, 0.5, 0.7, 0.4, 1.1, 0.25), (0.85, 0.4, 0.6, 0.5, 0.9, 0.35), (0.8, 0.6, 0.8, 0.3, 1.0, 0.3))      # phi, sigma, tau_1..4
# lib: the name __graft_entry__.build() builds the header under; theta: THREE different rows (R = 3: filter r lives at row offset
# r N_pad of every plane); edge: the header's name in user_edge_cases.HEADERS, whose StepFilter is its oracle side
LIBS = {
    "two_factor": dict(header="svol_two_factor", dx=2, dy=2, K=0, edge="svol_two_factor",
                       theta=uc.TH_2F + ((1.05, 0.92, 0.88, 0.22, 0.14, -0.35),)),
    "lin_gauss_3d": dict(header="lin_gauss_3d", dx=3, dy=1, K=0, edge="lin_gauss_3d",
                         theta=uc.TH_LG3 + ((0.8, 0.45, 0.25, 0.3, 0.65),)),
    "lin_gauss_4d_h": dict(header="lin_gauss_4d_h", dx=4, dy=4, K=0, edge=None, theta=TH_LG4),
    "svol_two_factor_cov": dict(header="svol_two_factor_cov", dx=2, dy=2, K=4, edge="svol_two_factor_cov",
                                theta=uc.TH_2F + ((1.05, 0.92, 0.88, 0.22, 0.14, -0.35),)),
}
# the same models with an observation draw (forecast after a series); one theta row
FORECAST_LIBS = {"two_factor_g": dict(header="svol_two_factor_g", dx=2, dy=2, K=0, theta=(uc.TH_2F[0],)),
                 "lin_gauss_4d_g": dict(header="lin_gauss_4d_g", dx=4, dy=4, K=0, theta=(TH_LG4[0],))}

R, T = 3, 8
# both sides of every switch of the route: the lane kernel's block sizes 64 | 128 | 256 | 512, lane | pair at 512, one | two pairs per
# lane at 1024, the last one-tile sizes 2047 and 2048; N = 1 and 2: one pair, half a pair
SIZES = (1, 2, 63, 64, 65, 128, 129, 256, 257, 500, 512, 513, 1024, 1025, 2047, 2048)
SWITCHES = (64, 128, 256, 512, 1024)                 # N <= s takes one kernel shape, N = s + 1 the next
RESAMPLERS = (0, 1, 2, 3)
SCHEDULES = (1, 3)
ORACLE_SIZES = (1, 65, 500, 1025, 2048)              # lane kernel with 64, 128 and 512 lanes; pair kernel, two pairs per lane (twice)
ORACLE_RESAMPLERS = (0, 1)
LONG = dict(lib="two_factor", n=500, T=300, then=(40, 300), R=2)       # series_accounting: five 64-step loads; buffers grow and are reused
EDGE_SHAPES = (300, 1500)                            # lane kernel, pair kernel
EDGE_CASES = {"two_factor": ("nan-y", "nan-y1", "nan-y0", "bad-first", "bad-row", "nan-sched3-carried"),
              "svol_two_factor_cov": ("nan-y", "nan-y1", "nan-y0", "bad-first", "bad-row", "nan-sched3-carried", "nan-z3-first", "nan-z1-prop",
                                      "null-z-nan-y")}
EDGE_RESAMPLERS = (0, 1)


def expected_route(n, tile=2048):
    """(route, threads) of a one-tile handle whose whole-series route is on: the rule of the host's series_route, restated."""
    if tile != 2048 or n > 2048:
        return ROUTE_TILED, 512
    if n <= 512:
        return ROUTE_SERIES_LANE, next(s for s in (64, 128, 256, 512) if n <= s)
    return ROUTE_SERIES_PAIR, 512


_SPY = None


def observations(dy, T):
    """[T, dy]: spy_returns.csv, component d from row 100 d on."""
    global _SPY
    if _SPY is None:
        _SPY = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
    return np.stack([_SPY[100 * d:100 * d + T] for d in range(dy)], axis=1).copy()


def series(lib, T):
    """(y [T, dy], Z [T, K] or None) of the healthy series of a library."""
    s = LIBS.get(lib) or FORECAST_LIBS[lib]
    return observations(s["dy"], T), (ucr.covariates(s["K"], T) if s["K"] else None)


def oracle_filter(O, lib, th, n, rep, resampler, sched):
    """An object with .step(y_row, z_row) -> log conditional likelihood, .state(), .loglik for one filter of a library."""
    s = LIBS[lib]
    if s["edge"]:
        return uc.StepFilter(O, s["edge"], th, n, rep, resampler, sched, 2048)
    import oracle_models as om
    f = om._lin_gauss_4d_oracle(O, n, SEED, rep, resampler, 2048, sched, th=tuple(th))

    class _F:
        loglik = property(lambda self: f.loglik)

        def step(self, y_row, z_row=None):
            return f.step(y_row)

        def state(self):
            return f.state()
    return _F()


_RUNS = {}


def oracle_series(O, lib, n, resampler, sched, T=T, nfilters=R):
    """(per [R, T], states[R] after the last step) of the healthy series; computed once and shared read-only."""
    key = (lib, n, resampler, sched, T, nfilters)
    if key not in _RUNS:
        y, Z = series(lib, T)
        per, sts = np.empty((nfilters, T)), []
        for r in range(nfilters):
            f = oracle_filter(O, lib, LIBS[lib]["theta"][r], n, r, resampler, sched)
            for t in range(T):
                per[r, t] = f.step(y[t], None if Z is None else Z[t])
            sts.append(f.state())
        _RUNS[key] = (per, sts)
    return _RUNS[key]


def series_sum(per_row):
    """The running sum loglik += ll_t in step order, as the device accumulates it."""
    s = 0.0
    for v in per_row:
        s = s + float(v)
    return s


def edge_items():
    """[(lib, case, n)] of the degenerate inputs."""
    return [(lib, uc.case_of(LIBS[lib]["edge"], name), n) for lib, names in EDGE_CASES.items() for name in names for n in EDGE_SHAPES]


def edge_route(n):
    return dict(name=f"vs-{n}", n=n, tile=2048, small=True, split=None, kind="small")
