"""The degenerate inputs at which the MODEL_USER0 instantiations are pinned (tests/test_user_edges_gpu.py), the routes through the code
on which each is run, and the oracle side of each.  test_user_edges_cpu.py walks the same lists without a GPU and proves from the
oracle's state that every case reaches what its `expect` says (written down from a run of the oracle alone, before any device ran the
case).  The user-model counterpart of bs_edge_cases.py; user_edge_worker.py runs the same lists on the device, one process per library.

HEADERS: six headers of tests/models/, built by ssme_amd.build.build_user_model under the names __graft_entry__.build() gives them.
Every handle holds R >= 2 filters with DIFFERENT theta rows and every filter is compared: filter 1 lives at row offset N_pad in every
plane, so a gather that forgets the row offset or the plane stride shows.

A CASE is an input: theta rows, R, T, the schedule, overwritten observations (`y_set`: {t: {component: value}}) and covariates
(`z_set`: {t: {j: value}}), `null_z` (z = NULL throughout).  Base series: user_cov_ref.observations (spy_returns.csv[:T], component 1
its rows 100 ..) and user_cov_ref.covariates(K, T); one seed.  `clean_tail`: the cloud is NaN from the degenerate step to the end of
the series, for every theta (a NaN that reaches the state through `first` or `prop` never leaves it), so the case goes on ON THE SAME
HANDLE: reset() and the healthy series through the step API, a second run_series of the healthy series in the hot form.  Those are
the finite terms such a case is compared on, and they prove that nothing of the NaN cloud outlives a reset.

A ROUTE is a shape (N, tile), the level-2 policy forced through set_debug, and whether run_series takes the whole-series kernel
(bs_edge_cases.routes(), the subset named in routes()).  route_of() is bs_edge_cases.route_of() with the one thing a user model adds: a
vector model (dim_x > 1 or dim_y > 1) has no whole-series kernel, ssme_pf_set_small_series ignores the switch, so its hot form at
N <= 2048 is the tiled kernel.

The oracle side: oracle.UserVectorModelFilter (dx = dy = 1 included) stepped one observation at a time, with closures that restate
each header's operation sequence on Python floats (IEEE doubles: +, -, *, / round as the device's do with -ffp-contract=off) and the
oracle's own exp_t / log through scalar calls.  They are the closures of user_cov_ref.py / oracle_models.py / test_parity_gpu.py
without numpy in the inner loop (one callback costs 2-4 us instead of 30-100 us; the lists need ~10^7 callbacks);
test_user_edges_cpu.py proves them equal to those closures bit for bit on every case."""
import ctypes as C
import math
import os

import numpy as np

import bs_edge_cases as bc
import user_cov_ref as ucr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240229
NAN = float("nan")
HALF_LOG_2PI = 0.91893853320467274178

TH_ST = ((1.1, 0.95, 0.25, 7.0), (0.9, 0.9, 0.3, 5.0))                          # beta, phi, sigma, nu
TH_LG3 = ((0.9, 0.5, 0.3, 0.2, 0.7), (0.85, 0.4, 0.35, 0.25, 0.6))              # phi, sigma_1..3, tau
TH_2F = tuple(tuple(float(v) for v in r) for r in ucr.TH_2F)
TH_REG = tuple(tuple(float(v) for v in r) for r in ucr.TH_REG)


def _bad(row, k, v):
    r = list(row)
    r[k] = v
    return tuple(r)


# lib: the name __graft_entry__.build() builds the header under; bad: an invalid theta row (derive() sets `bad`: log g = -inf)
HEADERS = {
    "svol_student_t": dict(lib="student_t", dx=1, dy=1, K=0, n_h=0, first=False, theta=TH_ST, bad=_bad(TH_ST[0], 0, -1.0)),
    "svol_two_factor": dict(lib="two_factor", dx=2, dy=2, K=0, n_h=0, first=False, theta=TH_2F, bad=_bad(TH_2F[0], 0, -1.0)),
    "lin_gauss_3d": dict(lib="lin_gauss_3d", dx=3, dy=1, K=0, n_h=0, first=False, theta=TH_LG3, bad=_bad(TH_LG3[0], 4, -0.7)),
    "svol_reg_cov": dict(lib="svol_reg_cov", dx=1, dy=1, K=3, n_h=3, first=True, theta=TH_REG, bad=_bad(TH_REG[0], 2, -0.25)),
    "svol_reg_cov_nofirst": dict(lib="svol_reg_cov_nofirst", dx=1, dy=1, K=3, n_h=3, first=False, theta=TH_REG, bad=_bad(TH_REG[0], 2, -0.25)),
    "svol_two_factor_cov": dict(lib="svol_two_factor_cov", dx=2, dy=2, K=4, n_h=4, first=True, theta=TH_2F, bad=_bad(TH_2F[0], 0, 0.0)),
}
SCALAR = tuple(h for h, s in HEADERS.items() if s["dx"] == 1 and s["dy"] == 1)
VECTOR = tuple(h for h in HEADERS if h not in SCALAR)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _c(name, expect, R=2, T=6, sched=1, theta=None, y_set=None, z_set=None, null_z=False, clean_tail=False):
    return dict(name=name, R=R, T=T, sched=sched, theta=theta, y_set=y_set or {}, z_set=z_set or {}, null_z=null_z, expect=expect,
                clean_tail=clean_tail)


ALL6 = (0, 1, 2, 3, 4, 5)
# What the oracle shows, per (header, case): written down from tests/test_user_edges_cpu.py's run of the oracle alone.  Vocabulary of
# bs_edge_cases.cases(): nan_steps (every filter) / nan_steps_r (per filter), S0_at, collapsed_at, x_nan_from, m_neg_inf_at; all of
# filter 0 unless nan_steps_r is given (then S0_at ... describe the first filter that has NaN steps).
_NAN2 = dict(nan_steps=(2,), S0_at=(2,), collapsed_at=(3,))
_INF2 = dict(nan_steps=(2,), S0_at=(2,), collapsed_at=(3,), m_neg_inf_at=(2,))
_FROM0 = dict(nan_steps=ALL6, S0_at=ALL6, collapsed_at=(1, 2, 3, 4, 5), x_nan_from=0)
_FROM2 = dict(nan_steps=(2, 3, 4, 5), S0_at=(2, 3, 4, 5), collapsed_at=(3, 4, 5), x_nan_from=2)
_Y0 = dict(nan_steps=(0,), S0_at=(0,), collapsed_at=(1,))
_Y0INF = dict(nan_steps=(0,), S0_at=(0,), collapsed_at=(1,), m_neg_inf_at=(0,))
_BAD0 = dict(nan_steps_r=(ALL6, ()), S0_at=ALL6, m_neg_inf_at=ALL6, collapsed_at=(1, 2, 3, 4, 5))
_BADMID = dict(nan_steps_r=((), ALL6, ()), S0_at=ALL6, m_neg_inf_at=ALL6, collapsed_at=(1, 2, 3, 4, 5))
# schedule 3 resamples at t = 3 and 6; T = 8 (one step more than the stock list's 7), so that two finite terms follow the NaN steps
_S3C = dict(nan_steps=(4, 5), collapsed_at=(6,))
_S3R = dict(nan_steps=(3, 4, 5), collapsed_at=(6,))
_COMMON = {"nan-y": _NAN2, "inf-y": _INF2, "huge-y": dict(nan_steps=(), big_step=2), "nan-y0": _Y0, "inf-y0": _Y0INF, "bad-first": _BAD0,
           "bad-row": _BADMID, "nan-sched3-carried": _S3C, "nan-sched3-resampling": _S3R, "nan-y1": _NAN2}
EXPECT = {h: dict(_COMMON) for h in HEADERS}
# the two-factor observation densities: (1e200)^2 e^-u = inf and -h - c - inf = -inf for every particle, as the scalar models
# svol_reg_cov.h, `first` reads y_0: a NaN first observation is in every x_0 and never leaves; 1e200 gives x_0 ~ 2.5e199, finite, with
# r^2 e^-x = inf * 0 = NaN at step 0 and a finite, enormous -x / 2 afterwards (x shrinks by phi per step)
EXPECT["svol_reg_cov"].update({"nan-y0": _FROM0, "inf-y0": dict(nan_steps=(0,), S0_at=(0,), collapsed_at=(1,)),
                               "nan-z1-prop": _FROM2, "nan-z2-logg": _NAN2, "nan-z0-first": _FROM0, "null-z-nan-y": _NAN2})
EXPECT["svol_reg_cov_nofirst"].update({"nan-z1-prop": _FROM2, "nan-z2-logg": _NAN2, "nan-z0-first": _Y0, "null-z-nan-y": _NAN2})
# svol_two_factor_cov.h, `first` reads y_0[1] and zc[3] into component 1 only: plane 1 is NaN from step 0, plane 0 stays finite
EXPECT["svol_two_factor_cov"].update({"nan-y0": dict(nan_steps=ALL6, S0_at=ALL6, collapsed_at=(1, 2, 3, 4, 5), x1_nan_from=0),
                                      "inf-y0": dict(nan_steps=(0,), S0_at=(0,), collapsed_at=(1,)),
                                      "nan-z3-first": dict(nan_steps=ALL6, S0_at=ALL6, collapsed_at=(1, 2, 3, 4, 5), x1_nan_from=0),
                                      "nan-z3-logg": _NAN2,
                                      "nan-z1-prop": dict(nan_steps=(2, 3, 4, 5), S0_at=(2, 3, 4, 5), collapsed_at=(3, 4, 5), x1_nan_from=2),
                                      "null-z-nan-y": _NAN2})
COV_CASES = {"svol_reg_cov": ("nan-z1-prop", "nan-z2-logg", "nan-z0-first", "null-z-nan-y"),
             "svol_reg_cov_nofirst": ("nan-z1-prop", "nan-z2-logg", "nan-z0-first", "null-z-nan-y"),
             "svol_two_factor_cov": ("nan-z3-first", "nan-z3-logg", "nan-z1-prop", "null-z-nan-y")}


def cases(header):
    s, e = HEADERS[header], EXPECT[header]
    th, bad, dy = s["theta"], s["bad"], s["dy"]
    row = lambda v: {d: v for d in range(dy)}            # a whole observation row
    tail = lambda name: any(k in e[name] for k in ("x_nan_from", "x1_nan_from"))
    c = [
        _c("nan-y", e["nan-y"], y_set={2: {0: NAN}}),
        _c("inf-y", e["inf-y"], y_set={2: {0: 1e200}}),
        _c("huge-y", e["huge-y"], y_set={2: {0: 1e3}}),
        _c("nan-y0", e["nan-y0"], y_set={0: row(NAN)}, clean_tail=tail("nan-y0")),
        _c("inf-y0", e["inf-y0"], y_set={0: row(1e200)}),
        _c("bad-first", e["bad-first"], theta=(bad, th[1])),
        _c("bad-row", e["bad-row"], R=3, theta=(th[0], bad, th[1])),
        _c("nan-sched3-carried", e["nan-sched3-carried"], sched=3, T=8, y_set={4: {0: NAN}}),
        _c("nan-sched3-resampling", e["nan-sched3-resampling"], sched=3, T=8, y_set={3: {0: NAN}}),
    ]
    if dy == 2:
        c.insert(1, _c("nan-y1", e["nan-y1"], y_set={2: {1: NAN}}))
    for name in COV_CASES.get(header, ()):
        if name == "null-z-nan-y":
            c.append(_c(name, e[name], y_set={2: {0: NAN}}, null_z=True))
        else:
            j = int(name[5])
            t = 0 if name.endswith("first") else 2
            c.append(_c(name, e[name], z_set={t: {j: NAN}}, clean_tail=tail(name)))
    for k in c:
        k["theta"] = k["theta"] or th
    return c


def case_of(header, name):
    return next(c for c in cases(header) if c["name"] == name)


def clean(case):
    """The same case without its degenerate values."""
    return dict(case, name=case["name"] + "+clean", y_set={}, z_set={}, clean_tail=False, expect=dict(nan_steps=()))


_SPY = None


def series(header, case):
    """(y [T, dy], Z [T, K] or None)"""
    global _SPY
    if _SPY is None:
        _SPY = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
    s, T = HEADERS[header], case["T"]
    y = np.asarray(ucr.observations(_SPY, s["dy"], T), dtype=np.float64).reshape(T, s["dy"]).copy()
    Z = None if (s["K"] == 0 or case["null_z"]) else ucr.covariates(s["K"], T)
    for t, comps in case["y_set"].items():
        for d, v in comps.items():
            y[t, d] = v
    for t, cols in case["z_set"].items():
        for j, v in cols.items():
            Z[t, j] = v
    return y, Z


# ---- routes and pairs --------------------------------------------------------------------------------------------------------------
SMALL_ROUTES = tuple(f"small-{n}" for n in (1, 64, 100, 200, 300, 1000, 2000))
EDGE_ROUTES = tuple(f"edge-n{n}" for n in (1, 2, 3, 2047, 2049))
TILED_ROUTES = ("wl2-512", "wl2-2048", "split-forced-5", "tables-5")


def routes():
    keep = SMALL_ROUTES + EDGE_ROUTES + TILED_ROUTES
    return [r for r in bc.routes() if r["name"] in keep]


ROUTES = {r["name"]: r for r in routes()}
ON_EVERY_TILED = ("nan-y", "nan-y1", "inf-y", "huge-y")
ON_EVERY_SMALL = ("nan-y", "nan-y0")                    # + the header's covariate cases; small-300 also takes the two below
ON_SMALL_300 = ("bad-first", "nan-sched3-carried")


def pairs(header):
    """[(case, route)] in route order.  Small routes: the scalar headers; nan-y, nan-y0 (the first step of the whole-series kernels)
    and the covariate cases on each, bad-first and a carried schedule on small-300.  Edge-N routes: nan-y, and bad-first for the
    vector headers.  Tiled routes: nan-y(1), inf-y, huge-y and the covariate cases on all four, every other case on wl2-512."""
    cov = COV_CASES.get(header, ())
    out = []
    for r in routes():
        for c in cases(header):
            n = c["name"]
            if r["kind"] == "small":
                take = header in SCALAR and (n in ON_EVERY_SMALL or n in cov or (r["name"] == "small-300" and n in ON_SMALL_300))
            elif r["kind"] == "edge":
                take = n == "nan-y" or (header in VECTOR and n == "bad-first")
            else:
                take = n in ON_EVERY_TILED or n in cov or r["name"] == "wl2-512"
            if take:
                out.append((c, r))
    return out


def pair_id(p):
    return f"{p[0]['name']}@{p[1]['name']}"


def shape(case, route):
    """(N, tile, B, T)"""
    n = route["n"]
    tile = route["tile"] or bc.default_tile(n, case["R"])
    return n, tile, -(-n // tile), case["T"]


def route_of(header, case, route, form, resampler, t=1):
    """bs_edge_cases.route_of() for a user model: a vector model never takes the whole-series kernels (ssme_pf_set_small_series)."""
    if header in VECTOR:
        route = dict(route, small=False)
    return bc.route_of(dict(case, model=3), route, form, resampler, t)


# ---- the headers restated on Python floats -----------------------------------------------------------------------------------------
def _scalar_fn(fn):
    a, b = (C.c_double * 1)(), (C.c_double * 1)()

    def f(v):
        a[0] = v
        fn(a, b, 1)
        return b[0]
    return f


def model_fns(O, header, th):
    """dict(bad, init(zn, y, zc) -> x0, prop(x, zn, zc) -> x', logg(y, x, zc, first) -> log g [+ first_logw]) of one theta row; x, zn,
    y, zc index as sequences of floats.  Each line is the header's, in its operation order."""
    E, LOG = _scalar_fn(O.lib().orc_exp_t), _scalar_fn(O.lib().orc_log)
    inf = float("inf")
    if header == "svol_student_t":
        libm = C.CDLL("libm.so.6")
        libm.lgamma.restype, libm.lgamma.argtypes = C.c_double, [C.c_double]
        beta, phi, sigma, nu = th
        a2 = sigma / math.sqrt(1.0 - phi * phi)
        a3 = ((libm.lgamma(0.5 * (nu + 1.0)) - libm.lgamma(0.5 * nu)) - 0.5 * LOG(nu * 3.14159265358979311600)) - (LOG(beta) if beta > 0.0 else NAN)
        a4, a5 = 1.0 / (nu * (beta * beta)), 0.5 * (nu + 1.0)
        return dict(bad=not (beta > 0.0) or not (nu > 0.0), init=lambda zn, y, zc: (zn[0] * a2,), prop=lambda x, zn, zc: (phi * x[0] + zn[0] * sigma,),
                    logg=lambda y, x, zc, first: (a3 - 0.5 * x[0]) - a5 * LOG(1.0 + ((y[0] * y[0]) * a4) * E(-x[0])))
    if header == "lin_gauss_3d":
        phi, s1, s2, s3, tau = th
        a4 = 1.0 / math.sqrt(1.0 - phi * phi)
        bad = not (tau > 0.0)
        a5, a6 = (NAN if bad else LOG(tau)), 1.0 / tau

        def logg(y, x, zc, first):
            d = (y[0] - ((x[0] + x[1]) + x[2])) * a6
            return (-a5 - HALF_LOG_2PI) - 0.5 * (d * d)
        return dict(bad=bad, init=lambda zn, y, zc: (zn[0] * (s1 * a4), zn[1] * (s2 * a4), zn[2] * (s3 * a4)),
                    prop=lambda x, zn, zc: (phi * x[0] + zn[0] * s1, phi * x[1] + zn[1] * s2, phi * x[2] + zn[2] * s3), logg=logg)
    if header == "svol_two_factor":
        beta, phi1, phi2, s1, s2, rho = th
        bad = not (beta > 0.0)
        a2, a3, a4 = s1, s2 * rho, s2 * math.sqrt(1.0 - rho * rho)
        a5, a6 = (NAN if bad else LOG(beta)), 1.0 / (beta * beta)

        def logg(y, x, zc, first):
            u1, u2 = x[0] + x[1], x[1]
            l1 = (-(a5 + 0.5 * u1) - HALF_LOG_2PI) - 0.5 * (((y[0] * y[0]) * a6) * E(-u1))
            l2 = (-(a5 + 0.5 * u2) - HALF_LOG_2PI) - 0.5 * (((y[1] * y[1]) * a6) * E(-u2))
            return l1 + l2
        return dict(bad=bad, init=lambda zn, y, zc: (zn[0] * a2, zn[1] * a4),
                    prop=lambda x, zn, zc: (phi1 * x[0] + zn[0] * a2, (phi2 * x[1] + zn[0] * a3) + zn[1] * a4), logg=logg)
    if header in ("svol_reg_cov", "svol_reg_cov_nofirst"):
        phi, mu, sigma, b0, b2, g = th
        a2 = sigma / math.sqrt(1.0 - phi * phi)
        has_first = header == "svol_reg_cov"

        def init(zn, y, zc):
            if not has_first:
                return (zn[0] * a2,)
            m = mu + 0.25 * (y[0] - b0 * zc[0])
            return (m + (2.0 * a2) * zn[0],)

        def logg(y, x, zc, first):
            r = (y[0] - b0 * zc[0]) - b2 * zc[2]
            hl = 0.5 * x[0]
            v = (-hl - HALF_LOG_2PI) - 0.5 * ((r * r) * E(-x[0]))
            if hl < -745.1332191019412:
                v = -inf
            if first and has_first:
                m = mu + 0.25 * (y[0] - b0 * zc[0])
                d1 = (x[0] - mu) / a2
                d2 = (x[0] - m) / (2.0 * a2)
                v = ((ucr.LOG2 - 0.5 * (d1 * d1)) + 0.5 * (d2 * d2)) + v
            return v
        return dict(bad=not (sigma > 0.0), init=init, prop=lambda x, zn, zc: (((mu + phi * (x[0] - mu)) + g * zc[1]) + zn[0] * sigma,), logg=logg)
    assert header == "svol_two_factor_cov"
    beta, phi1, phi2, s1, s2, rho = th
    bad = not (beta > 0.0)
    a2, a3, a4 = s1, s2 * rho, s2 * math.sqrt(1.0 - rho * rho)
    a5 = NAN if bad else LOG(beta)

    def logg(y, x, zc, first):
        r1, r2 = y[0] - 0.5 * zc[2], y[1] + 0.4 * zc[3]
        h1, h2 = a5 + 0.5 * (x[0] + x[1]), a5 + 0.5 * x[1]
        l1 = (-h1 - HALF_LOG_2PI) - 0.5 * ((r1 * r1) * E(-2.0 * h1))
        l2 = (-h2 - HALF_LOG_2PI) - 0.5 * ((r2 * r2) * E(-2.0 * h2))
        v = l1 + l2
        if first:
            p1, p2 = x[0] / a2, x[1] / a4
            q1 = (x[0] - 0.1 * zc[0]) / (1.5 * a2)
            q2 = (x[1] - 0.05 * (y[1] + 0.4 * zc[3])) / (1.5 * a4)
            v = ((ucr.TWO_LOG_1P5 - 0.5 * (p1 * p1 + p2 * p2)) + 0.5 * (q1 * q1 + q2 * q2)) + v
        return v
    return dict(bad=bad, init=lambda zn, y, zc: (0.1 * zc[0] + (1.5 * a2) * zn[0], 0.05 * (y[1] + 0.4 * zc[3]) + (1.5 * a4) * zn[1]),
                prop=lambda x, zn, zc: ((phi1 * x[0] + 0.3 * zc[0]) + zn[0] * a2, ((phi2 * x[1] - 0.2 * zc[1]) + zn[0] * a3) + zn[1] * a4), logg=logg)


class StepFilter:
    """oracle.UserVectorModelFilter (raw callbacks: C double pointers, no numpy view per call) of one header and theta row, driven one
    step at a time: .step(y_row, z_row) -> log conditional likelihood, .state(), .reset(), .loglik."""

    def __init__(self, O, header, th, n, rep, resampler, sched, tile):
        s = HEADERS[header]
        self.K = s["K"]
        f = model_fns(O, header, [float(v) for v in th])
        cur = self.cur = dict(y=None, z=(0.0,) * max(self.K, 1), first=True)

        def init(zn, x0):
            for d, v in enumerate(f["init"](zn, cur["y"], cur["z"])):
                x0[d] = v

        def prop(x, zn, zcov, xn):
            for d, v in enumerate(f["prop"](x, zn, cur["z"])):
                xn[d] = v

        def logg(y, x):
            return f["logg"](y, x, cur["z"], cur["first"])
        self.f = O.UserVectorModelFilter(n, SEED, s["dx"], s["dy"], init, prop, logg, rep=rep, resampler=resampler, resamp_sched=sched, tile=tile,
                                         bad=f["bad"], raw=True)
        self.t = 0

    def reset(self):
        self.f.reset()
        self.t = 0

    def step(self, y_row, z_row=None):
        self.cur["y"] = tuple(float(v) for v in np.ravel(y_row))
        self.cur["z"] = (0.0,) * max(self.K, 1) if z_row is None else tuple(float(v) for v in z_row)
        self.cur["first"] = self.t == 0
        self.t += 1
        return self.f.step(y_row)

    @property
    def loglik(self):
        return self.f.loglik

    def state(self):
        return self.f.state()


_RUNS = {}


def oracle_run(O, header, case, route, resampler):
    """[(lls[R], states[R])] after every step (x: [dx, N]); computed once per (header, case, shape, resampler) and shared read-only."""
    n, tile, B, T = shape(case, route)
    key = (header, case["name"], n, tile, resampler)
    if key not in _RUNS:
        fs = [StepFilter(O, header, case["theta"][r], n, r, resampler, case["sched"], tile) for r in range(case["R"])]
        y, Z = series(header, case)
        steps = []
        for t in range(T):
            lls = [f.step(y[t], None if Z is None else Z[t]) for f in fs]
            steps.append((lls, [f.state() for f in fs]))
        _RUNS[key] = steps
    return _RUNS[key]


def forget_runs():
    _RUNS.clear()


def key_file(key):
    """The file, in the worker's output directory, of one result key."""
    return key.replace("|", "__").replace("@", "_at_") + ".pkl"


FUNCTIONAL_MAX_N = 1613                 # the exact ratio is rational arithmetic over N particles (0.3 s at N = 2125): wl2-512, the small routes and N = 1, 2, 3
NO_FUNCTIONALS = ("inf-y0",)            # x ~ 1e199 after the step: exp(x / 2) = inf, the functionals have no finite reference


def probes(case):
    """The steps after which user_expectations() is compared: the first degenerate step (all NaN where S = 0), the step after it
    (the recovering one, where the case recovers) and the last."""
    if case["name"] in NO_FUNCTIONALS:
        return ()
    e = case["expect"]
    marks = [t for steps in (e["nan_steps_r"] if "nan_steps_r" in e else (e["nan_steps"],)) for t in steps] + ([e["big_step"]] if "big_step" in e else [])
    first = min(marks)
    return tuple(sorted({t for t in (first, first + 1, case["T"] - 1) if t < case["T"]}))


def h_rows(O, header, th, x, zc):
    """[n_h, N] of a covariate header (user_cov_ref.h_rows; NaN particles give NaN rows without a warning)."""
    with np.errstate(all="ignore"):
        return ucr.h_rows(O, header, th, x, zc)


# ---- series bookkeeping (zbuf of Tcap * K doubles, set_last_z, the graph keyed by T and has_z) --------------------------------------
BOOK_HEADERS = ("svol_reg_cov", "svol_two_factor_cov")
BOOK_SHAPES = ((300, 2048, True), (300, 2048, False), (1613, 512, False))        # (N, tile, whole-series kernel wanted)
BOOK_LENGTHS = (2, 40, 6)                                                         # on one handle, in this order; T = 1 on a handle of its own
BOOK_R = 2


def book_series(header, T, with_z=True):
    """(y [T, dy], Z [T, K] or None): covariates drawn PER LENGTH (seed 100 + T), so that a row left over from another length changes
    the bits."""
    global _SPY
    if _SPY is None:
        _SPY = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
    s = HEADERS[header]
    y = np.asarray(ucr.observations(_SPY, s["dy"], T), dtype=np.float64).reshape(T, s["dy"]).copy()
    return y, (ucr.covariates(s["K"], T, seed=100 + T) if with_z else None)


def book_oracle(O, header, n, tile, T, with_z, resampler=0):
    """(per [R, T], states[R] after the last step) of a fresh filter pair on book_series(header, T, with_z)."""
    key = ("book", header, n, tile, T, with_z, resampler)
    if key not in _RUNS:
        y, Z = book_series(header, T, with_z)
        per, sts = np.empty((BOOK_R, T)), []
        for r in range(BOOK_R):
            f = StepFilter(O, header, HEADERS[header]["theta"][r], n, r, resampler, 1, tile)
            for t in range(T):
                per[r, t] = f.step(y[t], None if Z is None else Z[t])
            sts.append(f.state())
        _RUNS[key] = (per, sts)
    return _RUNS[key]
