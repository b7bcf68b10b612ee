"""References for user models with covariates (ssme_amd/csrc/model_api.h: dim_cov, first, first_logw), shared by
test_user_cov_cpu.py, test_user_cov_gpu.py and user_cov_worker.py.  No device code.

1. MODELS: numpy restatements of the headers tests/models/svol_reg_cov.h, svol_reg_cov_nofirst.h, svol_leverage_cov1.h and
   svol_two_factor_cov.h, operation for operation, on the oracle's libm-free exp_t / log (module `O`).  States, normals and
   observations are lists of component arrays (or 1-element arrays for one particle), covariates a sequence of K floats.
2. oracle_filter: the oracle's callback-driven filters with closures over the covariate table Z [T, K].  The oracle needs no change:
   * scalar model without `first`: oracle.UserModelFilter, driven step by step; the closures read the row the driver sets;
   * vector model, or any model with `first`: oracle.UserVectorModelFilter.run_series with z = arange(T); prop takes t = int(zcov) and
     looks up Z[t], logg reads the t prop last saw (0 at the first step, where init is called instead); init serves as `first`
     and first_logw is added inside logg at t = 0.
3. forecast_cov: the covariate forecast on the primitives of forecast_ref.py / forecast_user_ref.py:
   x <- prop(x, zs, Z_f[k]);  y <- gsamp(x, zo, Z_f[k]), same start draw and counters as every other forecast."""
import numpy as np

from forecast_user_ref import start_draw, user_normals

HALF_LOG_2PI = 0.91893853320467274178
LOG2 = 0.69314718055994530942
TWO_LOG_1P5 = 0.81093021621632877

# parameters: R = 2 filters with different rows; the tests compare filter 1
TH_REG = np.array([[0.95, -0.2, 0.25, 0.3, -0.15, 0.1], [0.9, 0.1, 0.3, -0.2, 0.25, -0.05]])      # phi, mu, sigma, b0, b2, g
TH_LEV = np.array([[0.95, -0.1, 0.2, -0.4], [0.9, 0.05, 0.25, -0.3]])                             # phi, mu, sigma, rho
TH_2F = np.array([[1.1, 0.95, 0.9, 0.2, 0.15, -0.4], [0.95, 0.9, 0.93, 0.25, 0.12, -0.3]])        # beta, phi1, phi2, s1, s2, rho
T_STEPS = 6
SHAPES = ((500, 2048), (2500, 512), (2500, 2048))        # (N, tile): one ragged tile; five tiles, ragged; two tiles
SEED = 20240229


def covariates(K, T=T_STEPS, seed=7):
    """The fixed-seed normal draw of the tests: [T, K]."""
    return np.random.default_rng(seed).standard_normal((T, 4))[:, :K].copy()


def observations(spy, dy, T=T_STEPS):
    return spy[:T].copy() if dy == 1 else np.stack([spy[:T], spy[100:100 + T]], axis=1)


def _log1(O, v):
    return float(O.log(np.array([float(v)]))[0])


def _E(O, v):
    return O.exp_t(np.atleast_1d(np.asarray(v, dtype=np.float64)))


# ---- svol_reg_cov.h / svol_reg_cov_nofirst.h ---------------------------------------------------------------------------------------
def _reg_derive(O, th):
    phi, mu, sigma, b0, b2, g = th
    return dict(a0=phi, a1=mu, a2=sigma / np.sqrt(1.0 - phi * phi), a3=sigma, a4=b0, a5=b2, a6=g, bad=not (sigma > 0.0))


def _reg_prop(O, c, x, zn, zc):
    mean = (c["a1"] + c["a0"] * (x[0] - c["a1"])) + c["a6"] * zc[1]
    return [mean + zn[0] * c["a3"]]


def _reg_logg(O, c, y, x, zc):
    r = (y[0] - c["a4"] * zc[0]) - c["a5"] * zc[2]
    hl = 0.5 * x[0]
    e = _E(O, -x[0])
    v = (-hl - HALF_LOG_2PI) - 0.5 * ((r * r) * e)
    return np.where(hl < -745.1332191019412, -np.inf, v)


def _reg_gsamp(O, c, x, zo, zc):
    m = c["a4"] * zc[0] + c["a5"] * zc[2]
    return [m + _E(O, 0.5 * x[0]) * zo[0]]


def _reg_h(O, c, x, zc):
    return [x[0], _E(O, 0.5 * x[0]), x[0] + c["a5"] * zc[2]]


def _reg_first(O, c, zn, y, zc):
    m = c["a1"] + 0.25 * (y[0] - c["a4"] * zc[0])
    return [m + (2.0 * c["a2"]) * zn[0]]


def _reg_first_logw(O, c, y, x0, zc):
    m = c["a1"] + 0.25 * (y[0] - c["a4"] * zc[0])
    d1 = (x0[0] - c["a1"]) / c["a2"]
    d2 = (x0[0] - m) / (2.0 * c["a2"])
    return (LOG2 - 0.5 * (d1 * d1)) + 0.5 * (d2 * d2)


def _scalar_init(O, c, zn):
    return [zn[0] * c["a2"]]


# ---- svol_leverage_cov1.h ----------------------------------------------------------------------------------------------------------
def _lev_derive(O, th):
    phi, mu, sigma, rho = th
    return dict(a0=phi, a1=mu, a2=sigma / np.sqrt(1.0 - phi * phi), a3=sigma * np.sqrt(1.0 - phi * phi), a4=rho * sigma, bad=False)


def _lev_prop(O, c, x, zn, zc):
    e = _E(O, -0.5 * x[0])
    mean = (c["a1"] + c["a0"] * (x[0] - c["a1"])) + (c["a4"] * zc[0]) * e
    return [mean + zn[0] * c["a3"]]


def _lev_logg(O, c, y, x, zc):
    hl = 0.0 + 0.5 * x[0]
    e = _E(O, -x[0])
    q = (y[0] * y[0]) * 1.0
    v = (-hl - HALF_LOG_2PI) - 0.5 * (q * e)
    return np.where(hl < -745.1332191019412, -np.inf, v)


def _lev_gsamp(O, c, x, zo, zc):
    return [_E(O, 0.5 * x[0]) * zo[0]]


# ---- svol_two_factor_cov.h ---------------------------------------------------------------------------------------------------------
def _tf_derive(O, th):
    beta, phi1, phi2, s1, s2, rho = th
    return dict(a0=phi1, a1=phi2, a2=s1, a3=s2 * rho, a4=s2 * np.sqrt(1.0 - rho * rho), a5=_log1(O, beta), a6=beta, bad=not (beta > 0.0))


def _tf_first(O, c, zn, y, zc):
    return [0.1 * zc[0] + (1.5 * c["a2"]) * zn[0], 0.05 * (y[1] + 0.4 * zc[3]) + (1.5 * c["a4"]) * zn[1]]


def _tf_first_logw(O, c, y, x0, zc):
    p1, p2 = x0[0] / c["a2"], x0[1] / c["a4"]
    q1 = (x0[0] - 0.1 * zc[0]) / (1.5 * c["a2"])
    q2 = (x0[1] - 0.05 * (y[1] + 0.4 * zc[3])) / (1.5 * c["a4"])
    return (TWO_LOG_1P5 - 0.5 * (p1 * p1 + p2 * p2)) + 0.5 * (q1 * q1 + q2 * q2)


def _tf_prop(O, c, x, zn, zc):
    return [(c["a0"] * x[0] + 0.3 * zc[0]) + zn[0] * c["a2"], ((c["a1"] * x[1] - 0.2 * zc[1]) + zn[0] * c["a3"]) + zn[1] * c["a4"]]


def _tf_logg(O, c, y, x, zc):
    r1, r2 = y[0] - 0.5 * zc[2], y[1] + 0.4 * zc[3]
    h1, h2 = c["a5"] + 0.5 * (x[0] + x[1]), c["a5"] + 0.5 * x[1]
    l1 = (-h1 - HALF_LOG_2PI) - 0.5 * ((r1 * r1) * _E(O, -2.0 * h1))
    l2 = (-h2 - HALF_LOG_2PI) - 0.5 * ((r2 * r2) * _E(O, -2.0 * h2))
    return l1 + l2


def _tf_gsamp(O, c, x, zo, zc):
    return [0.5 * zc[2] + (c["a6"] * _E(O, 0.5 * (x[0] + x[1]))) * zo[0], -0.4 * zc[3] + (c["a6"] * _E(O, 0.5 * x[1])) * zo[1]]


def _tf_h(O, c, x, zc):
    return [x[0], x[1], x[0] * x[1] + zc[1], c["a6"] * _E(O, 0.5 * (x[0] + x[1])) + zc[3]]


MODELS = {
    "svol_reg_cov": dict(dx=1, dy=1, K=3, n_h=3, theta=TH_REG, derive=_reg_derive, prop=_reg_prop, logg=_reg_logg, gsamp=_reg_gsamp, h=_reg_h,
                         first=_reg_first, first_logw=_reg_first_logw),
    "svol_reg_cov_nofirst": dict(dx=1, dy=1, K=3, n_h=3, theta=TH_REG, derive=_reg_derive, prop=_reg_prop, logg=_reg_logg, gsamp=_reg_gsamp,
                                 h=_reg_h, first=None, first_logw=None),
    "svol_leverage_cov1": dict(dx=1, dy=1, K=1, n_h=0, theta=TH_LEV, derive=_lev_derive, prop=_lev_prop, logg=_lev_logg, gsamp=_lev_gsamp, h=None,
                               first=None, first_logw=None),
    "svol_two_factor_cov": dict(dx=2, dy=2, K=4, n_h=4, theta=TH_2F, derive=_tf_derive, prop=_tf_prop, logg=_tf_logg, gsamp=_tf_gsamp, h=_tf_h,
                                first=_tf_first, first_logw=_tf_first_logw),
}


def constants(O, name, theta):
    return MODELS[name]["derive"](O, [float(v) for v in np.asarray(theta, dtype=np.float64)])


# ---- the oracle's filters with covariate closures ----------------------------------------------------------------------------------
def _one(v):
    """A component list of 1-element arrays from a view of floats."""
    return [np.array([float(a)]) for a in v]


def scalar_oracle(O, name, theta, Z, n, seed, rep, resampler, sched, tile):
    """oracle.UserModelFilter of a scalar model WITHOUT `first`; .cov_step(t, y) sets row t of Z and steps."""
    m = MODELS[name]
    assert m["dx"] == 1 and m["dy"] == 1 and m["first"] is None
    c = constants(O, name, theta)
    cur = {"z": [0.0] * m["K"]}
    prop = lambda x, zn, zcov: float(m["prop"](O, c, _one([x]), _one([zn]), cur["z"])[0][0])
    logg = lambda y, x: float(m["logg"](O, c, [y], _one([x]), cur["z"])[0])
    f = O.UserModelFilter(n, seed, c["a2"], prop, logg, rep=rep, resampler=resampler, resamp_sched=sched, tile=tile, bad=c["bad"])

    def cov_step(t, y):
        cur["z"] = [0.0] * m["K"] if Z is None else [float(v) for v in Z[t]]
        return f.step(float(y), 0.0)
    f.cov_step = cov_step
    return f


def vector_oracle(O, name, theta, Z, n, seed, rep, resampler, sched, tile, T):
    """oracle.UserVectorModelFilter of any model (dx = dy = 1 included); .cov_run(y) runs the series with z = arange(T)."""
    m = MODELS[name]
    c = constants(O, name, theta)
    row = lambda t: [0.0] * m["K"] if Z is None else [float(v) for v in Z[t]]
    cur = {"t": 0}

    def init(zn):
        cur["t"] = 0
        if m["first"] is None:
            return [float(v[0]) for v in _scalar_init(O, c, _one(zn))]
        return [float(v[0]) for v in m["first"](O, c, _one(zn), cur["y0"], row(0))]

    def prop(x, zn, zcov):
        cur["t"] = int(zcov)
        return [float(v[0]) for v in m["prop"](O, c, _one(x), _one(zn), row(cur["t"]))]

    def logg(y, x):
        t = cur["t"]
        yv, xv = [float(v) for v in y], _one(x)
        g = m["logg"](O, c, yv, xv, row(t))
        if t == 0 and m["first"] is not None:
            g = m["first_logw"](O, c, yv, xv, row(0)) + g
        return float(np.atleast_1d(g)[0])
    f = O.UserVectorModelFilter(n, seed, m["dx"], m["dy"], init, prop, logg, rep=rep, resampler=resampler, resamp_sched=sched, tile=tile,
                                bad=c["bad"])

    def cov_run(y):
        y = np.asarray(y, dtype=np.float64).reshape(T, m["dy"])
        cur["y0"] = [float(v) for v in y[0]]        # `first` looks at the first observation
        return f.run_series(y, np.arange(T, dtype=np.float64))
    f.cov_run = cov_run
    return f


# ---- functionals and forecast on arrays ---------------------------------------------------------------------------------------------
def h_rows(O, name, theta, x, zc):
    """[n_h, N]: the header's h on every particle of x ([N] or [dim_x, N]) with the covariates zc."""
    m = MODELS[name]
    xs = np.asarray(x, dtype=np.float64).reshape(m["dx"], -1)
    return np.stack([np.asarray(r, dtype=np.float64) for r in m["h"](O, constants(O, name, theta), [xs[d] for d in range(m["dx"])], [float(v) for v in zc])])


def forecast_cov(O, name, theta, st, n, tile, seed, rep, t0, Zf, per_particle=False):
    """(start[n], x[H, dim_x, n], y[H, dim_y, n]) of one filter with the exogenous covariates Zf [H, K] (per_particle: Zf[k] may hold
    arrays over the particles, for the self-check against forecast_user_ref).  A filter without weight: NaN samples."""
    m = MODELS[name]
    dx, dy, H = m["dx"], m["dy"], len(Zf)
    c = constants(O, name, theta)
    start, alive = start_draw(O, st, n, tile, seed, rep, t0)
    xs, ys = np.full((H, dx, n), np.nan), np.full((H, dy, n), np.nan)
    if alive:
        with np.errstate(invalid="ignore", over="ignore"):
            x0 = np.asarray(st["x"], dtype=np.float64).reshape(dx, -1)
            x = [x0[d][start] for d in range(dx)]
            for k in range(H):
                zc = list(Zf[k]) if per_particle else [float(v) for v in Zf[k]]
                zs, zo = user_normals(O, np.arange(n), t0, rep, k, seed, max(dx, dy))
                x = m["prop"](O, c, x, zs[:dx], zc)
                y = m["gsamp"](O, c, x, zo[:dy], zc)
                xs[k], ys[k] = np.stack(x), np.stack(y)
    return start, xs, ys
