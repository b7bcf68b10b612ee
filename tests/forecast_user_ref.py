"""A numpy restatement of the forecast of USER models that declare their observation draw (ssme_amd/csrc/model_api.h: gsamp /
gsamp_vec), written from its definition on the primitives of forecast_ref.py (philox_rows, pair_normals,
start_draw, u01_mid40).  No device code; test_forecast_user_cpu.py and test_forecast_user_gpu.py share it.

Per horizon k and particle i, Philox call c in {0, 1} has the counter (i, t0, filter id, S_c + (k << 8)), S_0 = 161, S_1 = 164; words
0-1 of call c give (zs[2c], zo[2c]) and words 2-3 give (zs[2c + 1], zo[2c + 1]), the first output of pair_normals being the state
normal.  Only what max(dim_x, dim_y) needs is drawn; members past dim_x (state) or dim_y (observation) are dropped.  Then
    x <- prop(c, x, zs, zcov = y_prev[0]);  y <- gsamp(c, x, zo);  y_prev <- y.
MODELS restates derive / prop / gsamp of every test header of tests/models/ that declares the draw, in the header's operation order.
Every function takes the oracle module as `O` (its libm-free exp_t, log)."""
import numpy as np

from forecast_ref import STREAM_SIM, pair_normals, philox_rows, start_draw, u01_mid40  # noqa: F401  (u01_mid40: part of the draw layout)

STREAM_SIM2 = 164


def user_normals(O, i, t0, rep, k, seed, dm):
    """(zs, zo): two lists of dm arrays, the state and observation normals of particles i at horizon k."""
    zs, zo = [], []
    for c, stream in enumerate((STREAM_SIM, STREAM_SIM2)):
        if 2 * c >= dm:
            break
        w = philox_rows(O, i, t0, rep, stream + (k << 8), seed)
        for lo in (0, 2)[:min(2, dm - 2 * c)]:
            a, b = pair_normals(O, w[:, lo], w[:, lo + 1])
            zs.append(a)
            zo.append(b)
    return zs, zo


def _log1(O, v):
    return float(O.log(np.array([float(v)]))[0])


# ---- the test models: constants as the header's derive leaves them, prop / gsamp on lists of component arrays -----------------------
def _lev_derive(O, th):                                            # svol_leverage_user.h: (phi, mu, sigma, rho)
    phi, mu, sigma, rho = th
    return dict(a0=phi, a1=mu, a3=sigma * np.sqrt(1.0 - phi * phi), a4=rho * sigma)


def _lev_prop(O, c, x, zs, zcov):
    e = O.exp_t(-0.5 * x[0])
    mean = (c["a1"] + c["a0"] * (x[0] - c["a1"])) + (c["a4"] * zcov) * e
    return [mean + zs[0] * c["a3"]]


def _lev_gsamp(O, c, x, zo):
    return [O.exp_t(0.5 * x[0]) * zo[0]]


def _tf_derive(O, th):                                             # svol_two_factor_g.h: (beta, phi1, phi2, sigma1, sigma2, rho)
    beta, phi1, phi2, s1, s2, rho = th
    return dict(a0=phi1, a1=phi2, a2=s1, a3=s2 * rho, a4=s2 * np.sqrt(1.0 - rho * rho), a6=beta)


def _tf_prop(O, c, x, zs, zcov):
    return [c["a0"] * x[0] + zs[0] * c["a2"], (c["a1"] * x[1] + zs[0] * c["a3"]) + zs[1] * c["a4"]]


def _tf_gsamp(O, c, x, zo):
    return [(c["a6"] * O.exp_t(0.5 * (x[0] + x[1]))) * zo[0], (c["a6"] * O.exp_t(0.5 * x[1])) * zo[1]]


def _tfl_prop(O, c, x, zs, zcov):                                  # svol_two_factor_lev_g.h: the second factor reads the covariate
    return [c["a0"] * x[0] + zs[0] * c["a2"], ((c["a1"] * x[1] + zs[0] * c["a3"]) + zs[1] * c["a4"]) + (-0.05 * zcov)]


def _l3_derive(O, th):                                             # lin_gauss_3d_g.h: (phi, sigma_1, sigma_2, sigma_3, tau)
    return dict(a0=th[0], a1=th[1], a2=th[2], a3=th[3], a5=_log1(O, th[4]))


def _l3_prop(O, c, x, zs, zcov):
    return [c["a0"] * x[0] + zs[0] * c["a1"], c["a0"] * x[1] + zs[1] * c["a2"], c["a0"] * x[2] + zs[2] * c["a3"]]


def _l3_gsamp(O, c, x, zo):
    taup = float(O.exp_t(np.array([c["a5"]]))[0])
    return [((x[0] + x[1]) + x[2]) + taup * zo[0]]


def _l4_derive(O, th):                                             # lin_gauss_4d_g.h: (phi, sigma, tau_1 .. tau_4)
    return dict(a0=th[0], a1=th[1], inv=[1.0 / th[2], 1.0 / th[3], 1.0 / th[4], 1.0 / th[5]])


def _l4_prop(O, c, x, zs, zcov):
    return [c["a0"] * x[d] + zs[d] * c["a1"] for d in range(4)]


def _l4_gsamp(O, c, x, zo):
    return [x[d] + (1.0 / c["inv"][d]) * zo[d] for d in range(4)]


MODELS = {
    "svol_leverage_user": dict(dx=1, dy=1, derive=_lev_derive, prop=_lev_prop, gsamp=_lev_gsamp),
    "svol_two_factor_g": dict(dx=2, dy=2, derive=_tf_derive, prop=_tf_prop, gsamp=_tf_gsamp),
    "svol_two_factor_lev_g": dict(dx=2, dy=2, derive=_tf_derive, prop=_tfl_prop, gsamp=_tf_gsamp),
    "lin_gauss_3d_g": dict(dx=3, dy=1, derive=_l3_derive, prop=_l3_prop, gsamp=_l3_gsamp),
    "lin_gauss_4d_g": dict(dx=4, dy=4, derive=_l4_derive, prop=_l4_prop, gsamp=_l4_gsamp),
}


def forecast_user(O, name, theta, st, n, tile, seed, rep, t0, H, last_obs=0.0):
    """(start[n], x[H, dim_x, n], y[H, dim_y, n]) of one filter of the test model `name`.  st: the device's own download of the
    filter (ParticleFilterBank.state(): x[n] or x[dim_x, n], cdf, A, mb, rshift).  A filter without weight: NaN samples."""
    m = MODELS[name]
    dx, dy = m["dx"], m["dy"]
    c = m["derive"](O, [float(v) for v in np.asarray(theta, dtype=np.float64)])
    start, alive = start_draw(O, st, n, tile, seed, rep, t0)
    xs, ys = np.full((H, dx, n), np.nan), np.full((H, dy, n), np.nan)
    if alive:
        with np.errstate(invalid="ignore", over="ignore"):
            x0 = np.asarray(st["x"], dtype=np.float64).reshape(dx, -1)
            x = [x0[d][start] for d in range(dx)]
            yp = np.full(n, float(last_obs))
            for k in range(H):
                zs, zo = user_normals(O, np.arange(n), t0, rep, k, seed, max(dx, dy))
                x = m["prop"](O, c, x, zs[:dx], yp)
                y = m["gsamp"](O, c, x, zo[:dy])
                yp = y[0]
                xs[k], ys[k] = np.stack(x), np.stack(y)
    return start, xs, ys
