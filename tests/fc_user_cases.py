"""Shapes, parameters and inputs of the user-model forecast tests, shared by tests/forecast_user_model_worker.py (which runs them on
the device) and tests/test_forecast_user_gpu.py (which restates them on the CPU)."""
import numpy as np

SEED = 0x5eed0000c0ffee
FIRST_ID = 5                       # first_filter_id of the banks with more than one filter
T_STEPS = 4                        # filter steps before a forecast
# (N, tile, H, R): tile 0 = the default for (N, R)
TWIN_SHAPES = [(1, 0, 17, 1), (2, 0, 2, 3), (501, 0, 17, 3), (2049, 0, 2, 3), (3 * 2048 + 7, 512, 1, 1)]
PARITY_SHAPES = [(1, 0, 5, 1), (501, 0, 5, 3), (2049, 0, 1, 1), (3 * 2048 + 7, 512, 2, 3)]
ANCHOR_N, ANCHOR_H = 65536, 3

# one parameter row per model; thetas() perturbs it per filter
BASE_THETA = {
    "svol_leverage_user": [0.95, -0.4, 0.3, -0.6],                  # phi, mu, sigma, rho
    "svol_two_factor_g": [1.1, 0.95, 0.9, 0.2, 0.15, -0.4],         # beta, phi1, phi2, sigma1, sigma2, rho
    "svol_two_factor_lev_g": [1.1, 0.95, 0.9, 0.2, 0.15, -0.4],     # the same; x2 also reads the covariate
    "lin_gauss_3d_g": [0.9, 0.5, 0.3, 0.2, 0.7],                    # phi, sigma_1..3, tau
    "lin_gauss_4d_g": [0.9, 0.5, 0.7, 0.4, 1.1, 0.25],              # phi, sigma, tau_1..4
}
DIM_Y = {"svol_leverage_user": 1, "svol_two_factor_g": 2, "svol_two_factor_lev_g": 2, "lin_gauss_3d_g": 1, "lin_gauss_4d_g": 4}


def thetas(name, R):
    """[R, n_theta]: the base row scaled by up to +-3 % per filter and parameter (row 0 of R = 1 is the base row itself)."""
    base = np.asarray(BASE_THETA[name], dtype=np.float64)
    if R == 1:
        return base[None, :].copy()
    rng = np.random.default_rng(7)
    return base[None, :] * (1.0 + 0.03 * rng.uniform(-1.0, 1.0, (R, base.size)))


def bad_theta(name):
    """A row whose derive() sets `bad` (a scale parameter that is not positive): every weight is zero."""
    th = np.asarray(BASE_THETA[name], dtype=np.float64).copy()
    th[{"svol_two_factor_g": 0, "svol_two_factor_lev_g": 0, "lin_gauss_3d_g": 4, "lin_gauss_4d_g": 3}[name]] = -1.0
    return th


def last_obs(R):
    """y_prev[0] of the first horizon, one value per filter, none of them zero."""
    return 0.37 - 0.21 * np.arange(R)


def observation(spy, name, t):
    """The dim_y observations of step t: daily returns in percent, component j from day 100 j + t.  They are of the size of the states
    of every test model (standard deviations between 0.5 and 1.2), so the weights of a step spread over all tiles."""
    return np.array([spy[100 * j + t] for j in range(DIM_Y[name])])
