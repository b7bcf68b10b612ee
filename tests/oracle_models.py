"""The test models of tests/models/ restated for the oracle's callback-driven filters (oracle.UserModelFilter /
UserVectorModelFilter) with the oracle's own libm-free functions; shared by test_parity_gpu.py and test_expectations_gpu.py."""
import numpy as np


def _student_t_oracle(oracle, n, seed, rep, resampler, tile, th=(1.1, 0.95, 0.25, 7.0)):
    """tests/models/svol_student_t.h restated with the oracle's own libm-free functions (the operation order is the header's)."""
    import ctypes, math
    libm = ctypes.CDLL("libm.so.6")               # the header's std::lgamma is libm's (CPython's math.lgamma is its own code)
    libm.lgamma.restype = ctypes.c_double
    libm.lgamma.argtypes = [ctypes.c_double]
    beta, phi, sigma, nu = th
    e1 = lambda f, v: float(f(np.array([v]))[0])
    a2 = sigma / math.sqrt(1.0 - phi * phi)
    a3 = ((libm.lgamma(0.5 * (nu + 1.0)) - libm.lgamma(0.5 * nu)) - 0.5 * e1(oracle.log, nu * math.pi)) - e1(oracle.log, beta)
    a4 = 1.0 / (nu * (beta * beta))
    a5 = 0.5 * (nu + 1.0)
    prop = lambda x, zn, zcov: phi * x + zn * sigma
    logg = lambda y, x: (a3 - 0.5 * x) - a5 * e1(oracle.log, 1.0 + ((y * y) * a4) * e1(oracle.exp_t, -x))
    return oracle.UserModelFilter(n, seed, a2, prop, logg, rep=rep, resampler=resampler, tile=tile)


def _two_factor_oracle(oracle, n, seed, rep, resampler, tile, sched, th=(1.1, 0.95, 0.9, 0.2, 0.15, -0.4)):
    """tests/models/svol_two_factor.h (dim_x = 2, dim_y = 2) restated with the oracle's own functions, in the header's operation order."""
    import math
    beta, phi1, phi2, s1, s2, rho = th
    e1 = lambda f, v: float(f(np.array([v]))[0])
    a2, a3, a4 = s1, s2 * rho, s2 * math.sqrt(1.0 - rho * rho)
    a5, a6 = e1(oracle.log, beta), 1.0 / (beta * beta)
    half_log_2pi = 0.91893853320467274178
    init = lambda zn: np.array([zn[0] * a2, zn[1] * a4])
    prop = lambda x, zn, zcov: np.array([phi1 * x[0] + zn[0] * a2, (phi2 * x[1] + zn[0] * a3) + zn[1] * a4])

    def logg(y, x):
        u1, u2 = x[0] + x[1], x[1]
        l1 = (-(a5 + 0.5 * u1) - half_log_2pi) - 0.5 * (((y[0] * y[0]) * a6) * e1(oracle.exp_t, -u1))
        l2 = (-(a5 + 0.5 * u2) - half_log_2pi) - 0.5 * (((y[1] * y[1]) * a6) * e1(oracle.exp_t, -u2))
        return l1 + l2
    return oracle.UserVectorModelFilter(n, seed, 2, 2, init, prop, logg, rep=rep, resampler=resampler, resamp_sched=sched, tile=tile)


def _lin_gauss_4d_oracle(oracle, n, seed, rep, resampler, tile, sched=1, th=(0.9, 0.5, 0.7, 0.4, 1.1, 0.25)):
    """tests/models/lin_gauss_4d_h.h (dim_x = dim_y = 4) restated with the oracle's own functions, in the header's operation order."""
    import math
    phi, sigma = th[0], th[1]
    e1 = lambda f, v: float(f(np.array([v]))[0])
    a2 = (((e1(oracle.log, th[2]) + e1(oracle.log, th[3])) + e1(oracle.log, th[4])) + e1(oracle.log, th[5])) + 4.0 * 0.91893853320467274178
    inv = [1.0 / th[2], 1.0 / th[3], 1.0 / th[4], 1.0 / th[5]]
    sd = sigma * (1.0 / math.sqrt(1.0 - phi * phi))
    init = lambda zn: np.array([zn[0] * sd, zn[1] * sd, zn[2] * sd, zn[3] * sd])
    prop = lambda x, zn, zcov: np.array([phi * x[0] + zn[0] * sigma, phi * x[1] + zn[1] * sigma, phi * x[2] + zn[2] * sigma, phi * x[3] + zn[3] * sigma])

    def logg(y, x):
        d0, d1, d2, d3 = (y[0] - x[0]) * inv[0], (y[1] - x[1]) * inv[1], (y[2] - x[2]) * inv[2], (y[3] - x[3]) * inv[3]
        return -a2 - 0.5 * (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3)
    return oracle.UserVectorModelFilter(n, seed, 4, 4, init, prop, logg, rep=rep, resampler=resampler, resamp_sched=sched, tile=tile)


def lin_gauss_4d_h_rows(oracle, x, z):
    """The sixteen functionals of lin_gauss_4d_h.h in the header's operation sequence; x: [4, N]."""
    rows = [x[0], x[1], x[2], x[3]] + [x[i] * x[j] for i in range(4) for j in range(i, 4)]
    rows.append(oracle.exp_t(0.5 * (((x[0] + x[1]) + x[2]) + x[3])))
    rows.append(np.full_like(x[0], z + 1.0))
    return np.stack(rows)
