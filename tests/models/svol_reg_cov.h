// svol_reg_cov.h -- TEST MODEL for the covariate form of the extension point (ssme_amd/csrc/model_api.h: dim_cov, first, first_logw):
// what a class derived from pf::filters::BSFilterWC<nparts, 1, 1, 3, ...> would hold.  A stochastic-volatility model with a
// regression in BOTH equations, three covariates z = (z0, z1, z2) per step:
//     x_t = mu + phi (x_{t-1} - mu) + g z1 + sigma e_t,          y_t = b0 z0 + b2 z2 + exp(x_t / 2) v_t,
// theta = (phi, mu, sigma, b0, b2, g).  Every covariate enters with a coefficient of its own, so a swapped index shows.
// First step of its own: the proposal looks at y_1 and z_1 and is twice as wide as the stationary law,
//     q1: x_1 ~ N(mu + (y_1 - b0 z0) / 4, (2 s)^2),   mu1: x_1 ~ N(mu, s^2),   s = sigma / sqrt(1 - phi^2),
//     first_logw = log mu1(x_1) - log q1(x_1) = log 2 - d1^2 / 2 + d2^2 / 2,  d1 = (x_1 - mu) / s,  d2 = (x_1 - m) / (2 s).
// gsamp draws y from the observation equation; three functionals, the last one reads z2.
// svol_reg_cov_nofirst.h is the same model without first / first_logw (x_1 = s e, as a header without dim_cov).
// The numpy restatement, operation for operation, is tests/user_cov_ref.py.
#pragma once

struct ssme_user_model0 {
    static constexpr int n_theta = 6;
    static constexpr int dim_cov = 3;
    static constexpr int n_h = 3;
    static ssme::ModelConst derive(const double* th) {            // host only
        const double phi = th[0], mu = th[1], sigma = th[2];
        ssme::ModelConst c{};
        c.a0 = phi; c.a1 = mu;
        c.a2 = sigma / ssme::dsqrt(1.0 - phi * phi);
        c.a3 = sigma;
        c.a4 = th[3]; c.a5 = th[4]; c.a6 = th[5];
        c.bad = !(sigma > 0.0);
        return c;
    }
    static __device__ __forceinline__ double prop(const ssme::ModelConst& c, double x, double zn, const double* zcov, const ssme::ExpTabEntry*) {
        const double mean = (c.a1 + c.a0 * (x - c.a1)) + c.a6 * zcov[1];
        return mean + zn * c.a3;
    }
    static __device__ __forceinline__ double logg(const ssme::ModelConst& c, double y, double x, const double* zcov, const ssme::ExpTabEntry* etab) {
        const double r = (y - c.a4 * zcov[0]) - c.a5 * zcov[2];
        const double hl = 0.5 * x;
        const double e = ssme::dexp_scaled_t(-x, 0, etab);
        double v = (-hl - 0.91893853320467274178) - 0.5 * ((r * r) * e);
        if (hl < -745.1332191019412) v = -ssme::dinf();
        return v;
    }
    static __device__ __forceinline__ double gsamp(const ssme::ModelConst& c, double x, double zo, const double* zcov, const ssme::ExpTabEntry* etab) {
        const double m = c.a4 * zcov[0] + c.a5 * zcov[2];
        return m + ssme::dexp_scaled_t(0.5 * x, 0, etab) * zo;
    }
    static __device__ __forceinline__ void h(const ssme::ModelConst& c, const double* x, const double* zcov, const ssme::ExpTabEntry* etab, double* out) {
        out[0] = x[0];
        out[1] = ssme::dexp_scaled_t(0.5 * x[0], 0, etab);
        out[2] = x[0] + c.a5 * zcov[2];
    }
#ifndef SVOL_REG_COV_NO_FIRST
    static __device__ __forceinline__ void first(const ssme::ModelConst& c, const double* zn, const double* y, const double* zcov, double* x0,
                                                 const ssme::ExpTabEntry*) {
        const double m = c.a1 + 0.25 * (y[0] - c.a4 * zcov[0]);
        x0[0] = m + (2.0 * c.a2) * zn[0];
    }
    static __device__ __forceinline__ double first_logw(const ssme::ModelConst& c, const double* y, const double* x0, const double* zcov,
                                                        const ssme::ExpTabEntry*) {
        const double m = c.a1 + 0.25 * (y[0] - c.a4 * zcov[0]);
        const double d1 = (x0[0] - c.a1) / c.a2;
        const double d2 = (x0[0] - m) / (2.0 * c.a2);
        return (0.69314718055994530942 - 0.5 * (d1 * d1)) + 0.5 * (d2 * d2);
    }
#endif
};
