// svol_two_factor_cov.h -- TEST MODEL for the covariate grammar on a VECTOR state and observation (ssme_amd/csrc/model_api.h):
// (dim_x, dim_y, dim_cov) = (2, 2, 4), i.e. pf::filters::BSFilterWC<nparts, 2, 2, 4, ...>.  The two-factor model of
// svol_two_factor.h with a covariate in every equation, z = (z0, z1, z2, z3):
//     x1' = phi1 x1 + 0.3 z0 + sigma1 e1,      x2' = phi2 x2 - 0.2 z1 + sigma2 (rho e1 + sqrt(1 - rho^2) e2),
//     y1 = 0.5 z2 + beta exp((x1 + x2) / 2) v1,      y2 = -0.4 z3 + beta exp(x2 / 2) v2,
// theta = (beta, phi1, phi2, sigma1, sigma2, rho); the regression coefficients are constants of the header, all different.
// First step of its own: x_1 = (0.1 z0 + 1.5 sigma1 e1, 0.05 (y2 + 0.4 z3) + 1.5 sigma2' e2), sigma2' = sigma2 sqrt(1 - rho^2),
// against the prior N(0, sigma1^2) x N(0, sigma2'^2):
//     first_logw = 2 log 1.5 - (p1^2 + p2^2) / 2 + (q1^2 + q2^2) / 2,   p = x / sd,   q = (x - m) / (1.5 sd).
// gsamp_vec draws (y1, y2) from the observation equations; four functionals.  The numpy restatement is tests/user_cov_ref.py.
#pragma once

struct ssme_user_model0 {
    static constexpr int n_theta = 6;
    static constexpr int dim_x = 2, dim_y = 2, dim_cov = 4;
    static constexpr int n_h = 4;
    static ssme::ModelConst derive(const double* th) {            // host only
        const double beta = th[0], phi1 = th[1], phi2 = th[2], s1 = th[3], s2 = th[4], rho = th[5];
        ssme::ModelConst c{};
        c.a0 = phi1;
        c.a1 = phi2;
        c.a2 = s1;
        c.a3 = s2 * rho;
        c.a4 = s2 * ssme::dsqrt(1.0 - rho * rho);
        c.a5 = ssme::dlog(beta);
        c.a6 = beta;
        c.bad = !(beta > 0.0);
        return c;
    }
    static __device__ __forceinline__ void init_vec(const ssme::ModelConst& c, const double* zn, double* x0) {   // not reached: first is declared
        x0[0] = zn[0] * c.a2;
        x0[1] = zn[1] * c.a4;
    }
    static __device__ __forceinline__ void first(const ssme::ModelConst& c, const double* zn, const double* y, const double* zcov, double* x0,
                                                 const ssme::ExpTabEntry*) {
        x0[0] = 0.1 * zcov[0] + (1.5 * c.a2) * zn[0];
        x0[1] = 0.05 * (y[1] + 0.4 * zcov[3]) + (1.5 * c.a4) * zn[1];
    }
    static __device__ __forceinline__ double first_logw(const ssme::ModelConst& c, const double* y, const double* x0, const double* zcov,
                                                        const ssme::ExpTabEntry*) {
        const double p1 = x0[0] / c.a2, p2 = x0[1] / c.a4;
        const double q1 = (x0[0] - 0.1 * zcov[0]) / (1.5 * c.a2);
        const double q2 = (x0[1] - 0.05 * (y[1] + 0.4 * zcov[3])) / (1.5 * c.a4);
        return (0.81093021621632877 - 0.5 * (p1 * p1 + p2 * p2)) + 0.5 * (q1 * q1 + q2 * q2);
    }
    static __device__ __forceinline__ void prop_vec(const ssme::ModelConst& c, const double* x, const double* zn, const double* zcov, double* xn,
                                                    const ssme::ExpTabEntry*) {
        xn[0] = (c.a0 * x[0] + 0.3 * zcov[0]) + zn[0] * c.a2;
        xn[1] = ((c.a1 * x[1] - 0.2 * zcov[1]) + zn[0] * c.a3) + zn[1] * c.a4;
    }
    static __device__ __forceinline__ double logg_vec(const ssme::ModelConst& c, const double* y, const double* x, const double* zcov,
                                                      const ssme::ExpTabEntry* etab) {
        const double r1 = y[0] - 0.5 * zcov[2], r2 = y[1] + 0.4 * zcov[3];
        const double h1 = c.a5 + 0.5 * (x[0] + x[1]), h2 = c.a5 + 0.5 * x[1];
        const double l1 = (-h1 - 0.91893853320467274178) - 0.5 * ((r1 * r1) * ssme::dexp_scaled_t(-2.0 * h1, 0, etab));
        const double l2 = (-h2 - 0.91893853320467274178) - 0.5 * ((r2 * r2) * ssme::dexp_scaled_t(-2.0 * h2, 0, etab));
        return l1 + l2;
    }
    static __device__ __forceinline__ void gsamp_vec(const ssme::ModelConst& c, const double* x, const double* zo, const double* zcov, double* y,
                                                     const ssme::ExpTabEntry* etab) {
        y[0] = 0.5 * zcov[2] + (c.a6 * ssme::dexp_scaled_t(0.5 * (x[0] + x[1]), 0, etab)) * zo[0];
        y[1] = -0.4 * zcov[3] + (c.a6 * ssme::dexp_scaled_t(0.5 * x[1], 0, etab)) * zo[1];
    }
    static __device__ __forceinline__ void h(const ssme::ModelConst& c, const double* x, const double* zcov, const ssme::ExpTabEntry* etab, double* out) {
        out[0] = x[0];
        out[1] = x[1];
        out[2] = x[0] * x[1] + zcov[1];
        out[3] = c.a6 * ssme::dexp_scaled_t(0.5 * (x[0] + x[1]), 0, etab) + zcov[3];
    }
};
