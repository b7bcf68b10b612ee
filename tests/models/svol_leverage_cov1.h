// svol_leverage_cov1.h -- TEST MODEL: tests/models/svol_leverage_user.h restated in the pointer form of the covariate grammar
// (ssme_amd/csrc/model_api.h: dim_cov = 1).  Same operations in the same order, the one covariate read as zcov[0]: a library built
// from this header must return the bits that svol_leverage_user.h's library returns -- the covariate grammar draws no other random
// numbers and changes no arithmetic (tests/test_user_cov_gpu.py).
#pragma once

struct ssme_user_model0 {
    static constexpr int n_theta = 4;
    static constexpr int dim_cov = 1;
    static ssme::ModelConst derive(const double* th) {            // host only
        const double phi = th[0], mu = th[1], sigma = th[2], rho = th[3];
        ssme::ModelConst c{};
        c.a0 = phi; c.a1 = mu;
        c.a2 = sigma / ssme::dsqrt(1.0 - phi * phi);
        c.a3 = sigma * ssme::dsqrt(1.0 - phi * phi);
        c.a4 = rho * sigma;
        c.bad = 0;
        return c;
    }
    static __device__ __forceinline__ double prop(const ssme::ModelConst& c, double x, double zn, const double* zcov, const ssme::ExpTabEntry* etab) {
        const double e = ssme::dexp_scaled_t(-0.5 * x, 0, etab);
        const double mean = (c.a1 + c.a0 * (x - c.a1)) + (c.a4 * zcov[0]) * e;
        return mean + zn * c.a3;
    }
    static __device__ __forceinline__ double logg(const ssme::ModelConst&, double y, double x, const double*, const ssme::ExpTabEntry* etab) {
        const double hl = 0.0 + 0.5 * x;
        const double e = ssme::dexp_scaled_t(-x, 0, etab);
        const double q = (y * y) * 1.0;
        double v = (-hl - 0.91893853320467274178) - 0.5 * (q * e);
        if (hl < -745.1332191019412) v = -ssme::dinf();
        return v;
    }
    static __device__ __forceinline__ double gsamp(const ssme::ModelConst&, double x, double zo, const double*, const ssme::ExpTabEntry* etab) {
        const double e = ssme::dexp_scaled_t(0.5 * x, 0, etab);
        return e * zo;
    }
};
