// svol_reg_cov_nodraw.h -- TEST MODEL: the state and observation equations of svol_reg_cov.h (dim_cov = 3) with nothing optional: no
// first step of its own, no functionals and NO observation draw.  It filters like svol_reg_cov_nofirst.h; a forecast of it is
// SSME_ERR_UNSUPPORTED (ssme_pf_sim_future_obs_cov needs gsamp), which is what tests/test_user_cov_gpu.py asks of it.
#pragma once

struct ssme_user_model0 {
    static constexpr int n_theta = 6;
    static constexpr int dim_cov = 3;
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
};
