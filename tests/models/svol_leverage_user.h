// svol_leverage_user.h -- TEST MODEL for the observation draw of the extension point (ssme_amd/csrc/model_api.h: gsamp): the
// built-in leverage model (test/test_pswarm.cpp:64-116 of the reference) restated as a SCALAR user model,
//     x_t = mu + phi (x_{t-1} - mu) + rho sigma y_{t-1} exp(-x_{t-1} / 2) + sigma sqrt(1 - phi^2) e_t,      y_t = exp(x_t / 2) v_t,
// theta = (phi, mu, sigma, rho).  derive, prop and logg follow the built-in model's operation order (csrc/pf_api.hip: derive;
// csrc/pf_kernels.h: model_prop, model_logg), gsamp the built-in observation draw (csrc/forecast.h: model_gsamp), so that in ONE
// library an SSME_MODEL_USER0 handle and an SSME_MODEL_SVOL_LEVERAGE handle return the same bits: filter, start draw and forecast.
// An anchor without any tolerance for the user-model forecast kernels (tests/test_forecast_user_gpu.py).
#pragma once

struct ssme_user_model0 {
    static constexpr int n_theta = 4;
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
    static __device__ __forceinline__ double prop(const ssme::ModelConst& c, double x, double zn, double zcov, const ssme::ExpTabEntry* etab) {
        const double e = ssme::dexp_scaled_t(-0.5 * x, 0, etab);
        const double mean = (c.a1 + c.a0 * (x - c.a1)) + (c.a4 * zcov) * e;
        return mean + zn * c.a3;
    }
    static __device__ __forceinline__ double logg(const ssme::ModelConst&, double y, double x, const ssme::ExpTabEntry* etab) {
        const double hl = 0.0 + 0.5 * x;
        const double e = ssme::dexp_scaled_t(-x, 0, etab);
        const double q = (y * y) * 1.0;
        double v = (-hl - 0.91893853320467274178) - 0.5 * (q * e);
        if (hl < -745.1332191019412) v = -ssme::dinf();
        return v;
    }
    static __device__ __forceinline__ double gsamp(const ssme::ModelConst&, double x, double zo, const ssme::ExpTabEntry* etab) {
        const double e = ssme::dexp_scaled_t(0.5 * x, 0, etab);
        return e * zo;
    }
};
