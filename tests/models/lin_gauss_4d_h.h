// lin_gauss_4d_h.h -- TEST MODEL at the documented maxima of the extension point (ssme_amd/csrc/model_api.h): dim_x = dim_y = 4 and
// n_h = 16.  Four independent AR(1) components with a common phi and sigma, each observed with its own noise,
//     x_d' = phi x_d + sigma e_d,      y_d = x_d + tau_d v_d  (d = 1 .. 4),      x_d(0) ~ N(0, sigma^2 / (1 - phi^2)),
// theta = (phi, sigma, tau_1, tau_2, tau_3, tau_4).  Linear and Gaussian: the exact log-likelihood is the sum of four scalar Kalman
// filters.  The sixteen functionals are the four means x_i, the ten second moments x_i x_j (i <= j, row by row), exp((x_1 + x_2 + x_3 +
// x_4) / 2) and z + 1 (the covariate reaches h).
#pragma once

struct ssme_user_model0 {
    static constexpr int n_theta = 6;
    static constexpr int dim_x = 4, dim_y = 4;
    static constexpr int n_h = 16;
    static ssme::ModelConst derive(const double* th) {            // host only
        ssme::ModelConst c{};
        c.a0 = th[0];
        c.a1 = th[1];
        c.a2 = (((ssme::dlog(th[2]) + ssme::dlog(th[3])) + ssme::dlog(th[4])) + ssme::dlog(th[5])) + 4.0 * 0.91893853320467274178;
        c.a3 = 1.0 / th[2];
        c.a4 = 1.0 / th[3];
        c.a5 = 1.0 / th[4];
        c.a6 = 1.0 / th[5];
        c.bad = !(th[2] > 0.0 && th[3] > 0.0 && th[4] > 0.0 && th[5] > 0.0);
        return c;
    }
    static __device__ __forceinline__ void init_vec(const ssme::ModelConst& c, const double* zn, double* x0) {
        const double sd = c.a1 * (1.0 / ssme::dsqrt(1.0 - c.a0 * c.a0));        // stationary sd; sqrt and division are correctly rounded
        x0[0] = zn[0] * sd;
        x0[1] = zn[1] * sd;
        x0[2] = zn[2] * sd;
        x0[3] = zn[3] * sd;
    }
    static __device__ __forceinline__ void prop_vec(const ssme::ModelConst& c, const double* x, const double* zn, double, double* xn,
                                                    const ssme::ExpTabEntry*) {
        xn[0] = c.a0 * x[0] + zn[0] * c.a1;
        xn[1] = c.a0 * x[1] + zn[1] * c.a1;
        xn[2] = c.a0 * x[2] + zn[2] * c.a1;
        xn[3] = c.a0 * x[3] + zn[3] * c.a1;
    }
    static __device__ __forceinline__ double logg_vec(const ssme::ModelConst& c, const double* y, const double* x, const ssme::ExpTabEntry*) {
        const double d0 = (y[0] - x[0]) * c.a3, d1 = (y[1] - x[1]) * c.a4, d2 = (y[2] - x[2]) * c.a5, d3 = (y[3] - x[3]) * c.a6;
        return -c.a2 - 0.5 * (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3);
    }
    static __device__ __forceinline__ void h(const ssme::ModelConst&, const double* x, double zcov, const ssme::ExpTabEntry* etab, double* out) {
        out[0] = x[0];
        out[1] = x[1];
        out[2] = x[2];
        out[3] = x[3];
        int k = 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j) out[k++] = x[i] * x[j];
        out[14] = ssme::dexp_scaled_t(0.5 * (((x[0] + x[1]) + x[2]) + x[3]), 0, etab);
        out[15] = zcov + 1.0;
    }
};
