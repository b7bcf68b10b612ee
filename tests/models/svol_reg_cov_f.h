// svol_reg_cov_f.h -- TEST MODEL: svol_reg_cov.h (dim_cov = 3, a first step of its own) plus the transition log-density of its own prop
// (ssme_amd/csrc/model_api.h: logf with `const double* zcov`): the covariates of the step that made xn enter the mean,
//     x_t = mu + phi (x_{t-1} - mu) + g z1 + sigma e_t      =>      log f(xn | x, z) = -((xn - mean) / sigma)^2 / 2 + const.
// The operation order below is the specification; tests/backward_ref.py restates it.
#pragma once
#define ssme_user_model0 ssme_reg_cov_base
#include "svol_reg_cov.h"
#undef ssme_user_model0

struct ssme_user_model0 : ssme_reg_cov_base {
    static __device__ __forceinline__ double logf(const ssme::ModelConst& c, double xn, double x, const double* zcov, const ssme::ExpTabEntry*) {
        const double mean = (c.a1 + c.a0 * (x - c.a1)) + c.a6 * zcov[1];
        const double d = (xn - mean) / c.a3;
        return -0.5 * (d * d);
    }
};
