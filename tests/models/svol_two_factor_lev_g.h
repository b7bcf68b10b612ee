// svol_two_factor_lev_g.h -- TEST MODEL that pins the covariate convention of a forecast for a VECTOR observation (ssme_amd/csrc/
// model_api.h: a simulated step's zcov is component 0 of the previous simulated observation): the model of svol_two_factor_g.h (its
// derive, init_vec, logg_vec and gsamp_vec, unchanged, through the base class) with a leverage term in the second factor,
//     x2' = phi2 x2 + sigma2 (rho e1 + sqrt(1 - rho^2) e2) - 0.05 z,
// z the covariate of the step: the caller's in a filter step, y1 of the previous horizon (last_obs at the first) in a forecast.  y1 and y2
// differ in every particle, so a kernel that handed prop_vec another component, or a stale one, changes the bits of every later x and y.
#pragma once
#define SVOL_TWO_FACTOR_G_AS_BASE
#include "svol_two_factor_g.h"

struct ssme_user_model0 : svol_two_factor_g_model {
    static __device__ __forceinline__ void prop_vec(const ssme::ModelConst& c, const double* x, const double* zn, double zcov, double* xn,
                                                    const ssme::ExpTabEntry*) {
        xn[0] = c.a0 * x[0] + zn[0] * c.a2;
        xn[1] = ((c.a1 * x[1] + zn[0] * c.a3) + zn[1] * c.a4) + (-0.05 * zcov);
    }
};
