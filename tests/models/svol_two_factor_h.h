// svol_two_factor_h.h -- TEST MODEL for the functionals of the extension point (ssme_amd/csrc/model_api.h: n_h, h) on a VECTOR state:
// the model of svol_two_factor.h (its callbacks, unchanged, through the base class) with seven functionals of the whole state,
//     h(x, z) = (x1, x2, x1^2, x1 x2, x2^2, exp((x1 + x2) / 2), z + 1):
// the filtered mean, the three entries of the second-moment matrix, the volatility of the first series, and a constant that proves
// the covariate reaches h (its expectation is z + 1).
#pragma once
#define ssme_user_model0 svol_two_factor_callbacks
#include "svol_two_factor.h"
#undef ssme_user_model0

struct ssme_user_model0 : svol_two_factor_callbacks {
    static constexpr int n_h = 7;
    static __device__ __forceinline__ void h(const ssme::ModelConst&, const double* x, double zcov, const ssme::ExpTabEntry* etab, double* out) {
        out[0] = x[0];
        out[1] = x[1];
        out[2] = x[0] * x[0];
        out[3] = x[0] * x[1];
        out[4] = x[1] * x[1];
        out[5] = ssme::dexp_scaled_t(0.5 * (x[0] + x[1]), 0, etab);
        out[6] = zcov + 1.0;
    }
};
