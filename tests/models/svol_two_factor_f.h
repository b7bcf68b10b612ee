// svol_two_factor_f.h -- TEST MODEL: svol_two_factor.h ((dim_x, dim_y) = (2, 2)) plus the transition log-density of its own prop_vec
// (ssme_amd/csrc/model_api.h: logf_vec).  The innovations are recovered in the order prop_vec used them,
//     e1 = (xn1 - phi1 x1) / sigma1,      e2 = ((xn2 - phi2 x2) - sigma2 rho e1) / (sigma2 sqrt(1 - rho^2)),
// and log f = -(e1^2 + e2^2) / 2 + const.  The operation order below is the specification; tests/backward_ref.py restates it.
#pragma once
#define ssme_user_model0 ssme_two_factor_base
#include "svol_two_factor.h"
#undef ssme_user_model0

struct ssme_user_model0 : ssme_two_factor_base {
    static __device__ __forceinline__ double logf_vec(const ssme::ModelConst& c, const double* xn, const double* x, double,
                                                      const ssme::ExpTabEntry*) {
        const double e1 = (xn[0] - c.a0 * x[0]) / c.a2;
        const double e2 = ((xn[1] - c.a1 * x[1]) - c.a3 * e1) / c.a4;
        return -0.5 * (e1 * e1 + e2 * e2);
    }
};
