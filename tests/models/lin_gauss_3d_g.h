// lin_gauss_3d_g.h -- TEST MODEL for the observation draw of the extension point (ssme_amd/csrc/model_api.h: gsamp_vec) with an
// odd shape, dim_x = 3 and dim_y = 1: the model of lin_gauss_3d.h (its callbacks, unchanged, through the base class) with
//     y = ((x1 + x2) + x3) + tau' v,      tau' = exp(log(tau))
// formed from the constant the model has (a5 = log(tau)).  Three state normals and one observation normal per particle and horizon:
// the second Philox call of the forecast gives the third state normal, and three of the four observation normals are dropped.
#pragma once
#define ssme_user_model0 lin_gauss_3d_g_callbacks
#include "lin_gauss_3d.h"
#undef ssme_user_model0

struct ssme_user_model0 : lin_gauss_3d_g_callbacks {
    static __device__ __forceinline__ void gsamp_vec(const ssme::ModelConst& c, const double* x, const double* zo, double* y,
                                                     const ssme::ExpTabEntry* etab) {
        y[0] = ((x[0] + x[1]) + x[2]) + ssme::dexp_scaled_t(c.a5, 0, etab) * zo[0];
    }
};
