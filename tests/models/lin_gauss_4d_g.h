// lin_gauss_4d_g.h -- TEST MODEL for the observation draw of the extension point (ssme_amd/csrc/model_api.h: gsamp_vec) at the
// documented maxima, dim_x = dim_y = 4: the model of lin_gauss_4d_h.h (its callbacks and functionals, unchanged, through the base
// class) with
//     y_d = x_d + tau_d v_d  (d = 1 .. 4),      tau_d = 1 / a_{2+d}
// from the reciprocals the model keeps (division is correctly rounded, as the base model's init_vec already relies on; the four
// quotients do not depend on the horizon).  Linear and Gaussian: the forecast's moments are known exactly, which is what
// tests/test_forecast_user_gpu.py checks them against.
#pragma once
#define ssme_user_model0 lin_gauss_4d_g_callbacks
#include "lin_gauss_4d_h.h"
#undef ssme_user_model0

struct ssme_user_model0 : lin_gauss_4d_g_callbacks {
    static __device__ __forceinline__ void gsamp_vec(const ssme::ModelConst& c, const double* x, const double* zo, double* y,
                                                     const ssme::ExpTabEntry*) {
        y[0] = x[0] + (1.0 / c.a3) * zo[0];
        y[1] = x[1] + (1.0 / c.a4) * zo[1];
        y[2] = x[2] + (1.0 / c.a5) * zo[2];
        y[3] = x[3] + (1.0 / c.a6) * zo[3];
    }
};
