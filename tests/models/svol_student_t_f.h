// svol_student_t_f.h -- TEST MODEL: svol_student_t.h plus the transition log-density of its own prop (ssme_amd/csrc/model_api.h: logf),
// so that its filters can be smoothed by backward simulation (ssme_pf_sample_trajectories_backward).  A scalar model without covariates:
//     x_t = phi x_{t-1} + sigma e_t      =>      log f(xn | x) = -((xn - phi x) / sigma)^2 / 2 + const.
// The operation order below is the specification; tests/backward_ref.py restates it.
#pragma once
#define ssme_user_model0 ssme_student_t_base
#include "svol_student_t.h"
#undef ssme_user_model0

struct ssme_user_model0 : ssme_student_t_base {
    static __device__ __forceinline__ double logf(const ssme::ModelConst& c, double xn, double x, double, const ssme::ExpTabEntry*) {
        const double d = (xn - c.a0 * x) / c.a1;
        return -0.5 * (d * d);
    }
};
