// svol_student_t_h.h -- TEST MODEL for the functionals of the extension point (ssme_amd/csrc/model_api.h: n_h, h) on a SCALAR state:
// the model of svol_student_t.h (its callbacks, unchanged, through the base class) with the four built-in functionals restated in
// user form,
//     h(x) = (x, x^2, exp(x / 2), 42),
// so that ssme_pf_get_user_expectations can be held against ssme_pf_get_expectations_multi of the same handle.
#pragma once
#define ssme_user_model0 svol_student_t_callbacks
#include "svol_student_t.h"
#undef ssme_user_model0

struct ssme_user_model0 : svol_student_t_callbacks {
    static constexpr int n_h = 4;
    static __device__ __forceinline__ void h(const ssme::ModelConst&, const double* x, double, const ssme::ExpTabEntry*, double* out) {
        out[0] = x[0];
        out[1] = x[0] * x[0];
        out[2] = ssme::dexp(0.5 * x[0]);
        out[3] = 42.0;
    }
};
