// svol_two_factor_g.h -- TEST MODEL for the observation draw of the extension point (ssme_amd/csrc/model_api.h: gsamp_vec) on a
// VECTOR state and a VECTOR observation (dim_x = dim_y = 2): the model of svol_two_factor.h (its init_vec and prop_vec, unchanged,
// through the base class) with
//     y1 = (beta exp((x1 + x2) / 2)) v1,      y2 = (beta exp(x2 / 2)) v2.
// The draw needs beta itself and the base model fills all seven constants, so this header's derive frees one: a6 holds beta instead
// of 1 / beta^2, and logg_vec is restated with exp(-s) / beta^2 = exp(-2 (log(beta) + s / 2)) -- the same density.
#pragma once
#define ssme_user_model0 svol_two_factor_g_callbacks
#include "svol_two_factor.h"
#undef ssme_user_model0

struct svol_two_factor_g_model : svol_two_factor_g_callbacks {
    static ssme::ModelConst derive(const double* th) {            // host only
        ssme::ModelConst c = svol_two_factor_g_callbacks::derive(th);
        c.a6 = th[0];
        return c;
    }
    static __device__ __forceinline__ double logg_vec(const ssme::ModelConst& c, const double* y, const double* x, const ssme::ExpTabEntry* etab) {
        const double h1 = c.a5 + 0.5 * (x[0] + x[1]), h2 = c.a5 + 0.5 * x[1];
        const double l1 = (-h1 - 0.91893853320467274178) - 0.5 * ((y[0] * y[0]) * ssme::dexp_scaled_t(-2.0 * h1, 0, etab));
        const double l2 = (-h2 - 0.91893853320467274178) - 0.5 * ((y[1] * y[1]) * ssme::dexp_scaled_t(-2.0 * h2, 0, etab));
        return l1 + l2;
    }
    static __device__ __forceinline__ void gsamp_vec(const ssme::ModelConst& c, const double* x, const double* zo, double* y,
                                                     const ssme::ExpTabEntry* etab) {
        y[0] = (c.a6 * ssme::dexp_scaled_t(0.5 * (x[0] + x[1]), 0, etab)) * zo[0];
        y[1] = (c.a6 * ssme::dexp_scaled_t(0.5 * x[1], 0, etab)) * zo[1];
    }
};

// svol_two_factor_lev_g.h builds its own model on svol_two_factor_g_model
#ifndef SVOL_TWO_FACTOR_G_AS_BASE
struct ssme_user_model0 : svol_two_factor_g_model {};
#endif
