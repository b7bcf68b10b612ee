// svol_reg_cov_nofirst.h -- TEST MODEL: svol_reg_cov.h without a first step of its own (no first / first_logw): the first particle is
// x_1 = (sigma / sqrt(1 - phi^2)) e and its log-weight logg alone, as for a header without dim_cov.  The scalar oracle
// (oracle.UserModelFilter) reproduces it step by step.
#pragma once
#define SVOL_REG_COV_NO_FIRST
#include "svol_reg_cov.h"
