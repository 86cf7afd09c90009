// Split-bf16 weight gradients on large output tiles (gemm_tn_wide3.hip).  Which problems run here, in which tile configuration and on which
// split, is decided in gemm_tn_plan.hpp (tn_plan); launch_tn (gemm.hip) hands the plan's choice over.
#pragma once
#include "common.hpp"

int spgan_launch_tn_wide3(const spgan_gemm_tn_args& a, int cfg, int splits, int rows, hipStream_t s);   // cfg 24 / 22 / 14
