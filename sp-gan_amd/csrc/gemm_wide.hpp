// The 256-row-tile gemm_nt kernels for large aligned products.  Which problems they run is decided in gemm_nt_plan.hpp (nt_plan), with their
// eligibility and pay rules; spgan_gemm_nt (gemm.hip) launches what the plan names.
#pragma once
#include "common.hpp"

constexpr int SPGAN_WIDE_A_SPARSE = 3;  // internal operand mode: A_AFFINE_LRELU with the sparse addend (sp_val != NULL)

int spgan_launch_nt_wide(const spgan_gemm_nt_args& a, hipStream_t s);     // gemm_wide.hip: 256 x 256 tiles, fp32 or fp16 operands
int spgan_launch_nt_wide16(const spgan_gemm_nt_args& a, hipStream_t s);   // gemm_wide16.hip: fp16 operands, row-pipelined 256 x 256 tiles
// gemm_wide3.hip: split-bf16 operands; config = the plan's waves (rows x columns, of 128 x 64 each) as WGM*10 + WGN: 24, 22 or 14
int spgan_launch_nt_wide3(const spgan_gemm_nt_args& a, int config, hipStream_t s);
