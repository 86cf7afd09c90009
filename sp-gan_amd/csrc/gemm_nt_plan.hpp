// Which kernel spgan_gemm_nt runs for an argument block: ONE host-side decision (nt_plan) that the launch executes and every query
// (spgan_gemm_nt_kernel / _col_blocks / _owns_columns / _y16_ok / _uses_w_image, spgan_edge_attend_bwd_dt_selected) reads.
// The choice decides bits, not only speed: the kernels sum in different orders, a grouped launch is specified as bit-identical to its
// separate passes, and the fused dT route of edge_dt.hip is valid only where the chain's product would run gemm_wide.hip.
// Host only, plain C++17, no HIP header: a CPU program can compile it.  Nothing here reads through a pointer of the block.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include "spgan_hip.h"

// one value per launch target: the K <= 4 streaming kernel, the M <= 64 column-owning kernel and the 128-row MFMA family (gemm.hip:
// launch_nt_cfg); 256 x 256 tiles (gemm_wide.hip), their row-pipelined fp16 form (gemm_wide16.hip), split-bf16 256-row tiles (gemm_wide3.hip)
enum spgan_nt_kernel { NT_K4_STREAM = SPGAN_NT_KERNEL_K4_STREAM, NT_SMALL = SPGAN_NT_KERNEL_SMALL, NT_TILE = SPGAN_NT_KERNEL_TILE,
                       NT_WIDE = SPGAN_NT_KERNEL_WIDE, NT_WIDE16 = SPGAN_NT_KERNEL_WIDE16, NT_WIDE3 = SPGAN_NT_KERNEL_WIDE3 };

// internal operand modes (a_mode == SPGAN_A_AFFINE_LRELU with sp_val / A2 set): their own instantiations in gemm.hip
constexpr int NT_A_AFFINE_SPARSE = 3;
constexpr int NT_A_AFFINE2 = 4;

struct spgan_nt_plan {          // the ten ints in the order spgan_gemm_nt_plan() reports them
  int kernel = NT_TILE;         // spgan_nt_kernel
  int invalid = 0;              // tail.enabled with no column-owning kernel: the launch returns SPGAN_EINVAL
  // column-tile width.  NT_K4_STREAM and NT_SMALL have no column tiles of that kind: they report the width of the 128-row kernel that would
  // run otherwise (what spgan_gemm_nt_col_blocks has always answered for them)
  int tile_n = 0;
  int owns_columns = 0;         // one workgroup walks all rows of its columns (NT_SMALL): tail.enabled is acceptable
  int cfg = 0, db = 0, tile_fast = 0, operand = 0, store16 = 0;   // NT_TILE: launch_nt_cfg<.., CFG, DB, FAST, F16 (0 fp32 / 1 fp16 / 2 split-bf16), AH>
  int wide3_cfg = 0;            // NT_WIDE3: 24, 22 or 14 (spgan_nt_wide3_config)
  bool fast = false;            // K % 4 == 0 and every row / vector the operand mode reads 16-byte aligned
};
static_assert(offsetof(spgan_nt_plan, fast) == SPGAN_NT_PLAN_FIELDS * sizeof(int32_t), "spgan_gemm_nt_plan copies the leading ints");

inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// an environment switch set to 0 turns its kernel off (A/B measurements of whole programs)
inline bool nt_env_off(const char* name) { return getenv(name) && atoi(getenv(name)) == 0; }

// ------------------------------------------------------------------------------------------ K <= 4 streaming kernel
// which problems the streaming kernel takes (neither results nor layouts depend on it: bit-identical to the MFMA kernel)
inline bool nt_k4_ok(const spgan_gemm_nt_args& a) {
  constexpr int BM = 128;
  if (a.tile_hint == 1 || a.M <= 64 || a.batch > 1 || a.tail.enabled || a.pool_val || a.sp_val || a.A2 || a.a_half || a.y_bf16 || a.y_half) return false;
  if (a.K > 4 || a.a_mode != SPGAN_A_PLAIN || a.N % 4 || a.N < 8 || a.N > 512) return false;
  if (((a.N / 4) & (a.N / 4 - 1)) || a.ldy % 4 || !al16(a.Y)) return false;   // N / 4 a power of two
  if (a.stats) return false;   // column statistics stay with the MFMA epilogue: its reduction tree is part of the BatchNorm bits
  // per-group bias rows: only where the MFMA kernel would take its whole-tile path (bias + group row added first: same bits)
  if (a.rowbias && (a.rows_per_group <= 0 || a.rows_per_group % BM || a.M % BM || a.N % 64)) return false;
  if (a.epi_mode == SPGAN_EPI_MASK_OUT) return !a.bias && !a.rowbias && a.ld_ref % 4 == 0 && al16(a.ref);
  return a.epi_mode == SPGAN_EPI_LINEAR;
}

// ------------------------------------------------------------------------------------------ the 256-row-tile kernels
// what gemm_wide.hip, gemm_wide16.hip and gemm_wide3.hip ask alike: one unbatched product of whole 256-row tiles (per group too), aligned
// rows and prologue vectors, no per-edge mode, no two-tensor operand, no column tail, an epilogue their straight-line code has
inline bool nt_wide_common(const spgan_gemm_nt_args& a) {
  if (a.M < 256 || a.M % 256 || a.tail.enabled || a.batch > 1 || a.A2) return false;
  if (a.a_mode == SPGAN_A_EDGE || a.epi_mode == SPGAN_EPI_EDGE_BNBWD) return false;
  if (a.lda % 4 || a.ldw % 4 || !al16(a.A) || !al16(a.W)) return false;
  if (a.a_mode != SPGAN_A_PLAIN && (!al16(a.p_scale) || !al16(a.p_shift))) return false;
  if (a.p_group_rows > 0 && a.p_group_rows % 256) return false;
  if (a.sp_val && (a.a_mode != SPGAN_A_AFFINE_LRELU || a.sp_rows % 256 || !al16(a.sp_val) || !al16(a.sp_arg))) return false;
  if (a.epi_mode == SPGAN_EPI_LINEAR) {
    if (a.rowbias && a.rows_per_group != 1 && a.rows_per_group % 256) return false;
    if (!a.Y && !a.stats && !a.pool_val) return false;
  } else {
    if (a.epi_mode == SPGAN_EPI_MASK_OUT && (a.a_mode != SPGAN_A_PLAIN || a.bias || a.rowbias)) return false;
    if (a.epi_mode == SPGAN_EPI_BNBWD && a.rowbias && a.rows_per_group != 1) return false;
  }
  return true;
}
inline bool nt_slope01(const spgan_gemm_nt_args& a) { return a.a_mode == SPGAN_A_PLAIN || (a.p_slope >= 0.f && a.p_slope <= 1.f); }

// gemm_wide.hip: 256 x 256 tiles, K tiles of 32, fp32 or fp16 operands (not the split-bf16 mode); the sparse addend is an fp32-operand path
inline bool spgan_nt_wide_eligible(const spgan_gemm_nt_args& a) {  // the kernel can run this problem
  if (!nt_wide_common(a) || a.N % 256 || a.K % 32 || a.K < 32 || (a.mfma_f16 != 0 && a.mfma_f16 != 1) || (a.mfma_f16 == 1 && a.sp_val)) return false;
  if (a.epi_mode == SPGAN_EPI_ADAIN) return a.a_mode == SPGAN_A_PLAIN && a.mfma_f16 == 0 && !a.rowbias && !a.stats;   // fp32 operands only
  return true;
}

// 256 x 256 tiles of ONE group: a grouped launch (several passes of a layer as one product) must run the kernel its passes would run as
// separate calls -- the kernels sum in different orders, and the grouped form is specified as bit-identical
inline long nt_group_tiles256(const spgan_gemm_nt_args& a) { return (long)((a.p_group_rows > 0 ? a.p_group_rows : a.M) / 256) * (a.N / 256); }

// ... and is expected to be faster than the 128-row kernels (tile_hint 0).
// Measured inside the train step (tools/mfma_shapes.py, MI355X): one workgroup per CU means a launch whose tiles make a single round
// runs its load / MFMA / epilogue phases in lockstep on all CUs -- with a heavy epilogue (the BatchNorm-backward one reads and writes
// [M,N]) that costs what the leaner main loop gains (65536 x 256 x 256: 103 -> 107 us), and k-loops of two tiles are all ramp
// (K = 64: 40 -> 45 us).  Wins: 65536 x 1024 x 256 + statistics/pooling 327 -> 300 us, 65536 x 256 x 128: 57 -> 54, 65536 x 1280 x 128: 224 -> 214.
inline bool spgan_nt_wide_pays(const spgan_gemm_nt_args& a) {
  const long tiles = nt_group_tiles256(a);
  if (tiles < 256 || a.K < 128) return false;
  return a.epi_mode == SPGAN_EPI_LINEAR || a.epi_mode == SPGAN_EPI_ADAIN || tiles >= 512;   // (ADAIN: the kernel its plain style GEMM would run)
}

// gemm_wide16.hip: fp16 operands, row-pipelined, pairs of 32-wide k-tiles; 16-bit results from its LINEAR epilogue only.  256 x 256 tiles
// only: the 256 x 128 form (eight A slots per thread) spills and measured 2-3 x slower (profiles/r06_nt16_bench.txt)
inline bool spgan_nt_wide16_eligible(const spgan_gemm_nt_args& a) {
  if (!nt_wide_common(a) || !nt_slope01(a) || a.mfma_f16 != 1 || a.N % 256 || a.K % 64 || a.a_half || a.sp_val) return false;
  return a.epi_mode == SPGAN_EPI_LINEAR || !(a.y_bf16 || a.y_half);
}
// the tiles fill the chip, a k-loop worth its ramp
inline bool spgan_nt_wide16_pays(const spgan_gemm_nt_args& a) { return nt_group_tiles256(a) >= 256 && a.K >= 128; }

// gemm_wide3.hip: split-bf16 operands, 256 x 256 or 256 x 128 tiles, pairs of 16-wide k-tiles; the sparse addend on 256-wide tiles only; the
// stored tile gout_add + gout_scale * g on the activation operand's BatchNorm-backward epilogue only
inline bool spgan_nt_wide3_eligible(const spgan_gemm_nt_args& a) {
  if (!nt_wide_common(a) || !nt_slope01(a) || a.mfma_f16 != 2 || a.N % 128 || a.K % 32 || a.a_half || a.y_bf16 || a.y_half) return false;
  if (!al16(a.w_image) || (a.sp_val && a.N % 256)) return false;
  return !a.gout_add || (a.epi_mode == SPGAN_EPI_BNBWD && a.a_mode == SPGAN_A_AFFINE_LRELU && !a.sp_val);
}

// a workgroup per CU at least, and a k-loop worth its ramp (the 128-row split kernel serves the rest); tiles of ONE group, as in
// spgan_nt_wide3_config: a grouped launch must pick the kernel, and so the summation order, of its separate passes
inline bool spgan_nt_wide3_pays(const spgan_gemm_nt_args& a) {
  return (long)((a.p_group_rows > 0 ? a.p_group_rows : a.M) / 256) * (a.N / 128) >= 128 && a.K >= 64;
}

// Tile configuration (WGM*10 + WGN) of an eligible problem, from measurements on MI355X (tools/nt3_bench.py, profiles/r06_nt3_*):
//   N % 256 != 0 -> 256 x 128 tiles (22).  Short K (<= 128): two workgroups per CU pay (one's ramp and epilogue under the other's MFMAs; the k-loop
//   is 4-8 tiles long): 128 x 256 (14) with W's pre-split image, 256 x 128 (22) without (the B rows are then split in the workgroup, which a
//   128-row tile would do twice as often).  Longer K: 256 x 256 tiles (24) when they fill the chip at least once (decided from the rows of ONE
//   group, as spgan_nt_wide_pays does: a grouped launch runs the kernel its passes would run alone), else the two-workgroup forms.
//   The sparse addend keeps to (24) without image: its extra registers spill in the other forms.
inline int spgan_nt_wide3_config(const spgan_gemm_nt_args& a) {
  static const int force = getenv("SPGAN_NT3_CFG") ? atoi(getenv("SPGAN_NT3_CFG")) : 0;   // A/B measurements: 24 / 22 / 14
  if (a.N % 256) return 22;
  if (a.sp_val) return 24;
  if (force == 22 || force == 24 || (force == 14 && a.w_image)) return force;
  if (a.K <= 128 || nt_group_tiles256(a) < 256) return a.w_image ? 14 : 22;
  return 24;
}

// ------------------------------------------------------------------------------------------ the decision
inline spgan_nt_plan nt_plan(const spgan_gemm_nt_args& a) {
  // SPGAN_NT_WIDE=0 / SPGAN_NT_WIDE16=0 / SPGAN_NT_WIDE3=0 (read once per process) turn a 256-row-tile kernel off altogether
  static const bool wide_off = nt_env_off("SPGAN_NT_WIDE"), wide16_off = nt_env_off("SPGAN_NT_WIDE16"), wide3_off = nt_env_off("SPGAN_NT_WIDE3");
  const int epi = a.epi_mode;
  const int amode = a.a_mode != SPGAN_A_AFFINE_LRELU ? a.a_mode : (a.A2 ? NT_A_AFFINE2 : (a.sp_val ? NT_A_AFFINE_SPARSE : a.a_mode));
  const bool plain = amode == SPGAN_A_PLAIN, linear = epi == SPGAN_EPI_LINEAR;
  // tile_hint 1 -> 128-row kernels only, 2 -> a 256-row-tile kernel whenever eligible, 0 -> when eligible and expected to pay
  const auto wanted = [&a](bool off, bool eligible, bool pays) { return !off && a.tile_hint != 1 && eligible && (a.tile_hint == 2 || pays); };
  spgan_nt_plan p;
  p.fast = (a.K % 4 == 0) && (a.lda % 4 == 0) && (a.ldw % 4 == 0) && al16(a.A) && al16(a.W);
  if (!plain) p.fast = p.fast && al16(a.p_scale) && al16(a.p_shift);
  if (amode == SPGAN_A_EDGE) p.fast = p.fast && al16(a.e_bias);
  if (amode == NT_A_AFFINE_SPARSE) p.fast = p.fast && al16(a.sp_val) && al16(a.sp_arg);
  if (amode == NT_A_AFFINE2) p.fast = p.fast && al16(a.A2) && (a.lda2 % 4 == 0) && al16(a.p_scale2);

  // the 128-row family's form for this problem: what runs unless one of the other kernels takes it below
  const auto tile = [&p](int cfg, int db, int fast, int operand, int store16) {
    p.cfg = cfg; p.db = db; p.tile_fast = fast; p.operand = operand; p.store16 = store16;
    p.tile_n = 128 >> cfg;
  };
  const bool long_k = a.N > 64 && a.K >= 512;   // long K: 128x128 tiles, double-buffered LDS, one barrier per k-tile
  if (epi == SPGAN_EPI_ADAIN) {
    tile(0, 1, 1, 0, 0);   // the style GEMM's epilogue pairs column c with C + c: one form only (aligned fp32 operands, validated)
  } else if (a.a_half && ((amode == NT_A_AFFINE2 && epi == SPGAN_EPI_EDGE_BNBWD) || (plain && linear))) {
    // 16-bit stored operands (validated in spgan_gemm_nt: fp16 mode, aligned, N > 32, M > 64, one product): fp16 A of a plain linear
    // product, or bfloat16 g / fp16 y of the EdgeBlock's lazy BatchNorm-backward operand -- the 128-row kernels only
    long_k ? tile(0, 1, 1, 1, 1) : tile(1, 0, 1, 1, 1);
  } else if (amode != NT_A_AFFINE_SPARSE && a.mfma_f16 == 2 && p.fast && a.N > 32) {
    tile(1, 0, 1, 2, 0);   // fp32 operands split into three bf16 terms: 128x64 tiles (three operand planes in LDS)
  } else if (amode != NT_A_AFFINE_SPARSE && a.mfma_f16 == 1 && p.fast && a.N > 32) {
    long_k ? tile(0, 1, 1, 1, 0) : tile(1, 0, 1, 1, 0);   // fp16 operands (fp32 accumulate): same tiling rules
  } else if (long_k) {
    tile(0, 1, p.fast, 0, 0);
  } else if (a.N > 32) {
    // short K: 128x64 tiles.  With 2-8 k-tiles per workgroup the fixed load/epilogue latency dominates; the narrower tile
    // doubles the workgroups (2048 instead of 1024 at M=65536, N=256: finer quantisation over the 256 CUs, 5 resident per
    // CU instead of 3) -- measured 15-30 % faster than 128x128 on every N <= 1280, K <= 256 shape of the step.
    tile(1, 0, p.fast, 0, 0);
  } else {
    tile(2, 0, 0, 0, 0);
  }

  // the order of preference
  const auto take = [&p](spgan_nt_kernel k, int tile_n) {
    p.kernel = k; p.tile_n = tile_n; p.owns_columns = k == NT_SMALL;
    return p;
  };
  if (epi == SPGAN_EPI_ADAIN)   // chosen as for the plain product of the same sizes, whose k-order per output element both kernels share
    return wanted(wide_off, spgan_nt_wide_eligible(a), spgan_nt_wide_pays(a)) ? take(NT_WIDE, 256) : p;
  if (plain && (linear || epi == SPGAN_EPI_MASK_OUT) && nt_k4_ok(a)) return take(NT_K4_STREAM, p.tile_n);  // 3 coordinate columns in
  if (p.store16) return p;
  if (amode != SPGAN_A_EDGE && amode != NT_A_AFFINE2 && epi != SPGAN_EPI_EDGE_BNBWD) {   // large aligned products
    if (wanted(wide16_off, spgan_nt_wide16_eligible(a), spgan_nt_wide16_pays(a))) return take(NT_WIDE16, 256);   // preferred over gemm_wide.hip's fp16 form
    if (wanted(wide_off, spgan_nt_wide_eligible(a), spgan_nt_wide_pays(a))) return take(NT_WIDE, 256);
    if (wanted(wide3_off, spgan_nt_wide3_eligible(a), spgan_nt_wide3_pays(a))) {
      p.wide3_cfg = spgan_nt_wide3_config(a);
      return take(NT_WIDE3, p.wide3_cfg == 22 ? 128 : 256);
    }
  }
  if ((plain || amode == SPGAN_A_AFFINE_LRELU) && epi != SPGAN_EPI_EDGE_BNBWD && a.M <= 64 && p.fast && !a.sp_val && a.batch <= 1 && !a.pool_val)
    return take(NT_SMALL, p.tile_n);
  p.invalid = a.tail.enabled != 0;  // only the M <= 64 kernel finishes its columns in the launch
  return p;
}
