// Which kernel spgan_gemm_tn runs for an argument block, on how many split partials: ONE host-side decision (tn_plan) that the launch
// executes and every query (spgan_gemm_tn_kernel / _plan / _splits(_lp) / _ws_bytes(_lp), spgan_gemm_tn_skinny_multi's acceptance) reads.
// The choice decides bits, not only speed: the kernels sum in different orders, and the split count fixes the order of the split sum and
// the size of the workspace the caller allocates.
// Host only, plain C++17, no HIP header: a CPU program can compile it.  Nothing here reads through a pointer of the block.
#pragma once
#include <cstddef>
#include <cstdint>
#include "spgan_hip.h"

// one value per kernel family: the streaming kernel for a side of <= 4 columns, the fp32 MFMA kernel and its bf16-operand form (gemm.hip:
// gemm_tn_skinny_kernel, gemm_tn_kernel, gemm_tn_lp_kernel), the split-bf16 kernel on large output tiles (gemm_tn_wide3.hip)
enum spgan_tn_kernel { TN_SKINNY = SPGAN_TN_KERNEL_SKINNY, TN_TILE = SPGAN_TN_KERNEL_TILE, TN_LP = SPGAN_TN_KERNEL_LP, TN_WIDE3 = SPGAN_TN_KERNEL_WIDE3 };

constexpr int TKM = 32;  // m-rows per staging step (= MFMA k-steps * 2 between two barriers)
constexpr int TA = 128;  // output rows (columns of A) per workgroup

struct spgan_tn_plan {     // the nine ints in the order spgan_gemm_tn_plan() reports them
  int kernel = TN_TILE;    // spgan_tn_kernel
  int invalid = 0;         // 16-bit stored operands that no kernel takes: the launch returns SPGAN_EINVAL
  int splits = 0, rows = 0;  // split partials [splits][Na][Nb] in ws, each over `rows` m-rows (tn_split)
  int tile_b = 0;          // TN_TILE / TN_LP: columns of B per workgroup, 128 / 64 / 32
  int fast = 0;            // Na, Nb and the leading dimensions multiples of 4, A, B (and A2) 16-byte aligned: vector loads
  int narrow_b = 0;        // TN_SKINNY: B is the side of <= 4 columns (else A)
  int wide3_cfg = 0;       // TN_WIDE3: 24, 22 or 14 (spgan_tn_wide3_config)
  int sparse_rows = 0;     // tn_sparse_rows_kernel follows (the sparse addend of A, after the split sum)
};
static_assert(offsetof(spgan_tn_plan, sparse_rows) == (SPGAN_TN_PLAN_FIELDS - 1) * sizeof(int32_t) &&
              sizeof(spgan_tn_plan) == SPGAN_TN_PLAN_FIELDS * sizeof(int32_t), "spgan_gemm_tn_plan copies the ints");

struct spgan_tn_split {
  int splits, rows;
};

inline int tn_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
inline bool tn_aligned(const void* q, unsigned bytes) { return (reinterpret_cast<uintptr_t>(q) & (bytes - 1)) == 0; }

inline int tn_tb(int Nb) { return Nb > 64 ? 128 : (Nb > 32 ? 64 : 32); }

// One side of the product has <= 4 columns (the weight gradients of the 3-channel layers: D's first conv, the generator's tail.4
// and pc inputs): nothing for the matrix cores to do -- gemm_tn_skinny_kernel streams the wide operand once.
inline bool tn_skinny(int Na, int Nb) { return (Na <= 4 || Nb <= 4) && Na <= 2048 && Nb <= 2048; }

// ------------------------------------------------------------------------------------------ the split-bf16 kernel
// Tile configuration (WGM*10 + WGN: output tile 128*WGM x 64*WGN) for an [Na, Nb] weight gradient, 0 when the shape is not this kernel's
inline int spgan_tn_wide3_config(int M, int Na, int Nb) {
  if (M < 64 || M % 32 || Na % 128 || Nb % 128) return 0;
  const int cfg = (Na % 256 == 0 ? 20 : 10) + (Nb % 256 == 0 ? 4 : 2);
  return cfg == 12 ? 0 : cfg;      // 128 x 128 tiles (two waves per workgroup): measured slower than the fp32 kernel (38 -> 47 us at 65536 x 128 x 128)
}

// The split of the split-bf16 kernel: one 512-thread workgroup per CU, two 256-thread ones, four 128-thread ones
inline spgan_tn_split tn_wide3_split(int M, int Na, int Nb, int cfg) {
  const int xm = (cfg / 10) * 128, xn = (cfg % 10) * 64, threads = xm * xn / 128;
  const int tiles = (Na / xm) * (Nb / xn);
  const int target = 256 * 512 / threads;
  int want = tn_cdiv(target, tiles);
  int r = tn_cdiv(M, want);
  if (r < 64) r = 64;
  r = tn_cdiv(r, 32) * 32;
  return {tn_cdiv(M, r), r};
}

// the kernel can run this problem (its shape apart: spgan_tn_wide3_config)
inline bool spgan_tn_wide3_eligible(const spgan_gemm_tn_args& a) {
  if (a.mfma_lp != 2 || !spgan_tn_wide3_config(a.M, a.Na, a.Nb)) return false;
  if (a.b_mode == SPGAN_A_EDGE || a.a_half || a.b_half) return false;
  // the two-tensor lazy A operand doubles the A quads in flight (8 more registers per quad on top of 128 accumulators): the kernel spills and
  // measured no faster (65536 x 256 x 256: 112 us) or slower (256 x 128: 212 us against 63) than the fp32 kernel -- it keeps that one
  if (a.A2) return false;
  if (!tn_aligned(a.A, 4) || !tn_aligned(a.B, 4)) return false;
  if (a.b_mode != SPGAN_A_PLAIN && !(a.p_slope >= 0.f && a.p_slope <= 1.f)) return false;
  if (a.a_lrelu && !(a.a_slope >= 0.f && a.a_slope <= 1.f)) return false;
  if ((double)a.M * a.lda >= 4294967296.0 || (double)a.M * a.ldb >= 4294967296.0) return false;
  return true;
}

// ------------------------------------------------------------------------------------------ the split
// THE split rule, from the shape and the operand mode alone (the caller sizes ws with it before it has a block).  The split-bf16 kernel
// (lp == 2) has larger output tiles, hence its own split on the shapes it takes; a problem of such a shape that it cannot run for alignment
// or operand reasons (spgan_tn_wide3_eligible) runs THAT split on the fp32 kernel.  No positive size: {0, 0}.
inline spgan_tn_split tn_split(int M, int Na, int Nb, int lp) {
  if (M <= 0 || Na <= 0 || Nb <= 0) return {0, 0};
  if (tn_skinny(Na, Nb)) {
    int r = tn_cdiv(tn_cdiv(M, 1024), TKM) * TKM;  // <= 1024 partials, each over a multiple of TKM rows (the MFMA kernel may have to serve the plan)
    if (r < 128) r = 128;
    return {tn_cdiv(M, r), r};
  }
  if (lp == 2)
    if (const int cfg = spgan_tn_wide3_config(M, Na, Nb)) return tn_wide3_split(M, Na, Nb, cfg);
  // about two workgroups per CU in total, at least 256 m-rows each
  const int tiles = tn_cdiv(Na, TA) * tn_cdiv(Nb, tn_tb(Nb));
  int want = tn_cdiv(512, tiles);
  int r = tn_cdiv(M, want);
  if (r < 64) r = 64;  // two staging steps: short reductions (M ~ 1000: the K x K products of the collapsed backward) are latency-bound, spread them
  r = tn_cdiv(r, TKM) * TKM;
  return {tn_cdiv(M, r), r};
}

// ------------------------------------------------------------------------------------------ the decision
inline spgan_tn_plan tn_plan(const spgan_gemm_tn_args& a) {
  spgan_tn_plan p;
  const spgan_tn_split sp = tn_split(a.M, a.Na, a.Nb, a.mfma_lp);
  p.splits = sp.splits; p.rows = sp.rows;
  p.fast = (a.Na % 4 == 0) && (a.Nb % 4 == 0) && (a.lda % 4 == 0) && (a.ldb % 4 == 0) && tn_aligned(a.A, 16) && tn_aligned(a.B, 16) &&
           (!a.A2 || (tn_aligned(a.A2, 16) && a.lda2 % 4 == 0));
  const bool skinny = tn_skinny(a.Na, a.Nb), plain = a.b_mode == SPGAN_A_PLAIN;
  p.sparse_rows = a.a_sp_val && a.b_mode != SPGAN_A_EDGE;
  if (!skinny && spgan_tn_wide3_eligible(a)) {   // split-bf16 operands: the fp32-equivalent product on the bf16 matrix pipe
    p.kernel = TN_WIDE3;
    p.wide3_cfg = spgan_tn_wide3_config(a.M, a.Na, a.Nb);
    return p;
  }
  // 16-bit stored operands run on the bf16 kernel only (aligned problems, no sparse addend); fp16-stored B is a plain operand, and the
  // streaming kernel reads neither (fp16 B on a skinny shape runs the bf16 kernel; 16-bit A has no kernel there)
  p.invalid = (a.b_half && (!plain || a.mfma_lp != 1 || a.a_sp_val)) || (a.a_half && (a.mfma_lp != 1 || a.a_sp_val || skinny)) ||
              ((a.b_half || a.a_half) && !p.fast);
  if (p.invalid) return p;
  // the streaming kernels: no prologues -- except the two-tensor A operand on the wide side (a lazy BatchNorm-backward tensor against 3 input columns)
  if (plain && skinny && !a.a_colsum_ws && !a.b_half && (!a.a_scale || (a.A2 && a.Nb <= 4 && !a.a_lrelu && !a.a_sp_val))) {
    p.kernel = TN_SKINNY;
    p.narrow_b = a.Nb <= 4;
    p.sparse_rows = 0;
    return p;
  }
  p.kernel = (p.fast && a.mfma_lp == 1) ? TN_LP : TN_TILE;  // bf16 operands: aligned problems only; others keep the fp32 kernel
  p.tile_b = tn_tb(a.Nb);
  return p;
}
