/*
 * spgan_hip.h -- C ABI of libspgan_hip.so: the MI355X (gfx950) kernels behind the SP-GAN
 * G+D train-step hot path.
 *
 * The reference (liruihui/SP-GAN) has no native plugin on its train path: Generator /
 * Discriminator bottom out in ATen ops.  The boundary below is therefore
 * new; it follows the calling convention of the reference's own extensions
 * (metrics/pointops/src/pointops_api.cpp:15-40, knnquery/knnquery_cuda.cpp:15-28: leading
 * integer sizes, then raw device pointers, outputs pre-allocated by the caller) with three
 * deliberate changes: every entry point takes the HIP stream explicitly, returns a status
 * (0 = ok, otherwise a hipError_t / negative argument-error code) instead of exit(-1)
 * (knnquery_cuda_kernel.cu:66-70), and never allocates, frees or synchronises.
 *
 * Layout conventions
 *   "pm"  point-major   float32 [M, C] row-major, M = B*N rows (one row per point)
 *   "cm"  channel-major float32 [B, C, N]  (the reference's nn.Module boundary layout)
 *   edge tensors        float32 [M*k, C]   row e = i*k + r  (point i, neighbour rank r)
 *   idx                 int32   [M, k]     GLOBAL row index (b*N + j) of the r-th neighbour
 *
 * Each function documents the reference lines whose arithmetic it carries.
 */
#ifndef SPGAN_HIP_H
#define SPGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* spgan_stream_t; /* hipStream_t */

#define SPGAN_OK 0
#define SPGAN_EINVAL (-22)
#define SPGAN_ECOMM (-70) /* collective layer: RCCL not loadable, or an RCCL call failed (spgan_comm_last_error) */

int spgan_version(void);
/* returns the compiled-for architecture string, e.g. "gfx950" */
const char* spgan_arch(void);

/* ------------------------------------------------------------------------------------------
 * Graph construction.  Generation/modules.py:683-725 (get_edge_features): pairwise distances
 * (695-699), full ascending sort and ranks 1..k (702-703), gather + concat (708-720).
 * ---------------------------------------------------------------------------------------- */

/* mode 0: d = (-2*<xi,xj> + |xi|^2) + |xj|^2 in fp32 (the reference's expanded form);
 * mode 1: d = sum_c (xi_c - xj_c)^2 in fp64 from the fp32 inputs (coordinate-space inputs, C<=8).
 * Writes the ranks 1..k of the ascending (distance, index) order of every row: rank 0 is dropped
 * positionally (modules.py:703), ties go to the lower index (stable sort).  k <= 32, k+1 <= N. */
int spgan_knn(const float* x_pm, int B, int N, int C, int k, int mode, int32_t* idx, spgan_stream_t s);

/* The same selection with a caller-provided scratch buffer (csrc/knn_pipe.hip): for 16 < C <= 64, k <= 10, mode 0 a pre-pass writes every
 * 32-row tile once as three bfloat16 planes + squared norms into `ws`, and the scan is software-pipelined over those images; identical
 * indices, ~0.6x the time.  spgan_knn_ws_bytes returns the scratch size that route needs (16-byte aligned buffer), or 0 when the shape
 * is served by spgan_knn's kernels -- spgan_knn_ws then forwards to spgan_knn and ignores ws. */
size_t spgan_knn_ws_bytes(int B, int N, int C, int k, int mode);
int spgan_knn_ws(const float* x_pm, int B, int N, int C, int k, int mode, int32_t* idx, void* ws, size_t ws_bytes, spgan_stream_t s);

/* In-edge lists of the kNN graph (for deterministic gather-style backward instead of float
 * atomics; replaces the atomicAdd scatter of metrics/pointops/src/grouping/grouping_cuda_kernel.cu:28-45).
 * rowptr [M+1], src [M*k]: src[rowptr[j] .. rowptr[j+1]) = ascending edge ids e with idx[e] == j. */
int spgan_csr_build(const int32_t* idx, int B, int N, int k, int32_t* rowptr, int32_t* src, spgan_stream_t s);

/* ee[B,2C,N,k] = cat[x_i, x_j - x_i] from channel-major x and int64 idx [B, N*k] holding LOCAL
 * indices (the reference's return_idx format, modules.py:704,723). */
int spgan_edge_features_cm(const float* x_cm, const int64_t* idx_local, int B, int C, int N, int k,
                           float* ee, spgan_stream_t s);

/* int32 global [M,k]  <->  int64 local [B, N*k] */
int spgan_idx_to_local64(const int32_t* idx, int B, int N, int k, int64_t* out, spgan_stream_t s);
int spgan_idx_from_local64(const int64_t* idx_local, int B, int N, int k, int32_t* out, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Layout helpers
 * ---------------------------------------------------------------------------------------- */
int spgan_cm_to_pm(const float* x_cm, int B, int C, int N, float* y_pm, spgan_stream_t s);
int spgan_pm_to_cm(const float* x_pm, int B, int C, int N, float* y_cm, spgan_stream_t s);
/* out[m, 0:Ca] = a[m,:], out[m, Ca:Ca+Cb] = b[m,:]   (torch.cat([x,z],-1), Generator.py:166) */
int spgan_concat2(const float* a, int Ca, const float* b, int Cb, int M, float* out, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Shared-MLP contractions on the matrix cores (fp32-in / fp32-accumulate MFMA, exact f32).
 * Every 1x1 Conv1d/Conv2d/Linear of Generator.py:56-71,107-136 and Discriminator.py:55-95,
 * their input-gradients, and (spgan_gemm_tn) their weight-gradients.
 * ---------------------------------------------------------------------------------------- */

enum { SPGAN_A_PLAIN = 0, SPGAN_A_AFFINE_LRELU = 1, SPGAN_A_EDGE = 2 };
enum { SPGAN_EPI_LINEAR = 0, SPGAN_EPI_MASK_OUT = 1, SPGAN_EPI_BNBWD = 2, SPGAN_EPI_EDGE_BNBWD = 3, SPGAN_EPI_ADAIN = 4 };
enum { SPGAN_ACT_NONE = 0, SPGAN_ACT_LRELU = 1, SPGAN_ACT_TANH = 2 };

/* Column tail of the M <= 64 product kernel (the per-shape linears: one workgroup owns its columns entirely, so what would be a
 * follow-up spgan_colstats_finalize* launch is finished in the producing launch):
 *   mode 0: the column records are (sum, centred M2) -> out0 = mean, out1 = biased variance (either may be NULL) and, when
 *           scale != NULL, the train-mode BatchNorm bookkeeping of spgan_bn_prepare (scale, shift, invstd, mean_out; running
 *           statistics updated with momentum when rmean != NULL; count_rep multiplies the row count of the unbiased-variance factor);
 *   mode 1: plain sums -> out0 = sum of x, out1 = sum of y.
 * enabled = 0: off.  Only accepted with M <= 64.  (Round 2 carried a generalisation to many row tiles -- last-arriving workgroup
 * merges -- that measured slower than the finalize launch on every shape of the step; it lives in tools/exp/fanin.hpp now.) */
typedef struct spgan_coltail {
  int enabled;
  int mode;
  float* out0; float* out1;
  const float* gamma; const float* beta; float* rmean; float* rvar;
  float* scale; float* shift; float* invstd; float* mean_out;
  float eps, momentum;
  int count_rep;
} spgan_coltail;

typedef struct spgan_gemm_nt_args {
  /* Y[M,N] = epilogue( prologue(A)[M,K] . W[N,K]^T ) */
  const float* A; int lda;
  const float* W; int ldw;
  float* Y; int ldy;
  int M, N, K;
  int a_mode;                 /* SPGAN_A_* */
  /* A_AFFINE_LRELU: a = lrelu(A[m,k]*p_scale[k] + p_shift[k], p_slope)   (BatchNorm apply + LeakyReLU
   *                 of the previous layer fused into the operand load)
   * A_EDGE:         row e=(i,r): a = lrelu((A[idx[e],k] - A[i,k] + e_bias[k])*p_scale[k] + p_shift[k], p_slope)
   *                 (conv_w.0 of EdgeBlock restructured per point, Generator.py:57-59,78) */
  const float* p_scale; const float* p_shift; float p_slope;
  const int32_t* e_idx; int e_k; const float* e_bias;
  int epi_mode;               /* SPGAN_EPI_* */
  /* EPI_LINEAR: y = act(acc + bias[n] + rowbias[m / rows_per_group, n]); optional column statistics */
  const float* bias; const float* rowbias; int rows_per_group; int ld_rowbias;
  int act; float act_slope;
  float* stats;               /* NULL or partials [ceil(M/128), N, 2]: (sum, centred M2) per 128-row tile (pre-activation) */
  /* EPI_MASK_OUT:   y = acc * (ref[m,n] > 0 ? 1 : slope)                 (LeakyReLU backward from its output)
   * EPI_BNBWD:      z = ref*b_scale[n]+b_shift[n]; g = (acc + bias[n] + rowbias[m / rows_per_group, n])*(z>0?1:slope)
   *                 (bias / rowbias optional); xhat=(ref-b_mean[n])*b_invstd[n];
   *                 y = g; stats partials [tilesM, N, 2] = (sum g, sum g*xhat)   (plain sums)
   * EPI_EDGE_BNBWD: same with ref[e,n] := (P[idx[e],n] - P[i,n] + e_bias2[n])  (P = ref, ld_ref) */
  const float* ref; int ld_ref;
  const float* b_scale; const float* b_shift; const float* b_mean; const float* b_invstd; float b_slope;
  const float* e_bias2;
  /* Optional sparse addend of the A operand (A_AFFINE_LRELU only): a += sp_val[b,k] where sp_arg[b,k] == m, b = m / sp_rows.
   * With p_slope = 1 this expresses the BatchNorm backward behind a global max-pool without materialising it:
   *   dy[m,k] = alpha[k]*y[m,k] + beta[k] + (argmax[b,k]==m ? coef[k]*gval[b,k] : 0)   (Discriminator.py:77-81,104) */
  const float* sp_val; const int32_t* sp_arg; int sp_rows;
  /* Optional pooling partials (EPI_LINEAR, M > 64): per 128-row tile and column the max and min of the pre-activation output
   * and their rows (first row on ties): pool_val / pool_arg [ceil(M/128), N, 2] = (max, min) / (arg-max row, arg-min row).
   * With them Y may be NULL (the output is not stored): adaptive_max_pool1d behind BatchNorm + LeakyReLU
   * (Discriminator.py:77-81,104) is finished by spgan_pool_finalize once the batch statistics are known. */
  float* pool_val; int32_t* pool_arg;
  /* 1: round the operands to fp16 when staging them (after the prologue) and multiply with the fp16 MFMA, fp32 accumulation
   * (BASELINE configs[4] "fp16 MFMA MLPs"); aligned operands and N > 32 only, otherwise the fp32 path is used.  Default 0.
   * 2: split every fp32 operand value exactly into three bfloat16 terms and evaluate the six leading cross products on the bf16 matrix
   * pipe with fp32 accumulation: fp32-equivalent products (dropped terms <= 3*2^-24 relative) at 6/16 of the fp32-MFMA time. */
  int mfma_f16;
  /* batch > 1 (A_PLAIN + EPI_LINEAR without stats / rowbias / pooling only): `batch` independent products in one launch,
   * product z uses A + z*batch_stride_a, W + z*batch_stride_w, Y + z*batch_stride_y (strides in floats; bias is shared).
   * The per-shape [N,N] contractions of the --attn variant (Generation/modules.py:554-556).  Default 0 / 1: a single product. */
  int batch; long batch_stride_a, batch_stride_w, batch_stride_y;
  /* tail.enabled (needs `stats`, M <= 64): the column records are finished in this launch, see spgan_coltail */
  spgan_coltail tail;
  /* Tile geometry.  0: automatic -- 256 x 256 tiles (csrc/gemm_wide.hip) for large aligned products whose tiles fill the chip, the
   * 128-row kernels otherwise; 1: 128-row kernels only; 2: 256 x 256 tiles whenever the problem is eligible (M % 256 == 0,
   * N % 256 == 0, K % 32 == 0, 16-byte aligned rows, fp32 operands, no per-edge mode / batching): for tests and A/B runs. */
  int tile_hint;
  /* p_group_rows > 0: the rows form M / p_group_rows groups of p_group_rows consecutive rows, and p_scale / p_shift hold one vector per
   * group ([groups, K], row g for the rows of group g) -- several passes of a network with their own train-mode BatchNorm statistics
   * evaluated as ONE product (D(real), D(fake) and D(x_hat) of a D step).  A multiple of 128 (of 256 for the 256 x 256-tile kernel),
   * M a multiple of it, M > 64.  0: one vector for all rows.  Also accepted without a prologue (a_mode PLAIN): then it only tells the
   * automatic tile-size rule (tile_hint 0) to decide from the rows of ONE group, so that a grouped launch runs the kernel its groups
   * would run as separate calls (bit-identical results). */
  int p_group_rows;
  /* A2 != NULL (with a_mode = SPGAN_A_AFFINE_LRELU, no sparse addend): the operand is a = A*p_scale[k] + A2*p_scale2[k] + p_shift[k]
   * -- two tensors of the same shape [M,K] (leading dimensions lda, lda2), no activation (p_slope is ignored): the BatchNorm-backward
   * tensor dy = p*g + q*y + r (spgan_bn_bwd_coeffs) evaluated on the operand load of its consumers instead of by a pass of its own.
   * Epilogues LINEAR / BNBWD / EDGE_BNBWD; M > 64; 128-row kernels only. */
  const float* A2; int lda2; const float* p_scale2;
  /* 16-bit operand / result storage, "f16" operand mode (mfma_f16 == 1) only:
   * a_half = 1: A points at IEEE fp16 values (lda in elements; a_mode PLAIN): staged into LDS as they are (128-row kernels);
   * y_bf16 = 1: Y points at bfloat16 storage (ldy in elements; LINEAR epilogue of the 256 x 256-tile kernel: spgan_gemm_nt_y16_ok()). */
  int a_half, y_bf16;
  /* y_half = 1: Y points at IEEE fp16 storage (ldy in elements; same kernels and conditions as y_bf16; also the edge operand mode: the
   * EdgeBlock's h2pre, a pre-BatchNorm activation whose statistics are still taken from the fp32 accumulators).
   * a_half = 1 together with A2 (epi_mode EDGE_BNBWD): A points at bfloat16 values (g2 of spgan_edge_attend_bwd_b), A2 at fp16 values
   * (h2pre): the EdgeBlock's lazy BatchNorm-backward operand p*A + q*A2 + r with both tensors in 16-bit storage. */
  int y_half;
  /* w_image != NULL (mfma_f16 == 2 only): the split-bf16 image of W written by spgan_split_bf16x3_image (same N, K): the 256-row-tile kernel
   * copies W's three bf16 planes from it instead of splitting the fp32 rows of W again in every workgroup (weights: split once per optimiser
   * step).  Kernels that do not use it ignore it; W must still be given. */
  const void* w_image;
  /* gout_add != NULL (epi_mode BNBWD, a_mode AFFINE_LRELU, mfma_f16 == 2 on a problem its 256-row-tile kernel takes; SPGAN_EINVAL otherwise):
   * the stored tile is gout_add[m, :] + gout_scale[:] * g[m, :] (the statistics stay those of g), as spgan_gemm_dual_args.gout_add: phase B of
   * the double backward hands X = xbarA + gamma*g to the next BatchNorm backward. */
  const float* gout_add; int ld_gout_add; const float* gout_scale;
  /* EPI_ADAIN (a_mode PLAIN, fp32 operands, N = 2C with C % 32 == 0, W = the style layer's [2C, K] weight = [gamma rows | beta rows],
   * bias [2C] or NULL; aligned operands: K, lda, ldw multiples of 4, A and W 16-byte aligned): AdaptivePointNorm applied in the epilogue,
   *   gamma = acc[m, c] + bias[c];  beta = acc[m, C + c] + bias[C + c];  b = m / ad_rows
   *   xhat = (lrelu(x[b, m - b*ad_rows, c], ad_slope) - ad_mean[b, c]) * rsqrtf(ad_var[b, c] + ad_eps);  Y[m, c] = fmaf(gamma, xhat, beta)
   * Y is [M, C] (ldy >= C); [M, 2C] is never stored.  x: row stride ad_ldx, shape b starts at ad_x + b * ad_x_shape_stride (0: every shape
   * reads the same [ad_rows, C] block); M % ad_rows == 0; ad_mean / ad_var [M / ad_rows, C].
   * ad_gamma != NULL: gamma alone is stored for the rows m >= ad_gamma_row0, ad_gamma[(m - ad_gamma_row0) * ad_ld_gamma + c].
   * pool_val / pool_arg != NULL (ad_rows % 128 == 0): per 128-row tile (max, min) / (arg-max, arg-min) records [M/128, C, 2] of Y, in the
   * format of the LINEAR epilogue's records (first row on ties), for spgan_pool_finalize*. */
  const float* ad_x; int ad_ldx; long ad_x_shape_stride; int ad_rows;
  const float* ad_mean; const float* ad_var; float ad_eps, ad_slope;
  float* ad_gamma; int ad_ld_gamma, ad_gamma_row0;
} spgan_gemm_nt_args;
/* The kernel spgan_gemm_nt runs for this problem (0: a == NULL): the one decision (csrc/gemm_nt_plan.hpp) the launch executes and the
 * queries below read.  None of them reads through a pointer of the block; all honour tile_hint and the SPGAN_NT_* environment switches. */
enum { SPGAN_NT_KERNEL_K4_STREAM = 1, SPGAN_NT_KERNEL_SMALL = 2, SPGAN_NT_KERNEL_TILE = 3, SPGAN_NT_KERNEL_WIDE = 4, SPGAN_NT_KERNEL_WIDE16 = 5,
       SPGAN_NT_KERNEL_WIDE3 = 6 };
int spgan_gemm_nt_kernel(const spgan_gemm_nt_args* a);
/* The whole plan as integers, for tests and tools: out[0..9] = kernel, invalid (tail.enabled with no column-owning kernel: the launch returns
 * SPGAN_EINVAL), tile_n, owns_columns, the 128-row family's CFG, DB, FAST, operand form (0 fp32 / 1 fp16 / 2 split-bf16) and 16-bit-storage
 * flag (meaningful for SPGAN_NT_KERNEL_TILE), the split-bf16 256-row-tile configuration 24 / 22 / 14 (SPGAN_NT_KERNEL_WIDE3, else 0). */
#define SPGAN_NT_PLAN_FIELDS 10
int spgan_gemm_nt_plan(const spgan_gemm_nt_args* a, int32_t* out);
/* 1 when spgan_gemm_nt will honour y_bf16 for this problem (it runs on the 256 x 256-tile kernel with fp16 operands) */
int spgan_gemm_nt_y16_ok(const spgan_gemm_nt_args* a);
/* 1 when spgan_gemm_nt will run this problem on the M <= 64 kernel, i.e. when `tail.enabled` is acceptable (else the launch
 * returns SPGAN_EINVAL for a tail request) */
int spgan_gemm_nt_owns_columns(const spgan_gemm_nt_args* a);
/* number of column blocks (N-tiles) spgan_gemm_nt uses for this problem */
int spgan_gemm_nt_col_blocks(const spgan_gemm_nt_args* a);

int spgan_gemm_nt(const spgan_gemm_nt_args* a, spgan_stream_t s);
/* Split-bf16 image of a row-major fp32 matrix W [N,K] (N % 128 == 0, K % 16 == 0): every value as three bfloat16 terms hi + mid + lo (exact:
 * round to nearest at each level, each residual representable), laid out as the LDS tiles of the split-bf16 gemm_nt read them:
 * image[k / 16][plane][n][16 bf16], the two 16-byte halves of a row swapped where bit 3 of n is set, rows whose 32-row tile index is odd (bit 5 of
 * n) negated (the kernel's sign checkerboard, csrc/gemm_wide3.hip).  spgan_split_bf16x3_image_bytes: 6*N*K. */
size_t spgan_split_bf16x3_image_bytes(int N, int K);
int spgan_split_bf16x3_image(const float* W, int ldw, int N, int K, void* image, spgan_stream_t s);
/* 1 when spgan_gemm_nt would read a w_image for this problem (worth making one) */
int spgan_gemm_nt_uses_w_image(const spgan_gemm_nt_args* a);
/* pooled[b,c] = max_n lrelu(scale[c]*y[b*rows+n, c] + shift[c], slope) from the tile partials above (rows % 128 == 0, so
 * that no tile straddles two shapes): scale >= 0 takes the tile maxima, scale < 0 the minima.  argmax = global row,
 * yarg = the pre-BatchNorm value there.  Ties go to the lowest row of equal PRE-activation values; scale == 0 (all rows tie):
 * argmax = the first row like torch.max, yarg = the column maximum (y at the first row is not in the records:
 * spgan_pool_zero_scale_yarg below puts it there). */
int spgan_pool_finalize(const float* pool_val, const int32_t* pool_arg, int B, int rows, int C, const float* scale, const float* shift,
                        float slope, float* pooled, int32_t* argmax, float* yarg, spgan_stream_t s);
/* The same for B = groups * shapes_per_group shapes that belong to `groups` passes with their own BatchNorm: scale / shift are
 * [groups, group_stride >= C] (vector g for the shapes of group g).  relative_rows != 0: argmax counts rows from the first row of the
 * shape's own group (what a per-group view of the batched tensors needs). */
int spgan_pool_finalize_groups(const float* pool_val, const int32_t* pool_arg, int B, int rows, int C, const float* scale, const float* shift,
                               int group_stride, int shapes_per_group, float slope, float* pooled, int32_t* argmax, float* yarg,
                               int relative_rows, spgan_stream_t s);
/* Behind either of the two: yarg[b,c] = y[b*rows, c] = prologue(A[b*rows]) . W[c] + bias[c] for every column whose scale is exactly 0 (the
 * row argmax names there), formed from the GEMM's own operands in fp32 -- the value of Y at that row up to the summation order, exactly it
 * where the products are exact.  Other columns are left alone.  A [B*rows, K], W [N, K]; p_scale / p_shift / p_slope / p_group_rows as in
 * spgan_gemm_nt_args (NULL: plain operand); scale [C] (shapes_per_group == 0) or [groups, group_stride] as in spgan_pool_finalize_groups. */
int spgan_pool_zero_scale_yarg(const float* A, int lda, const float* W, int ldw, const float* bias, const float* p_scale, const float* p_shift,
                               float p_slope, int p_group_rows, int B, int rows, int N, int K, const float* scale, int group_stride,
                               int shapes_per_group, float* yarg, spgan_stream_t s);

typedef struct spgan_gemm_tn_args {
  /* C[Na,Nb] = beta*C + sum_m A[m,Na]^T . prologue(B)[m,Nb]  -- weight gradients (reduction over points/edges).
   * Deterministic split over M: partial tiles go to `ws` and are summed in a fixed order. */
  const float* A; int lda;
  const float* B; int ldb;
  float* C; int ldc;
  int M, Na, Nb;
  int b_mode;                 /* SPGAN_A_* applied to B (per column of B) */
  const float* p_scale; const float* p_shift; float p_slope;
  const int32_t* e_idx; int e_k; const float* e_bias;
  float beta;
  float* ws; size_t ws_bytes; /* >= spgan_gemm_tn_ws_bytes_lp(M,Na,Nb,mfma_lp) */
  /* Optional prologue on A (per column of A): a = A*a_scale[c] + a_shift[c] + (a_sp_arg[b,c]==m ? a_sp_val[b,c] : 0), b = m / a_sp_rows.
   * a_scale == NULL: A is used as is. */
  const float* a_scale; const float* a_shift; const float* a_sp_val; const int32_t* a_sp_arg; int a_sp_rows;
  /* 1: only write the split partials into ws; the caller finishes C = beta*C + sum(partials) later with
   * spgan_splitk_reduce_multi (one launch for all the weight gradients of a backward pass).  Not with a_sp_val.  Default 0. */
  int defer_reduce;
  /* 1: both operands are rounded to bfloat16 (after the fp32 prologues) when they are staged into LDS and multiplied on the bf16
   * matrix pipe, fp32 accumulation / partials / reduction (BASELINE configs[4]; bf16 rather than fp16: per-point gradients of
   * magnitude 1e-8 must not flush).  Honoured for 16-byte aligned operands with Na, Nb, lda, ldb multiples of 4 outside the
   * skinny (Na or Nb <= 4) path; ignored otherwise.  Default 0: exact fp32 products.
   * 2: every fp32 operand value split exactly into three bfloat16 terms, the six leading cross products on the bf16 matrix pipe, fp32
   * accumulation -- fp32-equivalent products (dropped terms <= 2^-26 relative), as spgan_gemm_nt_args.mfma_f16 == 2.  Honoured where the output
   * tiles as 256 x 256, 256 x 128 or 128 x 256 (Na, Nb multiples of 128, not both odd multiples), M % 32 == 0, fp32-stored operands, b_mode PLAIN /
   * AFFINE_LRELU with slopes in [0, 1]: csrc/gemm_tn_wide3.hip, with its own split (spgan_gemm_tn_splits_lp / _ws_bytes_lp below, from the
   * shape alone); a problem of such a shape that the kernel cannot run (spgan_gemm_tn_kernel tells) runs the exact fp32 kernel on that split. */
  int mfma_lp;
  /* A2 != NULL (needs a_scale, a_shift; not with a_sp_val): a = A*a_scale[c] + A2*a_scale2[c] + a_shift[c] -- the same two-tensor
   * operand as spgan_gemm_nt_args.A2, on the A side of the weight-gradient product. */
  const float* A2; int lda2; const float* a_scale2;
  /* != NULL: also write the column sums of the (transformed) A operand over the rows of every split: a_colsum_ws [splits, Na]
   * (splits = spgan_gemm_tn_splits_lp(M, Na, Nb, mfma_lp)); their fixed-order sum over the splits -- e.g. one more entry (Na = 1, Nb = Na) of
   * spgan_splitk_reduce_multi -- is colsum(A): the bias gradient that belongs to this weight gradient, without a pass of its own.
   * Not with a_sp_val.  The streaming kernel has no such by-product: a block that carries a_colsum_ws never runs it, so ask
   * spgan_gemm_tn_kernel BEFORE attaching it and attach it only where the answer is not SPGAN_TN_KERNEL_SKINNY. */
  float* a_colsum_ws;
  /* a_lrelu = 1 (needs a_scale, a_shift; not with A2 / a_sp_val): the A-side prologue is a = lrelu(A*a_scale[c] + a_shift[c], a_slope)
   * -- a BatchNorm + LeakyReLU'd activation as the A operand without materialising it (the Gram matrix a^T a of the collapsed
   * backward takes the same pre-activation tensor on both sides).  0: the affine map alone. */
  int a_lrelu; float a_slope;
  /* b_half = 1 (with mfma_lp == 1, b_mode PLAIN): B points at IEEE fp16 values (ldb in elements). */
  int b_half;
  /* a_half = 1 (with mfma_lp == 1): A points at bfloat16 values, A2 (when given) at IEEE fp16 values (lda / lda2 in elements). */
  int a_half;
} spgan_gemm_tn_args;

/* Coefficient vectors of the BatchNorm backward as an affine combination of two tensors (Generator.py:58-67 / Discriminator.py:57-79
 * backward): dy = gamma*invstd*(g - S0/count - xhat*S1/count), xhat = (y - mean)*invstd  ==  p*g + q*y + r  with
 *   p = gamma*invstd,  q = -p*invstd*S1/count,  r = -p*S0/count - q*mean        (gamma == NULL: 1)
 * sums = [S0 | S1] (2C); coef [3, C] = [p | q | r].  Consumers: spgan_gemm_nt_args.A2 / spgan_gemm_tn_args.A2. */
/* spgan_colstats_finalize (mode 1: plain sums, one group) that ALSO emits those coefficient vectors from the sums it just merged:
 * the finalize launch behind a BNBWD-epilogue GEMM hands the lazy operand to the next products without a launch of its own. */
int spgan_colstats_finalize_bnbwd(const float* partials, int tiles, int C, int G, int tile_rows, const float* mean, const float* invstd,
                                  const float* gamma, float count, float* s0, float* s1, float* coef, spgan_stream_t s);
/* spgan_colstats_finalize (mode 1, one group) that ALSO runs phase B of the BatchNorm double backward on the sums it just merged
 * (spgan_bn_dbl_phaseb_sums with s0 / s1 := the merged sums): -> s0, s1 [C], sums2C, dgamma */
int spgan_colstats_finalize_phaseb(const float* partials, int tiles, int C, int G, int tile_rows, const float* U0, const float* U1, const float* Ugz,
                                   const float* S0, const float* S1, const float* gamma, const float* invstd, int count, float* s0, float* s1,
                                   float* sums2C, float* dgamma, spgan_stream_t s);
int spgan_bn_bwd_coeffs(const float* sums, const float* mean, const float* invstd, const float* gamma, int C, float count, float* coef, spgan_stream_t s);

size_t spgan_gemm_tn_ws_bytes(int M, int Na, int Nb);
/* The same, and the number of split partials, for a launch with spgan_gemm_tn_args.mfma_lp = mfma_lp: the split-bf16 kernel (mfma_lp == 2) works
 * on larger output tiles and has its own split plan; for mfma_lp 0 / 1 these equal spgan_gemm_tn_ws_bytes / spgan_gemm_tn_splits. */
size_t spgan_gemm_tn_ws_bytes_lp(int M, int Na, int Nb, int mfma_lp);
int spgan_gemm_tn_splits_lp(int M, int Na, int Nb, int mfma_lp);
int spgan_gemm_tn(const spgan_gemm_tn_args* a, spgan_stream_t s);
/* The kernel family spgan_gemm_tn runs for this block (0: a == NULL): the one decision (csrc/gemm_tn_plan.hpp) that the launch executes and
 * that the queries above and below read.  None of them reads through a pointer of the block. */
enum { SPGAN_TN_KERNEL_SKINNY = 1, SPGAN_TN_KERNEL_TILE = 2, SPGAN_TN_KERNEL_LP = 3, SPGAN_TN_KERNEL_WIDE3 = 4 };
int spgan_gemm_tn_kernel(const spgan_gemm_tn_args* a);
/* The whole plan as integers, for tests and tools: out[0..8] = kernel, invalid (16-bit stored operands that no kernel takes: the launch
 * returns SPGAN_EINVAL), splits, rows per split, the B-tile width 128 / 64 / 32 (TILE, LP), fast (vector loads), narrow_b (SKINNY: B is the
 * narrow side), the split-bf16 tile configuration 24 / 22 / 14 (WIDE3, else 0), sparse_rows (the sparse-addend launch follows). */
#define SPGAN_TN_PLAN_FIELDS 9
int spgan_gemm_tn_plan(const spgan_gemm_tn_args* a, int32_t* out);
/* `count` (<= 4) streaming products with a narrow B (Nb <= 4: the weight gradient of D's first conv against the three input coordinates) of ONE
 * shape as one launch, partials only (defer_reduce != 0 required; summed by spgan_splitk_reduce_multi): real / fake / double-backward pass of a
 * grouped D step.  A plain or two-tensor (A2) A operand. */
int spgan_gemm_tn_skinny_multi(const spgan_gemm_tn_args* a, int count, spgan_stream_t s);

/* The backward of one 1x1-conv layer behind a train-mode BatchNorm + LeakyReLU as ONE launch (csrc/gemm_dual.hip): the weight-gradient
 * product and the input-gradient product from ONE staging of the incoming gradient tile -- what autograd does with two convolution
 * backward kernels for conv_w.3 of an EdgeBlock (Generation/Generator.py:56-63,78), mlps.3 / mlps.6 of the Discriminator and the
 * collapsed form of its fc2.0 (Generation/Discriminator.py:55-65,77-81,104); before: spgan_gemm_tn + spgan_gemm_nt with the BNBWD /
 * EDGE_BNBWD epilogue.
 *   dy[m,:]  = A[m,:]                                          a_mode 0 (dense)                      [M, Na]
 *            = A[m,:]*p + A2[m,:]*q + r                        a_mode 1 (the lazy BatchNorm-backward operand of spgan_bn_bwd_coeffs)
 *            = lrelu(A[m,:]*p + r, a_slope)                    a_mode 2 (an activation formed on load: the collapsed layer's a3)
 *   pre[m,:] = B[m,:]                                                                               [M, Nb]   the previous layer's pre-BatchNorm output, or
 *            = B[e_idx[m],:] - B[m / e_k,:] + e_bias   (e_idx != NULL: per-edge operand, B = the point tensor, Nb = 64)
 *   ws[run]  = sum over the rows of run `run` of dy^T . lrelu(pre*b_scale + b_shift, slope)          [runs, Na, Nb] partials of dW
 *   G[m,:]   = (dy[m,:] . W + bias + rowadd[m,:]) * (pre*b_scale + b_shift > 0 ? 1 : slope)          [M, Nb]   (bias [Nb], rowadd [M, Nb]: optional)
 *   stats    = per run (sum G, sum G*xhat), xhat = (pre - b_mean)*b_invstd                           [runs, Nb, 2] plain sums
 *   colsum_ws (optional) = per run the column sums of dy                                             [runs, Na]
 * runs = spgan_gemm_dual_wgs(M, Na, Nb, e_k) (0: shape not supported -- (Na, Nb) = (128, 64), (256, 128) or (256, 256), M % 32 == 0,
 * M >= 8192, e_k 10 only with (128, 64); the caller then uses the two separate launches).  dW = the fixed-order sum of the partials
 * (spgan_splitk_reduce_multi with splits = runs); the statistics are finished by spgan_colstats_finalize(_bnbwd) with tiles = runs,
 * tile_rows = spgan_gemm_dual_rows_per_wg(M, Na, Nb).  fp32 operands, 16-byte aligned rows. */
typedef struct spgan_gemm_dual_args {
  const float* A; int lda;
  const float* A2; int lda2; const float* p; const float* q; const float* r;
  const float* W; int ldw;                       /* [Na, Nb]: the layer's weight as stored (row = output channel) */
  const float* B; int ldb;
  const int32_t* e_idx; int e_k; const float* e_bias;
  const float* b_scale; const float* b_shift; const float* b_mean; const float* b_invstd; float slope;
  float* G; int ldg;
  float* stats; float* ws;
  int M, Na, Nb;
  int a_mode; float a_slope;
  const float* bias; const float* rowadd; int ld_rowadd;
  float* colsum_ws;
  /* optional: the stored tile is gout_add[m, :] + gout_scale[:] * G[m, :] (statistics: of G).  The double backward's phase B: the adjoint
   * X = xbarA + gamma*g that the next BatchNorm backward consumes leaves this launch, not a pass of its own. */
  const float* gout_add; int ld_gout_add; const float* gout_scale;
} spgan_gemm_dual_args;
int spgan_gemm_dual_wgs(int M, int Na, int Nb, int e_k);
int spgan_gemm_dual_rows_per_wg(int M, int Na, int Nb);   /* rows per run = the `tile_rows` of the statistics partials (tiles = runs = ceil(M / rows)) */
int spgan_gemm_dual(const spgan_gemm_dual_args* a, spgan_stream_t s);
/* Grouped launch: `count` (<= SPGAN_GROUP_MAX) independent spgan_gemm_dual problems of ONE geometry (equal M, Na, Nb; plain pre tensors) as a
 * single grid, problem g on the workgroups [g*grid1, (g+1)*grid1): every problem's results are bit-identical to its stand-alone launch.
 * The D step issues each Discriminator layer's backward for the real pass, the fake pass and phase B of the penalty's double backward
 * (Generation/Discriminator.py:97-115 called three times per D step, Common/gradient_penalty.py:19-37); count == 1 is spgan_gemm_dual. */
#define SPGAN_GROUP_MAX 4
int spgan_gemm_dual_multi(const spgan_gemm_dual_args* a, int count, spgan_stream_t s);
/* The launches around a grouped spgan_gemm_dual_multi, grouped the same way (every problem runs the body of its stand-alone kernel:
 * bit-identical results).
 * spgan_colstats_finalize_multi: `count` mode-1 finalize launches (plain sums s0/s1 of [tiles, C, 2] records) with per-problem tail --
 *   kind 0: none;  kind 1: spgan_colstats_finalize_bnbwd's coefficients (mean, invstd, gamma | NULL, count -> coef [3,C]);
 *   kind 2: spgan_colstats_finalize_phaseb (U0, U1, Ugz, S0, S1, gamma, invstd, count -> sums [2C], dgamma [C]).  tiles < 2048. */
typedef struct spgan_colfinalize_args {
  const float* partials; int tiles, C, G, tile_rows;
  float* s0; float* s1;
  int kind;
  const float* mean; const float* invstd; const float* gamma; float count;
  float* coef;
  const float* U0; const float* U1; const float* Ugz; const float* S0; const float* S1;
  float* sums; float* dgamma;
  float* pb_coef;          /* kind 2, optional (needs mean): coef [3,C] of the lazy operand p*X + q*y + r = the BatchNorm backward (gamma = 1) with `sums` */
} spgan_colfinalize_args;
int spgan_colstats_finalize_multi(const spgan_colfinalize_args* a, int count, spgan_stream_t s);
/* spgan_pool_bwd_stats_prep for `count` passes (the real and the fake pass behind one grouped forward) as one launch. */
typedef struct spgan_pool_bwd_args {
  const float* gpool; const float* pooled; const int32_t* argmax; const float* y; int ld;
  const float* mean; const float* invstd; float slope; int B, C;
  const float* gamma; int count;
  float* gval; float* sums; float* alpha; float* beta; float* cg;
} spgan_pool_bwd_args;
int spgan_pool_bwd_stats_prep_multi(const spgan_pool_bwd_args* a, int count, spgan_stream_t s);

/* Row-sparse products with the max-pool gradient pattern S (Discriminator.py:104 backward): one (value, row) pair per
 * shape b and channel c, val/arg [B, Cs], arg = global row (b*rows + local).  They let the backward of the layer in front
 * of the pool collapse algebraically (DESIGN.md "collapsed L4 backward"): with dz = alpha*y + beta + S and y = a.W^T + b,
 *   dz.W      = a.(W^T diag(alpha) W) + (alpha*b + beta).W + S.W          -- a [M,Cin]x[Cin,Cin] GEMM instead of [M,Cout]x[Cout,Cin]
 *   dz^T.a    = diag(alpha).W.(a^T a) + (alpha*b + beta) (x) colsum(a) + S^T.a
 * spgan_sparse_rows_nt: E[m, n]  = sum_{c: arg[b,c]==m} val[b,c] * W[c, n]      E [B*rows, N] is fully written (zero rows too)
 * spgan_sparse_rows_tn: C[c, n] += sum_b val[b,c] * pro(Bm)[arg[b,c], n]         pro = lrelu(x*p_scale[n]+p_shift[n], p_slope) or none
 * Both sum in ascending c / b order (deterministic). */
/* The two weight-only operands of that collapsed backward in one launch (csrc/collapse.hip), W [C, K]:
 *   G[i,j] = sum_c W[c,i]*alpha[c]*W[c,j]   (W^T diag(alpha) W, [K,K]);   cvec[j] = sum_c (alpha[c]*bias[c] + beta[c])*W[c,j]   (cvec NULL: skipped)
 * C % 256 == 0, K % 32 == 0; deterministic (fixed-order sums). */
int spgan_wt_diag_w(const float* W, int ldw, int C, int K, const float* alpha, const float* beta, const float* bias, float* G, int ldg,
                    float* cvec, spgan_stream_t s);
/* Both of the above's launches for one collapsed backward pass -- spgan_wt_diag_w (nprob = 1 .. 4 problems on the same W: the double backward needs
 * W^T diag(c1) W and W^T diag(c2) W; the grouped D step adds the real and the fake pass) and nsparse x spgan_sparse_rows_nt (E [B*rows, K] = S.W, Cs = C) -- as ONE launch: the weight-only part is latency-bound on
 * a fraction of the chip and finishes under the part that streams E out.  Results bit-identical to the separate launches.  cvec[p] / beta[p] /
 * bias[p] NULL: no cvec for problem p. */
typedef struct spgan_collapse_prep_args {
  const float* W; int ldw, C, K;
  int nprob;                                            /* 1 .. SPGAN_GROUP_MAX weight problems on the same W */
  const float* alpha[SPGAN_GROUP_MAX]; const float* beta[SPGAN_GROUP_MAX]; const float* bias[SPGAN_GROUP_MAX];
  float* G[SPGAN_GROUP_MAX]; int ldg; float* cvec[SPGAN_GROUP_MAX];
  int nsparse;                                          /* 1 .. SPGAN_GROUP_MAX sparse-row products E[q] = S[q].W, equal B and rows */
  const float* sp_val[SPGAN_GROUP_MAX]; const int32_t* sp_arg[SPGAN_GROUP_MAX]; int B, rows;
  float* E[SPGAN_GROUP_MAX]; int lde;
} spgan_collapse_prep_args;
int spgan_collapse_prep(const spgan_collapse_prep_args* a, spgan_stream_t s);
/* The weight gradient of the collapsed layer, all of its terms in one launch (csrc/collapse.hip):
 *   out[a,n] (+)= a1[a] * sum_k W[a,k]*X1[n,k]  +  (a1[a]*b1[a] + d1[a]) * v1[n]  +  a2[a] * sum_k W[a,k]*X2[n,k]
 *                 +  sum_b sp_val[b,a] * pro(Bm)[sp_arg[b,a], n]          (pro = lrelu(x*p_scale[n] + p_shift[n], p_slope), or identity)
 * W [C,K], X1 [N,K] (a Gram matrix / q^T a of the double backward), K <= 256, C, N, K multiples of 32, 16-byte aligned rows.  Optional: the rank-1 term
 * (v1, b1, d1), the second product (X2 [N,K], or [K,N] with x2_t = 1: used transposed; a2), the sparse term (sp_val / sp_arg [B,C], global rows of
 * Bm [B*rows, N]; B <= 64; shapes in ascending order), T [C,N] = the raw first product, accumulate != 0: out += .  Replaces spgan_gemm_nt +
 * spgan_rowscale_outer + spgan_sparse_rows_tn (and, in the double backward, a transpose, a second product and two axpby). */
typedef struct spgan_wgrad_collapse_args {
  const float* W; int ldw, C, K;
  const float* X1; int ldx1;
  const float* a1; const float* b1; const float* d1; const float* v1;
  const float* X2; int ldx2, x2_t; const float* a2;
  const float* sp_val; const int32_t* sp_arg; int B, rows;
  const float* Bm; int ldb; const float* p_scale; const float* p_shift; float p_slope;
  float* T; int ldt;
  float* out; int ldo, N, accumulate;
} spgan_wgrad_collapse_args;
int spgan_wgrad_collapse(const spgan_wgrad_collapse_args* a, spgan_stream_t s);
/* `count` (<= SPGAN_GROUP_MAX) problems with equal C, N, K as one launch (count == 1: spgan_wgrad_collapse) */
int spgan_wgrad_collapse_multi(const spgan_wgrad_collapse_args* a, int count, spgan_stream_t s);
int spgan_sparse_rows_nt(const float* val, const int32_t* arg, int B, int rows, int Cs, const float* W, int ldw, int N, float* E, int lde,
                         spgan_stream_t s);
int spgan_sparse_rows_tn(const float* val, const int32_t* arg, int B, int rows, int Cs, const float* Bm, int ldb, int Nb,
                         const float* p_scale, const float* p_shift, float p_slope, float* C, int ldc, spgan_stream_t s);
/* out[m,c] = lrelu(X[m,c]*scale[c] + shift[c], slope)   (train-mode BatchNorm + LeakyReLU output, Discriminator.py:57-64) */
int spgan_affine_act(const float* X, int ldx, size_t M, int C, const float* scale, const float* shift, float slope, float* out, spgan_stream_t s);
/* out[r,c] = a[r]*X[r,c] + (a[r]*b[r] + d[r])*v[c]   (v == NULL: first term only); weight-shaped [R,C] tensors */
/* accumulate != 0: out += that (the terms of a weight gradient summed in place instead of by axpby launches) */
int spgan_rowscale_outer(const float* X, int ldx, int R, int C, const float* a, const float* b, const float* d, const float* v, float* out,
                         int ldo, int accumulate, spgan_stream_t s);

/* Column reductions over row groups (group = G consecutive rows; M % G == 0).  Partials are
 * [groups * ceil(G/128)][C][2] floats: one (a, b) pair per 128-row tile and column -- the format
 * spgan_gemm_nt's `stats` epilogue writes (there: one group of M rows).
 * finalize mode 0 (Welford/Chan): partials (sum, centred M2) -> out0 = mean, out1 = biased variance.
 * finalize mode 1 (plain):         partials (s0, s1)          -> out0 = sum s0, out1 = sum s1.
 * Everything is combined in a fixed order: results are run-to-run deterministic. */
size_t spgan_colreduce_ws_bytes(int M, int C, int G);
int spgan_colstats_finalize(const float* partials, int groups, int tiles_per_group, int C, int G, int mode,
                            int tile_rows /* 0 -> 128 */, float* out0, float* out1, spgan_stream_t s);
/* One group of G rows: finalize (sum, M2) partials AND do the train-mode BatchNorm bookkeeping of spgan_bn_prepare in the
 * same launch (scale, shift, invstd, mean; running stats updated when given). */
int spgan_colstats_finalize_bn(const float* partials, int tiles, int C, int G, int tile_rows, const float* gamma, const float* beta,
                               float eps, float momentum, float* running_mean, float* running_var, float* scale, float* shift,
                               float* invstd, float* mean_out, spgan_stream_t s);
/* spgan_colstats_finalize_bn for `groups` consecutive row groups of G rows each (records [groups * tiles_per_group, C, 2]) that go
 * through the SAME BatchNorm layer one after the other: out [4, groups, C] = scale | shift | invstd | mean, each a contiguous [groups, C]
 * block (what spgan_gemm_nt_args.p_group_rows and spgan_pool_finalize_groups read); the running statistics are updated group after
 * group (group 0 first) exactly as `groups` separate calls would. */
int spgan_colstats_finalize_bn_groups(const float* partials, int groups, int tiles_per_group, int C, int G, int tile_rows, const float* gamma,
                                      const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* out,
                                      spgan_stream_t s);
/* The same for TWO BatchNorm layers whose channels lie side by side in one record set (columns [0,split) -> layer A, [split,C) ->
 * layer B, each with its own gamma/beta/running buffers): the two per-edge BatchNorms of an EdgeBlock (Generator.py:57-58,66-67) from
 * spgan_edge_stats' records in one launch.  out4 [4,C] = scale | shift | invstd | mean.  count_rep: the rows stand for count_rep
 * identical copies (only the unbiased-variance count of the running statistics changes). */
int spgan_colstats_finalize_bn2(const float* partials, int tiles, int C, int G, int tile_rows, int split, const float* gammaA,
                                const float* betaA, float* rmeanA, float* rvarA, const float* gammaB, const float* betaB, float* rmeanB,
                                float* rvarB, float eps, float momentum, int count_rep, float* out4, spgan_stream_t s);
/* mean / biased variance over each group of lrelu(X, slope) (slope = 1: plain).  InstanceNorm1d statistics of
 * AdaptivePointNorm (Generator.py:29,42) with G = N; BatchNorm statistics with G = M.  ws >= spgan_colreduce_ws_bytes. */
int spgan_colstats(const float* X, int ldx, int M, int C, int G, float slope, float* out_mean, float* out_var,
                   float* ws, size_t ws_bytes, spgan_stream_t s);
/* out[g, c] = sum over the G rows of group g of X[m,c]  (bias gradients; per-shape bias gradients).
 * ws >= spgan_colreduce_ws_bytes(M,C,G) + (M/G)*C*4. */
int spgan_colsum(const float* X, int ldx, int M, int C, int G, float* out, float* ws, size_t ws_bytes, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Train-mode BatchNorm bookkeeping (torch defaults: eps 1e-5, momentum 0.1, biased var for the
 * normalisation, unbiased var into running_var).  Generator.py:58,61,67,121,124; Discriminator.py:57-79.
 * ---------------------------------------------------------------------------------------- */
/* training=1: from batch (mean,var): scale=gamma*invstd, shift=beta-mean*scale, invstd; updates running stats
 *             when running_mean != NULL.   training=0: uses running stats instead of (mean,var). */
int spgan_bn_prepare(const float* mean, const float* var, const float* gamma, const float* beta, int C,
                     int count, float eps, float momentum, int training,
                     float* running_mean, float* running_var,
                     float* scale, float* shift, float* invstd, float* mean_used, spgan_stream_t s);
/* dy[m,c] = gamma[c]*invstd[c]*( g[m,c] - sums[c]/count - xhat[m,c]*sums[C+c]/count ),  xhat=(y-mean)*invstd */
int spgan_bn_bwd_apply(const float* g, const float* y, int ld, int M, int C, const float* mean, const float* invstd,
                       const float* gamma, const float* sums, int count, float* dy, spgan_stream_t s);
/* The same with g := g + g2scale[c]*g2 formed on the fly (contiguous [M,C], C % 4 == 0, 16-byte aligned): the double backward's
 * xbarA + gamma*g (BatchNorm backward of the gradient-penalty graph) without a separate elementwise pass. */
int spgan_bn_bwd_apply2(const float* g, const float* g2, const float* g2scale, const float* y, int M, int C, const float* mean,
                        const float* invstd, const float* gamma, const float* sums, int count, float* dy, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Global max over the N points of each shape (Generator.py:183; Discriminator.py:104) fused with
 * the preceding affine + LeakyReLU:  out[b,c] = max_n lrelu(y[b*N+n,c]*scale[c]+shift[c]).
 * ---------------------------------------------------------------------------------------- */
int spgan_maxpool(const float* y, int ld, int B, int N, int C, const float* scale, const float* shift, float slope,
                  float* out, int32_t* argmax, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * EdgeBlock (Generation/Generator.py:47-88), restructured per point:
 *   conv_w.0(x_j - x_i) = (P_j - P_i) + b1,  conv_x.0([x_i, x_j-x_i]) = (R_i + Q_j) + bx,
 *   PQR[M, H+2F] = x . Wcat^T,  Wcat = [W1; Wd; Wc-Wd],  Wx = [Wc | Wd],  H = F/2.
 * ---------------------------------------------------------------------------------------- */
/* WcatT (nullable) [C, H+2F] = Wcat^T from the same launch: the operand of the block's input-gradient GEMM (dx = dPQR . Wcat). */
int spgan_edge_wcat(const float* Ww0 /*[H,C]*/, const float* Wx /*[F,2C]*/, int H, int F, int C, float* Wcat, float* WcatT, spgan_stream_t s);
/* conv_out.weight [F,F,1,k] (Generator.py:70: Conv2d(F, F, [1,k])) in the two layouts the point-major EdgeBlock multiplies with:
 * Wo [F, k*F] with K index r*F + c (the order of the per-point feature row T[m, r*F + c]) for the forward product, and WoT (nullable)
 * [k*F, F] = Wo^T for the input gradient dT = dout . Wo -- one launch instead of a permuted copy now and a transpose in the backward. */
int spgan_conv_out_weight_pm(const float* w, int F, int k, float* Wo, float* WoT, spgan_stream_t s);
int spgan_edge_wcat_bwd(const float* dWcat, int H, int F, int C, float* dWw0, float* dWx, spgan_stream_t s);
/* BatchNorm2d statistics over the M*k edges of both per-edge pre-activations (Generator.py:58,67):
 * partials [ceil(M/32)][H+F][2] in the finalize-mode-0 format with tile_rows = spgan_edge_stats_tile_rows(k). */
int spgan_edge_stats_tile_rows(int k);
int spgan_edge_stats(const float* PQR, int ld, const int32_t* idx, int M, int k, int H, int F, const float* b1, const float* bx,
                     float* partials, spgan_stream_t s);
/* T[i, r*F+f] = softmax_r(lrelu(h2pre[i,r,f]*sc2+sh2)) * lrelu(((R_i+Q_j)+bx)*scx+shx)    (Generator.py:79,81-82) */
int spgan_edge_attend_fwd(const float* h2pre, const float* sc2, const float* sh2, const float* PQR, int ld, int H, int F,
                          const int32_t* idx, int M, int k, const float* bx, const float* scx, const float* shx, float slope,
                          float* T, spgan_stream_t s);
/* Backward of edge_attend: g2/gy = gradients w.r.t. the two BatchNorm outputs, and plain-sum partials
 * [ceil(M/spgan_edge_attend_bwd_tile_points())][2F][2]: col f -> (sum g2, sum g2*xhat2), col F+f -> (sum gy, sum gy*xhaty). */
/* 16-bit storage variants for the "f16" operand mode (BASELINE configs[4]).  Forward: T is written as IEEE fp16 (consumed by conv_out's
 * products: spgan_gemm_nt_args.a_half / spgan_gemm_tn_args.b_half).  Backward: dT is read as bfloat16 (written by spgan_gemm_nt_args.y_bf16: a
 * gradient keeps fp32's exponent range); g2 -- a GEMM operand only (a_half of spgan_gemm_tn_args / spgan_gemm_nt_args) -- and gy -- consumed
 * by spgan_edge_scatter_b -- are written as bfloat16; the partials stay float.  h2_half = 1: h2pre lies in memory as fp16 (written by the
 * edge GEMM with spgan_gemm_nt_args.y_half).  k = 10 and F % 4 == 0 only; everything else as the fp32 entry points. */
int spgan_edge_attend_fwd_h(const void* h2pre, int h2_half, const float* sc2, const float* sh2, const float* PQR, int ld, int H, int F,
                            const int32_t* idx, int M, int k, const float* bx, const float* scx, const float* shx, float slope, uint16_t* T_f16,
                            spgan_stream_t s);
int spgan_edge_attend_bwd_b(const uint16_t* dT_bf16, const void* h2pre, int h2_half, const float* sc2, const float* sh2, const float* mean2,
                            const float* inv2, const float* PQR, int ld, int H, int F, const int32_t* idx, int M, int k, const float* bx,
                            const float* scx, const float* shx, const float* meanx, const float* invx, float slope, uint16_t* g2_bf16,
                            uint16_t* gy_bf16, float* partials, spgan_stream_t s);
/* spgan_edge_scatter with the gy operand as written by spgan_edge_attend_bwd_b (bfloat16; k = 10) */
int spgan_edge_scatter_b(const float* g1, const uint16_t* gy_bf16, const float* PQR, int ld, int H, int F, const int32_t* idx,
                         const int32_t* rowptr, const int32_t* src, int M, int k, const float* b1, const float* mean1, const float* inv1,
                         const float* gam1, const float* sums1, const float* bx, const float* meanx, const float* invx, const float* gamx,
                         const float* sumsx, float* dPQR, spgan_stream_t s);
int spgan_edge_attend_bwd_tile_points(void);
int spgan_edge_attend_bwd(const float* dT, const float* h2pre, const float* sc2, const float* sh2, const float* mean2,
                          const float* inv2, const float* PQR, int ld, int H, int F, const int32_t* idx, int M, int k,
                          const float* bx, const float* scx, const float* shx, const float* meanx, const float* invx,
                          float slope, float* g2, float* gy, float* partials, spgan_stream_t s);
/* spgan_edge_attend_bwd with dT = dout . WoT^T formed inside the launch (csrc/edge_dt.hip): dout [M, ldo >= F], WoT [k*F, ldw >= F] as
 * written by spgan_conv_out_weight_pm; dT [M, k*F] never reaches memory.  k = 10, F = 128, M % 32 == 0, fp32, 16-byte aligned dout / WoT
 * rows only.  g2, gy and the partials are bit for bit those of spgan_gemm_nt (256 x 256-tile kernel) followed by spgan_edge_attend_bwd;
 * spgan_edge_attend_bwd_dt_selected is 1 exactly when that product would run the 256 x 256-tile kernel (tile_hint as in
 * spgan_gemm_nt_args; honours SPGAN_NT_WIDE=0), the only case in which the fused launch may replace the pair. */
int spgan_edge_attend_bwd_dt_selected(const float* dout, int ldo, const float* WoT, int ldw, int M, int k, int F, int tile_hint);
int spgan_edge_attend_bwd_dt(const float* dout, int ldo, const float* WoT, int ldw, const float* h2pre, const float* sc2, const float* sh2,
                             const float* mean2, const float* inv2, const float* PQR, int ld, int H, int F, const int32_t* idx, int M, int k,
                             const float* bx, const float* scx, const float* shx, const float* meanx, const float* invx, float slope,
                             float* g2, float* gy, float* partials, spgan_stream_t s);
/* BatchNorm backward of both per-edge pre-activations fused with the reduction onto points (gather over the CSR
 * in-edge lists; the backward obligation of modules.py:708-720): dPQR[M, H+2F]. sums* = [sum g | sum g*xhat]. */
int spgan_edge_scatter(const float* g1, const float* gy, const float* PQR, int ld, int H, int F, const int32_t* idx,
                       const int32_t* rowptr, const int32_t* src, int M, int k, const float* b1, const float* mean1,
                       const float* inv1, const float* gam1, const float* sums1, const float* bx, const float* meanx,
                       const float* invx, const float* gamx, const float* sumsx, float* dPQR, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * AdaptivePointNorm (Generator.py:24-45): out = gamma*xhat + beta with xhat = InstanceNorm1d(lrelu(x, slope))
 * (eps 1e-5, biased variance over the N points of each shape; slope = 1 for the bare module, 0.2 when the
 * Generator's lrelu1/lrelu2 is fused in, Generator.py:175-176,179-180) and [gamma|beta] = gb[M,2C].
 * ---------------------------------------------------------------------------------------- */
int spgan_adain_fwd(const float* x, int M, int C, int N, float slope, const float* imean, const float* ivar, float eps,
                    const float* gb, float* out, spgan_stream_t s);
/* dgb = [dout*xhat | dout]; partials [(M/N)*ceil(N/128)][C][2] = (sum dxh, sum dxh*xhat), dxh = dout*gamma (finalize mode 1).
 * gamma[m, c] = gb[m * ld_gamma + c]: ld_gamma = 2C for the [M,2C] style tensor [gamma|beta], C for the gamma-only tensor the
 * SPGAN_EPI_ADAIN epilogue stores.  Shape b's rows of x start at x + b * x_shape_stride (N*C: a dense [M,C] tensor; 0: all shapes share
 * one [N,C] block). */
int spgan_adain_bwd1(const float* dout, const float* x, int M, int C, int N, float slope, const float* imean, const float* ivar,
                     float eps, const float* gb, int ld_gamma, long x_shape_stride, float* dgb, float* partials, spgan_stream_t s);
int spgan_adain_bwd2(const float* dout, const float* x, int M, int C, int N, float slope, const float* imean, const float* ivar,
                     float eps, const float* gb, int ld_gamma, long x_shape_stride, const float* S0, const float* S1, float* dx,
                     spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Backward through [BatchNorm1d -> LeakyReLU -> global max over N] (Discriminator.py:77-81,104): the incoming
 * gradient is non-zero only at the arg-max rows, the BatchNorm backward makes it dense again.
 * ---------------------------------------------------------------------------------------- */
int spgan_pool_bwd_stats(const float* gpool, const float* pooled, const int32_t* argmax, const float* y, int ld, const float* mean,
                         const float* invstd, float slope, int B, int C, float* gval, float* sums /*[2C]*/, spgan_stream_t s);
/* spgan_pool_bwd_stats followed by spgan_sparse_bn_prep (the coefficients alpha, beta [C] and cg [B,C] of the lazily evaluated BatchNorm
 * backward behind the max-pool) in ONE launch: both are per-channel work on the same [B,C] values. */
int spgan_pool_bwd_stats_prep(const float* gpool, const float* pooled, const int32_t* argmax, const float* y, int ld, const float* mean,
                              const float* invstd, float slope, int B, int C, const float* gamma, int count, float* gval, float* sums /*[2C]*/,
                              float* alpha, float* beta, float* cg, spgan_stream_t s);
int spgan_bn_bwd_apply_sparse(const float* gval, const int32_t* argmax, const float* y, int ld, int M, int C, int N,
                              const float* mean, const float* invstd, const float* gamma, const float* sums, int count, float* dy,
                              spgan_stream_t s);
/* dst[argmax[b,c], c] += dpool[b,c]   (torch.max backward, Generator.py:183) */
int spgan_maxpool_bwd_add(const float* dpool, const int32_t* argmax, int B, int C, float* dst, int ld, spgan_stream_t s);
int spgan_tanh_bwd(const float* dy, const float* y, size_t n, float* out, spgan_stream_t s);
/* out = dy * act'(y) from the activation OUTPUT y (act = SPGAN_ACT_*; in-place LeakyReLU semantics, Generator.py:110-133) */
int spgan_act_bwd(const float* dy, const float* y, size_t n, int act, float slope, float* out, spgan_stream_t s);
/* out[M,C] = 0, out[argmax[b,c], c] = val[b,c];   out[b,c] = src[argmax[b,c], c] */
int spgan_scatter_rows(const float* val, const int32_t* argmax, int B, int C, int M, float* out, spgan_stream_t s);
int spgan_gather_rows(const float* src, int ld, const int32_t* argmax, int B, int C, float* out, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * WGAN-GP double backward through train-mode BatchNorm (Common/gradient_penalty.py:31-35 + .backward();
 * derivation in DESIGN.md).  u = adjoint of the BN-backward output, gz = first-order gradient w.r.t. the BN output.
 *   stats partials [ceil(M/128)][2C][2] (finalize mode 1): col c -> (sum u, sum u*xhat), col C+c -> (sum u*gz, 0)
 *   apply: q = gamma*invstd*(u - U0/M - xhat*U1/M)*lrelu'(y*scale+shift);  xbar = -(gamma*invstd/M)*(u*S1 + gz*U1)
 * ---------------------------------------------------------------------------------------- */
int spgan_bn_dbl_stats(const float* u, const float* y, const float* gz, int M, int C, const float* mean, const float* invstd,
                       float* partials, spgan_stream_t s);
int spgan_bn_dbl_apply(const float* u, const float* y, const float* gz, int M, int C, const float* mean, const float* invstd,
                       const float* scale, const float* shift, float slope, const float* gamma, const float* S1, const float* U0,
                       const float* U1, float* q, float* xbar, spgan_stream_t s);
/* ------------------------------------------------------------------------------------------
 * Losses on the [B,1] logits (Common/loss_utils.py:727-802 gen_loss, 854-972 dis_loss) with both logit
 * gradients in the same launch.  mode: 0 ls (default, config.py:72), 1 wgan, 2 hinge, 3 gan (BCE-with-logits);
 * which: 0 discriminator loss, 1 generator loss.  Labels [B] or NULL (ls only; the reference's F.mse_loss
 * broadcast of [B,1] logits against [B] labels to [B,B] is kept).
 * out5 = (loss, fake term, real term, real_acc, fake_acc).
 * ---------------------------------------------------------------------------------------- */
int spgan_gan_loss(int mode, int which, const float* d_real, const float* d_fake, const float* real_label, const float* fake_label,
                   int B, float* out5, float* g_real, float* g_fake, spgan_stream_t s);
/* WGAN-GP (Common/gradient_penalty.py:19-37): x_hat = real + alpha[b]*(fake-real);
 * penalty = lambda*mean_b(((||g_b||-gamma)/gamma)^2) and its gradient w.r.t. g (times upstream[0] if given). */
int spgan_lerp_rows(const float* real, const float* fake, const float* alpha, int B, size_t L, float* out, spgan_stream_t s);
int spgan_gp_penalty_fwd(const float* g, int B, size_t L, float gamma, float lambda, float* norms, float* loss, spgan_stream_t s);
int spgan_gp_penalty_bwd(const float* g, const float* norms, int B, size_t L, float gamma, float lambda, const float* upstream,
                         float* v, spgan_stream_t s);
/* spgan_gp_penalty_fwd and spgan_gp_penalty_bwd (upstream = 1) as two launches instead of three: row norms, then v and the penalty together;
 * optional loss_total[0] = loss_add[0] + penalty (the D step's reported loss).  Values bit-identical to the separate calls. */
int spgan_gp_penalty_fwd_bwd(const float* g, int B, size_t L, float gamma, float lambda, float* norms, float* loss, const float* loss_add,
                             float* loss_total, float* v, spgan_stream_t s);
/* ------------------------------------------------------------------------------------------
 * Ball-query / grouping family (Common/pointnet_util.py, Common/pointconv_util.py; orphans in the reference,
 * named by the north star).  xyz/new_xyz/points are [B,N,C] row-major like the reference; indices are int64.
 * ---------------------------------------------------------------------------------------- */
/* out[b,n,m] = -2<src_n,dst_m> + |src_n|^2 + |dst_m|^2            pointnet_util.py:19-40 */
int spgan_square_distance(const float* src, const float* dst, int B, int N, int M, int C, float* out, spgan_stream_t s);
/* out[b,s,:] = points[b, idx[b,s], :]  (idx [B,S] or [B,S,K] flattened to S*K)   pointnet_util.py:43-60 */
int spgan_index_points(const float* points, const int64_t* idx, int B, int N, int C, int S, float* out, spgan_stream_t s);
/* iterative farthest point sampling from start[b] (NULL: 0); dist_ws: B*N floats   pointnet_util.py:63-84, pointconv_util.py:60-83 */
int spgan_farthest_point_sample(const float* xyz, int B, int N, int npoint, const int64_t* start, int64_t* out, float* dist_ws,
                                spgan_stream_t s);
/* first nsample indices (ascending) with not (d^2 > thr), padded with the first hit (no hit: every slot N).  thr >= 0 is the THRESHOLD on
 * the squared distance, not the radius: the float32 nearest to the caller's double radius^2, which is what the reference's
 * `sqrdists > radius ** 2` compares with (squaring a float32 radius is one ulp off for many radii)     pointnet_util.py:87-107 */
int spgan_query_ball_point(float thr, int nsample, const float* xyz, const float* new_xyz, int B, int N, int S, int C,
                           int64_t* out, spgan_stream_t s);
/* nsample nearest (self included), ascending (distance, index)                      pointconv_util.py:107-118 */
int spgan_knn_point(int nsample, const float* xyz, const float* new_xyz, int B, int N, int S, int C, int64_t* out, spgan_stream_t s);
/* out[b,s,j,:] = [xyz[b,idx] - center[b,s] | feat[b,idx]]   pointnet_util.py:127-139, pointconv_util.py:186-195 */
int spgan_group_concat(const float* xyz, const float* center, const float* feat, const int64_t* idx, int B, int N, int S, int K,
                       int C, int D, float* out, spgan_stream_t s);
/* Adjoints of the gathers above (the reference gets them from torch indexing: index_put / the side-car's atomicAdd scatter,
 * metrics/pointops/src/grouping/grouping_cuda_kernel.cu:28-45, metrics/pointnet2/src/group_points_gpu.cu:8-30).  Deterministic:
 * spgan_gather_csr lists, per point, the gather slots that read it (ascending), the sums run over those lists in order.
 *   spgan_gather_csr:           idx int64 [B,S] local indices -> rowptr int32 [B*N,2] (begin,end) into src int32 [B*S]; *bad |= 1 on an index outside [0,N)
 *   spgan_scatter_slots:        dpoints[n,c] = sum_{e in slots(n)} dout[e*ld + col0 + c]      (index_points / grouping backward)
 *   spgan_group_center_bwd:     dcenter[q,c] = -sum_j dout[(q*K+j)*ld + c]                    (pointnet_util.py:128, pointconv_util.py:189)
 *   spgan_edge_features_cm_bwd: dx [B,C,N] from dE [B,2C,N,k] (central + "-central" + in-edge terms, Generation/modules.py:708-720) */
int spgan_gather_csr(const int64_t* idx, int B, int S, int N, int32_t* rowptr, int32_t* src, int32_t* bad, spgan_stream_t s);
int spgan_scatter_slots(const float* dout, int ld, int col0, int C, const int32_t* rowptr, const int32_t* src, int BN, float* dpoints,
                        spgan_stream_t s);
int spgan_group_center_bwd(const float* dout, int ld, int Q, int K, int C, float* dcenter, spgan_stream_t s);
int spgan_edge_features_cm_bwd(const float* dE, const int32_t* rowptr, const int32_t* src, int B, int C, int N, int k, float* dx,
                               spgan_stream_t s);
/* PointNet++ set abstraction / feature propagation (Common/pointnet_util.py:146-320; the extension ops of metrics/pointnet2_ops).
 *   spgan_three_nn:              idx int64 [B,N,k], weight [B,N,k], k = min(3,S): the k nearest centres xyz2 [B,S,3] of every point xyz1 [B,N,3]
 *                                (ascending distance, lower index first on exact ties) and w = (1/(d+1e-8)) / sum(1/(d+1e-8)); d in
 *                                spgan_square_distance's arithmetic; no [B,N,S] matrix, no workspace          pointnet_util.py:301-307
 *   spgan_three_interpolate:     out[(b*N+n)*ld_out + col0 + c] = sum_j weight[b,n,j]*points2[b,idx[b,n,j],c], points2 [B,S,D]; the slice
 *                                [col0, col0+D) of a wider row buffer takes the place of the torch.cat of :312; *bad |= 1 on an index
 *                                outside [0,S) (bad may be NULL; such a slot contributes 0)                   pointnet_util.py:308
 *   spgan_three_interpolate_bwd: dpoints2[m,c] = sum_{e in slots(m)} weight[e]*dout[(e/k)*ld + col0 + c] over spgan_gather_csr's slot
 *                                lists of idx [B, N*k] (deterministic; the weights carry no gradient, as three_nn in pointnet2_ops)
 *   spgan_group_max:             pooled[q,c] = max_{j<K} lrelu(y[(q*K+j)*ld + c]*scale[c] + shift[c], slope), argmax int32 = that global row
 *                                (first maximum); scale/shift may both be NULL                                pointnet_util.py:203-205, 261-262
 *   spgan_group_max_bwd:         g [Q*K,C] = gpool*lrelu'(pooled) at the arg-max row, 0 elsewhere; gstat [Q,2C] = [that value | value*xhat(y)]
 *                                (its column sums are the BatchNorm backward's sums); argmax NULL with K = 1: every row its own group
 *   spgan_cm_to_rows / spgan_rows_to_cm: x [B,C,N] <-> columns [col0, col0+C) of a [B*N, ld] row buffer    pointnet_util.py:190-192, 311-316 */
int spgan_three_nn(const float* xyz1, const float* xyz2, int B, int N, int S, int64_t* idx, float* weight, spgan_stream_t s);
int spgan_three_interpolate(const float* points2, const int64_t* idx, const float* weight, int B, int N, int S, int D, int k, float* out,
                            int ld_out, int col0, int32_t* bad, spgan_stream_t s);
int spgan_three_interpolate_bwd(const float* dout, int ld, int col0, int D, const float* weight, int k, const int32_t* rowptr,
                                const int32_t* src, int BS, float* dpoints2, spgan_stream_t s);
int spgan_group_max(const float* y, int ld, int Q, int K, int C, const float* scale, const float* shift, float slope, float* pooled,
                    int32_t* argmax, spgan_stream_t s);
int spgan_group_max_bwd(const float* gpool, const float* pooled, const int32_t* argmax, const float* y, int ld, const float* mean,
                        const float* invstd, float slope, int Q, int K, int C, float* g, float* gstat, spgan_stream_t s);
int spgan_cm_to_rows(const float* x_cm, int B, int C, int N, float* rows, int ld, int col0, spgan_stream_t s);
int spgan_rows_to_cm(const float* rows, int ld, int col0, int B, int C, int N, float* x_cm, spgan_stream_t s);
/* PointConv density set abstraction (Common/pointconv_util.py:199-383).  Deterministic: fixed summation orders, no float atomics.
 *   spgan_kde_density:             density[b,i] = mean_j exp(-d_ij / (2 h^2)) / (2.5 h), d = spgan_square_distance's expanded form evaluated in
 *                                  float64 (d_ii is a rounding residue or zero); inv_density (may be NULL) = 1/density in the same launch;
 *                                  xyz [B,N,3]; no [B,N,N] matrix, no workspace                                   pointconv_util.py:199-209, 357
 *   spgan_kde_density_bwd:         dxyz_i = -(1/(h^2 N 2.5h)) sum_j (G_i + G_j) w_ij (x_i - x_j), w_ij = exp(-d_ij/(2h^2)),
 *                                  G = g - ginv * inv_density^2 (g: gradient of density, ginv: of 1/density; either may be NULL)
 *   spgan_group_density_scale:     scale[q*K + k] = v_k / max_k v_k, v_k = inv_density[b, idx[b,s,k]], q = b*S + s; *bad |= 1 on an index
 *                                  outside [0,N) (bad may be NULL; such a slot gets 0)                              pointconv_util.py:147, 370-371
 *   spgan_group_density_scale_bwd: dslot[q*K + k] = g_k/m - [k == first arg-max] (sum_j g_j v_j)/m^2: the gradient per gathered slot, summed
 *                                  onto the points by spgan_gather_csr + spgan_scatter_slots
 *   spgan_pointconv_aggregate:     E[q, c*W + w] = sum_k F[q*K+k, c] * dens[q*K+k] * Wt[q*K+k, w]; F [Q*K,C], Wt [Q*K,W], dens [Q*K] or NULL,
 *                                  W = 16 (the reference's only width); any K (walked in chunks), any C; sum in ascending k
 *                                  (v_mfma_f32_16x16x4_f32: exact fp32 products)                                   pointconv_util.py:373-377
 *   spgan_pointconv_aggregate_bwd: dF [Q*K,C], dWt [Q*K,W], ddens [Q*K] (NULL exactly when dens is) from dE [Q, C*W] in one launch */
int spgan_kde_density(const float* xyz, int B, int N, float bandwidth, float* density, float* inv_density, spgan_stream_t s);
int spgan_kde_density_bwd(const float* xyz, const float* g, const float* ginv, const float* inv_density, int B, int N, float bandwidth,
                          float* dxyz, spgan_stream_t s);
int spgan_group_density_scale(const float* inv_density, const int64_t* idx, int B, int N, int S, int K, float* scale, int32_t* bad,
                              spgan_stream_t s);
int spgan_group_density_scale_bwd(const float* g, const float* inv_density, const int64_t* idx, int B, int N, int S, int K, float* dslot,
                                  spgan_stream_t s);
int spgan_pointconv_aggregate(const float* F, const float* Wt, const float* dens, int Q, int K, int C, int W, float* E, spgan_stream_t s);
int spgan_pointconv_aggregate_bwd(const float* dE, const float* F, const float* Wt, const float* dens, int Q, int K, int C, int W, float* dF,
                                  float* dWt, float* ddens, spgan_stream_t s);
/* Max-aggregation edge convolution (Generation/modules.py:779-796).  PQ [M, >= 2F] = [P | Q] with P = Wd x,
 * Q = (Wc - Wd) x + b; the pre-norm value of edge (i, j) is Q[i] + P[idx[i,j]]; idx int32 [M,k] global rows, 1 <= k <= 127.  No [M*k, F]
 * tensor is read or written.  Deterministic: fixed summation orders, no float atomics.
 *   spgan_edge_max_gather:    train (scale == NULL): pmax / pmin [M,F] = max / min over j of P[idx[i,j]], rmax / rmin [M,F] their ranks j
 *                             (first rank on an exact tie), partials [ceil(M / tile_points)][F][2] = (sum, centred M2)
 *                             of the M*k edge values (finalize-mode-0 records with tile_rows = tile_points * k; shift / out / sel NULL).
 *                             eval (scale, shift given; the four train outputs NULL, partials optional): out and sel of spgan_edge_max_finish
 *                             in the same pass.
 *   spgan_edge_max_finish:    out[i,c] = relu(scale*(Q + (scale >= 0 ? pmax : pmin)) + shift); sel = the rank of the chosen neighbour, bit 7 set
 *                             where the ReLU clipped.
 *   spgan_edge_max_bwd_point: g [M,F] is overwritten with r = g * 1[out > 0]; partials [ceil(M / tile_points)][F][2] = plain sums
 *                             (sum r, sum r * xhat(i, sel, c)), xhat = (Q + P[sel] - mean) * invstd  (finalize mode 1, tile_rows = tile_points).
 *   spgan_edge_max_bwd_graph: dPQ [M, ldd >= 2F] = [dP | dQ] over the in-edge lists of spgan_csr_build.  sums = [sum r | sum r*xhat] (2F): the
 *                             train-mode BatchNorm terms (idx, mean, invstd required; sum_j P[idx[m,j]] is gathered again); sums == NULL: eval mode, dQ = scale*r and
 *                             dP[m] = scale * sum of r over the in-edges whose rank was selected. */
int spgan_edge_max_tile_points(void);
int spgan_edge_max_gather(const float* PQ, int ld, const int32_t* idx, int M, int k, int F, float* pmax, float* pmin, uint8_t* rmax,
                          uint8_t* rmin, float* partials, const float* scale, const float* shift, float* out, uint8_t* sel,
                          spgan_stream_t s);
int spgan_edge_max_finish(const float* PQ, int ld, const float* pmax, const float* pmin, const uint8_t* rmax, const uint8_t* rmin,
                          const float* scale, const float* shift, int M, int F, float* out, uint8_t* sel, spgan_stream_t s);
int spgan_edge_max_bwd_point(float* g, const uint8_t* sel, const float* PQ, int ld, const int32_t* idx, int M, int k, int F, const float* mean,
                             const float* invstd, float* partials, spgan_stream_t s);
int spgan_edge_max_bwd_graph(const float* r, const uint8_t* sel, const float* PQ, int ld, const int32_t* rowptr, const int32_t* src,
                             const int32_t* idx, int M, int k, int F, const float* scale, const float* mean, const float* invstd,
                             const float* sums, float* dPQ, int ldd, spgan_stream_t s);
/* The second derivative of the max-aggregation edge convolution through dx: v is the cotangent of dx, point-major,
 * VPQ [M, ldv >= 2F] = [VP | VQ] = v Wst^T (no bias); the edge value of v is t(i,j) = VQ[i] + VP[idx[i,j]], gathered exactly like the pre-norm
 * value z.  r, sel, PQ, idx: as in the first backward (r = g * 1[out > 0]).  Same determinism: fixed summation orders, no float atomics.
 *   spgan_edge_max_dbl_point: two sets of plain-sum records [ceil(M / tile_points)][F][2] (finalize mode 1, tile_rows = tile_points):
 *                             partials_t = (T1, T2) = (sum_e t_e, sum_e t_e * xhat_e) over the point's own k edges -- train mode; NULL with
 *                             mean, invstd NULL in eval mode, where the statistics are constants and no edge sum is needed --, and
 *                             partials_s = (S, 0) = sum_i r_i * t(i, sel).
 *   spgan_edge_max_dbl_graph: ghat [M,F], the cotangent of the incoming cotangent g, and, in train mode, PQbar [M, ldb >= 2F] = [Pbar | Qbar],
 *                             the cotangent of PQ, over the in-edge lists of spgan_csr_build.  sums = [s1 | s2] of the first backward,
 *                             dsums = [T1 | T2 | S] (3F): train mode (mean, invstd, rowptr, src, PQbar required).  Both NULL: eval mode,
 *                             ghat = 1[out > 0] * scale * t(i, sel) and nothing else (rowptr, src, PQbar NULL). */
int spgan_edge_max_dbl_point(const float* r, const uint8_t* sel, const float* PQ, int ld, const float* VPQ, int ldv, const int32_t* idx, int M,
                             int k, int F, const float* mean, const float* invstd, float* partials_t, float* partials_s, spgan_stream_t s);
int spgan_edge_max_dbl_graph(const float* r, const uint8_t* sel, const float* PQ, int ld, const float* VPQ, int ldv, const int32_t* rowptr,
                             const int32_t* src, const int32_t* idx, int M, int k, int F, const float* scale, const float* mean,
                             const float* invstd, const float* sums, const float* dsums, float* ghat, float* PQbar, int ldb, spgan_stream_t s);
/* Rank-window edge convolution (csrc/edge_window.hip): the [1,w] Conv2d layers of upsample_edgeConv (Generation/modules.py:799-845) over
 * get_edge_features(x), as fp32 MFMA products over gathered neighbour rows.  x [M, ldx >= C] point-major, idx int32 [M,k] global rows
 * (a row outside [0,M) counts as the point itself: a zero difference), 1 <= w <= k <= 28, T = k - w + 1 window positions per point,
 * d(i,j) = x[idx[i,j]] - x[i].  Deterministic: fixed summation orders, no float atomics.
 *   spgan_edge_window_gemm:    Y[(i*T + t), o] = sum_{r<w, c<C} W[o, r*C + c] * d(i,t+r,c) + rowadd[i,o] + add2[(i*T + t), o]   (addends optional);
 *                              W [O, ldw >= w*C] = the difference half of the conv weight, tap-major.  partials (optional)
 *                              [ceil(M / tile_points(k,T))][O][2] = (sum, centred M2) of Y's columns: finalize-mode-0 records with
 *                              tile_rows = tile_points * T (spgan_colstats_finalize_bn).
 *   spgan_edge_window_wgrad:   dW[o, r*C + c] = sum_{i,t} G[(i*T + t), o] * d(i,t+r,c)   (dW [O, lddw >= w*C]); ws >= spgan_edge_window_wgrad_ws_bytes:
 *                              partial sums per point range, reduced in ascending range order.
 *   spgan_edge_window_dgrad:   S[i,j,c] (+)= sum_{t+r=j} sum_o G[(i*T + t), o] * Wt[r*C + c, o]   (Wt [w*C, ldwt >= O] = W transposed; S [M,k,C]
 *                              contiguous; accumulate != 0 adds to S).
 *   spgan_edge_window_scatter: dx[m,c] = add_a[m,c] + add_b[m,c] - sum_j S[m,j,c] + sum_{e in in(m)} S[e,c] over the in-edge lists of
 *                              spgan_csr_build (ascending edge ids); addends optional. */
int spgan_edge_window_tile_points(int k, int T);
int spgan_edge_window_gemm(const float* x, int ldx, const int32_t* idx, int M, int k, int C, const float* W, int ldw, int O, int w,
                           const float* rowadd, int ld_rowadd, const float* add2, int ld_add2, float* Y, int ldy, float* partials,
                           spgan_stream_t s);
size_t spgan_edge_window_wgrad_ws_bytes(int M, int k, int C, int O, int w);
int spgan_edge_window_wgrad(const float* x, int ldx, const int32_t* idx, int M, int k, int C, const float* G, int ldg, int O, int w, float* dW,
                            int lddw, float* ws, size_t ws_bytes, spgan_stream_t s);
int spgan_edge_window_dgrad(const float* G, int ldg, const float* Wt, int ldwt, int M, int k, int C, int O, int w, float* S, int accumulate,
                            spgan_stream_t s);
int spgan_edge_window_scatter(const float* S, const int32_t* rowptr, const int32_t* src, int M, int k, int C, const float* add_a, int ld_a,
                              const float* add_b, int ld_b, float* dx, int lddx, spgan_stream_t s);
/* Full-rank edge convolution (csrc/edge_rank.hip): the core of deform_edgeConv_simple / deform_edgeConv_first (Generation/modules.py:1394-1466),
 * Conv2d(2Fin -> F1, 1x1) + BatchNorm2d + LeakyReLU over the edge features, then Conv2d(F1 -> O, [1,k]) over the neighbour ranks.
 * PQ [M, ld >= 2F1] = [P | Q] is the per-point GEMM's result (as for the max-aggregation layer), idx [M,k] global rows, and
 * h(i,r,c) = lrelu(scale1[c] * (Q[i,c] + P[idx[i,r],c]) + shift1[c], slope) is formed inside the kernels, never stored.  1 <= k <= 32, any M, F1, O.
 *   spgan_edge_rank_gemm:    Y[i,o] = b2[o] + sum_{r<k, c<F1} W2i[o, r*F1 + c] * h(i,r,c)   (W2i [O, ldw >= k*F1] tap-major; b2 optional);
 *                            partials != NULL: [ceil(M / tile_points)][O][2] (sum, centred M2) records of Y's columns for
 *                            spgan_colstats_finalize_bn (tile_rows = spgan_edge_rank_tile_points(k); 0: k unsupported).
 *   spgan_edge_rank_wgrad:   dW2i[o, r*F1 + c] = sum_i dY[i,o] * h(i,r,c)   (dW2i [O, lddw >= k*F1]); ws >= spgan_edge_rank_wgrad_ws_bytes:
 *                            the point ranges' partial products, summed in range order.
 *   spgan_edge_rank_dgrad:   dA[i,r,c] = lrelu'(a(i,r,c)) * sum_o dY[i,o] * W2t[r*F1 + c, o]   (W2t [k*F1, ldwt >= O] = W2i transposed; dA [M,k,F1]
 *                            contiguous; a = the BatchNorm output, its sign recomputed) and partials [ceil(M / tile_points)][F1][2] = plain sums
 *                            (sum dA, sum dA * zhat), zhat = (Q + P - mean1) * invstd1, over the tile's points and all ranks (finalize mode 1).
 *   spgan_edge_rank_scatter: dPQ [M, ldd >= 2F1] = [dP | dQ]: dz = scale1 * (dA - sums[c] / E - zhat * sums[F1 + c] / E), E = M*k (train: PQ, idx,
 *                            mean1, invstd1 required) or scale1 * dA (sums == NULL: eval); dQ[i] = sum_r dz(i,r), dP[j] = sum of dz over the
 *                            in-edge list of j (spgan_csr_build, ascending edge ids; in-degree 0: zeros). */
int spgan_edge_rank_tile_points(int k);
int spgan_edge_rank_gemm(const float* PQ, int ld, const int32_t* idx, int M, int k, int F1, const float* scale1, const float* shift1, float slope,
                         const float* W2i, int ldw, const float* b2, int O, float* Y, int ldy, float* partials, spgan_stream_t s);
size_t spgan_edge_rank_wgrad_ws_bytes(int M, int k, int F1, int O);
int spgan_edge_rank_wgrad(const float* PQ, int ld, const int32_t* idx, int M, int k, int F1, const float* scale1, const float* shift1, float slope,
                          const float* dY, int ldg, int O, float* dW2i, int lddw, float* ws, size_t ws_bytes, spgan_stream_t s);
int spgan_edge_rank_dgrad(const float* dY, int ldg, const float* W2t, int ldwt, const float* PQ, int ld, const int32_t* idx, int M, int k, int F1,
                          int O, const float* scale1, const float* shift1, const float* mean1, const float* invstd1, float slope, float* dA,
                          float* partials, spgan_stream_t s);
int spgan_edge_rank_scatter(const float* dA, const int32_t* rowptr, const int32_t* src, const float* PQ, int ld, const int32_t* idx, int M, int k,
                            int F1, const float* scale1, const float* mean1, const float* invstd1, const float* sums, float* dPQ, int ldd,
                            spgan_stream_t s);
/* Weighted full-rank edge convolution (csrc/edge_rank.hip): the core of deform_edgeConv_feat (Generation/modules.py:1543-1599).  The activated
 * edge tensor h of the layer above is multiplied by a per-edge, per-channel weight s before the [1,k] convolution:
 *   a3(i,r,c) = lrelu(scale3[c] * z3[i,r,c] + shift3[c], slope),   z3 [M,k,F1] contiguous = the stored pre-norm output of the weight MLP;
 *   s = exp(a3 - wmax[i,c]) * wrs[i,c]  (the softmax over the k ranks; wmax, wrs [M,F1] from spgan_edge_weight_norm), or s = a3 when
 *   wmax == wrs == NULL (softmax=False).  h, s and h*s are formed inside the kernels, never stored.  1 <= k <= 32, any M, F1, O.
 *   spgan_edge_weight_gather: Z[(i*k + r), c] = Q[i,c] + P[idx[i,r],c]   (Z [M*k, F] contiguous: the pre-norm rows of a narrow edge layer).
 *   spgan_edge_weight_norm:   wmax[i,c] = max_r a3(i,r,c), wrs[i,c] = 1 / sum_r exp(a3(i,r,c) - wmax[i,c]), ranks in ascending order.
 *   spgan_edge_weight_gemm:   spgan_edge_rank_gemm with h * s in place of h (same tiling, partials and finalize).
 *   spgan_edge_weight_wgrad:  spgan_edge_rank_wgrad with h * s in place of h (workspace: spgan_edge_rank_wgrad_ws_bytes).
 *   spgan_edge_weight_dgrad:  dm = dY W2i per (point, rank, channel) as spgan_edge_rank_dgrad forms it, then
 *                               dU[i,r,c] = lrelu'(a_h) * dm * s                        partials_u: (sum dU, sum dU * uhat), uhat = (Q + P - mean1) * invstd1
 *                               G3[i,r,c] = lrelu'(a3) * s * (dm*h - sum_r' dm*h*s)     partials_3: (sum G3, sum G3 * z3hat), z3hat = (z3 - mean3) * invstd3
 *                             (softmax=False: G3 = lrelu'(a3) * dm*h).  dU, G3 [M,k,F1] contiguous and distinct; both partials
 *                             [ceil(M / tile_points)][F1][2] plain sums (finalize mode 1).  No float atomics: results repeat bit for bit. */
int spgan_edge_weight_gather(const float* PQ, int ld, const int32_t* idx, int M, int k, int F, float* Z, spgan_stream_t s);
int spgan_edge_weight_norm(const float* z3, int M, int k, int F1, const float* scale3, const float* shift3, float slope, float* wmax, float* wrs,
                           spgan_stream_t s);
int spgan_edge_weight_gemm(const float* PQ, int ld, const int32_t* idx, int M, int k, int F1, const float* scale1, const float* shift1, float slope,
                           const float* z3, const float* scale3, const float* shift3, const float* wmax, const float* wrs, const float* W2i, int ldw,
                           const float* b2, int O, float* Y, int ldy, float* partials, spgan_stream_t s);
int spgan_edge_weight_wgrad(const float* PQ, int ld, const int32_t* idx, int M, int k, int F1, const float* scale1, const float* shift1, float slope,
                            const float* z3, const float* scale3, const float* shift3, const float* wmax, const float* wrs, const float* dY, int ldg,
                            int O, float* dW2i, int lddw, float* ws, size_t ws_bytes, spgan_stream_t s);
int spgan_edge_weight_dgrad(const float* dY, int ldg, const float* W2t, int ldwt, const float* PQ, int ld, const int32_t* idx, int M, int k, int F1,
                            int O, const float* scale1, const float* shift1, const float* mean1, const float* invstd1, float slope, const float* z3,
                            const float* scale3, const float* shift3, const float* mean3, const float* invstd3, const float* wmax, const float* wrs,
                            float* dU, float* G3, float* partials_u, float* partials_3, spgan_stream_t s);
/* Coordinate-guided full-rank edge convolution (csrc/edge_rank.hip): the two passes deform_edgeConv (Generation/modules.py:1468-1540) adds
 * to the weighted layer above.  Its weight MLP reads the product of two activated branches over the same graph, each a per-point GEMM
 * PQx [M, ldx >= 2F] = [P | Q] with the affine (scale_x, shift_x) of its BatchNorm: a_x(i,r,c) = lrelu(scale_x[c] * (Qx[i,c] + Px[idx[i,r],c]) + shift_x[c]).
 *   spgan_edge_weight_gather2: W0[(i*k + r), c] = a_a * a_b   (W0 [M*k, F] contiguous).
 *   spgan_edge_weight_split:   GA[i,r,c] = lrelu'(pre_a) * dW0 * a_b,  GB[i,r,c] = lrelu'(pre_b) * dW0 * a_a   (dW0, GA, GB [M,k,F] contiguous,
 *                              GA != GB); partials_x [ceil(M / tile_points)][F][2] = (sum Gx, sum Gx * zhat_x), zhat_x = (Qx + Px - mean_x) *
 *                              invstd_x, plain sums (finalize mode 1; spgan_edge_rank_scatter takes the reduced sums).  Both passes form a_x
 *                              with one device function: the backward multiplies with the forward's bits.  No float atomics.
 * 1 <= k <= 32, any M and F; rows of F % 4 == 0 floats on 16-byte aligned operands move as 16-byte pieces. */
int spgan_edge_weight_gather2(const float* PQa, int lda, const float* PQb, int ldb, const int32_t* idx, int M, int k, int F, const float* scale_a,
                              const float* shift_a, const float* scale_b, const float* shift_b, float slope, float* W0, spgan_stream_t s);
int spgan_edge_weight_split(const float* dW0, const float* PQa, int lda, const float* PQb, int ldb, const int32_t* idx, int M, int k, int F,
                            const float* scale_a, const float* shift_a, const float* mean_a, const float* invstd_a, const float* scale_b,
                            const float* shift_b, const float* mean_b, const float* invstd_b, float slope, float* GA, float* GB, float* partials_a,
                            float* partials_b, spgan_stream_t s);
/* Bilateral upsampling edge convolution (csrc/edge_rank.hip): the core of bilateral_upsample_edgeConv (Generation/modules.py:847-925).  The
 * weighted product above with h read from a stored tensor instead of gathered rows: U [M,k,F1] contiguous holds the pre-norm value of
 * (point i, rank r, channel c) and the BatchNorm affine alternates with the rank's parity,
 *   h(i,r,c) = lrelu(scale1[(r&1)*F1 + c] * U[i,r,c] + shift1[(r&1)*F1 + c], slope)      (scale1, shift1, mean1, invstd1: [2*F1]);
 * z3, scale3, shift3, wmax, wrs and s as in the weighted layer.  k even, 2 <= k <= 28, any M, F1, O; rows of F1 % 4 == 0 floats on 16-byte
 * aligned operands are staged as 16-byte pieces, everything else by scalars.
 *   spgan_edge_stored_gemm:   spgan_edge_weight_gemm over the stored h (same tiling, partials and finalize; b2 and partials may be NULL).
 *   spgan_edge_stored_wgrad:  spgan_edge_weight_wgrad over the stored h (workspace: spgan_edge_rank_wgrad_ws_bytes).
 *   spgan_edge_stored_dgrad:  spgan_edge_weight_dgrad over the stored h: dU[i,r,c] = lrelu'(a_h) * dm * s with uhat = (U - mean1) * invstd1 and
 *                             partials_u [ceil(M / tile_points)][2*F1][2], one column per (rank parity, channel); G3 and partials_3 as there.
 *                             dU, G3 and U are distinct.  No float atomics: results repeat bit for bit. */
int spgan_edge_stored_gemm(const float* U, int M, int k, int F1, const float* scale1, const float* shift1, float slope, const float* z3,
                           const float* scale3, const float* shift3, const float* wmax, const float* wrs, const float* W2i, int ldw, const float* b2,
                           int O, float* Y, int ldy, float* partials, spgan_stream_t s);
int spgan_edge_stored_wgrad(const float* U, int M, int k, int F1, const float* scale1, const float* shift1, float slope, const float* z3,
                            const float* scale3, const float* shift3, const float* wmax, const float* wrs, const float* dY, int ldg, int O,
                            float* dW2i, int lddw, float* ws, size_t ws_bytes, spgan_stream_t s);
int spgan_edge_stored_dgrad(const float* dY, int ldg, const float* W2t, int ldwt, const float* U, int M, int k, int F1, int O, const float* scale1,
                            const float* shift1, const float* mean1, const float* invstd1, float slope, const float* z3, const float* scale3,
                            const float* shift3, const float* mean3, const float* invstd3, const float* wmax, const float* wrs, float* dU,
                            float* G3, float* partials_u, float* partials_3, spgan_stream_t s);
/* Block tail (csrc/block_tail.hip): what the bilateral / deform blocks (Generation/modules.py:928-1391) put behind their edge convolution --
 * BatchNorm1d + LeakyReLU over the layer's output and the concatenation with the broadcast global vectors -- as one pass.  All tensors are
 * float32, channel-major [B, channels, L] contiguous; Y [B,C,L] is the layer's pre-norm output, a "row" the L floats of one (b, c).
 *   a(b,c,n)    = lrelu(scale[c] * Y[b,c,n] + shift[c], slope)
 *   gact(b,c,n) = (dout_x[b, Cs+c, n] + dout_g[b, Cg+c, n] + extra[b,c,n]) * lrelu'(scale[c] * Y[b,c,n] + shift[c]);  each of dout_x
 *                 [B,Cs+C,L], dout_g [B,Cg+C,L], extra [B,C,L] may be NULL (= zeros, never read).
 *   spgan_cm_stats:              partials [B][C][2] = (sum, M2 about the row's own mean) of every row of Y: the records of
 *                                spgan_colstats_finalize_bn with tiles = B, G = B*L, tile_rows = L.
 *   spgan_block_tail_fwd:        out_x [B,Cs+C,L]: channels [0,Cs) = xs[b,c] broadcast over L (xs [B,Cs]), channels Cs + c = a;  out_g
 *                                [B,Cg+C,L] likewise with g [B,Cg].  Y is read once.  out_x or out_g may be NULL (not both), Cs / Cg may be 0.
 *   spgan_block_tail_bwd_reduce: partials [B][C][2] = plain sums (sum gact, sum gact * yhat) of every row, yhat = (Y - mean[c]) * invstd[c]
 *                                (finalize mode 1, tile_rows = L), and in the same launch dxs[b,c] = sum_n dout_x[b,c,n] (c < Cs), dg[b,c] =
 *                                sum_n dout_g[b,c,n] (c < Cg); dxs / dg NULL: not wanted; zeros where their cotangent is NULL.
 *   spgan_block_tail_bwd_apply:  dY = gamma * invstd * (gact - sums[c] / count - yhat * sums[C+c] / count) (sums [2C] != NULL: train mode, needs
 *                                mean, invstd; gamma NULL = 1) or dY = scale * gact (sums == NULL: eval mode).  gact is recomputed by the
 *                                device function of the reduce pass: the masked gradient is never stored.  dY is distinct from the inputs.
 * Any B, C, Cs, Cg and L >= 1: one wave walks one row, the grid strides over the rows; rows of L % 4 == 0 floats on 16-byte aligned tensors
 * move as 16-byte pieces, everything else by scalars (one choice per launch).  No float atomics: results repeat bit for bit. */
int spgan_cm_stats(const float* Y, int B, int C, int L, float* partials, spgan_stream_t s);
int spgan_block_tail_fwd(const float* Y, const float* xs, const float* g, int B, int C, int L, int Cs, int Cg, const float* scale,
                         const float* shift, float slope, float* out_x, float* out_g, spgan_stream_t s);
int spgan_block_tail_bwd_reduce(const float* Y, const float* dout_x, const float* dout_g, const float* extra, int B, int C, int L, int Cs,
                                int Cg, const float* scale, const float* shift, float slope, const float* mean, const float* invstd,
                                float* partials, float* dxs, float* dg, spgan_stream_t s);
int spgan_block_tail_bwd_apply(const float* Y, const float* dout_x, const float* dout_g, const float* extra, int B, int C, int L, int Cs,
                               int Cg, const float* scale, const float* shift, float slope, const float* mean, const float* invstd,
                               const float* gamma, const float* sums, float count, float* dY, spgan_stream_t s);
/* Per-channel scalar algebra of the double backward, one launch each:
 *   coeffs out4C = [dgammaA | sbarA | xsum0 | xsum1];  phaseb: sums2C = [xsum0+gamma*s0 | xsum1+gamma*s1+invstd*sbarA], dgamma = dgammaA+s1 */
int spgan_bn_dbl_coeffs(const float* U0, const float* U1, const float* Ugz, const float* S0, const float* S1, const float* gamma,
                        const float* invstd, int C, int count, float* out4C, spgan_stream_t s);
int spgan_bn_dbl_phaseb(const float* coeffs4C, const float* gamma, const float* invstd, const float* s0, const float* s1, int C,
                        float* sums2C, float* dgamma, spgan_stream_t s);
/* spgan_bn_dbl_coeffs followed by spgan_bn_dbl_phaseb in one launch (same arithmetic, the [4,C] coefficient block is not stored) */
int spgan_bn_dbl_phaseb_sums(const float* U0, const float* U1, const float* Ugz, const float* S0, const float* S1, const float* gamma,
                             const float* invstd, const float* s0, const float* s1, int C, int count, float* sums2C, float* dgamma,
                             spgan_stream_t s);
/* Collapsed double backward of the layer in front of the max-pool (Discriminator.py:74-81,104): the dense [M,C]
 * tensors of the generic path are only needed as per-channel sums and at the B*C arg-max positions.
 * spgan_gather_rowdot: out[b,c] = Q[arg[b,c], :] . W[c, :]          (u = q.W^T at the arg-max rows)
 * spgan_rowdot:        out[r]   = X[r,:] . Y[r,:]
 * spgan_bn_dbl_pool:   per channel: U1, Ugz, the phase-A coefficients; t [B,C] = adjoint of the pooled gradient;
 *                      out4C = [dgamma | c1 | c2 | c3], spB [B,C]: phase B's ybar = c1*u + c2*y + c3 + scatter(spB). */
int spgan_gather_rowdot(const float* Q, int ldq, const int32_t* arg, const float* W, int ldw, int B, int C, int K, float* out, spgan_stream_t s);
/* spgan_gather_rowdot (uarg [B,C] = Q[arg[b,c],:] . W[c,:]), spgan_rowdot (quad [C] = W[c,:] . T[c,:]) and U0 [C] = W[c,:] . cq in ONE launch:
 * the three independent per-channel dot products of the collapsed double backward's phase A (Discriminator.py:77-81 behind the max-pool). */
int spgan_dbl_top_dots(const float* Q, int ldq, const int32_t* arg, const float* W, int ldw, const float* T, int ldt, const float* cq, int B, int C,
                       int K, float* uarg, float* quad, float* U0, spgan_stream_t s);
int spgan_rowdot(const float* X, int ldx, const float* Y, int ldy, int R, int K, float* out, spgan_stream_t s);
int spgan_bn_dbl_pool(const float* uarg, const float* gval, const float* yarg, const float* pooled, const float* U0, const float* quad,
                      const float* bias, const float* mean, const float* invstd, const float* gamma, const float* S0, const float* S1,
                      int B, int C, int count, float slope, float* t, float* spB, float* out4C, spgan_stream_t s);
/* Lazy-operand form of the BatchNorm backward behind the max-pool: dy = alpha[c]*y + beta[c] + (argmax hit ? cg[b,c] : 0) */
int spgan_sparse_bn_prep(const float* gval, const float* mean, const float* invstd, const float* gamma, const float* sums, int B,
                         int C, int count, float* alpha, float* beta, float* cg, spgan_stream_t s);
/* out[m,c] = a[m,c] + gamma[c]*b[m,c] */
int spgan_col_scale_add(const float* a, const float* b, const float* gamma, int M, int C, float* out, spgan_stream_t s);
/* dst[t][i] += src[t][i], t < count <= SPGAN_MULTI_MAX, in ONE launch (gradient accumulation into the flat buffer) */
#define SPGAN_MULTI_MAX 64
typedef struct spgan_multi_add_args {
  int count;
  float* dst[SPGAN_MULTI_MAX];
  const float* src[SPGAN_MULTI_MAX];
  int n[SPGAN_MULTI_MAX];
} spgan_multi_add_args;
int spgan_multi_add(const spgan_multi_add_args* a, spgan_stream_t s);
/* dst[t] = ((dst[t] + src[0][t]) + src[1][t]) + src[2][t] with nsrc[t] in 1..3 sources: the per-pass parameter gradients of a grouped backward
 * accumulated in one launch, element for element the sums of nsrc successive spgan_multi_add calls. */
#define SPGAN_MULTI_ADDN_MAX 32
typedef struct spgan_multi_addn_args {
  int count;
  float* dst[SPGAN_MULTI_ADDN_MAX];
  const float* src[3][SPGAN_MULTI_ADDN_MAX];
  int nsrc[SPGAN_MULTI_ADDN_MAX];
  int n[SPGAN_MULTI_ADDN_MAX];
} spgan_multi_addn_args;
int spgan_multi_addn(const spgan_multi_addn_args* a, spgan_stream_t s);
/* The same for pairs that are 3-D strided views of one shape [n0, n1, n2] (n = n0*n1*n2; strides in elements):
 * dst[i0*ds[0] + i1*ds[1] + i2*ds[2]] += src[i0*ss[0] + i1*ss[1] + i2*ss[2]].  A permuted source (the conv_out weight gradient is computed
 * as [F,k,F] and accumulated into [F,F,1,k]) or a column block of the destination; n1 = n2 = 1 is the plain contiguous pair. */
typedef struct spgan_multi_add3_args {
  int count;
  float* dst[SPGAN_MULTI_MAX];
  const float* src[SPGAN_MULTI_MAX];
  int n[SPGAN_MULTI_MAX], n1[SPGAN_MULTI_MAX], n2[SPGAN_MULTI_MAX];
  long ds[3][SPGAN_MULTI_MAX], ss[3][SPGAN_MULTI_MAX];
} spgan_multi_add3_args;
int spgan_multi_add3(const spgan_multi_add3_args* a, spgan_stream_t s);
/* The local step of a ONE-HOP all-reduce of a flat gradient buffer over W ranks (on a fully connected xGMI node an
 * all-to-all is one hop per pair, so reduce-scatter = all-to-all + this sum, all-gather = one more hop; 2 hops instead of a ring's
 * 2(W-1) steps for the 2.3 / 3.9 MB latency-bound messages).  recv [parts, n] holds this rank's chunk as received from every rank
 * (row j from rank j); out[i] = sum_j recv[j, i] in ascending j -- every chunk is summed exactly once, on one rank, in a fixed order, so
 * all ranks end up with bit-identical sums.  recv and out 16-byte aligned.  The exchanges themselves are torch.distributed / RCCL
 * (spgan.parallel.DataParallel(collective="one_hop")). */
int spgan_reduce_chunks(const float* recv, int parts, size_t n, float* out, spgan_stream_t s);
/* ---- allreduce_flat: the data-parallel exchange of a train step -- what replaces nn.DataParallel's per-call
 * scatter / parameter broadcast / gather (Generation/model.py:79-84): ONE all-reduce (sum, in place) of a network's flat gradient
 * buffer over RCCL, enqueued on the caller's stream (capturable into a hipGraph together with the kernels around it).  RCCL is
 * dlopen'ed at first use (no link-time dependency).  Rendezvous: rank 0 calls spgan_comm_unique_id and hands the 128 bytes to
 * every rank through the host program's own channel; then every rank calls spgan_comm_init with the HIP device it trains on
 * current.  spgan_comm_available() == 0 (or status SPGAN_ECOMM) when librccl cannot be loaded; spgan_comm_last_error() is the
 * ncclResult_t of the last failing call.  The caller divides by the world size (spgan_adam_step's grad_scale). */
int spgan_comm_available(void);
int spgan_comm_last_error(void* comm);   /* RCCL code of the last failed call ON THIS communicator; comm == NULL: of the calling thread's last failed spgan_comm_unique_id / spgan_comm_init */
int spgan_comm_unique_id(void* id128);
int spgan_comm_init(const void* id128, int rank, int world, void** comm);
int spgan_comm_world(void* comm);
int spgan_allreduce_flat(void* comm, float* buf, size_t n, spgan_stream_t s);
int spgan_comm_destroy(void* comm);
/* dst[t][i] = src[t][i] for the same argument block: up to SPGAN_MULTI_MAX device-to-device copies in ONE launch. */
int spgan_multi_copy(const spgan_multi_add_args* a, spgan_stream_t s);
/* Finish up to SPGAN_MULTI_MAX deferred spgan_gemm_tn products in one launch: C[e] = beta[e]*C[e] + fixed-order sum of the
 * splits[e] = spgan_gemm_tn_splits(M,Na,Nb) partials [splits, Na, Nb] in ws[e].  block_start[e] = sum_{f<e}
 * spgan_splitk_reduce_blocks(splits[f], Na[f], Nb[f]) (64 outputs per workgroup, or 4 -- one wave each -- for many partials of few outputs). */
typedef struct spgan_splitk_multi_args {
  int count;
  const float* ws[SPGAN_MULTI_MAX];
  float* C[SPGAN_MULTI_MAX];
  int splits[SPGAN_MULTI_MAX], Na[SPGAN_MULTI_MAX], Nb[SPGAN_MULTI_MAX], ldc[SPGAN_MULTI_MAX];
  float beta[SPGAN_MULTI_MAX];
  int block_start[SPGAN_MULTI_MAX + 1];
} spgan_splitk_multi_args;
/* dst[e] (cols x rows, contiguous) = src[e]^T (rows x cols, row stride ld) for count <= SPGAN_MULTI_MAX matrices in ONE launch: the
 * transposed weights read by the input-gradient GEMMs, refreshed once per optimiser step.  tile_start[e] = sum_{f<e} of
 * ceil(rows/32)*ceil(cols/32). */
typedef struct spgan_multi_transpose_args {
  int count;
  const float* src[SPGAN_MULTI_MAX];
  float* dst[SPGAN_MULTI_MAX];
  int rows[SPGAN_MULTI_MAX], cols[SPGAN_MULTI_MAX], ld[SPGAN_MULTI_MAX];
  int tile_start[SPGAN_MULTI_MAX + 1];
} spgan_multi_transpose_args;
int spgan_multi_transpose(const spgan_multi_transpose_args* a, spgan_stream_t s);
int spgan_gemm_tn_splits(int M, int Na, int Nb);
int spgan_splitk_reduce_blocks(int splits, int Na, int Nb);
int spgan_splitk_reduce_multi(const spgan_splitk_multi_args* a, spgan_stream_t s);
/* y = a*x + b*y */
int spgan_axpby(float a, const float* x, float b, float* y, size_t n, spgan_stream_t s);
/* torch.optim.Adam step on a flat buffer (Generation/model.py:94-97: lr 1e-4, betas (0.5,0.99)); g is scaled by grad_scale first */
int spgan_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps, int step,
                    float grad_scale, spgan_stream_t s);
/* The same update with its step-dependent state in device memory: state[0] = int step count (advanced by this call), state[1..2] = its
 * bias corrections, state[3] = a multiplier on `lr` (1 = lr as passed; the StepLR schedule of Generation/model.py:99-110,309-312 writes
 * it): no host value changes from one step to the next, so a captured hipGraph of the train step replays it.  state: 4 floats.
 * zero_grad != 0: g is zeroed after it was read -- the optimizer.zero_grad() of the next iteration (model.py:243,268) without a launch. */
int spgan_adam_step_dev(float* p, float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                        float* state, float grad_scale, int zero_grad, spgan_stream_t s);
/* Generator weight EMA (Common/network_utils.py:97-108): e <- a*e + (1-a)*p over a flat shadow buffer e of the same layout as p.
 * a after the t-th update: ema_warmup != 0 -> min(1 - 1/t, ema_rate) (exp_mov_avg with global_step = t-1; t = 1 copies p exactly),
 * ema_warmup == 0 -> ema_rate (accumulate).  a and 1-a are evaluated in double (ema_rate is a double, as the reference's Python scalar)
 * and rounded once; the three entry points below share that formula and the per-element update, so for the same t, p and e they produce
 * bit-equal shadows.  0 <= ema_rate <= 1.
 * spgan_adam_ema_step_dev: spgan_adam_step_dev (same state, same zero_grad; p, m, v, g bit-identical to it, still two launches) with
 * the EMA applied to the updated p inside the update launch; t = state[0] after this call's advance.
 * spgan_adam_ema_step: the host-step twin of spgan_adam_step (p, m, v bit-identical to it), t = step.
 * spgan_ema_update_dev: the EMA alone, for callers with their own optimiser; counter = one int32 on the device, advanced by this call
 * (t = its value afterwards), so a captured hipGraph replays it. */
int spgan_adam_ema_step_dev(float* p, float* g, float* m, float* v, float* e, size_t n, float lr, float beta1, float beta2, float eps,
                            float* state, float grad_scale, int zero_grad, double ema_rate, int ema_warmup, spgan_stream_t s);
int spgan_adam_ema_step(float* p, const float* g, float* m, float* v, float* e, size_t n, float lr, float beta1, float beta2, float eps,
                        int step, float grad_scale, double ema_rate, int ema_warmup, spgan_stream_t s);
int spgan_ema_update_dev(float* e, const float* p, size_t n, double ema_rate, int ema_warmup, int* counter, spgan_stream_t s);

/* Measurement plumbing (bench.py's `roofline` entry): device timestamps that survive a hipGraph capture, where HIP events
 * cannot be queried.  spgan_stamp_begin stores the constant-rate wall clock in *slot; spgan_stamp_end adds (now - *slot) to acc2[0] and 1
 * to acc2[1]; launched on the kernel's stream directly in front of / behind it.  spgan_wall_clock_khz: ticks per millisecond (0: unknown). */
int spgan_stamp_begin(uint64_t* slot, spgan_stream_t s);
int spgan_stamp_end(const uint64_t* slot, uint64_t* acc2, spgan_stream_t s);
int spgan_wall_clock_khz(void);

/* ------------------------------------------------------------------------------------------
 * Evaluation metrics: Chamfer distance.
 * ---------------------------------------------------------------------------------------- */
/* dist[b,i] = min_j |xyz1[b,i] - xyz2[b,j]|^2, idx[b,i] = the first j attaining it (index into xyz2[b]): one direction of
 * chamfer.forward (metrics/CD_EMD/cd/chamferdist/chamfer.cu:12-113, ChamferDistance.py:13-31); xyz1 [B,N,3], xyz2 [B,M,3]. */
int spgan_nn_distance(const float* xyz1, const float* xyz2, int B, int N, int M, float* dist, int32_t* idx, spgan_stream_t s);
/* grad_a[b,i] = 2*ga[b,i]*(xa_i - xb[idxa[b,i]]) + sum_{j: idxb[b,j]==i} 2*gb[b,j]*(xa_i - xb_j): d/d(xa) of
 * sum(ga*dist_a) + sum(gb*dist_b) (chamfer.cu:155-195, gather form: deterministic, no float atomics).  Call once per cloud. */
int spgan_chamfer_bwd(const float* xa, const float* xb, int B, int Na, int Nb, const float* ga, const int32_t* idxa, const float* gb,
                      const int32_t* idxb, float* grad_a, spgan_stream_t s);
/* out[s,r] = mean_i min_j |A[s,i]-Bc[r,j]|^2 + mean_j min_i |A[s,i]-Bc[r,j]|^2 for every pair of clouds A[s] ([S,N,3]) and
 * Bc[r] ([R,M,3]): the all-pairs Chamfer matrix behind MMD-CD / COV-CD / 1-NNA-CD (metrics/evaluation_metrics.py:89-126). */
int spgan_chamfer_pairs(const float* A, const float* Bc, int S, int R, int N, int M, float* out, spgan_stream_t s);
/* Occupancy-grid statistics of the JSD metric (metrics/evaluation_metrics.py:247-283, entropy_of_occupancy_grid): cell [S,N] holds
 * the nearest grid cell of every point (spgan_nn_distance against the grid); counters[g] += points in cell g over all clouds,
 * bernoulli[g] += clouds with at least one point in g.  Accumulates: the caller zeroes both int32 [G] arrays.  G <= 524288. */
int spgan_occupancy_counts(const int32_t* cell, int S, int N, int G, int32_t* counters, int32_t* bernoulli, spgan_stream_t s);
/* Minimum matching distance / coverage over a distance matrix dist [S,R] between S sample clouds and R reference clouds
 * (metrics/evaluation_metrics.py:161-173, lgan_mmd_cov): out3 = [mean over references of their closest sample's distance,
 * fraction of references that are the closest reference of some sample (first one on ties), mean over samples of their closest
 * reference's distance].  ws: (S + 2R) floats of scratch.  Fixed-order sums. */
int spgan_mmd_cov(const float* dist, int S, int R, float* out3, float* ws, spgan_stream_t s);
/* Leave-one-out k-nearest-neighbour two-sample test (metrics/evaluation_metrics.py:129-158, knn): Mxx [n0,n0], Mxy [n0,n1],
 * Myy [n1,n1] are the blocks of the joint distance matrix (never concatenated); every cloud is classified by the majority label of
 * its k nearest OTHER clouds (votes >= k/2 -> first set; lower index on distance ties); take_sqrt compares sqrt(|d|).
 * out9 = [tp, fp, fn, tn, precision, recall, acc_t, acc_f, acc]; pred: int32 [n0+n1] scratch (the per-cloud predictions). */
int spgan_two_sample_knn(const float* Mxx, const float* Mxy, const float* Myy, int n0, int n1, int k, int take_sqrt, float* out9,
                         int32_t* pred, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Local-shape Chamfer (Common/loss_utils.py:196-259 get_local_pair, Common/GAN_metrics.py:596-656 local_CD / pairwise_local_CD)
 * and the GAN_metrics evaluation pieces (csrc/local_cd.hip).  Every float expression there is evaluated as written, without
 * fma contraction; the fixed orders are listed at the top of that file.
 * ---------------------------------------------------------------------------------------- */
/* The K nearest points of cloud[b] ([B,N,3]) to every query[b,m] ([B,M,3]) in pointops knnquery order (ascending d^2, lower
 * index first on equal d^2, the query itself included when it is a cloud point; metrics/pointops/src/knnquery/
 * knnquery_cuda_kernel.cu:6-50), and their mean mu [B,M,3] and biased covariance cov [B,M,6] = [xx, xy, xz, yy, yz, zz]
 * (compute_mean_covariance, loss_utils.py:196-205).  idx int64 [B,M,K] may be NULL.  1 <= K <= min(32, N). */
int spgan_knn_moments(const float* query, const float* cloud, int B, int M, int N, int K, int64_t* idx, float* mu, float* cov,
                      spgan_stream_t s);
/* Slot gradients of the moments: gslot[b,m,k,:] = dmu[b,m]/K + (G + G^T)(cloud[b, idx[b,m,k]] - mu[b,m])/K, G the 3x3 form of
 * dcov [B,M,6].  Summed onto the cloud points by spgan_gather_csr + spgan_scatter_slots (the query gets no gradient). */
int spgan_moments_bwd(const int64_t* idx, const float* cloud, const float* mu, const float* dmu, const float* dcov, int B, int M, int N,
                      int K, float* gslot, spgan_stream_t s);
/* Nearest neighbour in both directions between a [B,Na,D] and b [B,Nb,D]: dist_a[b,i] = min_j d(a_i, b_j), idx_a the first j
 * attaining it; dist_b / idx_b the other way.  D = 3 or 9: plain squared distance; D = 6: the 6-entry storage of symmetric 3x3
 * matrices with the off-diagonal squared differences weighted by 2 (the 9-D distance of the full matrices).  idx_* may be NULL. */
int spgan_nn_dim(const float* a, const float* b, int B, int Na, int Nb, int D, float* dist_a, int32_t* idx_a, float* dist_b,
                 int32_t* idx_b, spgan_stream_t s);
/* out[p*ostride] = (sum_i dist_a[p,i] + sum_j dist_b[p,j]) / div for p < P (fixed-order double sums rounded once to float) */
int spgan_pair_sum(const float* dist_a, int na, const float* dist_b, int nb, int P, float div, float* out, int ostride, spgan_stream_t s);
/* grad_a = d/d(a) of gscale[0] * (sum dist_a + sum dist_b) through the argmins of spgan_nn_dim (call once per side, swapping the
 * roles; gather form, ascending order, no float atomics) */
int spgan_chamfer_dim_bwd(const float* xa, const float* xb, int B, int Na, int Nb, int D, const int32_t* idxa, const int32_t* idxb,
                          const float* gscale, float* grad_a, spgan_stream_t s);
/* out [S,R,2] = the local Chamfer terms (mean, covariance) of every pair: the K-nearest moments of sample[s]'s points in sample[s]
 * (computed once per sample) against those in ref[r], each Chamfer sum divided by N.  Pairs run in chunks inside one call.
 * ws: spgan_pairwise_local_cd_ws_bytes(S, R, N, M) bytes. */
size_t spgan_pairwise_local_cd_ws_bytes(int S, int R, int N, int M);
int spgan_pairwise_local_cd(const float* sample, const float* ref, int S, int R, int N, int M, int K, float* out, void* ws, size_t ws_bytes,
                            spgan_stream_t s);
/* GAN_metrics.KNN (GAN_metrics.py:466-482): the vote of spgan_two_sample_knn with labels -1 (first set) / +1 (second set), a tied
 * vote predicting +1.  out1[0] = fraction of clouds predicted correctly; pred: int32 [n0+n1] scratch (the +-1 predictions). */
int spgan_two_sample_knn_pm(const float* Mxx, const float* Mxy, const float* Myy, int n0, int n1, int k, int take_sqrt, float* out1,
                            int32_t* pred, spgan_stream_t s);
/* Point counts of the JSD histogram (get_voxel_occ_dist, GAN_metrics.py:411-447): counts[(i*res+j)*res+k] += number of points with
 * e_i <= x < e_{i+1}, e_j <= y < e_{j+1}, e_k <= z < e_{k+1}, e_i = -0.5 + i*(1/res) in float64; points outside are not counted.
 * Accumulates into int32 [res^3] (the caller zeroes it). */
int spgan_voxel_counts(const float* pts, long npts, int res, int32_t* counts, spgan_stream_t s);
/* out [S,R] = sum_c (a[s,c] - b[r,c])^2, or sum_c |a[s,c] - b[r,c]| with l1, for feature rows a [S,D], b [R,D]
 * (GAN_metrics.py:562-593 pairwise_simple) */
int spgan_pairwise_simple(const float* a, const float* b, int S, int R, int D, int l1, float* out, spgan_stream_t s);

/* Approximate earth mover's distance by a synchronous auction: the algorithm of the reference's emd module
 * (metrics/emd/emd_cuda.cu:93-236 behind metrics/CD_EMD/emd_/emd_module.py:33-75: `emd.forward(xyz1, xyz2, dist, assignment, price,
 * assignment_inv, bid, bid_increments, max_increments, ..., eps, iters)`), with the scratch arrays folded into one workspace and a
 * timing-independent winner rule (highest increment, lowest bidder index).  xyz1/xyz2 [B,n,3] (coordinates normalised to [0,1] as
 * there); dist [B,n] = squared distance of every point of xyz1 to its assigned point, assignment [B,n] = that point's index in
 * xyz2[b] (not guaranteed to be a bijection when `iters` ends before the auction does).  Any n (the reference: n % 1024 == 0). */
size_t spgan_emd_ws_bytes(int B, int n);
int spgan_emd_forward(const float* xyz1, const float* xyz2, int B, int n, float eps, int iters, float* dist, int32_t* assignment,
                      void* ws, size_t ws_bytes, spgan_stream_t s);
/* grad_xyz1[b,i] = 2*grad_dist[b,i]*(xyz1[b,i] - xyz2[b,assignment[b,i]]) (emd_cuda.cu:279-313; xyz2 receives no gradient there) */
int spgan_emd_backward(const float* xyz1, const float* xyz2, int B, int n, const float* grad_dist, const int32_t* assignment,
                       float* grad_xyz1, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * --attn variant: `Attention(640)` between the concat and the tail (Generation/modules.py:534-558,
 * Generator.py:116-117,191-192).  The projections and the per-shape [N,N] contractions are spgan_gemm_nt / spgan_gemm_tn
 * calls; these are the HBM-bound pieces between them.
 * ---------------------------------------------------------------------------------------- */
/* S[r,:] = softmax(S[r,:]) in place, rows x cols contiguous (F.softmax(.,-1), modules.py:554) */
int spgan_softmax_rows(float* S, long rows, int cols, spgan_stream_t s);
/* dP[r,:] = P[r,:] * (dP[r,:] - sum_j dP[r,j]*P[r,j]) in place: the softmax Jacobian applied to the upstream gradient */
int spgan_softmax_rows_bwd(const float* P, float* dP, long rows, int cols, spgan_stream_t s);
/* y = gamma[0]*o + x (gamma: device scalar, the learnable gate of modules.py:546,558); n % 4 == 0 */
int spgan_scale_residual(const float* o, const float* x, const float* gamma, float* y, size_t n, spgan_stream_t s);
/* d_o = gamma[0]*dy, dgamma[0] = sum(dy*o) (two-stage, fixed order).  ws: spgan_scale_residual_bwd_ws_bytes(n) bytes. */
size_t spgan_scale_residual_bwd_ws_bytes(size_t n);
int spgan_scale_residual_bwd(const float* dy, const float* o, const float* gamma, float* d_o, float* dgamma, void* ws, size_t ws_bytes,
                             size_t n, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * PointTransformerLayer (Generation/modules.py:1602-1644): all-pairs vector attention without a per-pair vector in memory
 * (DESIGN 25).  With r_ij = relu(W_p1 (pos_i - pos_j) + b_p1), Wc = W_a1 W_p2 and c = W_a1 b_p2 + b_a1:
 *   sim_ij = w_a2 . relu(QaC_i - Ka_j + Wc r_ij),  a = softmax_j(sim),  Sv_i = sum_j a_ij v_j,  R_i = sum_j a_ij r_ij.
 * Operands are padded images: Mp = spgan_pair_attn_padded_m(dim * mult), a multiple of 128 up to 4096, Hp = spgan_pair_attn_padded_h(H) in
 * {32, 64} (0 = outside the domain), all padding zero.  pos [b,n,3]; Wp1p [Hp,4] = (W_p1 | b_p1); QaC = q W_a1^T + c and
 * Ka = k W_a1^T [b*n,Mp]; Wc [Mp,Hp]; WcT [Hp,Mp]; wa2 [Mp]; v [b*n,D] with row stride ldv; D <= spgan_pair_attn_max_dim().
 * Exact fp32 MFMA; every sum has a fixed order (no float atomics).
 * ---------------------------------------------------------------------------------------- */
int spgan_pair_attn_padded_m(int M);
int spgan_pair_attn_padded_h(int H);
int spgan_pair_attn_max_dim(void);
/* lse_in == NULL: the forward.  Online softmax over key tiles -> Sv [b*n,D], R [b*n,Hp], lse_out [b*n] (log-sum-exp of sim; b_a2
 * cancels and is left out).  lse_in != NULL: the backward's recomputation, P [b,n,n] = exp(sim - lse_in); v, Sv, R, lse_out unused. */
int spgan_pair_attn_fwd(const float* pos, const float* Wp1p, const float* QaC, const float* Ka, const float* Wc, const float* wa2,
                        const float* v, int ldv, int b, int n, int D, int Mp, int Hp, const float* lse_in, float* Sv, float* R,
                        float* lse_out, float* P, spgan_stream_t s);
/* dS [b,n,n] holds dout_i . v_j on entry (a per-cloud GEMM of the caller) and on return P_ij (g_ij - delta_i),
 * g_ij = dout_i . v_j + dR_i . r_ij, delta_i = sum_j P_ij g_ij / sum_j P_ij (= dout_i . (out_i - b_p2), from the numbers it is
 * subtracted from); dR = dout W_p2 [b*n,Hp] */
int spgan_pair_attn_dsim(const float* P, const float* dR, const float* pos, const float* Wp1p, int b, int n, int Hp, float* dS,
                         spgan_stream_t s);
/* The pair backward recomputes pre_ij; dpre_ij = dS_ij w_a2 [pre_ij > 0], dz_ij = [r_ij > 0] (Wc^T dpre_ij + P_ij dR_i).
 * role 0 (query-stationary): dA [b*n,Mp] = dQa_i = sum_j dpre_ij, Z [b*n,Hp] = sum_j dz_ij, and per workgroup one record of
 *   ws: [records][Mp*Hp + Mp] = partial dWc (row-major [Mp,Hp]) then partial dw_a2; the caller sums the records in ascending order.
 *   records = spgan_pair_attn_bwd_records(b, n) = b * min(n, max(1, 512 / b)): at most 512 for b <= 512, b beyond (128 KB per record
 *   at the default Mp 512, Hp 64; 1 MB at the largest Mp 4096).
 * role 1 (key-stationary): dA = dKa_j = -sum_i dpre_ij, Z = sum_i dz_ij; ws unused. */
int spgan_pair_attn_bwd_records(int b, int n);
size_t spgan_pair_attn_bwd_ws_bytes(int b, int n, int Mp, int Hp);
int spgan_pair_attn_bwd(int role, const float* pos, const float* Wp1p, const float* QaC, const float* Ka, const float* Wc,
                        const float* WcT, const float* wa2, const float* P, const float* dS, const float* dR, int b, int n, int Mp,
                        int Hp, float* dA, float* Z, void* ws, size_t ws_bytes, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Dot-product point self-attention without a [b,n,n] map (csrc/point_attn.hip): per shape, on point-major rows,
 *   S_ij = q_i . k_j (unscaled),  P = softmax_j(S),  O_i = sum_j P_ij v_j,  lse_i = log sum_j exp(S_ij).
 * q, k [b*n,dk], v, o, dO [b*n,dv] with row strides ld* (column slices of one projected tensor are fine).  dk = a multiple of 4 up to 128
 * (spgan_point_attn_padded_dk: the host pads with zero columns, which leaves S unchanged; 0 = outside the domain), dv = a multiple of 4 up
 * to spgan_point_attn_max_dv(); every row stride a multiple of 4 and every base pointer 16-byte aligned.  Any b in 1..65535, any n >= 1.
 * Exact fp32 MFMA; every sum has a fixed order (no float atomics).
 * ---------------------------------------------------------------------------------------- */
int spgan_point_attn_padded_dk(int dk);
int spgan_point_attn_max_dv(void);
/* online softmax over key tiles -> o [b*n,dv], lse [b*n]; nothing of size n^2 is written */
int spgan_point_attn_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int b, int n, int dk, int dv, float* o,
                         int ldo, float* lse, spgan_stream_t s);
/* The backward recomputes P = exp(S - lse); dS = P (dO V^T - D), D_i = dO_i . o_i.  The workspace is lse and D [b*n].
 * role 0 (query-stationary): writes D_i = sum_j P_ij (dO_i . v_j) / sum_j P_ij, then dq_i = sum_j dS_ij k_j [b*n,dk]; dkey / dval are unused.
 * role 1 (key-stationary), after role 0: dval_j = sum_i P_ij dO_i [b*n,dv], dkey_j = sum_i dS_ij q_i [b*n,dk]; dq is unused. */
int spgan_point_attn_bwd(int role, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* dO, int lddo,
                         const float* lse, float* D, int b, int n, int dk, int dv, float* dq, int lddq, float* dkey, int lddk,
                         float* dval, int lddv, spgan_stream_t s);

/* Dense edge / point layers (csrc/edge_dense.hip): DenseEdgeModule and DenseModule1D of Common/utilities.py:22-42, 123-144 without the
 * concatenated tensors.  Exact fp32 MFMA products; no float atomics: results repeat bit for bit.
 *   spgan_edge_dense_level:    Y[m, n] = sum_{c < K} op(A)[m, c] * W[n, c] + bias[n] + Q[m / k, n] + P[idx[m], n], m < M, n < N.
 *                              op(A)[m, c] = A[m*lda + c] for c < raw_cols and lrelu(A[m*lda + c]*scale[c] + shift[c], slope) for
 *                              raw_cols <= c < K (scale, shift [K]; entries below raw_cols are not read; both may be NULL with raw_cols == K):
 *                              A is the virtual concatenation [raw input | stored pre-norm blocks], each block activated while it is staged.
 *                              The addend is optional (PQ == NULL: none): P = columns [0, N) and Q = columns [qoff, qoff + N) of PQ [M/k, ldpq],
 *                              idx [M] int32 rows of PQ (an entry outside [0, M/k) reads the row's own point), M % k == 0.  bias optional.
 *                              Y [M, ldy >= N] may be a column slice of the buffer A is read from: the columns written and the K columns
 *                              read must be DISJOINT (nothing orders a workgroup's stores against another's loads).
 *                              partials (optional) [ceil(M / tile_rows)][N][2] = (sum, centred M2) of Y per row tile: the records
 *                              spgan_colstats_finalize / _finalize_bn read (mode 0, tile_rows = spgan_edge_dense_tile_rows()).
 *                              Any M, N >= 1, K >= 0 (K == 0: the addend / bias alone, a gather into a strided slice); tails in the kernel.
 *   spgan_edge_dense_scatter:  D [M*k, ldd >= C] on the edges -> dPQ [M, ldo >= 2C] = [dP | dQ]: dQ[i] = sum over the k rows of point i,
 *                              dP[j] = sum of D[e] over the in-edge list of j (spgan_csr_build, ascending edge ids; in-degree 0: zeros).
 *   spgan_edge_dense_bn_apply: spgan_bn_bwd_apply with a row stride per tensor: dz[m*ldd + c] = gamma*invstd*(g[m*ldg + c] - sums[c]/count
 *                              - xhat*sums[C + c]/count), xhat = (z[m*ldz + c] - mean)*invstd; dz must not alias g or z. */
int spgan_edge_dense_tile_rows(void);
int spgan_edge_dense_level(const float* A, int lda, int raw_cols, const float* scale, const float* shift, float slope, const float* W, int ldw,
                           const float* bias, const float* PQ, int ldpq, int qoff, const int32_t* idx, int k, int M, int N, int K, float* Y,
                           int ldy, float* partials, spgan_stream_t s);
int spgan_edge_dense_scatter(const float* D, int ldd, const int32_t* rowptr, const int32_t* src, int M, int k, int C, float* dPQ, int ldo,
                             spgan_stream_t s);
int spgan_edge_dense_bn_apply(const float* g, int ldg, const float* z, int ldz, int M, int C, const float* mean, const float* invstd,
                              const float* gamma, const float* sums, int count, float* dz, int ldd, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Global-context attention (csrc/gc_attn.hip): GC_attn of Common/utilities.py:357-426.  Per sample b over its L positions:
 *   m_n = w . x_n + bias,  p = softmax_n(m)  (w == NULL: p_n = 1/L),  ctx = sum_n p_n x_n,
 *   add = branch_add(ctx),  mul = sigmoid(branch_mul(ctx)),  branch = Conv1d(C,O,1) -> LayerNorm([O,1]) -> ReLU -> Conv1d(O,C,1),
 *   out_n = x_n * mul + add.
 * layout 0: channel-major, x / g / out / dx contiguous [B,C,L] (the ld arguments are not read).  layout 1: point-major rows [B*L, C] with
 * row strides ld >= C.  16-byte accesses when L % 4 == 0 (layout 0) or C % 4 == 0 and every stride % 4 == 0 (layout 1) and the bases are
 * 16-byte aligned; element accesses otherwise.  1 <= C, O <= 1024, 1 <= B <= 65535, L >= 1.  A workgroup reduces
 * spgan_gc_attn_chunk_points(layout) positions of a sample; nch = ceil(L / that).  Every sum has a fixed order; no float atomics.
 * Traffic: pool_fwd |x|, apply_fwd 2|x|, bwd_reduce 2|x|, bwd_apply 3|x|; layout 0 with C > 484 loads x twice in pool_fwd and bwd_apply
 * (2|x| and 4|x|): the [C, 32] tile of the one-read kernels no longer fits 64 KB of LDS.
 *   pool_fwd     part: workspace [B*nch*(C + 2)];  m [B*L]: the logits (not written when w == NULL);  ctx [B,C];  lse [B];
 *                stat [B,2] = (max_n m_n, sum_n exp(m_n - max)), the form the backward evaluates p from.  Two launches.
 *   channel_fwd  one launch for both branches (a NULL branch is skipped, its output untouched): hid [2,B,O] = the first convolution's
 *                output, lnstat [2,B,2] = the LayerNorm's (mean, rstd), add / mul [B,C].  Branch 0 = add, 1 = mul.
 *   channel_bwd  one launch: from dadd / dmul [B,C] (the cotangents of add / mul) -> dctx [B,C] and, per sample, the factors of the
 *                parameter gradients G [B, nb*(C + 4*O)], nb = the number of branches, the add branch first, per branch
 *                [dt (C) | dh (O) | dhn * xhat (O) | dhn (O) | r (O)]: dW2 = dt^T r, db2 = colsum dt, dW1 = dh^T ctx, db1 = colsum dh,
 *                dLN.weight = colsum dhn * xhat, dLN.bias = colsum dhn.
 *   apply_fwd    out = x * mul[b] + add[b] (NULL: 1 / 0).
 *   bwd_reduce   dmul [B,C] = sum_n g_n * x_n, dadd [B,C] = sum_n g_n (either may be NULL); part: workspace [B*nch*2*C], layout 1 only.
 *   bwd_apply    dx_n = g_n * mul + p_n dctx + s_n w,  s_n = p_n (dctx . x_n - dctx . ctx);  dwpart [B*nch, C]: per workgroup sum_n s_n x_n,
 *                whose column sums are the gradient of w.  w == NULL: dx_n = g_n * mul + dctx / L; ctx, m, stat, dwpart are not read.
 * ---------------------------------------------------------------------------------------- */
typedef struct spgan_gc_branch {
  const float *W1, *b1, *lnw, *lnb, *W2, *b2; /* [O,C], [O], [O], [O], [C,O], [C] */
} spgan_gc_branch_t;
int spgan_gc_attn_chunk_points(int layout);
int spgan_gc_attn_pool_fwd(const float* x, int layout, long ld, int B, int C, long L, const float* w, const float* bias, float* part, float* m,
                           float* ctx, float* lse, float* stat, spgan_stream_t s);
int spgan_gc_attn_channel_fwd(const float* ctx, int B, int C, int O, const spgan_gc_branch_t* add_p, const spgan_gc_branch_t* mul_p, float eps,
                              float* hid, float* lnstat, float* add, float* mul, spgan_stream_t s);
int spgan_gc_attn_channel_bwd(const float* dadd, const float* dmul, const float* mul, const float* hid, const float* lnstat, int B, int C, int O,
                              const spgan_gc_branch_t* add_p, const spgan_gc_branch_t* mul_p, float* G, float* dctx, spgan_stream_t s);
int spgan_gc_attn_apply_fwd(const float* x, int layout, long ldx, int B, int C, long L, const float* mul, const float* add, float* out, long ldo,
                            spgan_stream_t s);
int spgan_gc_attn_bwd_reduce(const float* x, long ldx, const float* g, long ldg, int layout, int B, int C, long L, float* part, float* dmul,
                             float* dadd, spgan_stream_t s);
int spgan_gc_attn_bwd_apply(const float* x, long ldx, const float* g, long ldg, int layout, int B, int C, long L, const float* mul,
                            const float* dctx, const float* ctx, const float* w, const float* m, const float* stat, float* dx, long lddx,
                            float* dwpart, spgan_stream_t s);

/* ------------------------------------------------------------------------------------------
 * MST expansion penalty and minimum-density sampling (csrc/expansion.hip): metrics/expansion_penalty/expansion_penalty_cuda.cu
 * and metrics/MDS/MDS_cuda.cu of the reference.  No float atomics, no adjacency workspace, every sum in a fixed order: results repeat bit for bit.
 *
 * spgan_expansion_penalty_fwd: xyz [B,n,3]; every run of primitive_size (p) consecutive points of a cloud is one primitive,
 * 2 <= p <= 512, n % p == 0.  Per primitive:
 *   1. Prim's algorithm from local point 0.  Edge length sqrtf((dx*dx + dy*dy) + dz*dz), each operation rounded on its own.  A candidate's
 *      parent changes only on a strictly smaller distance; the next vertex is the unvisited one of least distance, the HIGHEST local index
 *      among exact ties (the reference's reduction tree at power-of-two p; at other p that tree is not a minimum, this is the true arg-min).
 *   2. mean = (sum of the p-1 edge lengths) / (float)(p-1) -> prim_mean_ws [B * n/p].  Order of the sum, with w[v] the length of the edge
 *      that attached vertex v (w[0] = 0, w[v] = 0 for v >= p): s_l = (..((w[l] + w[64+l]) + w[128+l]) + ..) for l = 0..63, then for
 *      o = 32, 16, 8, 4, 2, 1: s_l = s_l + s_(l xor o) on all l at once; the sum is s_0.  mean_mst_length[b] = the same two-stage sum over the
 *      cloud's primitive means m[j] (s_l over j = l, l+64, ..), divided by (float)(n/p).
 *   3. Leaf peeling in synchronous rounds assigns each tree edge to one endpoint: the leaves of a round are the vertices of remaining
 *      degree 1 at its start; leaf t with remaining neighbour u takes the edge when cnt_start[u] > 1, or cnt_start[u] == 1 and t > u.
 *      (One of the outcomes the reference's racing loop can produce: the one where every read precedes every decrement.)
 *   4. An owned edge of length c > mean * alpha (a float product): dist[b, base+t] = c, assignment[b, base+t] = base_in_cloud + u;
 *      every other point: dist 0, assignment -1.
 * spgan_expansion_penalty_bwd: grad_xyz[b,j] = 2 * grad_dist[b,j] * (xyz[b,j] - xyz[b, assignment[b,j]]) where assignment != -1, else 0
 *   (only the owning endpoint receives a gradient and the factor is that of a squared length: both as the reference); plain stores.
 * spgan_minimum_density_sample: xyz [B,n,3] -> out int32 [B,npoint], 1 <= npoint <= n.  t = 5 * L * L (in double, rounded once), L =
 *   mean_mst_length[b]; out[0] = 0; a density T[k] starts at 0 and is set to 1e9 once k is selected; for j = 1 .. npoint-1 every k adds
 *   w_k * expf(-d_k / t), d_k = (dx*dx + dy*dy) + dz*dz to the last selected point, w_k = 1 for k < split else 2 (the reference hard-codes
 *   8192), and the point of least T is selected, the LOWEST index among exact ties (the reference: by thread id, which depends on its
 *   block size).  density_ws [B*n] is read only when spgan_minimum_density_sample_needs_ws(n) != 0 (n > 16384) and may be NULL otherwise.
 * spgan_gather_points_cm: out[b,c,j] = feat[b,c,idx[b,j]], feat [B,C,N], idx int32 [B,m] (gather_operation of MDS_module.py); an index
 *   outside [0,N) yields 0 and sets *bad (bad may be NULL).  spgan_gather_points_cm_bwd: dfeat[b,c,i] = the sum of dout[b,c,j] over the
 *   slots j with idx[b,j] == i in ascending j, from spgan_gather_csr(idx as int64 [B,m], S = m) -- duplicates are summed.
 * ---------------------------------------------------------------------------------------- */
int spgan_expansion_penalty_fwd(const float* xyz, int B, int n, int primitive_size, float alpha, float* dist, int32_t* assignment,
                                float* mean_mst_length, float* prim_mean_ws, spgan_stream_t s);
int spgan_expansion_penalty_bwd(const float* xyz, const float* grad_dist, const int32_t* assignment, int B, int n, float* grad_xyz,
                                spgan_stream_t s);
int spgan_minimum_density_sample_needs_ws(int n);
int spgan_minimum_density_sample(const float* xyz, int B, int n, int npoint, const float* mean_mst_length, int split, int32_t* out,
                                 float* density_ws, spgan_stream_t s);
int spgan_gather_points_cm(const float* feat, const int32_t* idx, int B, int C, int N, int m, float* out, int32_t* bad, spgan_stream_t s);
int spgan_gather_points_cm_bwd(const float* dout, const int32_t* rowptr, const int32_t* src, int B, int C, int N, int m, float* dfeat,
                               spgan_stream_t s);

/* ----------------------------------------------------------------------------------------
 * The pointops extension (metrics/pointops/src of the reference; csrc/pointops.hip).  Every index tensor is int32.  Every
 * squared distance is d2 = (dx*dx + dy*dy) + dz*dz with dx = query - candidate, each operation rounded on its own.  `bad` may be NULL.
 * spgan_pointops_knnquery: xyz [B,n,3], new_xyz [B,m,3], 1 <= nsample <= 200 -> idx [B,m,nsample], dist2 [B,m,nsample]: ascending d2, the
 *   lower index first on equal d2, the query itself included when it is a cloud point; slots past n hold index 0 and +inf.  Clouds of up to
 *   spgan_pointops_knn_capacity() points are selected from registers in one pass, larger ones in chunks of that size (any n >= 1).
 * spgan_pointops_nearestneighbor: the three nearest known [B,m,3] of every unknown [B,n,3] (the same kernel, nsample = 3) -> dist2, idx
 *   [B,n,3]; the caller takes the square root.
 * spgan_pointops_ballquery: the first nsample indices (ascending) with d2 < radius*radius (STRICT; a float product), every slot pre-filled
 *   with the first hit, all zeros for an empty ball.
 * spgan_pointops_labelstat_ballrange: new_label_stat[b,j,:] = the sum of label_stat[b,k,:] (int32 [B,n,nclass]) over ALL k with d2 < r*r.
 * spgan_pointops_labelstat_and_ballquery: the ball query, and the sum over the hits it returns only (the scan ends at nsample hits).
 * spgan_pointops_labelstat_idx: the sum of the rows named by idx [B,m,nsample]; an index outside [0,n) adds nothing and sets *bad.
 * spgan_pointops_featuredistribute: for every xyz [B,m,3] the index of the nearest max_xyz [B,n,3], the lowest index among equals, -1 when
 *   no d2 is below 100000 (the reference's starting value).
 * spgan_pointops_group_cm: out[b, c0+c, j, k] = src[b, c, idx[b,j,k]] for c < C into the channel slice [c0, c0+C) of out [B,Ctot,m,K]; src is
 *   [B,C,n], or with point_major != 0 [B,n,3] (C = 3); center [B,m,3] (C = 3), when given, is subtracted.  An index outside [0,n) writes 0
 *   and sets *bad.  Clouds of up to spgan_pointops_group_stage_limit() points are staged in LDS.
 * spgan_pointops_group_cm_bwd: dsrc[b,c,i] = the sum of dout[b, c0+c, s] over the slots s with idx[b,s] == i in ascending s, from
 *   spgan_gather_csr(idx as int64 [B, m*K]) (dsrc in src's layout; NULL skips it); dcenter[b,j,c] = -(sum over k ascending of
 *   dout[b, c0+c, j, k]) (NULL skips it).
 * spgan_pointops_group_int: out[b,c,j,k] = feat[b,c,idx[b,j,k]] on int64 features (grouping_int).
 * spgan_pointops_interpolate_cm: out[b,c,j] = (w0*f0 + w1*f1) + w2*f2, f_t = feat[b,c,idx[b,j,t]]; feat [B,C,m], idx / weight [B,n,3].
 * spgan_pointops_interpolate_cm_bwd: dfeat[b,c,i] = the sum over the slots e of (b,i) in ascending e (spgan_gather_csr of idx as int64
 *   [B, n*3]) of weight[e] * dout[b,c,e/3 - b*n].
 * ---------------------------------------------------------------------------------------- */
int spgan_pointops_knn_capacity(void);
int spgan_pointops_group_stage_limit(void);
int spgan_pointops_knnquery(const float* xyz, const float* new_xyz, int B, int n, int m, int nsample, int32_t* idx, float* dist2,
                            spgan_stream_t s);
int spgan_pointops_nearestneighbor(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx, spgan_stream_t s);
int spgan_pointops_ballquery(float radius, int nsample, const float* xyz, const float* new_xyz, int B, int n, int m, int32_t* idx,
                             spgan_stream_t s);
int spgan_pointops_labelstat_ballrange(float radius, const float* xyz, const float* new_xyz, const int32_t* label_stat, int B, int n, int m,
                                       int nclass, int32_t* new_label_stat, spgan_stream_t s);
int spgan_pointops_labelstat_and_ballquery(float radius, int nsample, const float* xyz, const float* new_xyz, const int32_t* label_stat, int B,
                                           int n, int m, int nclass, int32_t* idx, int32_t* new_label_stat, spgan_stream_t s);
int spgan_pointops_labelstat_idx(const int32_t* label_stat, const int32_t* idx, int B, int n, int m, int nsample, int nclass,
                                 int32_t* new_label_stat, int32_t* bad, spgan_stream_t s);
int spgan_pointops_featuredistribute(const float* max_xyz, const float* xyz, int B, int n, int m, int32_t* distribute_idx, spgan_stream_t s);
int spgan_pointops_group_cm(const float* src, int point_major, const float* center, const int32_t* idx, int B, int C, int n, int m, int K,
                            int c0, int Ctot, float* out, int32_t* bad, spgan_stream_t s);
int spgan_pointops_group_cm_bwd(const float* dout, const int32_t* rowptr, const int32_t* slots, int B, int C, int n, int m, int K, int c0,
                                int Ctot, int point_major, float* dsrc, float* dcenter, spgan_stream_t s);
int spgan_pointops_group_int(const int64_t* feat, const int32_t* idx, int B, int C, int n, int m, int K, int64_t* out, int32_t* bad,
                             spgan_stream_t s);
int spgan_pointops_interpolate_cm(const float* feat, const int32_t* idx, const float* weight, int B, int C, int m, int n, float* out,
                                  int32_t* bad, spgan_stream_t s);
int spgan_pointops_interpolate_cm_bwd(const float* dout, const float* weight, const int32_t* rowptr, const int32_t* slots, int B, int C, int m,
                                      int n, float* dfeat, spgan_stream_t s);

/* ----------------------------------------------------------------------------------------
 * Set abstraction with the first MLP layer hoisted onto the points (metrics/pointnet2/pointnet2_modules.py of the reference;
 * csrc/sa_group.hip).  Indices are int32 and local to their cloud.
 * spgan_sa_ballquery_multi: the ball queries of up to SPGAN_SA_MAX_SCALES radii around the same centres in one walk of the cloud: xyz
 *   [B,n,3], new_xyz [B,m,3] -> idx[s] [B,m,nsample[s]], each list equal to spgan_pointops_ballquery(radius[s], nsample[s]) bit for bit.
 * spgan_sa_gather: Y[(q*K + k), c] = (P[(b*n + idx[q,k]), colp + c] - Qc[q, colq + c]) + bias[c] for q = b*m + j < B*m, k < K, c < C;
 *   P [B*n, ldp], Qc [B*m, ldq], Y [B*m*K, ldy], bias [C] or NULL.  part [tiles, C, 2] (NULL: none) receives the (sum, centred M2)
 *   records of Y's columns per tile of spgan_sa_gather_tile_rows(K) rows, as spgan_colstats_finalize / _finalize_bn read them.  An index
 *   outside [0,n) reads point 0 and sets *bad (bad may be NULL).
 * spgan_sa_scatter: the gather's backward.  dP[p, colp + c] = the sum of dY[e, c] over the slots e that read point p, in ascending e
 *   (rowptr [BN,2], src: spgan_gather_csr of the index list as int64 [B, m*K]); dQ[q, colq + c] = -(sum over k ascending of dY[q*K + k, c]).
 *   dY [Q*K, ld >= C], dP [BN, ldp], dQ [Q, ldq]; dP or dQ may be NULL (not both).
 * spgan_sa_rows_to_cm_slice: cm[b, c0+c, s] = rows[(b*S + s), c] into the channel slice [c0, c0+C) of cm [B,Ctot,S]; rows [B*S, C].
 * spgan_sa_cm_slice_to_rows: the inverse (the gradient of the former).
 * ---------------------------------------------------------------------------------------- */
#define SPGAN_SA_MAX_SCALES 8
typedef struct spgan_sa_query_args {
  int count;
  float radius[SPGAN_SA_MAX_SCALES];
  int nsample[SPGAN_SA_MAX_SCALES];
  int32_t* idx[SPGAN_SA_MAX_SCALES];
} spgan_sa_query_args;
int spgan_sa_gather_tile_rows(int K);
int spgan_sa_ballquery_multi(const spgan_sa_query_args* a, const float* xyz, const float* new_xyz, int B, int n, int m, spgan_stream_t s);
int spgan_sa_gather(const float* P, int ldp, int colp, const float* Qc, int ldq, int colq, const float* bias, const int32_t* idx, int B, int n,
                    int m, int K, int C, float* Y, int ldy, float* part, int32_t* bad, spgan_stream_t s);
int spgan_sa_scatter(const float* dY, int ld, int C, const int32_t* rowptr, const int32_t* src, int BN, float* dP, int ldp, int colp, int Q, int K,
                     float* dQ, int ldq, int colq, spgan_stream_t s);
int spgan_sa_rows_to_cm_slice(const float* rows, int B, int S, int C, int c0, int Ctot, float* cm, spgan_stream_t s);
int spgan_sa_cm_slice_to_rows(const float* cm, int B, int S, int C, int c0, int Ctot, float* rows, spgan_stream_t s);

/* ----------------------------------------------------------------------------------------
 * Frechet point-cloud distance in float64 on v_mfma_f64_16x16x4_f64 (csrc/frechet.hip; Common/GAN_metrics.py:484-545).  Every matrix
 * is square [d,d], row-major, 2 <= d <= 2048; every sum has a fixed order (no float atomics): equal inputs give equal bits.
 * spgan_f64_gemm: C = alpha op(A) B + beta C + diag I, op(A) = A^T if trans_a (beta == 0: C is not read); C must not alias A or B.
 * spgan_f64_reduce: out[0] = trace(A) (kind 0), |A|_F (kind 1) or sum A o B (kind 2); ws of spgan_f64_reduce_ws_bytes().
 * spgan_fpd_moments_update: one chunk X [n,d] of float32 rows into the running state (count_before rows seen, sum2 [2,d], M2 [d,d]):
 *   the chunk's float64 column sums and centred Gram matrix (converted and centred while staged), merged by
 *   M2 += M2_chunk + (na nb / (na + nb)) delta delta^T.  sum2[0] is the pivot (the first row ever seen), sum2[1] the sums of
 *   x - pivot: a large common mean cancels exactly instead of rounding every sum; mean = sum2[0] + sum2[1] / count.
 *   count_before == 0 overwrites sum2 and M2.  The caller keeps the count.
 * spgan_fpd_distance: out5 = [|mu1 - mu2|^2 + tr(S1 + S2 - 2 sqrt(S1 S2)), iterations of stages 0, 1, 2, tr sqrt(S1 S2)].
 *   Stages 0 and 1: R = sqrt(S1), sqrt(S2) by the coupled Newton-Schulz iteration, stopped on the device when
 *   |Y_new - Y|_F <= 1e-13 |Y_new|_F; stage 2: the nuclear norm of R1 R2 (= tr sqrt(S1 S2)) by the polar iteration
 *   X <- X (1.5 I - 0.5 X^T X), stopped when sum X o (R1 R2) moves by <= 1e-14 of itself; each stage after at most
 *   spgan_fpd_max_iterations().  Stream-ordered, no host read; ws of spgan_fpd_distance_ws_bytes(d), 256-byte aligned.
 * ---------------------------------------------------------------------------------------- */
int spgan_f64_gemm(const double* A, const double* B, double* C, int d, int trans_a, double alpha, double beta, double diag, spgan_stream_t s);
size_t spgan_f64_reduce_ws_bytes(void);
int spgan_f64_reduce(int kind, const double* A, const double* B, int d, double* out, void* ws, spgan_stream_t s);
size_t spgan_fpd_moments_ws_bytes(int n, int d);
int spgan_fpd_moments_update(const float* X, int n, int d, long count_before, double* sum2, double* M2, void* ws, size_t ws_bytes, spgan_stream_t s);
int spgan_fpd_max_iterations(void);
size_t spgan_fpd_distance_ws_bytes(int d);
int spgan_fpd_distance(const double* mu1, const double* S1, const double* mu2, const double* S2, int d, double* out5, void* ws, size_t ws_bytes,
                       spgan_stream_t s);

/* ----------------------------------------------------------------------------------------
 * GAN-stabiliser and StyleGAN-style layers (csrc/gan_layers.hip; Generation/modules.py:32-390, 437-496).  fp32, no float atomics, fixed
 * summation orders (equal inputs give equal bits; a problem gives the same bits alone and inside a group), no host read.
 *
 * Grouped spectral normalisation: `count` (1 .. SPGAN_SN_MAX) weights W[p] [h,w] row-major (the parameter flattened from dim 0) as one
 * argument block; the number of launches does not depend on count (4 per power iteration + 1; 3 with n_iter == 0).
 *   forward: n_iter times  v <- norm(W^T u), u <- norm(W v)  (u [h], v [w] updated in place), sigma = u . (W v), out = W / sigma;
 *     rule 0: norm(x) = x / (|x| + eps) (the reference's l2normalize), rule 1: x / max(|x|, eps) (F.normalize).  n_iter == 0 leaves u, v
 *     alone (eval mode of the hook form).  save[p] [1 + h + w] receives (sigma, u, v) of this call; ws[p] holds
 *     spgan_sn_ws_floats(h, w) floats.  W^T u runs as 16-row chunks x 256-column blocks, W v as one wave per row, the quotient as
 *     2048-element tiles: a [512,1024] weight spreads over 128 / 128 / 256 workgroups.
 *   backward (u, v constant): dW = G / sigma - (<G,W> / sigma^2) u v^T from save[p]; one grouped reduction (2048-element tiles into
 *     ws[p]), one grouped apply.  Reads W, G, save, ws; writes dW.
 * ---------------------------------------------------------------------------------------- */
#define SPGAN_SN_MAX 32
typedef struct spgan_sn_args {
  int count;
  const float* W[SPGAN_SN_MAX]; float* u[SPGAN_SN_MAX]; float* v[SPGAN_SN_MAX]; float* out[SPGAN_SN_MAX];
  float* save[SPGAN_SN_MAX]; float* ws[SPGAN_SN_MAX];
  const float* G[SPGAN_SN_MAX]; float* dW[SPGAN_SN_MAX];          /* backward only */
  int h[SPGAN_SN_MAX], w[SPGAN_SN_MAX];
} spgan_sn_args;
size_t spgan_sn_ws_floats(int h, int w);
int spgan_sn_forward(const spgan_sn_args* a, int n_iter, int rule, float eps, spgan_stream_t s);
int spgan_sn_backward(const spgan_sn_args* a, spgan_stream_t s);
/* Minibatch stddev (modules.py:54-135): x [B,C,N], G | B, M = B/G, sample b = g*M + m belongs to statistic m; F | C new channels.
 *   forward: one pass copies x into out [B,C+F,N] channels [0,C) and reduces sqrt(mean_g (x - mean_g)^2 + alpha) per (m, c, 1024-point
 *     tile) into ws (spgan_mbstd_ws_floats floats); a second launch averages the records of a feature group and fills channels [C,C+F).
 *   backward: S [M,F] = sum over g, n of dout's new channels; dx = dout[:, :C] + S (x - mean) / (G std (C/F) N). */
size_t spgan_mbstd_ws_floats(int B, int C, int N, int G);
int spgan_mbstd_forward(const float* x, int B, int C, int N, int G, int F, float alpha, float* out, float* ws, spgan_stream_t s);
int spgan_mbstd_backward(const float* x, const float* dout, int B, int C, int N, int G, int F, float alpha, float* dx, float* S,
                         spgan_stream_t s);
/* The layer epilogue  y = gamma * IN(PN(act(x + w * noise))) + beta  on x [B,C,L], C <= SPGAN_EPILOGUE_MAX_C; every stage optional.
 *   noise [B,L] with w [C] (both or neither);  act 0 none, 1 ReLU, 2 LeakyReLU(slope);  pn 0 none, 1 t = a * rsqrt(mean_c a^2 + pn_eps),
 *   2 t = a / sqrt(mean_c a^2 + pn_eps);  stats 0 none, 1 per (b,c) over L, 2 per b over C*L jointly (biased variance, in_eps; C*L > 1);
 *   gamma, beta: element (b, c) at [b*ld_gb + c] (both or neither).
 *   rs [B,L] (pn != 0), stat [B,C,2] or [B,2] (mean, invstd; stats != 0) are written by the forward and read by the backward;
 *   rec holds spgan_epilogue_rec_floats(B, C, L) floats of per-(b, c, 256-point tile) records (stats != 0, or backward with dgamma / dw).
 *   forward: with statistics a column pass (rs and records), a finalising launch, an element-wise apply; pixel norm alone: the column pass
 *     writes y; neither: the apply alone.  t is never stored.
 *   backward: dx [B,C,L], dnoise [B,L], dw [C], dgamma / dbeta (element (b, c) at [b*ld_d + c]), each optional; grp [B,C,2] or [B,2]
 *     scratch (stats != 0).  A reduction pass and its finalising launch (statistics or dgamma), a column pass, and a launch for dw. */
#define SPGAN_EPILOGUE_MAX_C 1024
typedef struct spgan_epilogue_args {
  const float* x; const float* noise; const float* w; const float* gamma; const float* beta; int ld_gb;
  int B, C, L, act, pn, stats;
  float slope, pn_eps, in_eps;
  float* rs; float* stat; float* rec;
} spgan_epilogue_args;
size_t spgan_epilogue_rec_floats(int B, int C, int L);
int spgan_epilogue_forward(const spgan_epilogue_args* a, float* y, spgan_stream_t s);
int spgan_epilogue_backward(const spgan_epilogue_args* a, const float* dy, float* dx, float* dnoise, float* dw, float* dgamma, float* dbeta,
                            int ld_d, float* grp, spgan_stream_t s);
/* Truncation (modules.py:312-327) on x [B,Lr,D]: out = l < max_layer ? lerp(avg, x, thr) : x, avg [D] or (avg_per_layer) [Lr,D];
 * bwd != 0: out = x * (l < max_layer ? thr : 1), the cotangent's pass (avg not read). */
int spgan_truncation(const float* x, const float* avg, int avg_per_layer, int B, int Lr, int D, int max_layer, float thr, int bwd, float* out,
                     spgan_stream_t s);

/* ----------------------------------------------------------------------------------------
 * The point-distribution losses of Common/model_utils.py (csrc/point_losses.hip): the `keep` nearest slots of every point's
 * group, and the repulsion tails over them.  xyz [B,n,3]; val float [B,n,keep], idx int32 [B,n,keep] (cloud-local), coef float [B,n,keep].
 * Group of point i, slots 0..nsample-1, with dx = p_i - p_j and d2 = (dx*dx + dy*dy) + dz*dz, each operation rounded on its own:
 *   knn_idx == NULL (ball): the first nsample indices j (ascending) with d2 < radius*radius (STRICT; a float product), every further slot
 *     repeats the first hit; an empty ball holds point 0 in every slot (spgan_pointops_ballquery with new_xyz = xyz).  5 <= nsample <= 256,
 *     radius > 0.
 *   knn_idx int32 [B,n,nsample] (kNN): slot s is knn_idx[b,i,s], as written by spgan_pointops_knnquery.  5 <= nsample <= 200, nsample <= n.
 * Slot value by metric: 0 d2;  1 (|dx| + |dy|) + |dz|;  2 sqrtf(d2 + 1e-12f), ordered by d2.
 * Selection: the keep (2..8, <= nsample) smallest slots by (float bits of the value, slot), ascending; duplicated padding slots are slots
 *   of their own.  val / idx hold the winners' values and point indices.
 * tail != 0 (terms over the winners 1..keep-1, recomputed in float64 from the coordinates; winner 0 is dropped, its coef is 0):
 *   1: term = max(0, h - v), coef = -1 where h - v > 0, else 0
 *   2: w = max(1e-12, v), term = rterm - sqrt(w) * exp(-w / (h*h)), coef = the term's derivative in v where v > 1e-12, else 0
 *   loss[0] = (float)(sum of all terms / (B*n*(keep-1))): a wave adds its terms in ascending winner order, a workgroup its waves in
 *   ascending order into partial[g] (float64, spgan_point_losses_partials(B, n) entries), a second launch adds the partials (thread t of
 *   1024: t, t+1024, .. ascending, then a halving tree) and rounds once.  tail == 0: coef, partial and loss may be NULL; one launch.
 * spgan_point_losses_bwd: dxyz[b,i] = (gscale ? gscale[0] : 1) * scale * ( sum over t ascending of coef[b,i,t] * g(p_i - p_idx[b,i,t])
 *   - sum over the slots (i',t) with idx[b,i',t] == i, ascending, of coef[b,i',t] * g(p_i' - p_i) ), g(d) = 2d; sign(d) with sign(0) = 0;
 *   d / sqrt(d2 + 1e-12) for metric 0; 1; 2.  float64 throughout, rounded once, no atomics.  rowptr / slots given (spgan_gather_csr of idx
 *   as int64 [B, n*keep], n <= 16384): the incoming terms in ascending slot order over the per-point lists.  NULL: four waves per 64 points
 *   walk the cloud's index table through LDS, 4096 entries per round, wave w the w-th quarter of each round; the incoming terms are added
 *   per wave in ascending slot order and the waves' sums in ascending w (any n; the slower route).
 * Bad sizes return SPGAN_EINVAL before any launch.
 * ---------------------------------------------------------------------------------------- */
int spgan_point_losses_partials(int B, int n);
int spgan_point_losses_fwd(const float* xyz, const int32_t* knn_idx, int B, int n, int nsample, float radius, int metric, int keep, int tail,
                           double h, double rterm, float* val, int32_t* idx, float* coef, double* partial, float* loss, spgan_stream_t s);
int spgan_point_losses_bwd(const float* xyz, const int32_t* idx, const float* coef, const float* gscale, float scale, int B, int n, int keep,
                           int metric, const int32_t* rowptr, const int32_t* slots, float* dxyz, spgan_stream_t s);

/* ----------------------------------------------------------------------------------------
 * The approxmatch earth mover's distance (StructuralLosses.match_cost, tf_approxmatch; csrc/approxmatch.hip).
 * xyz1 [B,n,3] (k), xyz2 [B,m,3] (l), float32; the larger of n, m a multiple of the smaller; B <= 65535.  stride1 is xyz1's batch stride
 * in floats: n*3, or 0 (one cloud against B clouds).  With d2 = |xyz1[k] - xyz2[l]|^2, multiL = max(n,m)/n, multiR = max(n,m)/m:
 *   remainL = multiL, remainR = multiR;  for i = 0..9 (j = 7..-2), level = -(4^j), level(j = -2) = 0, E = exp(level * d2):
 *     ratioL[i][k] = remainL[k] / (1e-9 + sum_l E * remainR[l])
 *     sumr[l] = remainR[l] * sum_k E * ratioL[i][k];  ratioR[i][l] = min(remainR[l] / (sumr[l] + 1e-9), 1) * remainR[l];
 *     remainR[l] = max(0, remainR[l] - sumr[l])
 *     remainL[k] = max(0, remainL[k] - ratioL[i][k] * sum_l E * ratioR[i][l]);  cost += ratioL[i][k] * sum_l E * ratioR[i][l] * sqrt(d2)
 *   match(k,l) = sum_i E_i * ratioL[i][k] * ratioR[i][l] is never stored by the forward: it writes cost [B] and the records
 *   ratioL [B,10,n], ratioR [B,10,m].  ws: spgan_approxmatch_ws_bytes(B, n, m) bytes, 8-byte aligned.  d2 and E are float32; remainL,
 *   remainR, the ratios of the level in flight, the row costs and every sum are float64 (the records are their float32 roundings).
 *   23 launches, no host synchronisation, no atomics; every sum has a fixed order (a lane's four interleaved accumulators over
 *   ascending points, then the block's waves ascending).
 *   waves: 0 or 4 (four waves share a block's 64 stationary points), or 1 (the measured alternative, one wave per block).
 * spgan_approxmatch_bwd: grad_xyz1[k] = grad_cost[b] * sum_l match(k,l) * (xyz1[k] - xyz2[l]) / max(sqrt(d2), 1e-20), grad_xyz2[l] the
 *   negated sum over k; match is recomputed from the records and held constant.  Either output may be NULL; one launch each.
 * spgan_approxmatch_plan: match [B,m,n], entry [b,l,k] (tf_approxmatch.approx_match's layout), from the records; m <= 65535.
 * spgan_match_cost_dense_fwd / _bwd: cost [B] = sum match[b,l,k] * sqrt(d2) and the same two gradients from a caller's dense plan
 *   (ws: B*m doubles; spgan_approxmatch_ws_bytes covers it); sums in float64.
 * Bad sizes and null pointers return SPGAN_EINVAL before any launch.
 * ---------------------------------------------------------------------------------------- */
int spgan_approxmatch_levels(void);
int spgan_approxmatch_tile(void);
size_t spgan_approxmatch_ws_bytes(int B, int n, int m);
int spgan_approxmatch_fwd(const float* xyz1, long stride1, const float* xyz2, int B, int n, int m, int waves, float* cost, float* ratioL,
                          float* ratioR, void* ws, size_t ws_bytes, spgan_stream_t s);
int spgan_approxmatch_bwd(const float* xyz1, long stride1, const float* xyz2, int B, int n, int m, const float* ratioL, const float* ratioR,
                          const float* grad_cost, float* grad_xyz1, float* grad_xyz2, spgan_stream_t s);
int spgan_approxmatch_plan(const float* xyz1, long stride1, const float* xyz2, int B, int n, int m, const float* ratioL, const float* ratioR,
                           float* match, spgan_stream_t s);
int spgan_match_cost_dense_fwd(const float* xyz1, const float* xyz2, const float* match, int B, int n, int m, float* cost, void* ws,
                               size_t ws_bytes, spgan_stream_t s);
int spgan_match_cost_dense_bwd(const float* xyz1, const float* xyz2, const float* match, int B, int n, int m, const float* grad_cost,
                               float* grad_xyz1, float* grad_xyz2, spgan_stream_t s);

/* ----------------------------------------------------------------------------------------
 * Device-side batch augmentation (Common/data_utils.py, provider.py, point_operation.py; csrc/augment.hip).
 * One batch per call, two launches, no host synchronisation, no atomics; results repeat bit for bit.
 *
 * data [S,P,C] float32, C = 3 or 6 (xyz + normal); index int64 [B] (an entry outside 0..S-1 yields a cloud of NaN); 1 <= N <= P,
 * N <= spgan_augment_max_points() = 8192 (any value); B < 2^24.  out: layout 0 [B,N,C], layout 1 [B,C,N].  rec float32 [B,16] per cloud:
 *   rec[0..8] A row-major, rec[9..11] t, rec[12] the dropout ratio, rec[13], rec[14] the low and high 32 bits of the step value used
 *   (raw bit patterns, not numbers), rec[15] = 0.  Row-vector convention: xyz' = xyz A + t, i.e. xyz'[c] = sum_r xyz[r] * A[3r + c] + t[c].
 *
 * Random numbers: Philox4x32-10 (Salmon et al., SC'11; multipliers D2511F53 / CD9E8D57 on counter words 0 / 2, key increments 9E3779B9 /
 * BB67AE85, ten rounds).  key = (seed & 0xffffffff, seed >> 32); counter = (e, (purpose << 24) | b, step & 0xffffffff, step >> 32) with
 * b the slot in the batch.  X(purpose, b, e) are the four output words x0..x3; the WORD STREAM of (purpose, b) is word w = X(purpose, b,
 * w >> 2)[w & 3] (spgan_philox_fill writes it).  u(x) = (x >> 8) * 2^-24 in [0,1).  n(xa, xb) is the Box-Muller pair
 * r = sqrtf(-2 logf(((xa >> 8) + 1) * 2^-24)), th = 6.2831853f * u(xb): (r cosf(th), r sinf(th)), accurate library functions.
 * Draw assignment (every draw exists whether or not its stage is on, so switching a stage never moves another stage's draws):
 *   purpose 0, per cloud:  e = 0: x0, x1, x2 -> rotation angles a = 6.2831853f * u (axis mode uses x0 only; full mode x0, x1, x2 about
 *                                  x, y, z); x3 -> dropout ratio = u(x3) * dropout_max (one float32 product)
 *                          e = 1: perturbation: (g0, g1) = n(x0, x1), (g2, -) = n(x2, x3); angles clip(sigma * g, -clip, clip) about x, y, z
 *                          e = 2: scale lo + (hi - lo) * u: x0 (one for all axes), or x0, x1, x2 (per axis)
 *                          e = 3: translation (2 u - 1) * range: x0, x1, x2 (per axis), or x0 added to all three (scalar)
 *   purpose 1, permutation: point i's 32-bit draw is word i of the stream
 *   purpose 2, jitter:      point i, e = i: (jx, jy) = n(x0, x1), (jz, -) = n(x2, x3); xyz += clip(sigma * j, -clip, clip)
 *   purpose 3, dropout:     point i's u is u(word i of the stream); the row is dropped where u <= ratio (float32 compare)
 *   (purpose 4 is the host-side epoch order of spgan.dataset.DeviceDataset: stream of slot 0 with the epoch in place of step.)
 *
 * Stages in this fixed order, each on or off:
 *   1 gather      row i of cloud b is data[index[b]][i], i < N (the first N stored points)
 *   2 permute     output row i is gathered row perm[i], perm = the point indices in ascending order of the 64-bit keys
 *                 (draw << 32) | index; `keys` uint32 [B,N] (optional) replaces the draws.  Sorted in LDS, one workgroup per cloud.
 *   3 rotate      1: about `axis` (unit vector u; R = c I + s [u]x + (1 - c) u u^T, data_utils.angle_axis); 2: R = Rz Ry Rx
 *   4 perturb     R = Rz Ry Rx of the three clipped normal angles
 *                 with Rx = [1 0 0; 0 c -s; 0 s c], Ry = [c 0 s; 0 1 0; -s 0 c], Rz = [c -s 0; s c 0; 0 0 1] (provider.py).
 *                 A rotation multiplies as xyz @ R (transpose = 0: provider, point_operation) or xyz @ R^T (transpose = 1: data_utils)
 *   5 scale       xyz * s (one s, or one per axis)
 *   6 translate   xyz + t
 *   7 jitter, 8 dropout as above; a dropped row takes the FINAL value (all C channels) of output row 0 of its cloud.
 *   Stages 3-6 are composed once per cloud in float32, A = M3 M4 diag(s) (M = R or R^T; an absent stage is the identity) and t, and applied
 *   as xyz A + t; with all four off and no `params`, xyz passes through bit for bit.  Normals (C = 6) are multiplied by A with every column
 *   divided by its Euclidean norm (= M3 M4 when s > 0): rotated, neither scaled, translated nor jittered.
 *   params float32 [B,16] (optional) replaces stages 3-6: A, t are taken from it (apply-only mode; slots 12..15 are ignored).
 *
 * step: device-resident counter.  The first launch (one workgroup per cloud: parameters, record, sort) reads it and stores its value in
 * the record; the second launch (one thread per output row) takes the value from the record, and its first thread stores step + 1 when
 * `advance` != 0 -- after every reader, by the order of the two launches on the stream.  The wrapper passes advance = 1 whenever the call
 * draws anything.  perm_ws: int32 [B,N] scratch, needed when permute != 0.
 * Bad sizes, C other than 3 or 6, N beyond the limit and null pointers return SPGAN_EINVAL before any launch.
 * ---------------------------------------------------------------------------------------- */
typedef struct spgan_augment_cfg {
  int permute;                                           /* 0 / 1 */
  int rotate; float axis[3]; int transpose;              /* 0 off, 1 about axis (unit length), 2 full Rz Ry Rx */
  int perturb; float perturb_sigma, perturb_clip;        /* 0 / 1 */
  int scale; float scale_lo, scale_hi;                   /* 0 off, 1 one factor, 2 one per axis */
  int translate; float translate_range;                  /* 0 off, 1 one per axis, 2 one scalar for all three */
  int jitter; float jitter_sigma, jitter_clip;           /* 0 / 1 */
  int dropout; float dropout_max;                        /* 0 / 1 */
} spgan_augment_cfg;
int spgan_augment_max_points(void);
int spgan_augment_batch(const float* data, long S, int P, int C, const int64_t* index, int B, int N, int layout, const spgan_augment_cfg* cfg,
                        unsigned long long seed, unsigned long long* step, int advance, const uint32_t* keys, const float* params,
                        int32_t* perm_ws, float* out, float* rec, spgan_stream_t s);
/* out[w] = word w of the stream of (purpose, slot) at `step` under `seed`, w < n_words; purpose < 256, slot < 2^24. */
int spgan_philox_fill(unsigned long long seed, int purpose, int slot, unsigned long long step, long n_words, uint32_t* out, spgan_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* SPGAN_HIP_H */
