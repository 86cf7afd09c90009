// Frechet point-cloud distance (Common/GAN_metrics.py:484-545) in float64 on v_mfma_f64_16x16x4_f64:
//   d^2 = |mu1 - mu2|^2 + tr(S1 + S2 - 2 sqrt(S1 S2)),   tr sqrt(S1 S2) = |R1 R2|_* (nuclear norm),  R = sqrt(S).
// The reference calls scipy.linalg.sqrtm on the host.  Here every step is a matrix product or a fixed-order reduction:
//   * moments:  float32 activations [n,d] -> float64 column sums and the centred Gram matrix Xc^T Xc (converted and centred while the
//               tile is staged; never sum x x^T - n mu mu^T), mergeable chunk by chunk (pairwise update);
//   * product:  C = alpha op(A) B + beta C + diag I for square float64 operands of any d in 2..2048, ragged edges in the kernel;
//   * sqrt:     stages 0 and 1, the coupled Newton-Schulz iteration  T = 1.5 I - 0.5 Z Y,  Y <- Y T,  Z <- T Z  from Y0 = S / |S|_F,
//               Z0 = I, stopped on the device when |Y_new - Y|_F <= 1e-13 |Y_new|_F (rounding-level eigenvalues grow 1.5x per step:
//               the stop is part of the method);
//   * polar:    stage 2, X <- X (1.5 I - 0.5 X^T X) from X0 = R1 R2 / |R1 R2|_F; its singular values rise monotonically to 1, so
//               t = sum X o (R1 R2) rises to the nuclear norm; stopped when t moves by <= 1e-14 t.  A direction that has not converged
//               costs its own singular value times its distance from 1: rounding-level directions cost nothing, which is why this
//               route was chosen over tr sqrt(R1 S2 R1) (there the stop test has to fire before they outgrow it).
// The launch sequence is fixed (FPD_CAP iterations per stage); after a stage's stop its remaining launches return at once, so one
// distance costs one host read, at the end.
// f64 MFMA layout (differs from every other MFMA): A lane l = A[l & 15][l >> 4], B lane l = B[l >> 4][l & 15], one double each;
// C/D register r of lane l = C[(l >> 4) + 4 r][l & 15].
// LDS, 8-byte elements (64 banks x 4 B, a ds_read_b64 is served per half-wave of 32 lanes): a k-major tile [KT][BT + 16] puts the two
// k rows of a half-wave 32 banks apart; the row-major A tile [BT][17] (KT = 16) gives bank 34 r + 2 k and [BT][34] (KT = 32) gives
// 4 r + 2 k, both distinct over 16 rows x 2 k.
#include "common.hpp"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int FPD_CAP = 40;        // iterations per stage
constexpr int RED_BLOCKS = 256;    // partial sums per reduction (fixed: the order of every sum is independent of d)
constexpr double FPD_STOP = 1e-13;    // Newton-Schulz: |Y_new - Y|_F <= FPD_STOP |Y_new|_F
constexpr double FPD_STOP_T = 1e-14;  // polar: |t_new - t| <= FPD_STOP_T |t_new|

// which of a ping-pong pair: (completed iterations + x) & 1
struct Pick {
  const int* it;  // NULL: always [0]
  __device__ __forceinline__ int cur(int x) const { return it ? ((*it + x) & 1) : 0; }
};

struct GemmArgs {
  const double* A[2];
  const double* B[2];
  double* C[2];
  int xa, xb, xc;      // parity offsets of A, B, C
  int ta;              // op(A) = A^T
  const int* it;       // iteration counter of the stage (NULL: plain pointers in [0])
  const int* done;     // stage-finished flag (NULL: always run)
  int d;
  double alpha, beta, diag;
};

struct GramArgs {
  const float* X;          // [n, d]
  int n, d;
  const double* pivot;     // [d] the first row ever seen: every sum is taken of x - pivot, so that a large common mean cancels exactly
  const double* csum;      // [d] column sums of this chunk (of x - pivot)
  const double* osum;      // [d] sums of the rows seen before (merge only)
  double* M2;              // [d, d]
  double na;               // rows seen before; 0: overwrite
};

// One workgroup = 2 x 2 waves, each W x W MFMA tiles of 16 x 16: a (32 W) x (32 W) output tile, K walked KT at a time (32 for the small
// tile, whose waves issue only one MFMA per k step of 4 between two barriers; 16 for the large one).
template <int W, bool GRAM>
struct Core {
  static constexpr int BT = 32 * W, KT = W == 1 ? 32 : 16, EPT = BT * KT / 256, LDK = BT + 16, LDA = KT == 32 ? 34 : 17;
  static constexpr int KSTEP = 256 / BT, RSTEP = 256 / KT;   // k rows (k-major) and tile rows (row-major A) staged per pass
  static constexpr int A_ELEMS = GRAM ? KT * LDK : BT * LDA;

  template <class LoadA, class LoadB, class Store>
  static __device__ __forceinline__ void run(int K, LoadA loadA, LoadB loadB, Store store) {
    __shared__ double As[A_ELEMS];
    __shared__ double Bs[KT * LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 16 * W, wn = (wave & 1) * 16 * W;
    const int l15 = lane & 15, l4 = lane >> 4;
    f64x4 acc[W][W];
#pragma unroll
    for (int i = 0; i < W; ++i)
#pragma unroll
      for (int j = 0; j < W; ++j) acc[i][j] = f64x4{0., 0., 0., 0.};
    double ra[EPT], rb[EPT];
    // k-major staging: thread -> (k = tid / BT + KSTEP p, col = tid % BT); row-major A staging: (row = tid / KT + RSTEP p, k = tid % KT)
    const int kc = tid % BT, kk0 = tid / BT;
    const int ar = tid / KT, ak = tid % KT;
#pragma unroll
    for (int p = 0; p < EPT; ++p) {
      ra[p] = GRAM ? loadA(kk0 + KSTEP * p, kc) : loadA(ak, ar + RSTEP * p);
      rb[p] = loadB(kk0 + KSTEP * p, kc);
    }
    for (int k0 = 0; k0 < K; k0 += KT) {
      __syncthreads();
#pragma unroll
      for (int p = 0; p < EPT; ++p) {
        if (GRAM) As[(kk0 + KSTEP * p) * LDK + kc] = ra[p];
        else As[(ar + RSTEP * p) * LDA + ak] = ra[p];
        Bs[(kk0 + KSTEP * p) * LDK + kc] = rb[p];
      }
      __syncthreads();
      if (k0 + KT < K) {
#pragma unroll
        for (int p = 0; p < EPT; ++p) {
          ra[p] = GRAM ? loadA(k0 + KT + kk0 + KSTEP * p, kc) : loadA(k0 + KT + ak, ar + RSTEP * p);
          rb[p] = loadB(k0 + KT + kk0 + KSTEP * p, kc);
        }
      }
#pragma unroll
      for (int kk = 0; kk < KT / 4; ++kk) {
        double a[W], b[W];
#pragma unroll
        for (int i = 0; i < W; ++i)
          a[i] = GRAM ? As[(kk * 4 + l4) * LDK + wm + i * 16 + l15] : As[(wm + i * 16 + l15) * LDA + kk * 4 + l4];
#pragma unroll
        for (int j = 0; j < W; ++j) b[j] = Bs[(kk * 4 + l4) * LDK + wn + j * 16 + l15];
#pragma unroll
        for (int i = 0; i < W; ++i)
#pragma unroll
          for (int j = 0; j < W; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < W; ++i)
#pragma unroll
      for (int j = 0; j < W; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) store(wm + i * 16 + l4 + 4 * r, wn + j * 16 + l15, acc[i][j][r]);
  }
};

template <int W, bool TA>
__global__ __launch_bounds__(256) void f64_gemm_kernel(GemmArgs g) {
  if (g.done && *g.done) return;
  const Pick pk{g.it};
  const double* __restrict__ A = g.A[pk.cur(g.xa)];
  const double* __restrict__ B = g.B[pk.cur(g.xb)];
  double* __restrict__ C = g.C[pk.cur(g.xc)];
  const int d = g.d, row0 = blockIdx.y * (32 * W), col0 = blockIdx.x * (32 * W);
  Core<W, TA>::run(
      d,
      [&](int k, int r) {
        if (TA) return (k < d && row0 + r < d) ? A[(size_t)k * d + row0 + r] : 0.;   // op(A) = A^T: staged k-major like B
        return (row0 + r < d && k < d) ? A[(size_t)(row0 + r) * d + k] : 0.;
      },
      [&](int k, int c) { return (k < d && col0 + c < d) ? B[(size_t)k * d + col0 + c] : 0.; },
      [&](int r, int c, double v) {
        const int row = row0 + r, col = col0 + c;
        if (row < d && col < d) {
          double o = g.alpha * v;
          if (row == col) o += g.diag;
          if (g.beta != 0.) o += g.beta * C[(size_t)row * d + col];
          C[(size_t)row * d + col] = o;
        }
      });
}

// M2 = Xc^T Xc of one chunk, Xc = (double(X) - pivot) - csum / n; with na > 0 merged into the running state:
// M2 <- (M2 + Xc^T Xc) + (na n / (na + n)) delta delta^T,  delta = csum / n - osum / na.
template <int W>
__global__ __launch_bounds__(256) void gram_kernel(GramArgs g) {
  const int d = g.d, n = g.n, row0 = blockIdx.y * (32 * W), col0 = blockIdx.x * (32 * W);
  const float* __restrict__ X = g.X;
  const double inv_n = 1.0 / (double)n;
  const int kc = threadIdx.x % (32 * W);     // the one column this thread stages on each side
  const double mi = row0 + kc < d ? g.csum[row0 + kc] * inv_n : 0., pi = row0 + kc < d ? g.pivot[row0 + kc] : 0.;
  const double mj = col0 + kc < d ? g.csum[col0 + kc] * inv_n : 0., pj = col0 + kc < d ? g.pivot[col0 + kc] : 0.;
  const bool merge = g.na > 0.;
  const double coef = merge ? g.na * (double)n / (g.na + (double)n) : 0.;
  const double inv_na = merge ? 1.0 / g.na : 0.;
  Core<W, true>::run(
      n,
      [&](int k, int c) { return (k < n && row0 + c < d) ? ((double)X[(size_t)k * d + row0 + c] - pi) - mi : 0.; },
      [&](int k, int c) { return (k < n && col0 + c < d) ? ((double)X[(size_t)k * d + col0 + c] - pj) - mj : 0.; },
      [&](int r, int c, double v) {
        const int row = row0 + r, col = col0 + c;
        if (row < d && col < d) {
          if (merge) {
            const double di = g.csum[row] * inv_n - g.osum[row] * inv_na;
            const double dj = g.csum[col] * inv_n - g.osum[col] * inv_na;
            v = (g.M2[(size_t)row * d + col] + v) + coef * (di * dj);
          }
          g.M2[(size_t)row * d + col] = v;
        }
      });
}

__device__ __forceinline__ double block_sum_f64(double v, double* red) {  // fixed-order tree over 256 threads
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double t = red[0];
  __syncthreads();
  return t;
}

constexpr int SEG = 256;  // rows per column-sum segment

__global__ __launch_bounds__(256) void pivot_init_kernel(const float* __restrict__ X, int d, double* __restrict__ pivot) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < d) pivot[c] = (double)X[c];
}

// part[seg, c] = sum of x - pivot over rows [seg * SEG, ...) of column c: 4 row lanes x 64 columns per workgroup, lanes added in order
__global__ __launch_bounds__(256) void colsum_part_kernel(const float* __restrict__ X, int n, int d, const double* __restrict__ pivot,
                                                          double* __restrict__ part) {
  __shared__ double red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  const int r0 = blockIdx.y * SEG, r1 = min(n, r0 + SEG);
  double s = 0.;
  if (c < d) {
    const double pv = pivot[c];
    for (int r = r0 + q; r < r1; r += 4) s += (double)X[(size_t)r * d + c] - pv;
  }
  red[q][threadIdx.x & 63] = s;
  __syncthreads();
  if (q == 0 && c < d) part[(size_t)blockIdx.y * d + c] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void colsum_final_kernel(const double* __restrict__ part, int segs, int d, double* __restrict__ csum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  double s = 0.;
  for (int k = 0; k < segs; ++k) s += part[(size_t)k * d + c];
  csum[c] = s;
}

// sum <- csum (first chunk) or sum + csum; runs after the Gram kernel, which reads the old sums
__global__ __launch_bounds__(256) void sum_merge_kernel(const double* __restrict__ csum, int d, int first, double* __restrict__ sum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < d) sum[c] = first ? csum[c] : sum[c] + csum[c];
}

// part[b] = sum over the elements of workgroup b of A o B (fixed grid of RED_BLOCKS); A = A0 or A1 by the parity of *it + xa
__global__ __launch_bounds__(256) void dot_part_kernel(const double* A0, const double* A1, const double* B, size_t n, const int* __restrict__ it, int xa,
                                                       const int* __restrict__ done, double* __restrict__ part) {
  if (done && *done) return;
  __shared__ double red[256];
  const double* __restrict__ A = Pick{it}.cur(xa) ? A1 : A0;
  double s = 0.;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)RED_BLOCKS * 256) s += A[e] * B[e];
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// kind 0: trace of A [d,d]; 1: sqrt(sum of the partials); 2: sum of the partials
__global__ __launch_bounds__(256) void reduce_final_kernel(int kind, const double* __restrict__ A, int d, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.;
  if (kind == 0) {
    for (int i = threadIdx.x; i < d; i += 256) s += A[(size_t)i * d + i];
  } else {
    s = part[threadIdx.x];
  }
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) out[0] = kind == 1 ? sqrt(s) : s;
}

// Y0 = src / *nrm (0 where the norm is 0), Z0 = I (Z0 may be NULL)
__global__ __launch_bounds__(256) void scale_prep_kernel(const double* src, const double* __restrict__ nrm, int d, double* Y0, double* __restrict__ Z0) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)d * d) return;
  const double s = *nrm, inv = s > 0. ? 1.0 / s : 0.;
  Y0[e] = src[e] * inv;
  if (Z0) Z0[e] = (e / d == e % d) ? 1. : 0.;
}

// dst = the pair's current member (the stage's result)
__global__ __launch_bounds__(256) void pick_copy_kernel(const double* Y0, const double* Y1, const int* __restrict__ it, size_t n, double* __restrict__ dst) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) dst[e] = ((*it & 1) ? Y1 : Y0)[e];
}

// part[b] = |Y_new - Y|^2, part[RED_BLOCKS + b] = |Y_new|^2 over the elements of workgroup b
__global__ __launch_bounds__(256) void conv_part_kernel(const double* Y0, const double* Y1, size_t n, const int* __restrict__ state, double* __restrict__ part) {
  if (state[0]) return;
  __shared__ double red[256];
  const int cur = state[1] & 1;
  const double* __restrict__ Yo = cur ? Y1 : Y0;
  const double* __restrict__ Yn = cur ? Y0 : Y1;
  double sd = 0., sn = 0.;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)RED_BLOCKS * 256) {
    const double yn = Yn[e], df = yn - Yo[e];
    sd += df * df;
    sn += yn * yn;
  }
  sd = block_sum_f64(sd, red);
  sn = block_sum_f64(sn, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = sd;
    part[RED_BLOCKS + blockIdx.x] = sn;
  }
}

// state = (done, iterations): one more Newton-Schulz iteration is complete; stop on the test, on a non-finite norm, or at the cap
__global__ __launch_bounds__(256) void conv_final_kernel(const double* __restrict__ part, int* __restrict__ state) {
  if (state[0]) return;
  __shared__ double red[256];
  const double sd = block_sum_f64(part[threadIdx.x], red);
  const double sn = block_sum_f64(part[RED_BLOCKS + threadIdx.x], red);
  if (threadIdx.x == 0) {
    const int it = state[1] + 1;
    state[1] = it;
    if (sqrt(sd) <= FPD_STOP * sqrt(sn) || !(sn == sn) || it >= FPD_CAP) state[0] = 1;
  }
}

// one more polar iteration is complete: t = sum of the partials of X_new o X0; *tval = t; the previous t is *tval, or *t0 = |X0|_F
// before the first iteration (X = X0 / |X0|_F)
__global__ __launch_bounds__(256) void polar_final_kernel(const double* __restrict__ part, const double* __restrict__ t0, double* __restrict__ tval,
                                                          int* __restrict__ state) {
  if (state[0]) return;
  __shared__ double red[256];
  const double t = block_sum_f64(part[threadIdx.x], red);
  if (threadIdx.x == 0) {
    const double told = state[1] == 0 ? *t0 : *tval;
    const int it = state[1] + 1;
    state[1] = it;
    *tval = t;
    if (fabs(t - told) <= FPD_STOP_T * fabs(t) || !(t == t) || it >= FPD_CAP) state[0] = 1;
  }
}

// out = [distance, iterations of stages 0, 1, 2, tr sqrt(S1 S2)];  scal = (|S1|_F, |S2|_F, |Y1 Y2|_F, t)
__global__ __launch_bounds__(256) void fpd_final_kernel(const double* __restrict__ mu1, const double* __restrict__ S1, const double* __restrict__ mu2,
                                                        const double* __restrict__ S2, int d, const double* __restrict__ scal,
                                                        const int* __restrict__ state, double* __restrict__ out) {
  __shared__ double red[256];
  double dm = 0., t1 = 0., t2 = 0.;
  for (int i = threadIdx.x; i < d; i += 256) {
    const double df = mu1[i] - mu2[i];
    dm += df * df;
    t1 += S1[(size_t)i * d + i];
    t2 += S2[(size_t)i * d + i];
  }
  dm = block_sum_f64(dm, red);
  t1 = block_sum_f64(t1, red);
  t2 = block_sum_f64(t2, red);
  if (threadIdx.x == 0) {
    const double cm = sqrt(scal[0]) * sqrt(scal[1]) * scal[3];  // R = sqrt(|S|_F) Y, t = |Y1 Y2|_*
    out[0] = ((dm + t1) + t2) - 2. * cm;
    out[1] = (double)state[1];
    out[2] = (double)state[3];
    out[3] = (double)state[5];
    out[4] = cm;
  }
}

template <int W>
void launch_gemm_w(const GemmArgs& g, hipStream_t s) {
  const int t = cdiv(g.d, 32 * W);
  if (g.ta) hipLaunchKernelGGL((f64_gemm_kernel<W, true>), dim3(t, t), dim3(256), 0, s, g);
  else hipLaunchKernelGGL((f64_gemm_kernel<W, false>), dim3(t, t), dim3(256), 0, s, g);
}

// 32 x 32 tiles below GEMM_WIDE_D, 64 x 64 from there on.  The instruction is slow enough (a register-only loop needs 8 waves per SIMD
// to reach its rate) that more resident waves beat more accumulators per wave: measured, both with a K step of 16, 31 against 28 TFLOP/s
// at d = 1024 and 36 against 33 at d = 1536 for the small tile, 33 against 36 at d = 1808 and 37 against 46 at d = 2048 for the large one.
constexpr int GEMM_WIDE_D = 1664;
void launch_gemm(const GemmArgs& g, hipStream_t s) {
  if (g.d >= GEMM_WIDE_D) launch_gemm_w<2>(g, s);
  else launch_gemm_w<1>(g, s);
}

size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" int spgan_f64_gemm(const double* A, const double* B, double* C, int d, int trans_a, double alpha, double beta, double diag,
                              spgan_stream_t s_) {
  SPGAN_CHECK_ARG(A && B && C && d >= 2 && d <= 2048 && C != A && C != B);
  GemmArgs g{};
  g.A[0] = g.A[1] = A; g.B[0] = g.B[1] = B; g.C[0] = g.C[1] = C;
  g.d = d; g.ta = trans_a ? 1 : 0; g.alpha = alpha; g.beta = beta; g.diag = diag;
  launch_gemm(g, (hipStream_t)s_);
  return spgan_launch_status();
}

extern "C" size_t spgan_f64_reduce_ws_bytes(void) { return RED_BLOCKS * sizeof(double); }

extern "C" int spgan_f64_reduce(int kind, const double* A, const double* B, int d, double* out, void* ws, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(A && out && ws && d >= 1 && d <= 2048 && kind >= 0 && kind <= 2 && (kind != 2 || B));
  hipStream_t s = (hipStream_t)s_;
  double* part = (double*)ws;
  if (kind != 0)
    hipLaunchKernelGGL(dot_part_kernel, dim3(RED_BLOCKS), dim3(256), 0, s, A, A, kind == 1 ? A : B, (size_t)d * d, (const int*)nullptr, 0,
                       (const int*)nullptr, part);
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(256), 0, s, kind, A, d, part, out);
  return spgan_launch_status();
}

extern "C" size_t spgan_fpd_moments_ws_bytes(int n, int d) {
  if (n < 1 || d < 2 || d > 2048) return 0;
  return ((size_t)cdiv(n, SEG) + 1) * d * sizeof(double);
}

extern "C" int spgan_fpd_moments_update(const float* X, int n, int d, long count_before, double* sum2, double* M2, void* ws, size_t ws_bytes,
                                        spgan_stream_t s_) {
  SPGAN_CHECK_ARG(X && sum2 && M2 && ws && n >= 1 && d >= 2 && d <= 2048 && count_before >= 0);
  SPGAN_CHECK_ARG(ws_bytes >= spgan_fpd_moments_ws_bytes(n, d));
  hipStream_t s = (hipStream_t)s_;
  const int segs = cdiv(n, SEG);
  double* csum = (double*)ws;
  double* part = csum + d;
  double* pivot = sum2;
  double* sum = sum2 + d;
  if (count_before == 0) hipLaunchKernelGGL(pivot_init_kernel, dim3(cdiv(d, 256)), dim3(256), 0, s, X, d, pivot);
  hipLaunchKernelGGL(colsum_part_kernel, dim3(cdiv(d, 64), segs), dim3(256), 0, s, X, n, d, pivot, part);
  hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(d, 256)), dim3(256), 0, s, part, segs, d, csum);
  GramArgs g{X, n, d, pivot, csum, sum, M2, (double)count_before};
  if (d >= 1024) {
    const int t = cdiv(d, 64);
    hipLaunchKernelGGL(gram_kernel<2>, dim3(t, t), dim3(256), 0, s, g);
  } else {
    const int t = cdiv(d, 32);
    hipLaunchKernelGGL(gram_kernel<1>, dim3(t, t), dim3(256), 0, s, g);
  }
  hipLaunchKernelGGL(sum_merge_kernel, dim3(cdiv(d, 256)), dim3(256), 0, s, csum, d, count_before == 0 ? 1 : 0, sum);
  return spgan_launch_status();
}

extern "C" int spgan_fpd_max_iterations(void) { return FPD_CAP; }

extern "C" size_t spgan_fpd_distance_ws_bytes(int d) {
  if (d < 2 || d > 2048) return 0;
  return 6 * al256((size_t)d * d * sizeof(double)) + al256(2 * RED_BLOCKS * sizeof(double)) + 256;
}

extern "C" int spgan_fpd_distance(const double* mu1, const double* S1, const double* mu2, const double* S2, int d, double* out5, void* ws,
                                  size_t ws_bytes, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(mu1 && S1 && mu2 && S2 && out5 && ws && d >= 2 && d <= 2048 && ws_bytes >= spgan_fpd_distance_ws_bytes(d));
  hipStream_t s = (hipStream_t)s_;
  const size_t mat = al256((size_t)d * d * sizeof(double)), nel = (size_t)d * d;
  char* w = (char*)ws;
  double* Y[2] = {(double*)w, (double*)(w + mat)};
  double* Z[2] = {(double*)(w + 2 * mat), (double*)(w + 3 * mat)};
  double* T = (double*)(w + 4 * mat);
  double* R = (double*)(w + 5 * mat);
  double* part = (double*)(w + 6 * mat);
  double* scal = (double*)(w + 6 * mat + al256(2 * RED_BLOCKS * sizeof(double)));  // |S1|_F, |S2|_F, |Y1 Y2|_F, t
  int* state = (int*)(scal + 4);                                                   // (done, iterations) per stage
  const int* none = nullptr;
  const int eb = cdiv((long)nel, 256);
  (void)hipMemsetAsync(state, 0, 6 * sizeof(int), s);
  // stages 0 and 1: Y -> sqrt(S / |S|_F) in Y[iterations & 1]
  for (int stage = 0; stage < 2; ++stage) {
    int* st = state + 2 * stage;
    const double* S = stage == 0 ? S1 : S2;
    hipLaunchKernelGGL(dot_part_kernel, dim3(RED_BLOCKS), dim3(256), 0, s, S, S, S, nel, none, 0, none, part);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(256), 0, s, 1, S, d, part, scal + stage);
    hipLaunchKernelGGL(scale_prep_kernel, dim3(eb), dim3(256), 0, s, S, scal + stage, d, Y[0], Z[0]);
    for (int k = 0; k < FPD_CAP; ++k) {
      GemmArgs g{};
      g.d = d; g.it = st + 1; g.done = st;
      // T = 1.5 I - 0.5 Z Y
      g.A[0] = Z[0]; g.A[1] = Z[1]; g.B[0] = Y[0]; g.B[1] = Y[1]; g.C[0] = g.C[1] = T;
      g.alpha = -0.5; g.diag = 1.5;
      launch_gemm(g, s);
      // Y_new = Y T
      g.A[0] = Y[0]; g.A[1] = Y[1]; g.B[0] = g.B[1] = T; g.C[0] = Y[0]; g.C[1] = Y[1]; g.xc = 1;
      g.alpha = 1.; g.diag = 0.;
      launch_gemm(g, s);
      // Z_new = T Z
      g.A[0] = g.A[1] = T; g.B[0] = Z[0]; g.B[1] = Z[1]; g.C[0] = Z[0]; g.C[1] = Z[1];
      launch_gemm(g, s);
      hipLaunchKernelGGL(conv_part_kernel, dim3(RED_BLOCKS), dim3(256), 0, s, Y[0], Y[1], nel, st, part);
      hipLaunchKernelGGL(conv_final_kernel, dim3(1), dim3(256), 0, s, part, st);
    }
    if (stage == 0) hipLaunchKernelGGL(pick_copy_kernel, dim3(eb), dim3(256), 0, s, Y[0], Y[1], st + 1, nel, R);
  }
  // stage 2: X0 = Y1 Y2 into Z[0]; X = X0 / |X0|_F in Y[0], then the polar iteration on the pair Y
  double* X0 = Z[0];
  {
    GemmArgs g{};
    g.d = d; g.alpha = 1.; g.it = state + 3;
    g.A[0] = g.A[1] = R; g.B[0] = Y[0]; g.B[1] = Y[1]; g.C[0] = g.C[1] = X0;
    launch_gemm(g, s);
    hipLaunchKernelGGL(dot_part_kernel, dim3(RED_BLOCKS), dim3(256), 0, s, X0, X0, X0, nel, none, 0, none, part);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(256), 0, s, 1, X0, d, part, scal + 2);
    hipLaunchKernelGGL(scale_prep_kernel, dim3(eb), dim3(256), 0, s, X0, scal + 2, d, Y[0], (double*)nullptr);
  }
  int* st = state + 4;
  for (int k = 0; k < FPD_CAP; ++k) {
    GemmArgs g{};
    g.d = d; g.it = st + 1; g.done = st;
    // T = 1.5 I - 0.5 X^T X
    g.A[0] = Y[0]; g.A[1] = Y[1]; g.B[0] = Y[0]; g.B[1] = Y[1]; g.C[0] = g.C[1] = T; g.ta = 1;
    g.alpha = -0.5; g.diag = 1.5;
    launch_gemm(g, s);
    // X_new = X T
    g.ta = 0; g.B[0] = g.B[1] = T; g.C[0] = Y[0]; g.C[1] = Y[1]; g.xc = 1;
    g.alpha = 1.; g.diag = 0.;
    launch_gemm(g, s);
    hipLaunchKernelGGL(dot_part_kernel, dim3(RED_BLOCKS), dim3(256), 0, s, Y[0], Y[1], X0, nel, st + 1, 1, st, part);
    hipLaunchKernelGGL(polar_final_kernel, dim3(1), dim3(256), 0, s, part, scal + 2, scal + 3, st);
  }
  hipLaunchKernelGGL(fpd_final_kernel, dim3(1), dim3(256), 0, s, mu1, S1, mu2, S2, d, scal, state, out5);
  return spgan_launch_status();
}
