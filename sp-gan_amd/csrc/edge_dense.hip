// The dense family of Common/utilities.py (DenseEdgeModule, DenseModule1D): a product whose A operand is the virtual concatenation of
// stored pre-norm blocks, each activated while it is staged, so that neither the concatenation nor an activated per-edge tensor exists
// (include/spgan_hip.h: "Dense edge / point layers").  fp32-input MFMA (v_mfma_f32_32x32x2_f32): exact fp32 products.
#include "common.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128;        // rows of a workgroup's tile = the tile of the (sum, M2) records
constexpr int BN = 64;         // output columns of a workgroup: two 32x32 accumulators per wave
constexpr int BK = 32;         // reduction step staged in LDS
constexpr int LDT = BK + 1;    // row stride of both LDS tiles: lane l reads row (l & 31), column kk + (l >> 5): conflict free
constexpr int A_PER = BM * BK / 256;   // staged elements per thread
constexpr int W_PER = BN * BK / 256;

struct LevelArgs {
  const float* A; int lda;
  const float* W; int ldw;
  const float* scale; const float* shift; float slope; int raw_cols;
  const float* bias;
  const float* PQ; int ldpq; int qoff; const int32_t* idx; int k;     // the addend Q[row / k] + P[idx[row]]: P at column 0, Q at column qoff
  float* Y; int ldy;
  float* part;
  int M, N, K;
};

// thread t stages column (t & 31) of rows (t >> 5) + 8 * u: one 128-byte row segment per half wave
struct ScalarStage {
  float ra[A_PER], rw[W_PER];
  __device__ __forceinline__ void load(const LevelArgs& a, int m0, int n0, int k0, int t) {
    const int c = k0 + (t & 31);
    const bool cin = c < a.K;
    float sc = 1.f, sh = 0.f;
    const bool act = cin && c >= a.raw_cols;
    if (act) { sc = a.scale[c]; sh = a.shift[c]; }
#pragma unroll
    for (int u = 0; u < A_PER; ++u) {
      const int m = m0 + (t >> 5) + 8 * u;
      float v = 0.f;
      if (cin && m < a.M) {
        v = a.A[(size_t)m * a.lda + c];
        if (act) v = lrelu_f(v * sc + sh, a.slope);
      }
      ra[u] = v;
    }
#pragma unroll
    for (int u = 0; u < W_PER; ++u) {
      const int n = n0 + (t >> 5) + 8 * u;
      rw[u] = (cin && n < a.N) ? a.W[(size_t)n * a.ldw + c] : 0.f;
    }
  }
  __device__ __forceinline__ void store(float* As, float* Ws, int t) const {
#pragma unroll
    for (int u = 0; u < A_PER; ++u) As[((t >> 5) + 8 * u) * LDT + (t & 31)] = ra[u];
#pragma unroll
    for (int u = 0; u < W_PER; ++u) Ws[((t >> 5) + 8 * u) * LDT + (t & 31)] = rw[u];
  }
};

// thread t stages columns 4 * (t & 7) .. + 3 of rows (t >> 3) + 32 * u with one 16-byte load each: the launcher takes this path when
// both operands' row strides are multiples of 4 floats and their bases 16-byte aligned.  The last group of a row may reach past K
// (K % 4 != 0): it is loaded element by element.
struct VectorStage {
  f32x4 ra[A_PER / 4], rw[W_PER / 4];
  __device__ __forceinline__ static f32x4 row4(const float* p, int c, int K) {
    if (c + 3 < K) return *reinterpret_cast<const f32x4*>(p + c);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < K) v[e] = p[c + e];
    return v;
  }
  __device__ __forceinline__ void load(const LevelArgs& a, int m0, int n0, int k0, int t) {
    const int c = k0 + 4 * (t & 7);
    float sc[4], sh[4];
    bool act[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      act[e] = c + e < a.K && c + e >= a.raw_cols;
      sc[e] = act[e] ? a.scale[c + e] : 1.f;
      sh[e] = act[e] ? a.shift[c + e] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < A_PER / 4; ++u) {
      const int m = m0 + (t >> 3) + 32 * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m < a.M) {
        v = row4(a.A + (size_t)m * a.lda, c, a.K);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (act[e]) v[e] = lrelu_f(v[e] * sc[e] + sh[e], a.slope);
      }
      ra[u] = v;
    }
#pragma unroll
    for (int u = 0; u < W_PER / 4; ++u) {
      const int n = n0 + (t >> 3) + 32 * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (n < a.N) v = row4(a.W + (size_t)n * a.ldw, c, a.K);
      rw[u] = v;
    }
  }
  __device__ __forceinline__ void store(float* As, float* Ws, int t) const {
#pragma unroll
    for (int u = 0; u < A_PER / 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) As[((t >> 3) + 32 * u) * LDT + 4 * (t & 7) + e] = ra[u][e];
#pragma unroll
    for (int u = 0; u < W_PER / 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) Ws[((t >> 3) + 32 * u) * LDT + 4 * (t & 7) + e] = rw[u][e];
  }
};

// sum of v over the BM rows of the tile for the column this lane holds in accumulator j: the lane's 16 rows, then the other half
// wave (same column, other rows), then the four waves through LDS -- a fixed order
__device__ __forceinline__ float tile_colsum(float v, float (*red)[BN], int wave, int lane, int j) {
  v += __shfl_xor(v, 32);
  __syncthreads();                      // the previous use of red is over
  if (lane < 32) red[wave][j * 32 + lane] = v;
  __syncthreads();
  const int c = j * 32 + (lane & 31);
  return (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

template <class Stage>
__global__ __launch_bounds__(256) void edge_dense_level_kernel(const LevelArgs a) {
  __shared__ float As[BM * LDT];
  __shared__ float Ws[BN * LDT];
  __shared__ float red[4][BN];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  Stage st;
  if (a.K > 0) st.load(a, m0, n0, 0, t);
  for (int k0 = 0; k0 < a.K; k0 += BK) {
    __syncthreads();                    // the previous step's reads of the tiles are over
    st.store(As, Ws, t);
    __syncthreads();
    if (k0 + BK < a.K) st.load(a, m0, n0, k0 + BK, t);                 // in flight during the products below
    const float* ap = &As[(wave * 32 + (lane & 31)) * LDT + (lane >> 5)];
    const float* w0 = &Ws[(lane & 31) * LDT + (lane >> 5)];
    const float* w1 = w0 + 32 * LDT;
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const float av = ap[kk];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, w0[kk], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, w1[kk], acc[1], 0, 0, 0);
    }
  }

  // C/D map of the 32x32 shape: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  const int rbase = m0 + wave * 32 + 4 * (lane >> 5);
  const int rows_valid = min(BM, a.M - m0);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + j * 32 + (lane & 31);
    const bool nin = n < a.N;
    const float bv = (nin && a.bias) ? a.bias[n] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = rbase + (r & 3) + 8 * (r >> 2);
      float v = 0.f;
      if (nin && m < a.M) {
        v = acc[j][r] + bv;
        if (a.PQ) {
          const int i = m / a.k;
          int nb = a.idx[m];
          if ((unsigned)nb >= (unsigned)(a.M / a.k)) nb = i;     // a row outside the cloud is never read
          v += a.PQ[(size_t)i * a.ldpq + a.qoff + n] + a.PQ[(size_t)nb * a.ldpq + n];
        }
        a.Y[(size_t)m * a.ldy + n] = v;
      }
      acc[j][r] = v;
      s += v;
    }
    if (a.part) {                       // uniform over the workgroup
      const float mean = tile_colsum(s, red, wave, lane, j) / (float)rows_valid;
      float q = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = rbase + (r & 3) + 8 * (r >> 2);
        const float d = acc[j][r] - mean;
        if (m < a.M) q += d * d;
      }
      const float m2 = tile_colsum(q, red, wave, lane, j);
      if (wave == 0 && lane < 32 && nin) {
        float* p = a.part + ((size_t)blockIdx.x * a.N + n) * 2;
        p[0] = mean * (float)rows_valid;
        p[1] = m2;
      }
    }
  }
}

// one workgroup row per point, one thread per column: dP = the sum over the in-edge list, dQ = the sum over the point's own k ranks
__global__ __launch_bounds__(256) void edge_dense_scatter_kernel(const float* __restrict__ D, int ldd, const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ src, int M, int k, int C,
                                                                 float* __restrict__ dPQ, int ldo) {
  const int i = blockIdx.x;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= C) return;
  const size_t E = (size_t)M * k;
  float q = 0.f;
  for (int r = 0; r < k; ++r) q += D[((size_t)i * k + r) * ldd + c];
  float p = 0.f;
  const int e0 = max(rowptr[i], 0), e1 = (int)min((size_t)max(rowptr[i + 1], 0), E);
  for (int s = e0; s < e1; ++s) {
    const int e = src[s];
    if ((unsigned)e < E) p += D[(size_t)e * ldd + c];
  }
  dPQ[(size_t)i * ldo + c] = p;
  dPQ[(size_t)i * ldo + C + c] = q;
}

__global__ __launch_bounds__(256) void edge_dense_bn_apply_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ z, int ldz,
                                                                  size_t total, int C, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                  const float* __restrict__ sums, float rcount, float* __restrict__ dz,
                                                                  int ldd) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const size_t m = t / C;
  const int c = (int)(t - m * C);
  const float inv = invstd[c];
  const float xh = (z[m * ldz + c] - mean[c]) * inv;
  const float ga = gamma ? gamma[c] : 1.f;
  dz[m * ldd + c] = ga * inv * (g[m * ldg + c] - sums[c] * rcount - xh * (sums[C + c] * rcount));
}

}  // namespace

extern "C" int spgan_edge_dense_level(const float* A, int lda, int raw_cols, const float* scale, const float* shift, float slope, const float* W,
                                      int ldw, const float* bias, const float* PQ, int ldpq, int qoff, const int32_t* idx, int k, int M, int N,
                                      int K, float* Y, int ldy, float* partials, spgan_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  SPGAN_CHECK_ARG(Y && M > 0 && N > 0 && K >= 0 && ldy >= N);
  SPGAN_CHECK_ARG(K == 0 || (A && W && lda >= K && ldw >= K && raw_cols >= 0 && raw_cols <= K));
  SPGAN_CHECK_ARG(K == 0 || raw_cols == K || (scale && shift));
  SPGAN_CHECK_ARG(K > 0 || PQ || bias);
  SPGAN_CHECK_ARG(!PQ || (idx && k >= 1 && M % k == 0 && qoff >= N && ldpq >= qoff + N));
  SPGAN_CHECK_ARG(cdiv(N, BN) <= 65535);
  LevelArgs a;
  a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.scale = scale; a.shift = shift; a.slope = slope; a.raw_cols = raw_cols; a.bias = bias;
  a.PQ = PQ; a.ldpq = ldpq; a.qoff = qoff; a.idx = idx; a.k = PQ ? k : 1; a.Y = Y; a.ldy = ldy; a.part = partials; a.M = M; a.N = N; a.K = K;
  auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  if (K > 0 && lda % 4 == 0 && ldw % 4 == 0 && al(A) && al(W))
    hipLaunchKernelGGL(edge_dense_level_kernel<VectorStage>, dim3(cdiv(M, BM), cdiv(N, BN)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(edge_dense_level_kernel<ScalarStage>, dim3(cdiv(M, BM), cdiv(N, BN)), dim3(256), 0, s, a);
  return spgan_launch_status();
}

extern "C" int spgan_edge_dense_tile_rows(void) { return BM; }

extern "C" int spgan_edge_dense_scatter(const float* D, int ldd, const int32_t* rowptr, const int32_t* src, int M, int k, int C, float* dPQ,
                                        int ldo, spgan_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  SPGAN_CHECK_ARG(D && rowptr && src && dPQ && M > 0 && k >= 1 && C > 0 && ldd >= C && ldo >= 2 * C && cdiv(C, 256) <= 65535);
  hipLaunchKernelGGL(edge_dense_scatter_kernel, dim3(M, cdiv(C, 256)), dim3(256), 0, s, D, ldd, rowptr, src, M, k, C, dPQ, ldo);
  return spgan_launch_status();
}

extern "C" int spgan_edge_dense_bn_apply(const float* g, int ldg, const float* z, int ldz, int M, int C, const float* mean, const float* invstd,
                                         const float* gamma, const float* sums, int count, float* dz, int ldd, spgan_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  SPGAN_CHECK_ARG(g && z && dz && mean && invstd && sums && M > 0 && C > 0 && ldg >= C && ldz >= C && ldd >= C && count > 0);
  const size_t total = (size_t)M * C;
  hipLaunchKernelGGL(edge_dense_bn_apply_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, g, ldg, z, ldz, total, C, mean, invstd, gamma, sums,
                     1.0f / (float)count, dz, ldd);
  return spgan_launch_status();
}
