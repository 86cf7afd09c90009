// PointNet++ set abstraction / feature propagation kernels (Common/pointnet_util.py:146-320 and the extension ops they stand for,
// metrics/pointnet2_ops: three_nn, three_interpolate and its gradient).  The shared MLPs of the modules run on the GEMM / BatchNorm
// kernels of the rest of the library (gemm.hip, norm.hip); this file holds what those do not cover:
//   * three_nn:              the 3 nearest centres of every point and their inverse-distance weights in one launch, no [B,N,S] matrix
//   * three_interpolate:     the weighted gather (optionally into a column slice of a wider row buffer) and its deterministic adjoint
//   * group_max (+ adjoint): BatchNorm + (leaky) ReLU + max over the K consecutive rows of a centre, arg-max saved as int32
//   * cm_to_rows/rows_to_cm: [B,C,N] <-> a column slice of a [B*N, ld] row buffer (the `torch.cat` of pointnet_util.py:312 without a launch
//                            of its own: both halves are written into one buffer)
// All of it is HBM/latency-bound fp32 + integer work: one thread per output element (or per query, streaming the centres through
// LDS tiles as spgan_knn_point does), vector stores only, no float atomics.
#include "common.hpp"
#include "pointnet_dist.hpp"

namespace {

// idx[b,n,0..k) = the k = min(3,S) nearest centres of point n, ascending distance, lower index first on exact ties;
// weight = (1/(d+1e-8)) / sum_j (1/(d_j+1e-8))      pointnet_util.py:301-307
// The squared distance is sqdist_expanded -- the arithmetic of square_distance_kernel (pointnet.hip), which reproduces the reference's
// `-2ab + |a|^2 + |b|^2` form bit for bit (golden G9): a point that coincides with a centre (xyz2 is normally an FPS subset of xyz1)
// gets the reference's tiny, possibly non-zero or negative distance and therefore the reference's weights, not an exact 0.
// The reference materialises and sorts [B,N,S]; here every thread keeps a running top-3 while the centres stream through LDS.
__global__ __launch_bounds__(256) void three_nn_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2, int N, int S, int k,
                                                       int64_t* __restrict__ idx, float* __restrict__ weight) {
  constexpr int TC = 256, C = 3;
  __shared__ float cand[TC * C];
  __shared__ float cn[TC];
  const int b = blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const bool ok = n < N;
  float q[C];
#pragma unroll
  for (int c = 0; c < C; ++c) q[c] = ok ? xyz1[((size_t)b * N + n) * C + c] : 0.f;
  float qn = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) qn = fmaf(q[c], q[c], qn);
  float bd[3];
  int bi[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) { bd[t] = INFINITY; bi[t] = 0; }
  for (int c0 = 0; c0 < S; c0 += TC) {
    const int nc = min(TC, S - c0);
    __syncthreads();
    for (int e = threadIdx.x; e < nc * C; e += 256) cand[e] = xyz2[((size_t)b * S + c0) * C + e];
    __syncthreads();
    if (threadIdx.x < nc) cn[threadIdx.x] = norm2(cand + threadIdx.x * C, C);
    __syncthreads();
    if (!ok) continue;
    for (int j = 0; j < nc; ++j) {
      const float d = sqdist_expanded<C>(q, qn, cand + j * C, cn[j]);
      if (d < bd[2]) {   // strict: on an exact tie the earlier (lower) index stays in front
        bd[2] = d;
        bi[2] = c0 + j;
#pragma unroll
        for (int t = 2; t > 0; --t)
          if (bd[t] < bd[t - 1]) {
            const float td = bd[t]; bd[t] = bd[t - 1]; bd[t - 1] = td;
            const int ti = bi[t]; bi[t] = bi[t - 1]; bi[t - 1] = ti;
          }
      }
    }
  }
  if (!ok) return;
  float r[3], norm = 0.f;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    r[t] = t < k ? 1.0f / (bd[t] + 1e-8f) : 0.f;
    if (t < k) norm = t == 0 ? r[0] : norm + r[t];
  }
#pragma unroll
  for (int t = 0; t < 3; ++t)
    if (t < k) {
      idx[((size_t)b * N + n) * k + t] = bi[t];
      weight[((size_t)b * N + n) * k + t] = r[t] / norm;
    }
}

// out[(b*N+n)*ld + col0 + c] = sum_j weight[b,n,j] * points2[b, idx[b,n,j], c]      pointnet_util.py:308
// (products rounded, then summed in slot order, like the reference's elementwise product + sum over dim 2)
__global__ void three_interpolate_kernel(const float* __restrict__ points2, const int64_t* __restrict__ idx, const float* __restrict__ weight,
                                         int N, int S, int D, int k, size_t total, float* __restrict__ out, int ld, int col0, int* __restrict__ bad) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const size_t row = t / D;      // (b, n)
  const int c = t % D;
  const size_t b = row / N;
  float acc = 0.f;
  for (int j = 0; j < k; ++j) {
    const int64_t s = idx[row * k + j];
    if (s < 0 || s >= S) { if (bad) atomicOr(bad, 1); continue; }
    const float v = __fmul_rn(points2[((size_t)b * S + s) * D + c], weight[row * k + j]);
    acc = j == 0 ? v : __fadd_rn(acc, v);
  }
  out[row * ld + col0 + c] = acc;
}

// dpoints2[m, c] = sum over the slots e = (b, n, j) that read centre m (ascending, spgan_gather_csr) of weight[e] * dout[(e/k)*ld + col0 + c]
// (metrics/pointnet2_ops three_interpolate_grad is an atomicAdd scatter; here a gather over per-centre slot lists: deterministic)
__global__ void three_interpolate_bwd_kernel(const float* __restrict__ dout, int ld, int col0, int D, const float* __restrict__ weight, int k,
                                             const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src, size_t total,
                                             float* __restrict__ dpoints2) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const size_t m = t / D;
  const int c = t % D;
  float acc = 0.f;
  for (int e = rowptr[2 * m], e1 = rowptr[2 * m + 1]; e < e1; ++e) {
    const int slot = src[e];
    acc = fmaf(weight[slot], dout[(size_t)(slot / k) * ld + col0 + c], acc);
  }
  dpoints2[t] = acc;
}

// pooled[q,c] = max_j lrelu(y[(q*K+j)*ld + c]*scale[c] + shift[c], slope), argmax = the global row q*K+j of the first maximum
// pointnet_util.py:203-205, 261-262 (BatchNorm + ReLU of the last layer fused in front of the max; slope 0 = ReLU)
__global__ void group_max_kernel(const float* __restrict__ y, int ld, int K, int C, const float* __restrict__ scale, const float* __restrict__ shift,
                                 float slope, size_t total, float* __restrict__ pooled, int32_t* __restrict__ argmax) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const size_t q = t / C;
  const int c = t % C;
  const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
  const float* p = y + q * K * (size_t)ld + c;
  float best = -INFINITY;
  int bj = 0;
  for (int j = 0; j < K; ++j) {
    const float v = lrelu_f(fmaf(p[(size_t)j * ld], sc, sh), slope);
    if (v > best) { best = v; bj = j; }
  }
  pooled[t] = best;
  argmax[t] = (int32_t)(q * K + bj);
}

// The adjoint of group_max as the dense incoming gradient of the last layer's BatchNorm backward:
//   g[(q*K+j), c] = row == argmax[q,c] ? gpool[q,c] * lrelu'(pooled[q,c]) : 0
//   gstat[q, c] = that value, gstat[q, C + c] = that value * xhat(y[argmax row, c])   -- column-summed by the caller into the BatchNorm
//   backward's (sum g | sum g*xhat) with the library's deterministic column reduction.
// argmax == NULL (K = 1): every row is its own group (the per-point ReLU behind the last layer of feature propagation).
__global__ void group_max_bwd_kernel(const float* __restrict__ gpool, const float* __restrict__ pooled, const int32_t* __restrict__ argmax,
                                     const float* __restrict__ y, int ld, const float* __restrict__ mean, const float* __restrict__ invstd,
                                     float slope, int K, int C, size_t total, float* __restrict__ g, float* __restrict__ gstat) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const size_t row = t / C;      // q*K + j
  const int c = t % C;
  const size_t q = row / K;
  const size_t qc = q * C + c;
  const size_t arow = argmax ? (size_t)argmax[qc] : q;
  const float gv = gpool[qc] * lrelu_mask(pooled[qc], slope);
  g[t] = row == arow ? gv : 0.f;
  if (row == q * K) {
    gstat[q * 2 * C + c] = gv;
    gstat[q * 2 * C + C + c] = gv * ((y[arow * ld + c] - mean[c]) * invstd[c]);
  }
}

// out[(b*N+n)*ld + col0 + c] = x[b,c,n]  /  x[b,c,n] = src[(b*N+n)*ld + col0 + c]      (32 x 32 tiles through LDS: both sides coalesced)
template <bool TO_ROWS>
__global__ __launch_bounds__(256) void cm_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int N, int ld, int col0) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  if (TO_ROWS) {
    for (int r = ty; r < 32; r += 8) {
      const int c = c0 + r, n = n0 + tx;
      tile[r][tx] = (c < C && n < N) ? src[((size_t)b * C + c) * N + n] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int n = n0 + r, c = c0 + tx;
      if (n < N && c < C) dst[((size_t)b * N + n) * ld + col0 + c] = tile[tx][r];
    }
  } else {
    for (int r = ty; r < 32; r += 8) {
      const int n = n0 + r, c = c0 + tx;
      tile[r][tx] = (n < N && c < C) ? src[((size_t)b * N + n) * ld + col0 + c] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int c = c0 + r, n = n0 + tx;
      if (c < C && n < N) dst[((size_t)b * C + c) * N + n] = tile[tx][r];
    }
  }
}

}  // namespace

extern "C" int spgan_three_nn(const float* xyz1, const float* xyz2, int B, int N, int S, int64_t* idx, float* weight, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz1 && xyz2 && idx && weight && B > 0 && N > 0 && S > 0 && B <= 65535);
  const int k = S < 3 ? S : 3;
  hipLaunchKernelGGL(three_nn_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, (hipStream_t)s_, xyz1, xyz2, N, S, k, idx, weight);
  return spgan_launch_status();
}

extern "C" int spgan_three_interpolate(const float* points2, const int64_t* idx, const float* weight, int B, int N, int S, int D, int k,
                                       float* out, int ld_out, int col0, int32_t* bad, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(points2 && idx && weight && out && B > 0 && N > 0 && S > 0 && D > 0 && k > 0 && k <= 3 && col0 >= 0 && col0 + D <= ld_out);
  const size_t total = (size_t)B * N * D;
  SPGAN_CHECK_ARG(total / 256 < 2147483647u);
  hipLaunchKernelGGL(three_interpolate_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, points2, idx, weight, N, S, D, k, total, out,
                     ld_out, col0, (int*)bad);
  return spgan_launch_status();
}

extern "C" int spgan_three_interpolate_bwd(const float* dout, int ld, int col0, int D, const float* weight, int k, const int32_t* rowptr,
                                           const int32_t* src, int BS, float* dpoints2, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dout && weight && rowptr && src && dpoints2 && ld > 0 && col0 >= 0 && D > 0 && col0 + D <= ld && k > 0 && k <= 3 && BS > 0);
  const size_t total = (size_t)BS * D;
  hipLaunchKernelGGL(three_interpolate_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, dout, ld, col0, D, weight, k, rowptr, src,
                     total, dpoints2);
  return spgan_launch_status();
}

extern "C" int spgan_group_max(const float* y, int ld, int Q, int K, int C, const float* scale, const float* shift, float slope, float* pooled,
                               int32_t* argmax, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(y && pooled && argmax && Q > 0 && K > 0 && C > 0 && ld >= C && (!scale == !shift) && (uint64_t)Q * (uint64_t)K < (1ull << 31));
  const size_t total = (size_t)Q * C;
  hipLaunchKernelGGL(group_max_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, y, ld, K, C, scale, shift, slope, total, pooled, argmax);
  return spgan_launch_status();
}

extern "C" int spgan_group_max_bwd(const float* gpool, const float* pooled, const int32_t* argmax, const float* y, int ld, const float* mean,
                                   const float* invstd, float slope, int Q, int K, int C, float* g, float* gstat, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(gpool && pooled && y && mean && invstd && g && gstat && Q > 0 && K > 0 && C > 0 && ld >= C && (argmax || K == 1) &&
                  (uint64_t)Q * (uint64_t)K < (1ull << 31));
  const size_t total = (size_t)Q * K * C;
  SPGAN_CHECK_ARG(total / 256 < 2147483647u);
  hipLaunchKernelGGL(group_max_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, gpool, pooled, argmax, y, ld, mean, invstd, slope, K,
                     C, total, g, gstat);
  return spgan_launch_status();
}

extern "C" int spgan_cm_to_rows(const float* x_cm, int B, int C, int N, float* rows, int ld, int col0, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(x_cm && rows && B > 0 && C > 0 && N > 0 && col0 >= 0 && col0 + C <= ld && B <= 65535 && cdiv(C, 32) <= 65535);
  hipLaunchKernelGGL((cm_rows_kernel<true>), dim3(cdiv(N, 32), cdiv(C, 32), B), dim3(256), 0, (hipStream_t)s_, x_cm, rows, C, N, ld, col0);
  return spgan_launch_status();
}

extern "C" int spgan_rows_to_cm(const float* rows, int ld, int col0, int B, int C, int N, float* x_cm, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(x_cm && rows && B > 0 && C > 0 && N > 0 && col0 >= 0 && col0 + C <= ld && B <= 65535 && cdiv(C, 32) <= 65535);
  hipLaunchKernelGGL((cm_rows_kernel<false>), dim3(cdiv(N, 32), cdiv(C, 32), B), dim3(256), 0, (hipStream_t)s_, rows, x_cm, C, N, ld, col0);
  return spgan_launch_status();
}
