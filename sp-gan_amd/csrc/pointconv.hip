// PointConv density set abstraction kernels (Common/pointconv_util.py:199-383).  The three small MLPs (feature MLP, WeightNet,
// DensityNet) and the final linear run on the GEMM / BatchNorm kernels of the rest of the library; this file holds what those do
// not cover:
//   * kde_density (+ adjoint):         the Gaussian kernel density of every point over its whole cloud, N x N pairs streamed through
//                                      LDS tiles; the reference materialises [B,N,N] (:205-207), here there is no matrix and no workspace
//   * group_density_scale (+ adjoint): gather 1/density per neighbour and divide by the group's maximum (:147, :370-371)
//   * pointconv_aggregate (+ adjoint): per centre E[c,w] = sum_k F[k,c] * dens[k] * Wt[k,w], the [C x K].[K x 16] product the
//                                      reference runs as a batched torch.matmul over permuted views (:377)
// Everything is deterministic: fixed summation orders, no float atomics, vector stores only.
#include "common.hpp"
#include "pointnet_dist.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// density[b,i] = (1/N) sum_j exp(-d_ij / (2 h^2)) / (2.5 h), d_ij = the reference's expanded form -2ab + |a|^2 + |b|^2 (so that d_ii is a
// tiny number of either sign or zero, not a subtraction of coordinates), evaluated in float64 (sqdist_expanded_f64): in float32 the
// form's cancellation error, divided by 2 h^2 in the exponent, is the largest error of the whole PointConv module (DESIGN.md section
// 17).  The exponential, the weights and the sum are float32.  One thread per query point, the cloud in tiles of 256 points with their
// squared norms in LDS (as float64: no conversion per pair), a running sum in ascending j.  inv (optional) = 1 / density.
__device__ __forceinline__ double norm2_f64(const double* __restrict__ p, int C) {
  double s = 0.0;
  for (int c = 0; c < C; ++c) s = fma(p[c], p[c], s);
  return s;
}

__global__ __launch_bounds__(256) void kde_density_kernel(const float* __restrict__ xyz, int N, double neg_inv_2h2, float inv_25h,
                                                          float* __restrict__ density, float* __restrict__ inv) {
  constexpr int TC = 256, C = 3;
  __shared__ double cand[TC * C];
  __shared__ double cn[TC];
  const int b = blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const bool ok = n < N;
  float q[C];
#pragma unroll
  for (int c = 0; c < C; ++c) q[c] = ok ? xyz[((size_t)b * N + n) * C + c] : 0.f;
  double qn = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) qn = fma((double)q[c], (double)q[c], qn);
  float sum = 0.f;
  for (int c0 = 0; c0 < N; c0 += TC) {
    const int nc = min(TC, N - c0);
    __syncthreads();
    for (int e = threadIdx.x; e < nc * C; e += 256) cand[e] = (double)xyz[((size_t)b * N + c0) * C + e];
    __syncthreads();
    if (threadIdx.x < nc) cn[threadIdx.x] = norm2_f64(cand + threadIdx.x * C, C);
    __syncthreads();
    for (int j = 0; j < nc; ++j) sum += expf((float)(sqdist_expanded_f64<C>(q, qn, cand + j * C, cn[j]) * neg_inv_2h2)) * inv_25h;
  }
  if (!ok) return;
  const float dens = sum / (float)N;
  density[(size_t)b * N + n] = dens;
  if (inv) inv[(size_t)b * N + n] = 1.0f / dens;
}

// dxyz_i = coef * sum_j (G_i + G_j) * w_ij * (x_i - x_j), coef = -1 / (h^2 * N * 2.5 h), w_ij = exp(-d_ij / (2 h^2)) bit for bit as in the forward,
// G = g (gradient w.r.t. density) - ginv * inv^2 (gradient w.r.t. 1/density folded in); either of g / ginv may be NULL.
// Gather form: one thread per point i, the second N x N pass, again without a matrix.
__global__ __launch_bounds__(256) void kde_density_bwd_kernel(const float* __restrict__ xyz, const float* __restrict__ g,
                                                              const float* __restrict__ ginv, const float* __restrict__ inv, int N,
                                                              double neg_inv_2h2, float coef, float* __restrict__ dxyz) {
  constexpr int TC = 256, C = 3;
  __shared__ double cand[TC * C];
  __shared__ double cn[TC];
  __shared__ float cg[TC];
  const int b = blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const bool ok = n < N;
  const size_t base = (size_t)b * N;
  float q[C];
#pragma unroll
  for (int c = 0; c < C; ++c) q[c] = ok ? xyz[(base + n) * C + c] : 0.f;
  double qn = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) qn = fma((double)q[c], (double)q[c], qn);
  float gi = 0.f;
  if (ok) {
    if (g) gi = g[base + n];
    if (ginv) { const float v = inv[base + n]; gi = fmaf(-ginv[base + n], v * v, gi); }
  }
  float acc[C] = {0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < N; c0 += TC) {
    const int nc = min(TC, N - c0);
    __syncthreads();
    for (int e = threadIdx.x; e < nc * C; e += 256) cand[e] = (double)xyz[(base + c0) * C + e];
    if (threadIdx.x < nc) {
      float gj = g ? g[base + c0 + threadIdx.x] : 0.f;
      if (ginv) { const float v = inv[base + c0 + threadIdx.x]; gj = fmaf(-ginv[base + c0 + threadIdx.x], v * v, gj); }
      cg[threadIdx.x] = gj;
    }
    __syncthreads();
    if (threadIdx.x < nc) cn[threadIdx.x] = norm2_f64(cand + threadIdx.x * C, C);
    __syncthreads();
    for (int j = 0; j < nc; ++j) {
      const float w = expf((float)(sqdist_expanded_f64<C>(q, qn, cand + j * C, cn[j]) * neg_inv_2h2)) * (gi + cg[j]);
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = fmaf(w, q[c] - (float)cand[j * C + c], acc[c]);
    }
  }
  if (!ok) return;
#pragma unroll
  for (int c = 0; c < C; ++c) dxyz[(base + n) * C + c] = coef * acc[c];
}

// One wave per centre q = (b,s): v_k = inv[b, idx[q,k]], m = max_k v_k (first maximum), scale[q*K + k] = v_k / m.
// The maximum and its slot are reduced over the lanes in a fixed order (value first, lower slot on equal values).
__device__ __forceinline__ void wave_argmax(float& m, int& a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off);
    const int oa = __shfl_xor(a, off);
    if (om > m || (om == m && oa < a)) { m = om; a = oa; }
  }
}

__global__ __launch_bounds__(256) void group_density_scale_kernel(const float* __restrict__ inv, const int64_t* __restrict__ idx, int N, int S,
                                                                  int K, int Q, float* __restrict__ scale, int* __restrict__ bad) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= Q) return;
  const size_t b = q / S;
  const int64_t* id = idx + (size_t)q * K;
  float m = -INFINITY;
  int a = 0x7fffffff;
  for (int k = lane; k < K; k += 64) {
    const int64_t p = id[k];
    if (p < 0 || p >= N) { if (bad) atomicOr(bad, 1); continue; }
    const float v = inv[b * N + p];
    if (v > m) { m = v; a = k; }
  }
  wave_argmax(m, a);
  for (int k = lane; k < K; k += 64) {
    const int64_t p = id[k];
    scale[(size_t)q * K + k] = (p < 0 || p >= N) ? 0.f : inv[b * N + p] / m;
  }
}

// dslot[q*K + k] = g_k / m - [k == k*] * (sum_j g_j * v_j) / m^2: the quotient rule with the maximum's share at its arg-max slot k*.
// The sum over j runs per lane in ascending k, then over the lanes in a fixed butterfly order.
__global__ __launch_bounds__(256) void group_density_scale_bwd_kernel(const float* __restrict__ g, const float* __restrict__ inv,
                                                                      const int64_t* __restrict__ idx, int N, int S, int K, int Q,
                                                                      float* __restrict__ dslot) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= Q) return;
  const size_t b = q / S;
  const int64_t* id = idx + (size_t)q * K;
  float m = -INFINITY, dot = 0.f;
  int a = 0x7fffffff;
  for (int k = lane; k < K; k += 64) {
    const int64_t p = id[k];
    if (p < 0 || p >= N) continue;
    const float v = inv[b * N + p];
    dot = fmaf(g[(size_t)q * K + k], v, dot);
    if (v > m) { m = v; a = k; }
  }
  wave_argmax(m, a);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
  const float rm = 1.0f / m;
  for (int k = lane; k < K; k += 64) {
    const int64_t p = id[k];
    float d = (p < 0 || p >= N) ? 0.f : g[(size_t)q * K + k] * rm;
    if (k == a) d -= dot * rm * rm;
    dslot[(size_t)q * K + k] = d;
  }
}

// E[q, c*16 + w] = sum_k F[q*K + k, c] * dens[q*K + k] * Wt[q*K + k, w]                      pointconv_util.py:373-377
// One workgroup per centre.  The [K x 16] WeightNet tile is staged once per 32-row chunk in LDS with dens folded in; the feature rows
// are used exactly once each (the product's N side is a single 16-wide tile), so they go from global memory straight into the
// B operand of v_mfma_f32_16x16x4_f32: A[w][k] = tile, B[k][c] = F, D[w][c].  The D fragment of a lane is 4 consecutive w of one c,
// i.e. 16 contiguous bytes of E's c-major / w-minor row, and a wave's two tiles cover 32 c = 2 KB of the row.
// The MFMA is a k-ordered fp32 fma chain (exact fp32 products, one rounding per step): the sum over k runs in ascending k.
template <bool HAS_DENS>
__global__ __launch_bounds__(256) void pointconv_aggregate_kernel(const float* __restrict__ F, const float* __restrict__ Wt,
                                                                  const float* __restrict__ dens, int K, int C, float* __restrict__ E) {
  constexpr int KC = 32, W = 16;
  __shared__ float sW[KC * W];
  const size_t q = blockIdx.x;
  const size_t row0 = q * (size_t)K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  for (int cp = 0; cp < C; cp += 128) {
    const int c0 = cp + wave * 32 + col, c1 = c0 + 16;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < K; kc += KC) {
      __syncthreads();
      for (int e = threadIdx.x; e < KC * W; e += 256) {
        const int k = kc + e / W;
        float v = 0.f;
        if (k < K) {
          v = Wt[(row0 + k) * W + (e % W)];
          if (HAS_DENS) v *= dens[row0 + k];
        }
        sW[e] = v;
      }
      __syncthreads();
      float b0[KC / 4], b1[KC / 4];
#pragma unroll
      for (int j = 0; j < KC / 4; ++j) {
        const int k = kc + 4 * j + g;
        const bool kok = k < K;
        b0[j] = (kok && c0 < C) ? F[(row0 + k) * C + c0] : 0.f;
        b1[j] = (kok && c1 < C) ? F[(row0 + k) * C + c1] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < KC / 4; ++j) {
        const float a = sW[(4 * j + g) * W + col];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0[j], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1[j], acc1, 0, 0, 0);
      }
    }
    float* e = E + q * (size_t)C * W;
    if (c0 < C) *reinterpret_cast<f32x4*>(e + (size_t)c0 * W + 4 * g) = acc0;
    if (c1 < C) *reinterpret_cast<f32x4*>(e + (size_t)c1 * W + 4 * g) = acc1;
  }
}

// The adjoint, per centre, from dE [16*C] (c-major, w-minor), in 16-row chunks of k, one launch for all three gradients:
//   dWtraw[k,w] = sum_c dE[c,w] * F[k,c];  dWt[k,w] = dens[k] * dWtraw[k,w];  ddens[k] = sum_w Wt[k,w] * dWtraw[k,w]
//   dF[k,c]     = dens[k] * sum_w dE[c,w] * Wt[k,w]
// Phase 1 (sum over c): A[k][c] = F (16 bytes per lane: the lane's four MFMA steps take c = base + 4*(lane>>4) + j), B[c][w] = dE,
// D[k][w]; the four waves take every fourth 16-wide c block and their partial tiles are summed through LDS in wave order.
// Phase 2 (sum over w): A[c][w] = dE, B[w][k] = dens[k] * Wt[k,w], D[c][k]: a lane's fragment is 4 consecutive c of one row k of dF.
// dE (16*C floats) is read from global memory / L1 in both phases; nothing but the 4 x 256 partial sums lives in LDS, so C is not capped.
template <bool HAS_DENS>
__global__ __launch_bounds__(256) void pointconv_aggregate_bwd_kernel(const float* __restrict__ dE, const float* __restrict__ F,
                                                                      const float* __restrict__ Wt, const float* __restrict__ dens, int K, int C,
                                                                      int vec4, float* __restrict__ dF, float* __restrict__ dWt,
                                                                      float* __restrict__ ddens) {
  constexpr int W = 16;
  __shared__ float part[4][256];
  const size_t q = blockIdx.x;
  const size_t row0 = q * (size_t)K;
  const float* de = dE + q * (size_t)C * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  for (int kc = 0; kc < K; kc += 16) {
    const int krow = kc + col;          // the row of this lane's A (phase 1) / B and D (phase 2) fragments
    const bool kok = krow < K;
    // ---- phase 1
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int cb = wave * 16; cb < C; cb += 64) {
      const int c = cb + 4 * g;
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      if (kok) {
        const float* p = F + (row0 + krow) * C + c;
        if (vec4 && c < C) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(p);
          a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = c + j < C ? p[j] : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bv = c + j < C ? de[(size_t)(c + j) * W + col] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bv, acc, 0, 0, 0);
      }
    }
    __syncthreads();       // the previous chunk's readers of part[] are done
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][(4 * g + r) * W + col] = acc[r];
    __syncthreads();
    {
      const int k = kc + (threadIdx.x >> 4), w = threadIdx.x & 15;
      const float raw = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
      const bool ok = k < K;
      const float d = (HAS_DENS && ok) ? dens[row0 + k] : 1.f;
      if (ok) dWt[(row0 + k) * W + w] = d * raw;
      if (HAS_DENS) {
        float s = ok ? Wt[(row0 + k) * W + w] * raw : 0.f;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (ok && w == 0) ddens[row0 + k] = s;
      }
    }
    // ---- phase 2
    float bw[4] = {0.f, 0.f, 0.f, 0.f};
    if (kok) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(Wt + (row0 + krow) * W + 4 * g);
      const float d = HAS_DENS ? dens[row0 + krow] : 1.f;
      bw[0] = v.x * d; bw[1] = v.y * d; bw[2] = v.z * d; bw[3] = v.w * d;
    }
    for (int cb = wave * 16; cb < C; cb += 64) {
      const int ca = cb + col;
      f32x4 av = {0.f, 0.f, 0.f, 0.f};
      if (ca < C) av = *reinterpret_cast<const f32x4*>(de + (size_t)ca * W + 4 * g);
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bw[0], o, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bw[1], o, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bw[2], o, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bw[3], o, 0, 0, 0);
      const int c = cb + 4 * g;
      if (kok && c < C) {
        float* p = dF + (row0 + krow) * C + c;
        if (vec4) {
          *reinterpret_cast<f32x4*>(p) = o;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (c + r < C) p[r] = o[r];
        }
      }
    }
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int spgan_kde_density(const float* xyz, int B, int N, float bandwidth, float* density, float* inv_density, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz && density && B > 0 && N > 0 && B <= 65535 && bandwidth > 0.f);
  const double h = bandwidth;
  hipLaunchKernelGGL(kde_density_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, (hipStream_t)s_, xyz, N, -1.0 / (2.0 * h * h), (float)(1.0 / (2.5 * h)),
                     density, inv_density);
  return spgan_launch_status();
}

extern "C" int spgan_kde_density_bwd(const float* xyz, const float* g, const float* ginv, const float* inv_density, int B, int N, float bandwidth,
                                     float* dxyz, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz && dxyz && (g || ginv) && (!ginv || inv_density) && B > 0 && N > 0 && B <= 65535 && bandwidth > 0.f);
  const double h = bandwidth;
  const float coef = (float)(-1.0 / (h * h * (double)N * 2.5 * h));
  hipLaunchKernelGGL(kde_density_bwd_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, (hipStream_t)s_, xyz, g, ginv, inv_density, N,
                     -1.0 / (2.0 * h * h), coef, dxyz);
  return spgan_launch_status();
}

extern "C" int spgan_group_density_scale(const float* inv_density, const int64_t* idx, int B, int N, int S, int K, float* scale, int32_t* bad,
                                         spgan_stream_t s_) {
  SPGAN_CHECK_ARG(inv_density && idx && scale && B > 0 && N > 0 && S > 0 && K > 0 && (uint64_t)B * (uint64_t)S < (1ull << 31));
  const int Q = B * S;
  hipLaunchKernelGGL(group_density_scale_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, (hipStream_t)s_, inv_density, idx, N, S, K, Q, scale, (int*)bad);
  return spgan_launch_status();
}

extern "C" int spgan_group_density_scale_bwd(const float* g, const float* inv_density, const int64_t* idx, int B, int N, int S, int K,
                                             float* dslot, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(g && inv_density && idx && dslot && B > 0 && N > 0 && S > 0 && K > 0 && (uint64_t)B * (uint64_t)S < (1ull << 31));
  const int Q = B * S;
  hipLaunchKernelGGL(group_density_scale_bwd_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, (hipStream_t)s_, g, inv_density, idx, N, S, K, Q, dslot);
  return spgan_launch_status();
}

extern "C" int spgan_pointconv_aggregate(const float* F, const float* Wt, const float* dens, int Q, int K, int C, int W, float* E,
                                         spgan_stream_t s_) {
  SPGAN_CHECK_ARG(F && Wt && E && Q > 0 && K > 0 && C > 0 && W == 16 && al16(E));
  if (dens)
    hipLaunchKernelGGL((pointconv_aggregate_kernel<true>), dim3(Q), dim3(256), 0, (hipStream_t)s_, F, Wt, dens, K, C, E);
  else
    hipLaunchKernelGGL((pointconv_aggregate_kernel<false>), dim3(Q), dim3(256), 0, (hipStream_t)s_, F, Wt, dens, K, C, E);
  return spgan_launch_status();
}

extern "C" int spgan_pointconv_aggregate_bwd(const float* dE, const float* F, const float* Wt, const float* dens, int Q, int K, int C, int W,
                                             float* dF, float* dWt, float* ddens, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dE && F && Wt && dF && dWt && Q > 0 && K > 0 && C > 0 && W == 16 && (!dens == !ddens) && al16(dE) && al16(Wt));
  const int vec4 = (C % 4 == 0 && al16(F) && al16(dF)) ? 1 : 0;
  if (dens)
    hipLaunchKernelGGL((pointconv_aggregate_bwd_kernel<true>), dim3(Q), dim3(256), 0, (hipStream_t)s_, dE, F, Wt, dens, K, C, vec4, dF, dWt, ddens);
  else
    hipLaunchKernelGGL((pointconv_aggregate_bwd_kernel<false>), dim3(Q), dim3(256), 0, (hipStream_t)s_, dE, F, Wt, dens, K, C, vec4, dF, dWt, ddens);
  return spgan_launch_status();
}
