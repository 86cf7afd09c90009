// Local-shape Chamfer ("shape-preserving loss", Common/loss_utils.py:196-259 get_local_pair / compute_mean_covariance, and
// Common/GAN_metrics.py:596-656 local_CD / pairwise_local_CD) and the small pieces of the GAN_metrics evaluation module
// (the +-1-label KNN vote, GAN_metrics.py:466-482, and the 28^3 point-count histogram of its JSD, GAN_metrics.py:411-455).
//
//   knn_moments:  the K nearest cloud points of every query (pointops knnquery order: ascending d^2, the lower index first on
//                 equal d^2, the query itself included when it is a cloud point) and the mean / biased covariance of that
//                 neighbourhood.  Cloud staged in LDS, the top-K list in registers; no [B,M,N] distance matrix.
//   nn_dim:       nearest neighbour with index in D = 3 or 9 dimensions, or on the 6-entry storage of a symmetric 3x3 matrix with
//                 the off-diagonal squared differences weighted by 2 (= the 9-D distance of the full matrices).  Both directions
//                 in one launch (blockIdx.z).  Exact differences, not the |x|^2 + |y|^2 - 2<x,y> expansion.
//   pair_sum:     fixed-order sum of the per-row minima of both directions (one workgroup per pair).
//   chamfer_dim_bwd, moments_bwd: the adjoints (gather form, ascending order, no float atomics; the moments' slot gradients are
//                 scattered to the cloud through spgan_gather_csr / spgan_scatter_slots).
//
// Rounding order.  Every floating-point expression in this file is evaluated as written, without contraction into fma:
//   d^2      = ((qx - cx)^2 + (qy - cy)^2) + (qz - cz)^2
//   mu_c     = (sum_{j ascending} p_jc) / K
//   cov_ab   = (sum_{j ascending} (p_ja - mu_a) * (p_jb - mu_b)) / K,   stored [xx, xy, xz, yy, yz, zz]
//   dist_D   = sum_{c ascending} w_c * (x_c - y_c)^2,                     w_c = 2 on the off-diagonal entries of the 6-entry form
// so that a float32 CPU model evaluating the same expressions reproduces the neighbour indices exactly.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int KM_THREADS = 128;  // queries per workgroup (one per thread)
constexpr int KM_CHUNK = 1024;   // cloud points per LDS stage: 16 KB as float4
constexpr int NN_THREADS = 256;
constexpr int NN_CHUNK = 512;    // candidates per LDS stage: <= 18 KB at D = 9

// p = base + blockIdx.y; the query cloud is batch p / qdiv, the searched cloud batch p % cmod.  Plain batches: base 0, qdiv 1,
// cmod B.  All pairs (s, r) of pairwise_local_cd: qdiv = cmod = R.
struct PairMap {
  int base, qdiv, cmod;
};

// insert (d, k) into the ascending (distance, index) list.  Slots [0, KC-K) hold (-inf, -1) and are never displaced; the new
// candidate has the largest index seen so far, so among equal distances it lands after the ones already listed.
template <int KC>
__device__ __forceinline__ void topk_insert(float (&bd)[KC], int (&bi)[KC], float d, int k) {
  float cd = d;
  int ci = k;
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    const bool sw = cd < bd[j] || (cd == bd[j] && ci < bi[j]);
    const float td = bd[j];
    const int ti = bi[j];
    bd[j] = sw ? cd : td;
    bi[j] = sw ? ci : ti;
    cd = sw ? td : cd;
    ci = sw ? ti : ci;
  }
}

template <int KC>
__global__ __launch_bounds__(KM_THREADS) void knn_moments_kernel(const float* __restrict__ query, const float* __restrict__ cloud, int M,
                                                                  int N, int K, PairMap pm, int64_t* __restrict__ idx, float* __restrict__ mu,
                                                                  float* __restrict__ cov) {
  __shared__ float4 buf[KM_CHUNK];
  const int p = pm.base + blockIdx.y;
  const int qb = p / pm.qdiv, cb = p % pm.cmod;
  const int i = blockIdx.x * KM_THREADS + threadIdx.x;
  const bool ok = i < M;
  const float* cl = cloud + (size_t)cb * N * 3;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (ok) {
    const float* q = query + ((size_t)qb * M + i) * 3;
    qx = q[0]; qy = q[1]; qz = q[2];
  }
  float bd[KC];
  int bi[KC];
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    const bool pad = j < KC - K;
    bd[j] = pad ? -INFINITY : INFINITY;
    bi[j] = pad ? -1 : 0;  // an unfilled slot reads point 0, as knnquery's besti[] initialisation does
  }
  for (int c0 = 0; c0 < N; c0 += KM_CHUNK) {
    const int nc = min(KM_CHUNK, N - c0);
    __syncthreads();
    for (int e = threadIdx.x; e < nc; e += KM_THREADS) {
      const float* q = cl + (size_t)(c0 + e) * 3;
      buf[e] = make_float4(q[0], q[1], q[2], 0.f);
    }
    __syncthreads();
    if (ok) {
      for (int j = 0; j < nc; ++j) {
        const float4 c = buf[j];
        const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (d < bd[KC - 1]) topk_insert<KC>(bd, bi, d, c0 + j);
      }
    }
  }
  if (!ok) return;
  const int k0 = KC - K;
  const size_t row = (size_t)blockIdx.y * M + i;
  float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    if (j >= k0) {
      const float* q = cl + (size_t)bi[j] * 3;
      sx += q[0]; sy += q[1]; sz += q[2];
      if (idx) idx[row * K + (j - k0)] = bi[j];
    }
  }
  const float fk = (float)K;
  const float mx = sx / fk, my = sy / fk, mz = sz / fk;
  float cxx = 0.f, cxy = 0.f, cxz = 0.f, cyy = 0.f, cyz = 0.f, czz = 0.f;
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    if (j >= k0) {
      const float* q = cl + (size_t)bi[j] * 3;
      const float tx = q[0] - mx, ty = q[1] - my, tz = q[2] - mz;
      cxx += tx * tx; cxy += tx * ty; cxz += tx * tz;
      cyy += ty * ty; cyz += ty * tz; czz += tz * tz;
    }
  }
  float* o = mu + row * 3;
  o[0] = mx; o[1] = my; o[2] = mz;
  float* c = cov + row * 6;
  c[0] = cxx / fk; c[1] = cxy / fk; c[2] = cxz / fk; c[3] = cyy / fk; c[4] = cyz / fk; c[5] = czz / fk;
}

// D-dimensional squared distance in the fixed order; SYM: the 6-entry symmetric storage, off-diagonal terms (1, 2, 4) doubled
template <int D, bool SYM>
__device__ __forceinline__ float dist_dim(const float (&x)[D], const float* __restrict__ y) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const float df = x[c] - y[c];
    const float sq = df * df;
    acc = c == 0 ? sq : acc + ((SYM && (c == 1 || c == 2 || c == 4)) ? 2.f * sq : sq);
  }
  return acc;
}

// blockIdx.z = 0: rows of a against the candidates b; 1: rows of b against a.  a belongs to batch (base + blockIdx.y) / adiv,
// b to batch blockIdx.y; the outputs are indexed by blockIdx.y.  Strict < over ascending candidates: the first index on ties.
template <int D, bool SYM>
__global__ __launch_bounds__(NN_THREADS) void nn_dim_kernel(const float* __restrict__ a, const float* __restrict__ b, int Na, int Nb,
                                                            int base, int adiv, float* __restrict__ da, int32_t* __restrict__ ia,
                                                            float* __restrict__ db, int32_t* __restrict__ ib) {
  __shared__ float buf[NN_CHUNK * D];
  const int pb = blockIdx.y;
  const float* A = a + (size_t)((base + pb) / adiv) * Na * D;
  const float* Bp = b + (size_t)pb * Nb * D;
  const bool dir = blockIdx.z != 0;
  const float* X = dir ? Bp : A;
  const float* Y = dir ? A : Bp;
  const int nx = dir ? Nb : Na, ny = dir ? Na : Nb;
  if ((int)(blockIdx.x * NN_THREADS) >= nx) return;  // the whole workgroup: uniform
  const int i = blockIdx.x * NN_THREADS + threadIdx.x;
  const bool ok = i < nx;
  float x[D];
#pragma unroll
  for (int c = 0; c < D; ++c) x[c] = ok ? X[(size_t)i * D + c] : 0.f;
  float best = INFINITY;
  int bj = 0;
  for (int c0 = 0; c0 < ny; c0 += NN_CHUNK) {
    const int nc = min(NN_CHUNK, ny - c0);
    __syncthreads();
    for (int e = threadIdx.x; e < nc * D; e += NN_THREADS) buf[e] = Y[(size_t)c0 * D + e];
    __syncthreads();
    if (ok) {
      for (int j = 0; j < nc; ++j) {
        const float d = dist_dim<D, SYM>(x, buf + j * D);
        if (d < best) { best = d; bj = c0 + j; }
      }
    }
  }
  if (!ok) return;
  float* dout = dir ? db : da;
  int32_t* iout = dir ? ib : ia;
  dout[(size_t)pb * nx + i] = best;
  if (iout) iout[(size_t)pb * nx + i] = bj;
}

// out[p * ostride] = (float)(sum_i da[p, i] + sum_j db[p, j]) / div   (double partial sums in a fixed order, one workgroup per p)
__global__ __launch_bounds__(256) void pair_sum_kernel(const float* __restrict__ da, int na, const float* __restrict__ db, int nb, float div,
                                                       float* __restrict__ out, int ostride) {
  __shared__ double red[256];
  const int p = blockIdx.x;
  double acc = 0.;
  for (int e = threadIdx.x; e < na; e += 256) acc += (double)da[(size_t)p * na + e];
  for (int e = threadIdx.x; e < nb; e += 256) acc += (double)db[(size_t)p * nb + e];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(size_t)p * ostride] = (float)red[0] / div;
}

// grad_a[b,i,c] = g * 2 w_c (a_ic - b[idxa[b,i]]_c) + sum_{j ascending: idxb[b,j] == i} g * 2 w_c (a_ic - b_jc),  g = gs[0]:
// d/d(a) of g * (sum_i min_j dist + sum_j min_i dist) with the argmins of nn_dim
template <int D, bool SYM>
__global__ __launch_bounds__(256) void chamfer_dim_bwd_kernel(const float* __restrict__ xa, const float* __restrict__ xb, int Na, int Nb,
                                                              const int32_t* __restrict__ idxa, const int32_t* __restrict__ idxb,
                                                              const float* __restrict__ gs, float* __restrict__ grad_a) {
  __shared__ int ibuf[NN_CHUNK];
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool ok = i < Na;
  const float g2 = 2.f * gs[0];
  float w[D], x[D], acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) w[c] = (SYM && (c == 1 || c == 2 || c == 4)) ? 2.f * g2 : g2;
  if (ok) {
    const float* pa = xa + ((size_t)b * Na + i) * D;
    const float* pb = xb + ((size_t)b * Nb + idxa[(size_t)b * Na + i]) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) { x[c] = pa[c]; acc[c] = w[c] * (x[c] - pb[c]); }
  }
  for (int c0 = 0; c0 < Nb; c0 += NN_CHUNK) {
    const int nc = min(NN_CHUNK, Nb - c0);
    __syncthreads();
    for (int e = threadIdx.x; e < nc; e += 256) ibuf[e] = idxb[(size_t)b * Nb + c0 + e];
    __syncthreads();
    if (ok) {
      for (int j = 0; j < nc; ++j) {
        if (ibuf[j] == i) {
          const float* pb = xb + ((size_t)b * Nb + c0 + j) * D;
#pragma unroll
          for (int c = 0; c < D; ++c) acc[c] += w[c] * (x[c] - pb[c]);
        }
      }
    }
  }
  if (ok) {
    float* o = grad_a + ((size_t)b * Na + i) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) o[c] = acc[c];
  }
}

// gslot[b,m,k,:] = (dmu[b,m] + H (p_k - mu[b,m])) / K,  H = G + G^T of the 6-entry gradient (diagonal 2 g_aa, off-diagonal g_ab)
__global__ __launch_bounds__(256) void moments_bwd_kernel(const int64_t* __restrict__ idx, const float* __restrict__ cloud,
                                                          const float* __restrict__ mu, const float* __restrict__ dmu,
                                                          const float* __restrict__ dcov, int M, int N, int K, size_t total,
                                                          float* __restrict__ gslot) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const size_t bm = t / K;
  const size_t b = bm / M;
  const float* p = cloud + (b * N + (size_t)idx[t]) * 3;
  const float* m = mu + bm * 3;
  const float* gm = dmu + bm * 3;
  const float* gc = dcov + bm * 6;
  const float tx = p[0] - m[0], ty = p[1] - m[1], tz = p[2] - m[2];
  const float fk = (float)K;
  float* o = gslot + t * 3;
  o[0] = (gm[0] + ((2.f * gc[0] * tx + gc[1] * ty) + gc[2] * tz)) / fk;
  o[1] = (gm[1] + ((gc[1] * tx + 2.f * gc[3] * ty) + gc[4] * tz)) / fk;
  o[2] = (gm[2] + ((gc[2] * tx + gc[4] * ty) + 2.f * gc[5] * tz)) / fk;
}

__device__ __forceinline__ float joint_pm(const float* Mxx, const float* Mxy, const float* Myy, int n0, int n1, int i, int j,
                                          int take_sqrt) {
  float v;
  if (i < n0) v = j < n0 ? Mxx[(size_t)i * n0 + j] : Mxy[(size_t)i * n1 + (j - n0)];
  else v = j < n0 ? Mxy[(size_t)j * n1 + (i - n0)] : Myy[(size_t)(i - n0) * n1 + (j - n0)];
  return take_sqrt ? sqrtf(fabsf(v)) : v;
}

// GAN_metrics.KNN: one workgroup per cloud j; its k nearest OTHER clouds (column j of the joint matrix, smallest first, lower
// index on ties) vote with labels -1 (first set) / +1 (second set); pred[j] = +1 when the vote is >= 0 (a tie predicts the second
// set, the reference clouds), else -1
__global__ __launch_bounds__(256) void knn_pm_vote_kernel(const float* __restrict__ Mxx, const float* __restrict__ Mxy,
                                                          const float* __restrict__ Myy, int n0, int n1, int k, int take_sqrt,
                                                          int32_t* __restrict__ pred) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const int n = n0 + n1, j = blockIdx.x;
  float pv = -INFINITY;
  int pi = -1, count = 0;
  for (int round = 0; round < k; ++round) {
    float best = INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256) {
      if (i == j) continue;
      const float v = joint_pm(Mxx, Mxy, Myy, n0, n1, i, j, take_sqrt);
      const bool after = v > pv || (v == pv && i > pi);
      if (after && (v < best || (v == best && i < bi))) { best = v; bi = i; }
    }
    sv[threadIdx.x] = best;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (threadIdx.x < o) {
        const float v = sv[threadIdx.x + o];
        const int i = si[threadIdx.x + o];
        if (v < sv[threadIdx.x] || (v == sv[threadIdx.x] && i < si[threadIdx.x])) { sv[threadIdx.x] = v; si[threadIdx.x] = i; }
      }
      __syncthreads();
    }
    pv = sv[0];
    pi = si[0];
    __syncthreads();
    count += pi < n0 ? -1 : 1;
  }
  if (threadIdx.x == 0) pred[j] = count >= 0 ? 1 : -1;
}

// out[0] = (float)#{j : pred[j] == label[j]} / (float)(n0 + n1)
__global__ __launch_bounds__(256) void knn_pm_final_kernel(const int32_t* __restrict__ pred, int n0, int n1, float* __restrict__ out) {
  __shared__ int red[256];
  int hit = 0;
  for (int j = threadIdx.x; j < n0 + n1; j += 256) hit += pred[j] == (j < n0 ? -1 : 1);
  red[threadIdx.x] = hit;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)red[0] / (float)(n0 + n1);
}

// half-open bin of v among the edges e_i = -0.5 + i * (1/res) (float64, as numpy's -0.5 + arange(res+1) * (1./res)); -1 outside
__device__ __forceinline__ int voxel_bin(float v, int res) {
  const double x = (double)v, step = 1.0 / (double)res;
  if (!(x >= -0.5)) return -1;  // also NaN
  int i = (int)floor((x + 0.5) * (double)res);
  i = min(max(i, 0), res - 1);
  if (x < -0.5 + (double)i * step) --i;
  else if (x >= -0.5 + (double)(i + 1) * step) ++i;
  if (i < 0 || i >= res) return -1;
  return (x >= -0.5 + (double)i * step && x < -0.5 + (double)(i + 1) * step) ? i : -1;
}

// counts[(i*res + j)*res + k] += 1 for every point with all three coordinates inside a bin (integer atomics: the counts do not
// depend on the order)
__global__ __launch_bounds__(256) void voxel_counts_kernel(const float* __restrict__ pts, long npts, int res, int32_t* __restrict__ counts) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= npts) return;
  const float* p = pts + t * 3;
  const int i = voxel_bin(p[0], res), j = voxel_bin(p[1], res), k = voxel_bin(p[2], res);
  if (i < 0 || j < 0 || k < 0) return;
  atomicAdd(&counts[((size_t)i * res + j) * res + k], 1);
}

// out[s,r] = sum_{c ascending} (a[s,c] - b[r,c])^2, or |a[s,c] - b[r,c]| with l1 (GAN_metrics.py:562-593 pairwise_simple)
__global__ __launch_bounds__(256) void pairwise_simple_kernel(const float* __restrict__ a, const float* __restrict__ b, int R, int D, int l1,
                                                              size_t total, float* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const float* x = a + (t / R) * D;
  const float* y = b + (t % R) * D;
  float acc = 0.f;
  for (int c = 0; c < D; ++c) {
    const float df = x[c] - y[c];
    acc += l1 ? fabsf(df) : df * df;
  }
  out[t] = acc;
}

int launch_knn_moments(const float* query, const float* cloud, int P, int M, int N, int K, PairMap pm, int64_t* idx, float* mu, float* cov,
                       hipStream_t s) {
  const dim3 grid(cdiv(M, KM_THREADS), P), blk(KM_THREADS);
  if (K <= 4) hipLaunchKernelGGL(knn_moments_kernel<4>, grid, blk, 0, s, query, cloud, M, N, K, pm, idx, mu, cov);
  else if (K <= 8) hipLaunchKernelGGL(knn_moments_kernel<8>, grid, blk, 0, s, query, cloud, M, N, K, pm, idx, mu, cov);
  else if (K <= 16) hipLaunchKernelGGL(knn_moments_kernel<16>, grid, blk, 0, s, query, cloud, M, N, K, pm, idx, mu, cov);
  else if (K <= 20) hipLaunchKernelGGL(knn_moments_kernel<20>, grid, blk, 0, s, query, cloud, M, N, K, pm, idx, mu, cov);
  else hipLaunchKernelGGL(knn_moments_kernel<32>, grid, blk, 0, s, query, cloud, M, N, K, pm, idx, mu, cov);
  return spgan_launch_status();
}

int launch_nn_dim(const float* a, const float* b, int P, int Na, int Nb, int D, int base, int adiv, float* da, int32_t* ia, float* db,
                  int32_t* ib, hipStream_t s) {
  const dim3 grid(cdiv(max(Na, Nb), NN_THREADS), P, 2), blk(NN_THREADS);
  if (D == 3) hipLaunchKernelGGL((nn_dim_kernel<3, false>), grid, blk, 0, s, a, b, Na, Nb, base, adiv, da, ia, db, ib);
  else if (D == 9) hipLaunchKernelGGL((nn_dim_kernel<9, false>), grid, blk, 0, s, a, b, Na, Nb, base, adiv, da, ia, db, ib);
  else hipLaunchKernelGGL((nn_dim_kernel<6, true>), grid, blk, 0, s, a, b, Na, Nb, base, adiv, da, ia, db, ib);
  return spgan_launch_status();
}

// pairs per chunk of pairwise_local_cd: the chunk's moments and minima take P * N * 13 floats (about 64 MB)
int pairs_per_chunk(int S, int R, int N) {
  const long cap = (16L << 20) / ((long)N * 13);
  const long total = (long)S * R;
  return (int)max(1L, min(min(total, cap), 65535L));
}

}  // namespace

extern "C" int spgan_knn_moments(const float* query, const float* cloud, int B, int M, int N, int K, int64_t* idx, float* mu, float* cov,
                                 spgan_stream_t s_) {
  SPGAN_CHECK_ARG(query && cloud && mu && cov && B > 0 && B <= 65535 && M > 0 && N > 0 && K >= 1 && K <= 32 && K <= N);
  return launch_knn_moments(query, cloud, B, M, N, K, PairMap{0, 1, B}, idx, mu, cov, (hipStream_t)s_);
}

extern "C" int spgan_moments_bwd(const int64_t* idx, const float* cloud, const float* mu, const float* dmu, const float* dcov, int B, int M,
                                 int N, int K, float* gslot, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(idx && cloud && mu && dmu && dcov && gslot && B > 0 && M > 0 && N > 0 && K >= 1 && K <= 32);
  const size_t total = (size_t)B * M * K;
  hipLaunchKernelGGL(moments_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, idx, cloud, mu, dmu, dcov, M, N, K, total,
                     gslot);
  return spgan_launch_status();
}

extern "C" int spgan_nn_dim(const float* a, const float* b, int B, int Na, int Nb, int D, float* dist_a, int32_t* idx_a, float* dist_b,
                            int32_t* idx_b, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(a && b && dist_a && dist_b && B > 0 && B <= 65535 && Na > 0 && Nb > 0 && (D == 3 || D == 6 || D == 9));
  return launch_nn_dim(a, b, B, Na, Nb, D, 0, 1, dist_a, idx_a, dist_b, idx_b, (hipStream_t)s_);
}

extern "C" int spgan_pair_sum(const float* dist_a, int na, const float* dist_b, int nb, int P, float div, float* out, int ostride,
                              spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dist_a && dist_b && out && na > 0 && nb > 0 && P > 0 && ostride > 0);
  hipLaunchKernelGGL(pair_sum_kernel, dim3(P), dim3(256), 0, (hipStream_t)s_, dist_a, na, dist_b, nb, div, out, ostride);
  return spgan_launch_status();
}

extern "C" int spgan_chamfer_dim_bwd(const float* xa, const float* xb, int B, int Na, int Nb, int D, const int32_t* idxa, const int32_t* idxb,
                                     const float* gscale, float* grad_a, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xa && xb && idxa && idxb && gscale && grad_a && B > 0 && B <= 65535 && Na > 0 && Nb > 0 && (D == 3 || D == 6 || D == 9));
  const dim3 grid(cdiv(Na, 256), B), blk(256);
  hipStream_t s = (hipStream_t)s_;
  if (D == 3) hipLaunchKernelGGL((chamfer_dim_bwd_kernel<3, false>), grid, blk, 0, s, xa, xb, Na, Nb, idxa, idxb, gscale, grad_a);
  else if (D == 9) hipLaunchKernelGGL((chamfer_dim_bwd_kernel<9, false>), grid, blk, 0, s, xa, xb, Na, Nb, idxa, idxb, gscale, grad_a);
  else hipLaunchKernelGGL((chamfer_dim_bwd_kernel<6, true>), grid, blk, 0, s, xa, xb, Na, Nb, idxa, idxb, gscale, grad_a);
  return spgan_launch_status();
}

extern "C" size_t spgan_pairwise_local_cd_ws_bytes(int S, int R, int N, int M) {
  if (S <= 0 || R <= 0 || N <= 0 || M <= 0) return 0;
  const size_t P = (size_t)pairs_per_chunk(S, R, N);
  return ((size_t)S * N * 9 + P * N * 13) * sizeof(float);
}

extern "C" int spgan_pairwise_local_cd(const float* sample, const float* ref, int S, int R, int N, int M, int K, float* out, void* ws,
                                       size_t ws_bytes, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(sample && ref && out && ws && S > 0 && S <= 65535 && R > 0 && N > 0 && M > 0 && K >= 1 && K <= 32 && K <= N && K <= M &&
                  (long)S * R < (1L << 31) && ws_bytes >= spgan_pairwise_local_cd_ws_bytes(S, R, N, M));
  hipStream_t s = (hipStream_t)s_;
  const int P = pairs_per_chunk(S, R, N);
  float* self_mu = (float*)ws;                       // [S,N,3]
  float* self_cov = self_mu + (size_t)S * N * 3;     // [S,N,6]
  float* pair_mu = self_cov + (size_t)S * N * 6;     // [P,N,3]
  float* pair_cov = pair_mu + (size_t)P * N * 3;     // [P,N,6]
  float* dm = pair_cov + (size_t)P * N * 6;          // [2,P,N]: both directions of the mean term
  float* dc = dm + (size_t)2 * P * N;                // [2,P,N]: the covariance term
  int st = launch_knn_moments(sample, sample, S, N, N, K, PairMap{0, 1, S}, nullptr, self_mu, self_cov, s);
  if (st) return st;
  const long total = (long)S * R;
  for (long p0 = 0; p0 < total; p0 += P) {
    const int np = (int)min((long)P, total - p0);
    if ((st = launch_knn_moments(sample, ref, np, N, M, K, PairMap{(int)p0, R, R}, nullptr, pair_mu, pair_cov, s))) return st;
    if ((st = launch_nn_dim(self_mu, pair_mu, np, N, N, 3, (int)p0, R, dm, nullptr, dm + (size_t)P * N, nullptr, s))) return st;
    if ((st = launch_nn_dim(self_cov, pair_cov, np, N, N, 6, (int)p0, R, dc, nullptr, dc + (size_t)P * N, nullptr, s))) return st;
    hipLaunchKernelGGL(pair_sum_kernel, dim3(np), dim3(256), 0, s, dm, N, dm + (size_t)P * N, N, (float)N, out + p0 * 2, 2);
    hipLaunchKernelGGL(pair_sum_kernel, dim3(np), dim3(256), 0, s, dc, N, dc + (size_t)P * N, N, (float)N, out + p0 * 2 + 1, 2);
    if ((st = spgan_launch_status())) return st;
  }
  return SPGAN_OK;
}

extern "C" int spgan_two_sample_knn_pm(const float* Mxx, const float* Mxy, const float* Myy, int n0, int n1, int k, int take_sqrt, float* out1,
                                       int32_t* pred, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(Mxx && Mxy && Myy && out1 && pred && n0 > 0 && n1 > 0 && k > 0 && k < n0 + n1);
  hipStream_t s = (hipStream_t)s_;
  hipLaunchKernelGGL(knn_pm_vote_kernel, dim3(n0 + n1), dim3(256), 0, s, Mxx, Mxy, Myy, n0, n1, k, take_sqrt, pred);
  hipLaunchKernelGGL(knn_pm_final_kernel, dim3(1), dim3(256), 0, s, pred, n0, n1, out1);
  return spgan_launch_status();
}

extern "C" int spgan_voxel_counts(const float* pts, long npts, int res, int32_t* counts, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(pts && counts && npts > 0 && res > 0 && res <= 1024);
  hipLaunchKernelGGL(voxel_counts_kernel, dim3(cdiv(npts, 256)), dim3(256), 0, (hipStream_t)s_, pts, npts, res, counts);
  return spgan_launch_status();
}

extern "C" int spgan_pairwise_simple(const float* a, const float* b, int S, int R, int D, int l1, float* out, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(a && b && out && S > 0 && R > 0 && D > 0);
  const size_t total = (size_t)S * R;
  hipLaunchKernelGGL(pairwise_simple_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, a, b, R, D, l1 ? 1 : 0, total, out);
  return spgan_launch_status();
}
