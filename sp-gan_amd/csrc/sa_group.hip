// Bipartite set abstraction with the first MLP layer hoisted onto the points (metrics/pointnet2/pointnet2_modules.py of the reference;
// DESIGN 33).  S centres, K padded slots per centre, N points: the first 1x1 convolution is linear in [x_j - c_i | f_j], so it is one
// per-point product P = [xyz | f] W1^T and one per-centre product Qc = new_xyz W1[:, :3]^T (both on the MFMA GEMM), and the grouped layer
// is a gather: Y1[(i,k), :] = P[idx[i,k]] - Qc[i] (+ bias).  edge_max.hip does the same on a square graph; here the graph is bipartite
// and the result is the row-major operand of layer 2, so the gather writes it out instead of reducing it.
// Nothing here uses a float atomic; every sum has a fixed order, so results repeat bit for bit.
//
// Multi-radius ball query (sa_ballquery_kernel).  One wave per centre walks the cloud once in steps of 64 candidates; the squared distance
// d2 = (dx*dx + dy*dy) + dz*dz (dx = centre - candidate, every operation rounded on its own) is formed once per candidate and compared
// against every scale's r*r (strict).  Per scale the ballot, the ranks and the padding are those of pointops.hip's scan_kernel, so every
// list equals spgan_pointops_ballquery's bit for bit.  A scale stops taking hits at its nsample; the walk ends when all scales are full.
//
// Gather (sa_gather_kernel).  A workgroup owns SG_PT centres = SG_PT*K consecutive rows of Y1, which is also the tile of the BatchNorm
// (sum, centred M2) records that spgan_colstats_finalize_bn reads (tile_rows = spgan_sa_gather_tile_rows(K)).  Threads are laid out as
// (channel group, row slot): consecutive lanes read consecutive columns of one P row (coalesced; at most SG_LANES groups per pass, wider
// layers take several passes), a slot walks rows slot, slot + nslots, ...
// The records use sums shifted by the tile's first row (M2 = sum d^2 - (sum d)^2 / n without cancellation), merged over the row slots in
// slot order through LDS.  Padded duplicate slots are rows like any other.  An index outside [0, n) sets *bad and reads point 0.
//
// Backward of the gather (sa_scatter_kernel).  dP[p, :] = the sum of dY1's rows over the slots that read point p, in ascending slot order
// (the reverse CSR of spgan_gather_csr), and dQc[q, :] = -(the sum of dY1's K rows of centre q, ascending), one thread per output element,
// each into a column slice of the buffer all scales share, so no per-scale temporary and no concatenation exist.
//
// Channel-major slices (sa_rows_cm_kernel).  out[b, c0+c, s] = rows[(b*S+s), c] and its inverse: the scales of a module write their pooled
// rows into channel slices of one [B, Ctot, S] tensor, so no concatenation runs.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;
constexpr int SQ_WAVES = 4;
constexpr int SG_PT = 8;      // centres per workgroup of the gather
constexpr int SG_LANES = 64;  // channel groups per pass of the gather: a wave reads one contiguous row segment

__device__ __forceinline__ float dist2(float qx, float qy, float qz, float cx, float cy, float cz) {
  const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
  return (dx * dx + dy * dy) + dz * dz;
}

struct QueryArgs {
  int count;
  float r2[SPGAN_SA_MAX_SCALES];
  int nsample[SPGAN_SA_MAX_SCALES];
  int32_t* idx[SPGAN_SA_MAX_SCALES];
};

__global__ __launch_bounds__(SQ_WAVES * 64) void sa_ballquery_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz, int n, int m,
                                                                     long total, const QueryArgs a) {
  const int lane = threadIdx.x & 63;
  const long q = (long)blockIdx.x * SQ_WAVES + (threadIdx.x >> 6);
  if (q >= total) return;
  const long b = q / m;
  const float* cloud = xyz + (size_t)b * n * 3;
  const float qx = new_xyz[q * 3], qy = new_xyz[q * 3 + 1], qz = new_xyz[q * 3 + 2];
  int cnt[SPGAN_SA_MAX_SCALES], first[SPGAN_SA_MAX_SCALES];
#pragma unroll
  for (int s = 0; s < SPGAN_SA_MAX_SCALES; ++s) cnt[s] = first[s] = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    float d2 = __builtin_inff();
    if (i < n) d2 = dist2(qx, qy, qz, cloud[(size_t)i * 3], cloud[(size_t)i * 3 + 1], cloud[(size_t)i * 3 + 2]);
    bool open = false;      // wave-uniform: a scale still takes hits
#pragma unroll
    for (int s = 0; s < SPGAN_SA_MAX_SCALES; ++s) {
      if (s < a.count && cnt[s] < a.nsample[s]) {
        bool hit = i < n && d2 < a.r2[s];
        u64 mask = __ballot(hit);
        if (mask != 0) {
          const int rank = __popcll(mask & ((1ull << lane) - 1ull));
          hit = hit && cnt[s] + rank < a.nsample[s];      // keep the hits that still fit
          mask = __ballot(hit);
          if (cnt[s] == 0) first[s] = base + __builtin_ctzll(mask);
          if (hit) a.idx[s][(size_t)q * a.nsample[s] + cnt[s] + rank] = i;
          cnt[s] += __popcll(mask);
        }
        open = open || cnt[s] < a.nsample[s];
      }
    }
    if (!open) break;
  }
#pragma unroll
  for (int s = 0; s < SPGAN_SA_MAX_SCALES; ++s) {
    if (s < a.count) {
      const int fill = cnt[s] == 0 ? 0 : first[s];
      for (int t = min(cnt[s], a.nsample[s]) + lane; t < a.nsample[s]; t += 64) a.idx[s][(size_t)q * a.nsample[s] + t] = fill;
    }
  }
}

template <int V>
__device__ __forceinline__ void ldv(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// P [B*n, ldp] (columns colp ..), Qc [Q, ldq] (columns colq ..), idx [Q, K] local indices, Y [Q*K, ldy]; part [tiles, C, 2] or NULL
template <int V>
__global__ __launch_bounds__(256) void sa_gather_kernel(const float* __restrict__ P, int ldp, const float* __restrict__ Qc, int ldq,
                                                        const float* __restrict__ bias, const int32_t* __restrict__ idx, int n, int m, long Q, int K,
                                                        int C, float* __restrict__ Y, int ldy, float* __restrict__ part, int* __restrict__ bad) {
  __shared__ float red[2][256 * V];
  const long q0 = (long)blockIdx.x * SG_PT;
  if (q0 >= Q) return;
  const int nq = (int)min((long)SG_PT, Q - q0);
  const long rows = (long)nq * K;      // of this tile
  const long e0 = q0 * K;
  const int QF = C / V;
  int QFp = 1;
  while (QFp < QF && QFp < SG_LANES) QFp <<= 1;
  const int cq = threadIdx.x & (QFp - 1), slot = threadIdx.x / QFp, nslots = 256 / QFp;
  const float cnt = (float)rows;
  // the tile's first row shifts the sums
  int j0 = idx[e0];
  if (j0 < 0 || j0 >= n) j0 = 0;
  const float* p_first = P + ((size_t)(q0 / m) * n + j0) * ldp;
  for (int c0 = 0; c0 < C; c0 += QFp * V) {
    const int c = c0 + cq * V;
    const bool ok = c < C;
    float s1[V], s2[V], y0[V], bv[V];
#pragma unroll
    for (int u = 0; u < V; ++u) s1[u] = s2[u] = y0[u] = bv[u] = 0.f;
    if (ok) {
      if (bias) ldv<V>(bias + c, bv);
      if (part) {
        float pv[V], qv[V];
        ldv<V>(p_first + c, pv);
        ldv<V>(Qc + (size_t)q0 * ldq + c, qv);
#pragma unroll
        for (int u = 0; u < V; ++u) y0[u] = (pv[u] - qv[u]) + bv[u];
      }
      for (long r = slot; r < rows; r += nslots) {
        const long e = e0 + r;
        const long q = e / K;
        int j = idx[e];
        if (j < 0 || j >= n) {
          if (bad) *bad = 1;
          j = 0;
        }
        float pv[V], qv[V], yv[V];
        ldv<V>(P + ((size_t)(q / m) * n + j) * ldp + c, pv);
        ldv<V>(Qc + (size_t)q * ldq + c, qv);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          yv[u] = (pv[u] - qv[u]) + bv[u];
          const float d = yv[u] - y0[u];
          s1[u] += d;
          s2[u] = fmaf(d, d, s2[u]);
        }
        stv<V>(Y + (size_t)e * ldy + c, yv);
      }
    }
    if (part) {      // a kernel argument: uniform
#pragma unroll
      for (int u = 0; u < V; ++u) {
        red[0][threadIdx.x * V + u] = s1[u];
        red[1][threadIdx.x * V + u] = s2[u];
      }
      __syncthreads();
      if (slot == 0 && ok) {
#pragma unroll
        for (int u = 0; u < V; ++u) {
          float t1 = 0.f, t2 = 0.f;
          for (int s = 0; s < nslots; ++s) {      // fixed order
            t1 += red[0][(s * QFp + cq) * V + u];
            t2 += red[1][(s * QFp + cq) * V + u];
          }
          float* o = part + ((size_t)blockIdx.x * C + c + u) * 2;
          o[0] = fmaf(cnt, y0[u], t1);
          o[1] = fmaxf(t2 - t1 * t1 / cnt, 0.f);
        }
      }
      __syncthreads();
    }
  }
}

// to_cm: cm[b, c0+c, s] = rows[(b*S+s)*C + c], one thread per element of the slice with s fastest;  else the inverse with c fastest
__global__ void sa_rows_cm_kernel(float* __restrict__ rows, float* __restrict__ cm, int S, int C, int c0, int Ctot, size_t total, bool to_cm) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  if (to_cm) {
    const size_t s = t % S, c = (t / S) % C, b = t / ((size_t)S * C);
    cm[(b * Ctot + c0 + c) * S + s] = rows[(b * S + s) * C + c];
  } else {
    const size_t c = t % C, q = t / C, b = q / S, s = q % S;
    rows[t] = cm[(b * Ctot + c0 + c) * S + s];
  }
}

// threads [0, totalP): dP[p, c] over the slot list of p;  threads [totalP, totalP + totalQ): dQ[q, c] = -sum_k dY[(q*K + k), c]
__global__ void sa_scatter_kernel(const float* __restrict__ dY, int ld, int C, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                  size_t totalP, float* __restrict__ dP, int ldp, size_t totalQ, int K, float* __restrict__ dQ, int ldq) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < totalP) {
    const size_t p = t / C;
    const int c = (int)(t % C);
    const int e0 = rowptr[2 * p], e1 = rowptr[2 * p + 1];
    float acc = 0.f;
    for (int i = e0; i < e1; ++i) acc += dY[(size_t)src[i] * ld + c];
    dP[p * ldp + c] = acc;
    return;
  }
  t -= totalP;
  if (t < totalQ) {
    const size_t q = t / C;
    const int c = (int)(t % C);
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc += dY[(q * K + k) * ld + c];
    dQ[q * ldq + c] = -acc;
  }
}

bool aligned4(const void* p, int a, int b) { return ((uintptr_t)p & 15) == 0 && a % 4 == 0 && b % 4 == 0; }

}  // namespace

extern "C" int spgan_sa_gather_tile_rows(int K) { return K > 0 ? SG_PT * K : 0; }

extern "C" int spgan_sa_ballquery_multi(const spgan_sa_query_args* a, const float* xyz, const float* new_xyz, int B, int n, int m, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(a && xyz && new_xyz && B >= 1 && n >= 1 && m >= 1 && a->count >= 1 && a->count <= SPGAN_SA_MAX_SCALES);
  SPGAN_CHECK_ARG((size_t)B * n < 2147483647u / 3 && (size_t)B * m < 2147483647u / 3);
  QueryArgs k;
  k.count = a->count;
  for (int s = 0; s < SPGAN_SA_MAX_SCALES; ++s) {
    const bool on = s < a->count;
    SPGAN_CHECK_ARG(!on || (a->idx[s] && a->nsample[s] >= 1 && (size_t)B * m * a->nsample[s] < 2147483647u));
    k.r2[s] = on ? a->radius[s] * a->radius[s] : 0.f;
    k.nsample[s] = on ? a->nsample[s] : 0;
    k.idx[s] = on ? a->idx[s] : nullptr;
  }
  const long total = (long)B * m;
  hipLaunchKernelGGL(sa_ballquery_kernel, dim3(cdiv(total, SQ_WAVES)), dim3(SQ_WAVES * 64), 0, (hipStream_t)s_, xyz, new_xyz, n, m, total, k);
  return spgan_launch_status();
}

extern "C" int spgan_sa_gather(const float* P, int ldp, int colp, const float* Qc, int ldq, int colq, const float* bias, const int32_t* idx, int B,
                               int n, int m, int K, int C, float* Y, int ldy, float* part, int32_t* bad, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(P && Qc && idx && Y && B >= 1 && n >= 1 && m >= 1 && K >= 1 && C >= 1 && colp >= 0 && colq >= 0);
  SPGAN_CHECK_ARG(ldp >= colp + C && ldq >= colq + C && ldy >= C && (size_t)B * n < 2147483647u && (size_t)B * m * K < 2147483647u);
  const long Q = (long)B * m;
  const float* Pc = P + colp;
  const float* Qcc = Qc + colq;
  const dim3 grid(cdiv(Q, SG_PT));
  if (C % 4 == 0 && aligned4(Pc, ldp, 0) && aligned4(Qcc, ldq, 0) && aligned4(Y, ldy, 0) && (!bias || aligned4(bias, 0, 0)))
    hipLaunchKernelGGL(sa_gather_kernel<4>, grid, dim3(256), 0, (hipStream_t)s_, Pc, ldp, Qcc, ldq, bias, idx, n, m, Q, K, C, Y, ldy, part, bad);
  else
    hipLaunchKernelGGL(sa_gather_kernel<1>, grid, dim3(256), 0, (hipStream_t)s_, Pc, ldp, Qcc, ldq, bias, idx, n, m, Q, K, C, Y, ldy, part, bad);
  return spgan_launch_status();
}

extern "C" int spgan_sa_scatter(const float* dY, int ld, int C, const int32_t* rowptr, const int32_t* src, int BN, float* dP, int ldp, int colp, int Q,
                                int K, float* dQ, int ldq, int colq, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dY && C >= 1 && ld >= C && Q >= 1 && K >= 1 && (dP || dQ) && (size_t)Q * K < 2147483647u);
  SPGAN_CHECK_ARG(!dP || (rowptr && src && BN >= 1 && colp >= 0 && ldp >= colp + C));
  SPGAN_CHECK_ARG(!dQ || (colq >= 0 && ldq >= colq + C));
  const size_t totalP = dP ? (size_t)BN * C : 0, totalQ = dQ ? (size_t)Q * C : 0;
  hipLaunchKernelGGL(sa_scatter_kernel, dim3(cdiv((long)(totalP + totalQ), 256)), dim3(256), 0, (hipStream_t)s_, dY, ld, C, rowptr, src, totalP,
                     dP ? dP + colp : nullptr, ldp, totalQ, K, dQ ? dQ + colq : nullptr, ldq);
  return spgan_launch_status();
}

extern "C" int spgan_sa_rows_to_cm_slice(const float* rows, int B, int S, int C, int c0, int Ctot, float* cm, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(rows && cm && B >= 1 && S >= 1 && C >= 1 && c0 >= 0 && c0 + C <= Ctot);
  const size_t total = (size_t)B * S * C;
  hipLaunchKernelGGL(sa_rows_cm_kernel, dim3(cdiv((long)total, 256)), dim3(256), 0, (hipStream_t)s_, const_cast<float*>(rows), cm, S, C, c0, Ctot,
                     total, true);
  return spgan_launch_status();
}

extern "C" int spgan_sa_cm_slice_to_rows(const float* cm, int B, int S, int C, int c0, int Ctot, float* rows, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(rows && cm && B >= 1 && S >= 1 && C >= 1 && c0 >= 0 && c0 + C <= Ctot);
  const size_t total = (size_t)B * S * C;
  hipLaunchKernelGGL(sa_rows_cm_kernel, dim3(cdiv((long)total, 256)), dim3(256), 0, (hipStream_t)s_, rows, const_cast<float*>(cm), S, C, c0, Ctot,
                     total, false);
  return spgan_launch_status();
}
