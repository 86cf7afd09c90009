// Max-aggregation edge convolution (Generation/modules.py:779-796: get_edge_features -> Conv2d 1x1 -> BatchNorm2d -> ReLU -> max over k).
//
// With W = [Wc | Wd] the pre-norm value of edge (i, j) is
//     y(i,j,c) = Q(i,c) + P(n(i,j),c),      P = Wd x,   Q = (Wc - Wd) x + b,
// so one per-point GEMM produces PQ[M, 2F] = [P | Q] and every per-edge quantity is a gather of rows of P (L2-resident: a shape's P is
// N*F*4 bytes).  BatchNorm + ReLU is t -> relu(a*t + s) per channel, monotone (rising for a >= 0, falling for a < 0) in floating point as
// well as p -> Q + p, hence
//     max_j relu(a*y_j + s) = relu(a*(Q + max_j P_n) + s)   for a >= 0,   the same with min_j for a < 0.
// No [.., N, k] tensor exists in forward or backward:
//   gather   per (point, channel): max / min of P over the neighbours with their ranks (first rank wins a tie), and the
//            train-mode BatchNorm2d statistics over the M*k edges as (sum, centred M2) records per tile of EM_PT points
//            (finalised by spgan_colstats_finalize_bn).  With scale / shift given (eval mode) it finishes in the same pass.
//   finish   picks max or min by the sign of a_c, writes out[M,F] and the selected rank (bit 7 set: clipped by the ReLU).
//   bwd_point  r = g * 1[out > 0] in place, and the plain-sum records of (sum r, sum r*xhat_sel)  ->  d beta, d gamma.
//   bwd_graph  dQ per point and dP over the reverse CSR (in-edge lists in ascending edge order: no float atomics, reproducible sums).
//   dbl_point / dbl_graph  the second derivative through dx (opt-in: edgeConv(double_backward=True)): the same two passes with the
//            direction's per-point product VPQ = v Wst^T as a second operand.
//
// Thread mapping: a workgroup owns EM_PT consecutive points; a thread owns V consecutive channels (V = 4: 16-byte loads of P, Q, r) of
// the points p = slot, slot + nslots, ...  Workgroups are dealt so that an XCD works through a contiguous eighth of the points.
#include "common.hpp"

namespace {

constexpr int EM_PT = 32;      // points per workgroup = rows of a statistics record / k
constexpr int EM_CLIPPED = 0x80;

// XCD-aware workgroup order (as in edge.hip): logical block xcd * per + t runs on XCD xcd, so the rows of P one shape gathers are fetched
// into one L2.  Grids are rounded up to a multiple of 8; logical blocks past the end find no points.
__device__ __forceinline__ int xcd_block() {
  const int per = gridDim.x >> 3;
  return (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
}
inline int grid8(long n) { return (int)((n + 7) / 8 * 8); }

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
template <int V>
__device__ __forceinline__ void ldb(const uint8_t* __restrict__ p, int (&v)[V]) {
  if constexpr (V == 4) {
    const uchar4 t = *reinterpret_cast<const uchar4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void stb(uint8_t* __restrict__ p, const int (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<uchar4*>(p) = make_uchar4((uint8_t)v[0], (uint8_t)v[1], (uint8_t)v[2], (uint8_t)v[3]);
  else *p = (uint8_t)v[0];
}

// the (channel group, point slot) of a thread: QFp = channel groups per pass (a power of two <= 256), 256 / QFp point slots
struct Lanes {
  int QFp, q, slot, nslots;
};
__device__ __forceinline__ Lanes lanes_of(int F, int V) {
  const int QF = F / V;
  int QFp = 1;
  while (QFp < QF && QFp < 256) QFp <<= 1;
  return Lanes{QFp, (int)threadIdx.x & (QFp - 1), (int)threadIdx.x / QFp, 256 / QFp};
}

// out = relu(a*(Q + p) + s) with p = max or min of P by the sign of a; rank | EM_CLIPPED when the ReLU clips
__device__ __forceinline__ float finish_one(float a, float s, float q, float pmx, float pmn, int jmx, int jmn, int& sel) {
  const bool up = a >= 0.f;
  const float o = fmaxf(fmaf(a, q + (up ? pmx : pmn), s), 0.f);
  sel = (up ? jmx : jmn) | (o > 0.f ? 0 : EM_CLIPPED);
  return o;
}

// ------------------------------------------------------------------------------------------ forward: gather (+ statistics | + finish)
template <int V>
__global__ __launch_bounds__(256) void edge_max_gather_kernel(const float* __restrict__ PQ, int ld, const int32_t* __restrict__ idx, int M, int k, int F,
                                                              float* __restrict__ pmax, float* __restrict__ pmin, uint8_t* __restrict__ rmax,
                                                              uint8_t* __restrict__ rmin, float* __restrict__ part,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              float* __restrict__ out, uint8_t* __restrict__ sel) {
  __shared__ float red[2][256 * V];
  const int bx = xcd_block();
  const int p0 = bx * EM_PT;
  if (p0 >= M) return;
  const int np = min(EM_PT, M - p0);
  const Lanes L = lanes_of(F, V);
  const float cnt = (float)(np * k);
  for (int c0 = 0; c0 < F; c0 += L.QFp * V) {
    const int c = c0 + L.q * V;
    const bool ok = c < F;
    // shifted sums (d = y - y0, y0 = the tile's first edge value of the channel): M2 = sum d^2 - (sum d)^2 / n without cancellation
    float s1[V], s2[V], y0[V], a[V], sh[V];
#pragma unroll
    for (int u = 0; u < V; ++u) s1[u] = s2[u] = y0[u] = a[u] = sh[u] = 0.f;
    if (ok) {
      if (part) {
        float qv[V], pv[V];
        ldv<V>(PQ + (size_t)p0 * ld + F + c, qv);
        ldv<V>(PQ + (size_t)idx[(size_t)p0 * k] * ld + c, pv);
#pragma unroll
        for (int u = 0; u < V; ++u) y0[u] = qv[u] + pv[u];
      }
      if (scale) {
        ldv<V>(scale + c, a);
        ldv<V>(shift + c, sh);
      }
      for (int p = L.slot; p < np; p += L.nslots) {
        const int i = p0 + p;
        const int32_t* nb = idx + (size_t)i * k;
        float qv[V], mx[V], mn[V];
        int jx[V], jn[V];
        ldv<V>(PQ + (size_t)i * ld + F + c, qv);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          mx[u] = -INFINITY; mn[u] = INFINITY; jx[u] = jn[u] = 0;
        }
#pragma unroll 4
        for (int r = 0; r < k; ++r) {
          float pv[V];
          ldv<V>(PQ + (size_t)nb[r] * ld + c, pv);
#pragma unroll
          for (int u = 0; u < V; ++u) {
            if (pv[u] > mx[u]) { mx[u] = pv[u]; jx[u] = r; }     // strict: the first rank keeps an exact tie
            if (pv[u] < mn[u]) { mn[u] = pv[u]; jn[u] = r; }
            const float d = (qv[u] + pv[u]) - y0[u];
            s1[u] += d;
            s2[u] = fmaf(d, d, s2[u]);
          }
        }
        const size_t o = (size_t)i * F + c;
        if (scale) {
          float ov[V];
          int sv[V];
#pragma unroll
          for (int u = 0; u < V; ++u) ov[u] = finish_one(a[u], sh[u], qv[u], mx[u], mn[u], jx[u], jn[u], sv[u]);
          stv<V>(out + o, ov);
          stb<V>(sel + o, sv);
        } else {
          stv<V>(pmax + o, mx); stv<V>(pmin + o, mn);
          stb<V>(rmax + o, jx); stb<V>(rmin + o, jn);
        }
      }
    }
    if (part) {   // a kernel argument: uniform
#pragma unroll
      for (int u = 0; u < V; ++u) {
        red[0][threadIdx.x * V + u] = s1[u];
        red[1][threadIdx.x * V + u] = s2[u];
      }
      __syncthreads();
      if (L.slot == 0 && ok) {
#pragma unroll
        for (int u = 0; u < V; ++u) {
          float t1 = 0.f, t2 = 0.f;
          for (int s = 0; s < L.nslots; ++s) {      // fixed order
            t1 += red[0][(s * L.QFp + L.q) * V + u];
            t2 += red[1][(s * L.QFp + L.q) * V + u];
          }
          float* o = part + ((size_t)bx * F + c + u) * 2;
          o[0] = fmaf(cnt, y0[u], t1);
          o[1] = fmaxf(t2 - t1 * t1 / cnt, 0.f);
        }
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------ forward: finish (train mode, after the statistics)
template <int V>
__global__ __launch_bounds__(256) void edge_max_finish_kernel(const float* __restrict__ PQ, int ld, const float* __restrict__ pmax,
                                                              const float* __restrict__ pmin, const uint8_t* __restrict__ rmax,
                                                              const uint8_t* __restrict__ rmin, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int M, int F, float* __restrict__ out,
                                                              uint8_t* __restrict__ sel) {
  const int QF = F / V;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)M * QF) return;
  const int i = (int)(t / QF), c = (int)(t % QF) * V;
  const size_t o = (size_t)i * F + c;
  float a[V], sh[V], qv[V], mx[V], mn[V], ov[V];
  int jx[V], jn[V], sv[V];
  ldv<V>(scale + c, a); ldv<V>(shift + c, sh);
  ldv<V>(PQ + (size_t)i * ld + F + c, qv);
  ldv<V>(pmax + o, mx); ldv<V>(pmin + o, mn);
  ldb<V>(rmax + o, jx); ldb<V>(rmin + o, jn);
#pragma unroll
  for (int u = 0; u < V; ++u) ov[u] = finish_one(a[u], sh[u], qv[u], mx[u], mn[u], jx[u], jn[u], sv[u]);
  stv<V>(out + o, ov);
  stb<V>(sel + o, sv);
}

// ------------------------------------------------------------------------------------------ backward: per point
// g[M,F] is overwritten with r = g * 1[out > 0]; part [tiles][F][2] = (sum r, sum r * xhat(i, sel, c)) per tile of EM_PT points.
template <int V>
__global__ __launch_bounds__(256) void edge_max_bwd_point_kernel(float* __restrict__ g, const uint8_t* __restrict__ sel, const float* __restrict__ PQ,
                                                                 int ld, const int32_t* __restrict__ idx, int M, int k, int F,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 float* __restrict__ part) {
  __shared__ float red[2][256 * V];
  const int bx = xcd_block();
  const int p0 = bx * EM_PT;
  if (p0 >= M) return;
  const int np = min(EM_PT, M - p0);
  const Lanes L = lanes_of(F, V);
  for (int c0 = 0; c0 < F; c0 += L.QFp * V) {
    const int c = c0 + L.q * V;
    const bool ok = c < F;
    float s1[V], s2[V];
#pragma unroll
    for (int u = 0; u < V; ++u) s1[u] = s2[u] = 0.f;
    if (ok) {
      float mu[V], iv[V];
      ldv<V>(mean + c, mu); ldv<V>(invstd + c, iv);
      for (int p = L.slot; p < np; p += L.nslots) {
        const int i = p0 + p;
        const size_t o = (size_t)i * F + c;
        float gv[V], qv[V];
        int sv[V];
        ldv<V>(g + o, gv); ldb<V>(sel + o, sv);
        ldv<V>(PQ + (size_t)i * ld + F + c, qv);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          if (sv[u] & EM_CLIPPED) {
            gv[u] = 0.f;
          } else {
            const int n = idx[(size_t)i * k + sv[u]];          // the selected neighbour differs from channel to channel
            const float xh = ((qv[u] + PQ[(size_t)n * ld + c + u]) - mu[u]) * iv[u];
            s1[u] += gv[u];
            s2[u] = fmaf(gv[u], xh, s2[u]);
          }
        }
        stv<V>(g + o, gv);
      }
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
      red[0][threadIdx.x * V + u] = s1[u];
      red[1][threadIdx.x * V + u] = s2[u];
    }
    __syncthreads();
    if (L.slot == 0 && ok) {
#pragma unroll
      for (int u = 0; u < V; ++u) {
        float t1 = 0.f, t2 = 0.f;
        for (int s = 0; s < L.nslots; ++s) {
          t1 += red[0][(s * L.QFp + L.q) * V + u];
          t2 += red[1][(s * L.QFp + L.q) * V + u];
        }
        float* o = part + ((size_t)bx * F + c + u) * 2;
        o[0] = t1;
        o[1] = t2;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------ backward: dQ per point, dP over the in-edges
// sums = [sum r | sum r*xhat] (train mode) or NULL (eval mode: the statistics are constants, only the first terms survive).
//   dQ(i,c) = a [ r - k*s1/E - (s2/E) * invstd * (k*Q + sum_j P_n - k*mean) ]
//   dP(m,c) = a [ sum_{(i,j)->m, j = sel(i,c)} r(i,c) - deg*s1/E - (s2/E) * invstd * (sum_{(i,j)->m} Q(i,c) + deg*(P(m,c) - mean)) ],   E = M*k
template <int V>
__global__ __launch_bounds__(256) void edge_max_bwd_graph_kernel(const float* __restrict__ r, const uint8_t* __restrict__ sel, const float* __restrict__ PQ,
                                                                 int ld, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                                                 const int32_t* __restrict__ idx, int M, int k, int F, const float* __restrict__ scale,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 const float* __restrict__ sums, float rE, float* __restrict__ dPQ, int ldd) {
  const int bx = xcd_block();
  const int p0 = bx * EM_PT;
  if (p0 >= M) return;
  const int np = min(EM_PT, M - p0);
  const Lanes L = lanes_of(F, V);
  const float kf = (float)k;
  for (int c0 = 0; c0 < F; c0 += L.QFp * V) {
    const int c = c0 + L.q * V;
    if (c >= F) continue;
    float a[V], mu[V], m1[V], m2[V];
    ldv<V>(scale + c, a);
#pragma unroll
    for (int u = 0; u < V; ++u) mu[u] = m1[u] = m2[u] = 0.f;
    if (sums) {
      float iv[V], t1[V], t2[V];
      ldv<V>(mean + c, mu); ldv<V>(invstd + c, iv);
      ldv<V>(sums + c, t1); ldv<V>(sums + F + c, t2);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        m1[u] = t1[u] * rE;
        m2[u] = t2[u] * rE * iv[u];
      }
    }
    for (int p = L.slot; p < np; p += L.nslots) {
      const int m = p0 + p;
      const int t0 = rowptr[m], t1 = rowptr[m + 1];
      float acc[V], sq[V];
#pragma unroll
      for (int u = 0; u < V; ++u) acc[u] = sq[u] = 0.f;
      for (int t = t0; t < t1; ++t) {          // ascending edge ids: a fixed summation order
        const int e = src[t];
        const int i = e / k, j = e - i * k;
        float rv[V];
        int sv[V];
        ldv<V>(r + (size_t)i * F + c, rv); ldb<V>(sel + (size_t)i * F + c, sv);
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] += (sv[u] & (EM_CLIPPED - 1)) == j ? rv[u] : 0.f;   // r is zero where the ReLU clipped
        if (sums) {
          float qv[V];
          ldv<V>(PQ + (size_t)i * ld + F + c, qv);
#pragma unroll
          for (int u = 0; u < V; ++u) sq[u] += qv[u];
        }
      }
      const float deg = (float)(t1 - t0);
      float rm[V], dP[V], dQ[V];
      ldv<V>(r + (size_t)m * F + c, rm);
      if (sums) {
        float pm[V], qm[V], ps[V];
        ldv<V>(PQ + (size_t)m * ld + c, pm); ldv<V>(PQ + (size_t)m * ld + F + c, qm);
        // sum_j P_n of the point's own k edges, gathered again (L2-resident rows) instead of kept from the forward pass: a saved
        // [M,F] float tensor would be a tenth of the edge tensor this layer exists to avoid
        const int32_t* nb = idx + (size_t)m * k;
#pragma unroll
        for (int u = 0; u < V; ++u) ps[u] = 0.f;
#pragma unroll 4
        for (int rr = 0; rr < k; ++rr) {
          float pv[V];
          ldv<V>(PQ + (size_t)nb[rr] * ld + c, pv);
#pragma unroll
          for (int u = 0; u < V; ++u) ps[u] += pv[u];
        }
#pragma unroll
        for (int u = 0; u < V; ++u) {
          dQ[u] = a[u] * (rm[u] - kf * m1[u] - m2[u] * (kf * (qm[u] - mu[u]) + ps[u]));
          dP[u] = a[u] * (acc[u] - deg * m1[u] - m2[u] * (sq[u] + deg * (pm[u] - mu[u])));
        }
      } else {
#pragma unroll
        for (int u = 0; u < V; ++u) {
          dQ[u] = a[u] * rm[u];
          dP[u] = a[u] * acc[u];
        }
      }
      stv<V>(dPQ + (size_t)m * ldd + c, dP);
      stv<V>(dPQ + (size_t)m * ldd + F + c, dQ);
    }
  }
}

// ------------------------------------------------------------------------------------------ double backward: the edge sums of the direction
// VPQ [M, >= 2F] = [VP | VQ] = v Wst^T; t(i,j) = VQ_i + VP_n(i,j) is gathered like the pre-norm value.  part_t [tiles][F][2] = (sum_e t_e,
// sum_e t_e * xhat_e) over the tile's own edges (NULL: eval mode, no edge sum is needed), part_s [tiles][F][2] = (sum_i r_i * t(i, sel), 0).
template <int V>
__global__ __launch_bounds__(256) void edge_max_dbl_point_kernel(const float* __restrict__ r, const uint8_t* __restrict__ sel, const float* __restrict__ PQ,
                                                                 int ld, const float* __restrict__ VPQ, int ldvq, const int32_t* __restrict__ idx, int M,
                                                                 int k, int F, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 float* __restrict__ part_t, float* __restrict__ part_s) {
  __shared__ float red[3][256 * V];
  const int bx = xcd_block();
  const int p0 = bx * EM_PT;
  if (p0 >= M) return;
  const int np = min(EM_PT, M - p0);
  const Lanes L = lanes_of(F, V);
  for (int c0 = 0; c0 < F; c0 += L.QFp * V) {
    const int c = c0 + L.q * V;
    const bool ok = c < F;
    float s1[V], s2[V], s3[V];
#pragma unroll
    for (int u = 0; u < V; ++u) s1[u] = s2[u] = s3[u] = 0.f;
    if (ok) {
      float mu[V], iv[V];
#pragma unroll
      for (int u = 0; u < V; ++u) mu[u] = iv[u] = 0.f;
      if (part_t) {   // a kernel argument: uniform
        ldv<V>(mean + c, mu); ldv<V>(invstd + c, iv);
      }
      for (int p = L.slot; p < np; p += L.nslots) {
        const int i = p0 + p;
        const int32_t* nb = idx + (size_t)i * k;
        const size_t o = (size_t)i * F + c;
        float rv[V], vq[V];
        int sv[V];
        ldv<V>(r + o, rv); ldb<V>(sel + o, sv);
        ldv<V>(VPQ + (size_t)i * ldvq + F + c, vq);
        if (part_t) {
          float qv[V];
          ldv<V>(PQ + (size_t)i * ld + F + c, qv);
#pragma unroll 4
          for (int rr = 0; rr < k; ++rr) {
            float pv[V], vp[V];
            ldv<V>(PQ + (size_t)nb[rr] * ld + c, pv);
            ldv<V>(VPQ + (size_t)nb[rr] * ldvq + c, vp);
#pragma unroll
            for (int u = 0; u < V; ++u) {
              const float t = vq[u] + vp[u];
              s1[u] += t;
              s2[u] = fmaf(t, ((qv[u] + pv[u]) - mu[u]) * iv[u], s2[u]);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < V; ++u) {
          if (!(sv[u] & EM_CLIPPED)) {                                  // r is zero where the ReLU clipped
            const int n = nb[sv[u]];                                    // the selected neighbour differs from channel to channel
            s3[u] = fmaf(rv[u], vq[u] + VPQ[(size_t)n * ldvq + c + u], s3[u]);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
      red[0][threadIdx.x * V + u] = s1[u];
      red[1][threadIdx.x * V + u] = s2[u];
      red[2][threadIdx.x * V + u] = s3[u];
    }
    __syncthreads();
    if (L.slot == 0 && ok) {
#pragma unroll
      for (int u = 0; u < V; ++u) {
        float t1 = 0.f, t2 = 0.f, t3 = 0.f;
        for (int s = 0; s < L.nslots; ++s) {      // fixed order
          t1 += red[0][(s * L.QFp + L.q) * V + u];
          t2 += red[1][(s * L.QFp + L.q) * V + u];
          t3 += red[2][(s * L.QFp + L.q) * V + u];
        }
        const size_t o = ((size_t)bx * F + c + u) * 2;
        if (part_t) {
          part_t[o] = t1;
          part_t[o + 1] = t2;
        }
        part_s[o] = t3;
        part_s[o + 1] = 0.f;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------ double backward: ghat per point, PQbar over the in-edges
// With E = M*k, cc = a*invstd/E, A = S - s1*T1/E - s2*T2/E the cotangent of the (never stored) edge value z_e is
//   zbar_e = K0 + K1*xhat_e + K2*t_e + K3*r_i*d(e = e*(i)),
//   K0 = cc*(T2*s1 + s2*T1)/E,  K1 = cc*(2*s2*T2/E - A),  K2 = -cc*s2,  K3 = -cc*T2,
// so, as in edge_max_bwd_graph_kernel with VPQ as a second operand,
//   Qbar(i,c) = k*K0 + K1*invstd*(k*(Q - mean) + sum_j P_n) + K2*(k*VQ + sum_j VP_n) + K3*r
//   Pbar(m,c) = deg*K0 + K1*invstd*(sum_{(i,j)->m} Q_i + deg*(P_m - mean)) + K2*(sum_{(i,j)->m} VQ_i + deg*VP_m) + K3*sum_{(i,j)->m, j = sel(i,c)} r(i,c)
//   ghat(i,c) = 1[out > 0] * a * (t_sel - T1/E - xhat_sel*T2/E).
// sums == NULL (eval mode: the statistics are constants): ghat = 1[out > 0] * a * t_sel and there is no PQbar.
template <int V>
__global__ __launch_bounds__(256) void edge_max_dbl_graph_kernel(const float* __restrict__ r, const uint8_t* __restrict__ sel, const float* __restrict__ PQ,
                                                                 int ld, const float* __restrict__ VPQ, int ldvq, const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ src, const int32_t* __restrict__ idx, int M, int k, int F,
                                                                 const float* __restrict__ scale, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, const float* __restrict__ sums,
                                                                 const float* __restrict__ dsums, float rE, float* __restrict__ ghat,
                                                                 float* __restrict__ PQbar, int ldbar) {
  const int bx = xcd_block();
  const int p0 = bx * EM_PT;
  if (p0 >= M) return;
  const int np = min(EM_PT, M - p0);
  const Lanes L = lanes_of(F, V);
  const float kf = (float)k;
  for (int c0 = 0; c0 < F; c0 += L.QFp * V) {
    const int c = c0 + L.q * V;
    if (c >= F) continue;
    float a[V], mu[V], K0[V], K1[V], K2[V], K3[V], g1[V], g2[V];
    ldv<V>(scale + c, a);
#pragma unroll
    for (int u = 0; u < V; ++u) mu[u] = K0[u] = K1[u] = K2[u] = K3[u] = g1[u] = g2[u] = 0.f;
    if (sums) {
      float iv[V], s1[V], s2[V], T1[V], T2[V], S[V];
      ldv<V>(mean + c, mu); ldv<V>(invstd + c, iv);
      ldv<V>(sums + c, s1); ldv<V>(sums + F + c, s2);
      ldv<V>(dsums + c, T1); ldv<V>(dsums + F + c, T2); ldv<V>(dsums + 2 * F + c, S);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const float A = S[u] - s1[u] * T1[u] * rE - s2[u] * T2[u] * rE;
        const float cc = a[u] * iv[u] * rE;
        K0[u] = cc * (T2[u] * s1[u] + s2[u] * T1[u]) * rE;
        K1[u] = cc * (2.f * s2[u] * T2[u] * rE - A) * iv[u];          // times invstd: xhat = (z - mean) * invstd
        K2[u] = -cc * s2[u];
        K3[u] = -cc * T2[u];
        g1[u] = T1[u] * rE;
        g2[u] = T2[u] * rE * iv[u];
      }
    }
    for (int p = L.slot; p < np; p += L.nslots) {
      const int m = p0 + p;
      const int32_t* nb = idx + (size_t)m * k;
      float rm[V], qm[V], vqm[V], gh[V];
      int sm[V];
      ldv<V>(r + (size_t)m * F + c, rm); ldb<V>(sel + (size_t)m * F + c, sm);
      ldv<V>(PQ + (size_t)m * ld + F + c, qm);
      ldv<V>(VPQ + (size_t)m * ldvq + F + c, vqm);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        gh[u] = 0.f;
        if (!(sm[u] & EM_CLIPPED)) {
          const int n = nb[sm[u]];
          const float ts = vqm[u] + VPQ[(size_t)n * ldvq + c + u];
          const float zs = (qm[u] + PQ[(size_t)n * ld + c + u]) - mu[u];
          gh[u] = a[u] * ((ts - g1[u]) - zs * g2[u]);
        }
      }
      stv<V>(ghat + (size_t)m * F + c, gh);
      if (!sums) continue;
      const int t0 = rowptr[m], t1 = rowptr[m + 1];
      float acc[V], sq[V], svq[V];
#pragma unroll
      for (int u = 0; u < V; ++u) acc[u] = sq[u] = svq[u] = 0.f;
      for (int t = t0; t < t1; ++t) {          // ascending edge ids: a fixed summation order
        const int e = src[t];
        const int i = e / k, j = e - i * k;
        float rv[V], qv[V], vq[V];
        int sv[V];
        ldv<V>(r + (size_t)i * F + c, rv); ldb<V>(sel + (size_t)i * F + c, sv);
        ldv<V>(PQ + (size_t)i * ld + F + c, qv);
        ldv<V>(VPQ + (size_t)i * ldvq + F + c, vq);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          acc[u] += (sv[u] & (EM_CLIPPED - 1)) == j ? rv[u] : 0.f;   // r is zero where the ReLU clipped
          sq[u] += qv[u];
          svq[u] += vq[u];
        }
      }
      const float deg = (float)(t1 - t0);
      float pm[V], vpm[V], ps[V], vps[V], bP[V], bQ[V];
      ldv<V>(PQ + (size_t)m * ld + c, pm);
      ldv<V>(VPQ + (size_t)m * ldvq + c, vpm);
#pragma unroll
      for (int u = 0; u < V; ++u) ps[u] = vps[u] = 0.f;
#pragma unroll 4
      for (int rr = 0; rr < k; ++rr) {
        float pv[V], vp[V];
        ldv<V>(PQ + (size_t)nb[rr] * ld + c, pv);
        ldv<V>(VPQ + (size_t)nb[rr] * ldvq + c, vp);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          ps[u] += pv[u];
          vps[u] += vp[u];
        }
      }
#pragma unroll
      for (int u = 0; u < V; ++u) {
        bQ[u] = kf * K0[u] + K1[u] * (kf * (qm[u] - mu[u]) + ps[u]) + K2[u] * (kf * vqm[u] + vps[u]) + K3[u] * rm[u];
        bP[u] = deg * K0[u] + K1[u] * (sq[u] + deg * (pm[u] - mu[u])) + K2[u] * (svq[u] + deg * vpm[u]) + K3[u] * acc[u];
      }
      stv<V>(PQbar + (size_t)m * ldbar + c, bP);
      stv<V>(PQbar + (size_t)m * ldbar + F + c, bQ);
    }
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool sizes_ok(int M, int k, int F, int ld) {
  return M > 0 && k > 0 && k < EM_CLIPPED && F > 0 && ld >= 2 * F && (long)M * k <= 0x7fffffffL;   // edge ids are int32; a rank fits 7 bits
}

}  // namespace

extern "C" int spgan_edge_max_tile_points(void) { return EM_PT; }

extern "C" int spgan_edge_max_gather(const float* PQ, int ld, const int32_t* idx, int M, int k, int F, float* pmax, float* pmin, uint8_t* rmax,
                                     uint8_t* rmin, float* partials, const float* scale, const float* shift, float* out,
                                     uint8_t* sel, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(PQ && idx && sizes_ok(M, k, F, ld));
  const bool fin = scale != nullptr;
  if (fin) SPGAN_CHECK_ARG(shift && out && sel && !pmax && !pmin && !rmax && !rmin);   // one pass: eval mode
  else SPGAN_CHECK_ARG(pmax && pmin && rmax && rmin && partials && !shift && !out && !sel);
  const dim3 g(grid8(cdiv(M, EM_PT))), b(256);
  const bool v4 = F % 4 == 0 && ld % 4 == 0 && al16(PQ) && (fin ? al16(scale) && al16(shift) && al16(out) && al4(sel)
                                                                : al16(pmax) && al16(pmin) && al4(rmax) && al4(rmin));
  if (v4)
    hipLaunchKernelGGL(edge_max_gather_kernel<4>, g, b, 0, (hipStream_t)s_, PQ, ld, idx, M, k, F, pmax, pmin, rmax, rmin, partials, scale, shift, out, sel);
  else
    hipLaunchKernelGGL(edge_max_gather_kernel<1>, g, b, 0, (hipStream_t)s_, PQ, ld, idx, M, k, F, pmax, pmin, rmax, rmin, partials, scale, shift, out, sel);
  return spgan_launch_status();
}

extern "C" int spgan_edge_max_finish(const float* PQ, int ld, const float* pmax, const float* pmin, const uint8_t* rmax, const uint8_t* rmin,
                                     const float* scale, const float* shift, int M, int F, float* out, uint8_t* sel, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(PQ && pmax && pmin && rmax && rmin && scale && shift && out && sel && sizes_ok(M, 1, F, ld));
  const bool v4 = F % 4 == 0 && ld % 4 == 0 && al16(PQ) && al16(pmax) && al16(pmin) && al4(rmax) && al4(rmin) && al16(scale) && al16(shift) &&
                  al16(out) && al4(sel);
  const long items = (long)M * (v4 ? F / 4 : F);
  if (v4)
    hipLaunchKernelGGL(edge_max_finish_kernel<4>, dim3(cdiv(items, 256)), dim3(256), 0, (hipStream_t)s_, PQ, ld, pmax, pmin, rmax, rmin, scale, shift, M, F, out, sel);
  else
    hipLaunchKernelGGL(edge_max_finish_kernel<1>, dim3(cdiv(items, 256)), dim3(256), 0, (hipStream_t)s_, PQ, ld, pmax, pmin, rmax, rmin, scale, shift, M, F, out, sel);
  return spgan_launch_status();
}

extern "C" int spgan_edge_max_bwd_point(float* g, const uint8_t* sel, const float* PQ, int ld, const int32_t* idx, int M, int k, int F,
                                        const float* mean, const float* invstd, float* partials, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(g && sel && PQ && idx && mean && invstd && partials && sizes_ok(M, k, F, ld));
  const dim3 gr(grid8(cdiv(M, EM_PT))), b(256);
  const bool v4 = F % 4 == 0 && ld % 4 == 0 && al16(PQ) && al16(g) && al4(sel) && al16(mean) && al16(invstd);
  if (v4) hipLaunchKernelGGL(edge_max_bwd_point_kernel<4>, gr, b, 0, (hipStream_t)s_, g, sel, PQ, ld, idx, M, k, F, mean, invstd, partials);
  else hipLaunchKernelGGL(edge_max_bwd_point_kernel<1>, gr, b, 0, (hipStream_t)s_, g, sel, PQ, ld, idx, M, k, F, mean, invstd, partials);
  return spgan_launch_status();
}

extern "C" int spgan_edge_max_bwd_graph(const float* r, const uint8_t* sel, const float* PQ, int ld, const int32_t* rowptr, const int32_t* src,
                                        const int32_t* idx, int M, int k, int F, const float* scale, const float* mean, const float* invstd,
                                        const float* sums, float* dPQ, int ldd, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(r && sel && PQ && rowptr && src && scale && dPQ && sizes_ok(M, k, F, ld) && ldd >= 2 * F);
  if (sums) SPGAN_CHECK_ARG(idx && mean && invstd);       // train mode
  const dim3 gr(grid8(cdiv(M, EM_PT))), b(256);
  const bool v4 = F % 4 == 0 && ld % 4 == 0 && ldd % 4 == 0 && al16(PQ) && al16(r) && al4(sel) && al16(scale) && al16(dPQ) &&
                  (!sums || (al16(mean) && al16(invstd) && al16(sums)));
  const float rE = 1.0f / ((float)M * (float)k);
  if (v4)
    hipLaunchKernelGGL(edge_max_bwd_graph_kernel<4>, gr, b, 0, (hipStream_t)s_, r, sel, PQ, ld, rowptr, src, idx, M, k, F, scale, mean, invstd, sums, rE, dPQ, ldd);
  else
    hipLaunchKernelGGL(edge_max_bwd_graph_kernel<1>, gr, b, 0, (hipStream_t)s_, r, sel, PQ, ld, rowptr, src, idx, M, k, F, scale, mean, invstd, sums, rE, dPQ, ldd);
  return spgan_launch_status();
}

extern "C" int spgan_edge_max_dbl_point(const float* r, const uint8_t* sel, const float* PQ, int ld, const float* VPQ, int ldvq, const int32_t* idx,
                                        int M, int k, int F, const float* mean, const float* invstd, float* partials_t, float* partials_s,
                                        spgan_stream_t s_) {
  SPGAN_CHECK_ARG(r && sel && PQ && VPQ && idx && partials_s && sizes_ok(M, k, F, ld) && ldvq >= 2 * F);
  if (partials_t) SPGAN_CHECK_ARG(mean && invstd);         // train mode
  else SPGAN_CHECK_ARG(!mean && !invstd);
  const dim3 gr(grid8(cdiv(M, EM_PT))), b(256);
  const bool v4 = F % 4 == 0 && ld % 4 == 0 && ldvq % 4 == 0 && al16(PQ) && al16(VPQ) && al16(r) && al4(sel) &&
                  (!partials_t || (al16(mean) && al16(invstd)));
  if (v4)
    hipLaunchKernelGGL(edge_max_dbl_point_kernel<4>, gr, b, 0, (hipStream_t)s_, r, sel, PQ, ld, VPQ, ldvq, idx, M, k, F, mean, invstd, partials_t, partials_s);
  else
    hipLaunchKernelGGL(edge_max_dbl_point_kernel<1>, gr, b, 0, (hipStream_t)s_, r, sel, PQ, ld, VPQ, ldvq, idx, M, k, F, mean, invstd, partials_t, partials_s);
  return spgan_launch_status();
}

extern "C" int spgan_edge_max_dbl_graph(const float* r, const uint8_t* sel, const float* PQ, int ld, const float* VPQ, int ldvq, const int32_t* rowptr,
                                        const int32_t* src, const int32_t* idx, int M, int k, int F, const float* scale, const float* mean,
                                        const float* invstd, const float* sums, const float* dsums, float* ghat, float* PQbar, int ldbar,
                                        spgan_stream_t s_) {
  SPGAN_CHECK_ARG(r && sel && PQ && VPQ && idx && scale && ghat && sizes_ok(M, k, F, ld) && ldvq >= 2 * F);
  if (sums) SPGAN_CHECK_ARG(dsums && mean && invstd && rowptr && src && PQbar && ldbar >= 2 * F);       // train mode
  else SPGAN_CHECK_ARG(!dsums && !PQbar);
  const dim3 gr(grid8(cdiv(M, EM_PT))), b(256);
  const bool v4 = F % 4 == 0 && ld % 4 == 0 && ldvq % 4 == 0 && al16(PQ) && al16(VPQ) && al16(r) && al4(sel) && al16(scale) && al16(ghat) &&
                  (!sums || (ldbar % 4 == 0 && al16(PQbar) && al16(mean) && al16(invstd) && al16(sums) && al16(dsums)));
  const float rE = 1.0f / ((float)M * (float)k);
  if (v4)
    hipLaunchKernelGGL(edge_max_dbl_graph_kernel<4>, gr, b, 0, (hipStream_t)s_, r, sel, PQ, ld, VPQ, ldvq, rowptr, src, idx, M, k, F, scale, mean, invstd,
                       sums, dsums, rE, ghat, PQbar, ldbar);
  else
    hipLaunchKernelGGL(edge_max_dbl_graph_kernel<1>, gr, b, 0, (hipStream_t)s_, r, sel, PQ, ld, VPQ, ldvq, rowptr, src, idx, M, k, F, scale, mean, invstd,
                       sums, dsums, rE, ghat, PQbar, ldbar);
  return spgan_launch_status();
}
