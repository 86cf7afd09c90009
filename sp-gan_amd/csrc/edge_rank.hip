// Full-rank edge convolution: the core of the reference's deform_edgeConv_simple / deform_edgeConv_first (Generation/modules.py:1394-1466):
// Conv2d(2Fin -> F1, 1x1) over get_edge_features, BatchNorm2d, LeakyReLU, then Conv2d(F1 -> O, [1,k]) that collapses the k neighbour
// ranks with one weight per rank.
//
// With W1 = [Wc | Wd] the pre-norm value of edge (i, r) is z(i,r,:) = Q_i + P_n(i,r), P = x Wd^T, Q = x (Wc - Wd)^T + b1 (one per-point
// GEMM -> PQ [M, 2F1] = [P | Q], as edge_max.hip), so the activated edge tensor h(i,r,c) = lrelu(scale1[c] * z + shift1[c]) is a
// function of gathered rows of P and never has to exist in memory in forward:
//   spgan_edge_rank_gemm     y[i,o] = b2[o] + sum_{r<k, c<F1} W2i[o, r*F1 + c] h(i,r,c): a product with K = k*F1 whose A operand is
//                            formed in LDS.  A workgroup owns ER_PT points; per step it stages h of ER_RS ranks x ER_CK channels
//                            (16 lanes fetch 256 contiguous bytes of one row of P: the whole row for F1 <= 64) and feeds
//                            v_mfma_f32_16x16x4_f32 from there; the B operand comes straight from the weight image (L2).  Epilogue:
//                            bias and the (sum, centred M2) column records of y (spgan_colstats_finalize_bn).
//   spgan_edge_rank_wgrad    dW2i[o, r*F1 + c] = sum_i dy[i,o] h(i,r,c), h recomputed and staged the same way; a workgroup owns 128 output
//                            channels x 64 input channels x ER_RB ranks of one point range; the ranges are summed in split order.
//   spgan_edge_rank_dgrad    da(i,r,c) = lrelu'(a(i,r,c)) * sum_o dy[i,o] W2i[o, r*F1 + c]  [M,k,F1] (the one per-edge buffer, backward
//                            only), a plain MFMA product per rank with both operands from global memory / L2 (W2t = the transposed
//                            image [k*F1, O]); the epilogue recomputes the sign of a = scale1 * z + shift1 and writes per-tile column
//                            sums of da and da * zhat (zhat = (z - mean1) * invstd1), summed over points and ranks in a fixed order.
//   spgan_edge_rank_scatter  dPQ [M, 2F1] = [dP | dQ] from da: dz = scale1 * (da - A - zhat * Bc) (train; A, Bc = the reduced sums / E) or
//                            scale1 * da (eval); dQ_i = sum_r dz(i,r), dP_j = sum over the in-edge list of j (spgan_csr_build) in
//                            ascending edge order.  No float atomics anywhere.
//
// The weighted layer (deform_edgeConv_feat, Generation/modules.py:1543-1599) multiplies h by a per-edge weight s before the [1,k] convolution
// (WMod below).  spgan_edge_weight_gemm / _wgrad are the gemm / wgrad kernels staging h * s; spgan_edge_weight_dgrad turns dm = dy W2i into
// the gradients reaching both pre-activation BatchNorm outputs (du, g3) with their column records; spgan_edge_weight_norm writes the
// softmax normaliser per (point, channel) and spgan_edge_weight_gather the pre-norm rows of the weight MLP's first layer.
//
// The coordinate-guided layer (deform_edgeConv, Generation/modules.py:1468-1540) feeds that weight MLP the product of two activated
// 16-channel branches, one over the features and one over the coordinates, both gathered through the same graph:
//   spgan_edge_weight_gather2  W0[(i*k + r), c] = a_a * a_b, a_x = lrelu(scale_x * (Qx_i + Px_n(i,r)) + shift_x)   [M*k, F]
//   spgan_edge_weight_split    GA = lrelu'(pre_a) * dW0 * a_b, GB = lrelu'(pre_b) * dW0 * a_a  [M,k,F] with the per-tile column records
//                              (sum G, sum G * zhat) of each branch, as spgan_edge_rank_dgrad writes them
// Both are gather passes over rows of F floats: consecutive lanes take consecutive 16-byte pieces of consecutive edge rows.
//
// The bilateral upsampling layer (bilateral_upsample_edgeConv, Generation/modules.py:847-925) multiplies the stored pre-norm tensor of
// upsample_edgeConv's interpolation, U [M,k,F1] with rows (point, rank) and a BatchNorm affine that alternates with the rank's parity, by the
// same per-edge weight.  spgan_edge_stored_gemm / _wgrad / _dgrad are spgan_edge_weight_gemm / _wgrad / _dgrad with h read from U
// (stored_h4) instead of gathered through the graph; s comes from weight_s() as everywhere.
//
// MFMA operand order as in edge_window.hip: a 16-wide K block is one 16-byte fragment per lane (lane group g = lane>>4 holds K elements
// 4g..4g+3), consumed by four MFMA steps; A and B agree on that order.  fp32 operands, fp32 accumulation: exact products.
#include "common.hpp"

namespace {

constexpr int ER_KMAX = 32;
constexpr int ER_PT = 32;               // points per workgroup of gemm / dgrad = rows of a statistics record
constexpr int ER_CK = 64;               // channels staged per step
constexpr int ER_RS = 4;                // ranks staged per step
constexpr int ER_PST = ER_CK + 4;       // 4 (mod 32) floats between points: the 16 points of a ds_read_b128 group spread over all banks
constexpr int ER_RB = 2;                // ranks per weight-gradient workgroup
constexpr int ER_WPST = ER_CK + 8;      // ER_RB * ER_WPST = 16 (mod 32): the two point groups of a ds_read_b32 half hit disjoint banks

__device__ __forceinline__ int xcd_block() {
  const int per = gridDim.x >> 3;
  return (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
}
inline int grid8(long n) { return (int)((n + 7) / 8 * 8); }

// four consecutive floats of which the first `nvalid` exist (VEC: extents and addresses are multiples of 4 floats: all or nothing)
template <bool VEC>
__device__ __forceinline__ f32x4 ld4(const float* __restrict__ p, int nvalid) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {
    if (nvalid >= 4) v = *reinterpret_cast<const f32x4*>(p);
  } else {
    if (nvalid > 0) v.x = p[0];
    if (nvalid > 1) v.y = p[1];
    if (nvalid > 2) v.z = p[2];
    if (nvalid > 3) v.w = p[3];
  }
  return v;
}

__device__ __forceinline__ f32x4 mfma4(const f32x4& a, const f32x4& b, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  return acc;
}

__device__ __forceinline__ int neighbour(const int32_t* __restrict__ idx, int i, int k, int r, int M) {
  const int n = idx[(size_t)i * k + r];
  return (unsigned)n >= (unsigned)M ? i : n;
}

// a = scale * (Q_i + P_n) + shift: every kernel forms it with these operations, so that the sign the backward recomputes is the forward's
__device__ __forceinline__ float pre_act(float q, float p, float sc, float sh) { return fmaf(sc, q + p, sh); }

// h(i, r, c..c+3) for r = the rank whose neighbour is n; channels past F1 give 0
template <bool VEC>
__device__ __forceinline__ f32x4 rank_h4(const float* __restrict__ PQ, int ld, int F1, int i, int n, int c, const float* __restrict__ sc,
                                         const float* __restrict__ sh, float slope) {
  const int nv = F1 - c;
  const f32x4 p = ld4<VEC>(PQ + (size_t)n * ld + c, nv), q = ld4<VEC>(PQ + (size_t)i * ld + F1 + c, nv);
  const f32x4 a = ld4<VEC>(sc + c, nv), s = ld4<VEC>(sh + c, nv);
  f32x4 h;
#pragma unroll
  for (int u = 0; u < 4; ++u) h[u] = lrelu_f(pre_act(q[u], p[u], a[u], s[u]), slope);
  return h;
}

// The stored form of h (bilateral_upsample_edgeConv): U [M,k,F1] holds the pre-norm value of (point i, rank r, channel c) itself and the
// BatchNorm affine alternates with the rank's parity: sc, sh [2*F1], entry (r & 1) * F1 + c.  No graph: the row is (i*k + r).
template <bool VEC>
__device__ __forceinline__ f32x4 stored_h4(const float* __restrict__ U, int F1, int k, int i, int r, int c, const float* __restrict__ sc,
                                           const float* __restrict__ sh, float slope) {
  const int nv = F1 - c, ch = (r & 1) * F1 + c;
  const f32x4 u = ld4<VEC>(U + ((size_t)i * k + r) * F1 + c, nv), a = ld4<VEC>(sc + ch, nv), s = ld4<VEC>(sh + ch, nv);
  f32x4 h;
#pragma unroll
  for (int v = 0; v < 4; ++v) h[v] = lrelu_f(fmaf(a[v], u[v], s[v]), slope);
  return h;
}

// The per-edge weight of the weighted layers (deform_edgeConv_feat): s(i,r,c) = softmax over r of a3 = lrelu(sc3 * z3 + sh3) with
// z3 [M,k,F1] the stored pre-norm output of the weight MLP, evaluated from the per-(point, channel) normaliser wmax = max_r a3 and
// wrs = 1 / sum_r exp(a3 - wmax) (spgan_edge_weight_norm); wmax == nullptr: s = a3 (softmax=False).  Every kernel forms s with
// weight_s(), so that forward and backward agree bit for bit.
struct WMod {
  const float* z3; const float* sc3; const float* sh3; const float* wmax; const float* wrs;
};
__device__ __forceinline__ float weight_s(float a3, float mx, float rs, bool soft) { return soft ? expf(a3 - mx) * rs : a3; }

template <bool VEC>
__device__ __forceinline__ f32x4 weight_s4(const WMod& m, int F1, int k, int i, int r, int c, float slope) {
  const int nv = F1 - c;
  const f32x4 z = ld4<VEC>(m.z3 + ((size_t)i * k + r) * F1 + c, nv), a = ld4<VEC>(m.sc3 + c, nv), b = ld4<VEC>(m.sh3 + c, nv);
  const bool soft = m.wmax != nullptr;
  f32x4 mx = {0.f, 0.f, 0.f, 0.f}, rs = mx, s;
  if (soft) {
    mx = ld4<VEC>(m.wmax + (size_t)i * F1 + c, nv);
    rs = ld4<VEC>(m.wrs + (size_t)i * F1 + c, nv);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) s[u] = weight_s(lrelu_f(fmaf(a[u], z[u], b[u]), slope), mx[u], rs[u], soft);
  return s;
}

// ------------------------------------------------------------------------------------------ forward
// Per wave: 2 blocks of 16 points x (2 groups of 128 columns) x 2 blocks of 16 output columns; the four waves of a workgroup take 128
// consecutive output columns of each group, so one staging serves 256 output columns.
// MOD: the staged operand is h * s (WMod above): spgan_edge_weight_gemm.
// STORED: h comes from the stored rows PQ = U [M,k,F1] (stored_h4; ld and idx are not read): spgan_edge_stored_gemm.
template <bool VEC, bool MOD, bool STORED = false>
__global__ __launch_bounds__(256, 2) void edge_rank_gemm_kernel(const float* __restrict__ PQ, int ld, const int32_t* __restrict__ idx, int M, int k,
                                                                int F1, const float* __restrict__ sc, const float* __restrict__ sh, float slope,
                                                                const float* __restrict__ W, int ldw, const float* __restrict__ b2, int O,
                                                                float* __restrict__ Y, int ldy, float* __restrict__ part, WMod md) {
  __shared__ __attribute__((aligned(16))) float sm[ER_RS * ER_PT * ER_PST];
  const int bx = xcd_block();
  const int p0 = bx * ER_PT;
  if (p0 >= M) return;
  const int np = min(ER_PT, M - p0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  const float cnt = (float)np;
  for (int ob = 0; ob < O; ob += 256) {
    const int oc0 = ob + wave * 32;                  // + og * 128 + cb * 16 + col
    const bool wave_on = oc0 < O;                    // uniform per wave; idle waves still stage and meet the barriers
    f32x4 acc[2][2][2];
#pragma unroll
    for (int pb = 0; pb < 2; ++pb)
#pragma unroll
      for (int og = 0; og < 2; ++og) acc[pb][og][0] = acc[pb][og][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < k; r0 += ER_RS) {
      const int nr = min(ER_RS, k - r0);
      for (int c0 = 0; c0 < F1; c0 += ER_CK) {
        __syncthreads();
        for (int e = threadIdx.x; e < nr * ER_PT * (ER_CK / 4); e += 256) {
          const int cc = (e & 15) * 4, p = (e >> 4) & (ER_PT - 1), rs = e >> 9;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (p < np && c0 + cc < F1) {
            const int i = p0 + p;
            if constexpr (STORED) v = stored_h4<VEC>(PQ, F1, k, i, r0 + rs, c0 + cc, sc, sh, slope);
            else v = rank_h4<VEC>(PQ, ld, F1, i, neighbour(idx, i, k, r0 + rs, M), c0 + cc, sc, sh, slope);
            if constexpr (MOD) v *= weight_s4<VEC>(md, F1, k, i, r0 + rs, c0 + cc, slope);
          }
          *reinterpret_cast<f32x4*>(sm + (rs * ER_PT + p) * ER_PST + cc) = v;
        }
        __syncthreads();
        if (!wave_on) continue;
        const int nkb = (min(ER_CK, F1 - c0) + 15) >> 4;
        for (int rs = 0; rs < nr; ++rs) {
          for (int kb = 0; kb < nkb; ++kb) {
            const int cc = kb * 16 + 4 * g;
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(sm + (rs * ER_PT + col) * ER_PST + cc);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(sm + (rs * ER_PT + 16 + col) * ER_PST + cc);
#pragma unroll
            for (int og = 0; og < 2; ++og) {
              if (oc0 + og * 128 < O) {              // uniform per wave
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                  const int o = oc0 + og * 128 + cb * 16 + col;
                  const f32x4 b = ld4<VEC>(W + (size_t)min(o, O - 1) * ldw + (size_t)(r0 + rs) * F1 + c0 + cc, o < O ? F1 - (c0 + cc) : 0);
                  acc[0][og][cb] = mfma4(a0, b, acc[0][og][cb]);
                  acc[1][og][cb] = mfma4(a1, b, acc[1][og][cb]);
                }
              }
            }
          }
        }
      }
    }
    if (!wave_on) continue;
    // epilogue: the D fragment of a lane is rows (points) 4g..4g+3 of column col
#pragma unroll
    for (int og = 0; og < 2; ++og) {
      if (oc0 + og * 128 >= O) continue;             // uniform per wave
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const int o = oc0 + og * 128 + cb * 16 + col;
        const float bias = (b2 && o < O) ? b2[o] : 0.f;
        float s1 = 0.f, s2 = 0.f, y0 = 0.f;
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int p = pb * 16 + 4 * g + v;
            const bool ok = p < np && o < O;
            const float val = acc[pb][og][cb][v] + bias;
            if (ok) Y[(size_t)(p0 + p) * ldy + o] = val;
            if (part) {                              // a kernel argument: uniform
              // shifted sums around the tile's first row of the column (point p0: lane `col`, element 0 of the first fragment)
              if (pb == 0 && v == 0) y0 = __shfl(val, col);
              if (ok) {
                const float d = val - y0;
                s1 += d;
                s2 = fmaf(d, d, s2);
              }
            }
          }
        if (part) {
          s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);      // the four point groups of a column, in a fixed order
          s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
          if (g == 0 && o < O) {
            float* rec = part + ((size_t)bx * O + o) * 2;
            rec[0] = fmaf(cnt, y0, s1);
            rec[1] = fmaxf(s2 - s1 * s1 / cnt, 0.f);
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ gradient of the activated edge tensor
// A[p][o] = dy(p,o), B[o][c] = W2t[(r*F1 + c), o], D[p][c]: 32 points x 128 channels per workgroup pass, no LDS.
template <bool VEC>
__global__ __launch_bounds__(256) void edge_rank_dgrad_kernel(const float* __restrict__ G, int ldg, const float* __restrict__ Wt, int ldwt,
                                                              const float* __restrict__ PQ, int ld, const int32_t* __restrict__ idx, int M, int k,
                                                              int F1, int O, const float* __restrict__ sc, const float* __restrict__ sh,
                                                              const float* __restrict__ mean, const float* __restrict__ invstd, float slope,
                                                              float* __restrict__ dA, float* __restrict__ part) {
  const int bx = xcd_block();
  const int p0 = bx * ER_PT;
  if (p0 >= M) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  for (int cp = 0; cp < F1; cp += 128) {
    const int cw = cp + wave * 32;
    if (cw >= F1) continue;
    float a_[2], s_[2], mu[2], is[2], t1[2] = {0.f, 0.f}, t2[2] = {0.f, 0.f};
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int c = cw + cb * 16 + col;
      const bool ok = c < F1;
      a_[cb] = ok ? sc[c] : 0.f; s_[cb] = ok ? sh[c] : 0.f; mu[cb] = ok ? mean[c] : 0.f; is[cb] = ok ? invstd[c] : 0.f;
    }
    for (int r = 0; r < k; ++r) {
      f32x4 acc[2][2];
      acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int ob = 0; ob < O; ob += 16) {
        const int o = ob + 4 * g;
        f32x4 a[2], b[2];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          const int p = p0 + pb * 16 + col;
          a[pb] = ld4<VEC>(G + (size_t)min(p, M - 1) * ldg + o, p < M ? O - o : 0);
        }
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          const int c = cw + cb * 16 + col;
          b[cb] = ld4<VEC>(Wt + ((size_t)r * F1 + min(c, F1 - 1)) * ldwt + o, c < F1 ? O - o : 0);
        }
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) acc[pb][cb] = mfma4(a[pb], b[cb], acc[pb][cb]);
      }
#pragma unroll
      for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int p = p0 + pb * 16 + 4 * g + v;
          if (p >= M) continue;
          const int n = neighbour(idx, p, k, r, M);
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            const int c = cw + cb * 16 + col;
            if (c < F1) {
              const float q = PQ[(size_t)p * ld + F1 + c], pv = PQ[(size_t)n * ld + c];
              const float da = acc[pb][cb][v] * lrelu_mask(pre_act(q, pv, a_[cb], s_[cb]), slope);
              dA[((size_t)p * k + r) * F1 + c] = da;
              t1[cb] += da;
              t2[cb] = fmaf(da, ((q + pv) - mu[cb]) * is[cb], t2[cb]);
            }
          }
        }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float a = t1[cb], b = t2[cb];
      a += __shfl_xor(a, 16); b += __shfl_xor(b, 16);         // the four point groups of a column, in a fixed order
      a += __shfl_xor(a, 32); b += __shfl_xor(b, 32);
      const int c = cw + cb * 16 + col;
      if (g == 0 && c < F1) {
        float* rec = part + ((size_t)bx * F1 + c) * 2;
        rec[0] = a;
        rec[1] = b;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ weight gradient
// D[o][c] (one per rank) += A[o][point] B[point][c]: A = dy (global), B = the staged h; an MFMA step reduces over four consecutive points.
struct RwPlan {
  int n_ot, n_ct, n_rp, tiles, splits, pps;
};
inline RwPlan er_wg_plan(int M, int k, int F1, int O) {
  RwPlan p;
  p.n_ot = cdiv(O, 128); p.n_ct = cdiv(F1, ER_CK); p.n_rp = cdiv(k, ER_RB);
  p.tiles = p.n_ot * p.n_ct * p.n_rp;
  // about 1024 workgroups: a narrow layer is split over up to 512 point ranges, a wide one over a few
  int s = cdiv(1024, p.tiles);
  s = s < 1 ? 1 : (s > 512 ? 512 : s);
  // the workspace (splits * O * k*F1 floats) stays below a quarter of the backward's [M,k,F1] buffer
  const int cap = M / (4 * O);
  s = s > cap ? (cap < 1 ? 1 : cap) : s;
  p.pps = cdiv(cdiv(M, s), 32) * 32;
  p.splits = cdiv(M, p.pps);
  return p;
}

template <bool VEC, bool MOD, bool STORED = false>
__global__ __launch_bounds__(256) void edge_rank_wgrad_kernel(const float* __restrict__ PQ, int ld, const int32_t* __restrict__ idx, int M, int k, int F1,
                                                              const float* __restrict__ sc, const float* __restrict__ sh, float slope,
                                                              const float* __restrict__ G, int ldg, int O, float* __restrict__ ws, RwPlan pl, WMod md) {
  __shared__ __attribute__((aligned(16))) float sm[32 * ER_RB * ER_WPST];
  const int L = xcd_block();
  if (L >= pl.tiles * pl.splits) return;
  const int s = L / pl.tiles, tile = L % pl.tiles;
  const int ot = tile % pl.n_ot, ct = (tile / pl.n_ot) % pl.n_ct, rp = tile / (pl.n_ot * pl.n_ct);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int c0 = ct * ER_CK, r0 = rp * ER_RB, o0 = ot * 128 + wave * 32;
  const int begin = s * pl.pps, end = min(M, begin + pl.pps);
  f32x4 acc[2][ER_RB][4];
#pragma unroll
  for (int rb = 0; rb < ER_RB; ++rb)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[0][rb][cb] = acc[1][rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int pb = begin; pb < end; pb += 32) {
    __syncthreads();
    for (int e = threadIdx.x; e < 32 * ER_RB * (ER_CK / 4); e += 256) {
      const int cc = (e & 15) * 4, rb = (e >> 4) % ER_RB, p = e / (16 * ER_RB);
      const int i = pb + p;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i < end && r0 + rb < k && c0 + cc < F1) {
        if constexpr (STORED) v = stored_h4<VEC>(PQ, F1, k, i, r0 + rb, c0 + cc, sc, sh, slope);
        else v = rank_h4<VEC>(PQ, ld, F1, i, neighbour(idx, i, k, r0 + rb, M), c0 + cc, sc, sh, slope);
        if constexpr (MOD) v *= weight_s4<VEC>(md, F1, k, i, r0 + rb, c0 + cc, slope);
      }
      *reinterpret_cast<f32x4*>(sm + (p * ER_RB + rb) * ER_WPST + cc) = v;
    }
    __syncthreads();
    if (o0 >= O) continue;
    for (int q = 0; q < 8; ++q) {
      if (pb + q * 4 >= end) break;                    // uniform
      const int pt = q * 4 + g;
      const int i = pb + pt;
      float a[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int o = o0 + h * 16 + col;
        a[h] = (i < end && o < O) ? G[(size_t)i * ldg + o] : 0.f;
      }
#pragma unroll
      for (int rb = 0; rb < ER_RB; ++rb) {
        if (r0 + rb < k) {
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) {
            const float b = sm[(pt * ER_RB + rb) * ER_WPST + cb * 16 + col];
            acc[0][rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b, acc[0][rb][cb], 0, 0, 0);
            acc[1][rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b, acc[1][rb][cb], 0, 0, 0);
          }
        }
      }
    }
  }
  const size_t ldw = (size_t)k * F1;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int rb = 0; rb < ER_RB; ++rb)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int o = o0 + h * 16 + 4 * g + v, c = c0 + cb * 16 + col;
          if (r0 + rb < k && o < O && c < F1) ws[((size_t)s * O + o) * ldw + (size_t)(r0 + rb) * F1 + c] = acc[h][rb][cb][v];
        }
}

// dW[o, e] = sum_s ws[s][o][e]: eight lanes per element take the splits s = q, q + 8, ... in ascending order and their partial sums are
// combined in a fixed order (a fixed assignment: run-to-run identical, no float atomics)
__global__ __launch_bounds__(256) void edge_rank_wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int O, int KW, float* __restrict__ dW,
                                                                     int lddw) {
  const size_t t = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 3, n = (size_t)O * KW;
  const int q = threadIdx.x & 7;
  float a = 0.f;
  if (t < n)
    for (int s = q; s < splits; s += 8) a += ws[(size_t)s * n + t];
  a += __shfl_xor(a, 1);
  a += __shfl_xor(a, 2);
  a += __shfl_xor(a, 4);
  if (t < n && q == 0) dW[(t / KW) * lddw + (t % KW)] = a;
}

// ------------------------------------------------------------------------------------------ edge gradients -> point gradients
// one thread per (point, V channels): dQ over the point's own k edges, dP over its in-edge list in ascending edge order
template <int V>
__device__ __forceinline__ void ldv(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  else *p = v[0];
}

template <int V>
__global__ __launch_bounds__(256) void edge_rank_scatter_kernel(const float* __restrict__ dA, const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ src, const float* __restrict__ PQ, int ld,
                                                                const int32_t* __restrict__ idx, int M, int k, int F1, const float* __restrict__ sc,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const float* __restrict__ sums, float inv_e, float* __restrict__ dPQ, int ldd) {
  const int QC = F1 / V;
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= (size_t)M * QC) return;
  const int m = (int)(tid / QC), c = (int)(tid % QC) * V;
  const bool train = sums != nullptr;
  float a[V], mu[V], is[V], A[V], Bc[V], pm[V], qm[V], dq[V], dp[V], d[V], o[V];
  ldv<V>(sc + c, a);
#pragma unroll
  for (int u = 0; u < V; ++u) mu[u] = is[u] = A[u] = Bc[u] = pm[u] = qm[u] = o[u] = dq[u] = dp[u] = 0.f;
  if (train) {
    ldv<V>(mean + c, mu); ldv<V>(invstd + c, is);
    ldv<V>(sums + c, A); ldv<V>(sums + F1 + c, Bc);
    ldv<V>(PQ + (size_t)m * ld + c, pm); ldv<V>(PQ + (size_t)m * ld + F1 + c, qm);
#pragma unroll
    for (int u = 0; u < V; ++u) {
      A[u] *= inv_e; Bc[u] *= inv_e;
    }
  }
  for (int r = 0; r < k; ++r) {
    ldv<V>(dA + ((size_t)m * k + r) * F1 + c, d);
    if (train) ldv<V>(PQ + (size_t)neighbour(idx, m, k, r, M) * ld + c, o);
#pragma unroll
    for (int u = 0; u < V; ++u) {
      float dz = d[u];
      if (train) dz = dz - A[u] - (((qm[u] + o[u]) - mu[u]) * is[u]) * Bc[u];
      dq[u] += a[u] * dz;
    }
  }
  const int t0 = rowptr[m], t1 = rowptr[m + 1];
  for (int t = t0; t < t1; ++t) {            // ascending edge ids: a fixed summation order
    const int e = src[t];
    ldv<V>(dA + (size_t)e * F1 + c, d);
    if (train) ldv<V>(PQ + (size_t)(e / k) * ld + F1 + c, o);
#pragma unroll
    for (int u = 0; u < V; ++u) {
      float dz = d[u];
      if (train) dz = dz - A[u] - (((o[u] + pm[u]) - mu[u]) * is[u]) * Bc[u];
      dp[u] += a[u] * dz;
    }
  }
  stv<V>(dPQ + (size_t)m * ldd + c, dp);
  stv<V>(dPQ + (size_t)m * ldd + F1 + c, dq);
}

// ------------------------------------------------------------------------------------------ the weighted layer's own passes
// z(i,r,c) = Q_i + P_n(i,r) written out [M*k, F]: the narrow first layer of the weight MLP (F = 16), the rows of the products that follow
__global__ __launch_bounds__(256) void edge_weight_gather_kernel(const float* __restrict__ PQ, int ld, const int32_t* __restrict__ idx, int M, int k, int F,
                                                                 float* __restrict__ Z) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= (size_t)M * k * F) return;
  const int c = (int)(tid % F);
  const size_t e = tid / F;
  const int i = (int)(e / k), r = (int)(e % k);
  Z[tid] = PQ[(size_t)i * ld + F + c] + PQ[(size_t)neighbour(idx, i, k, r, M) * ld + c];
}

// one thread per (point, channel): the softmax normaliser over the k ranks, in ascending rank order
__global__ __launch_bounds__(256) void edge_weight_norm_kernel(const float* __restrict__ z3, int M, int k, int F1, const float* __restrict__ sc3,
                                                               const float* __restrict__ sh3, float slope, float* __restrict__ wmax,
                                                               float* __restrict__ wrs) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= (size_t)M * F1) return;
  const int c = (int)(tid % F1);
  const float* z = z3 + (tid / F1) * (size_t)k * F1 + c;
  const float a = sc3[c], b = sh3[c];
  float mx = -INFINITY, sum = 0.f;
  for (int r = 0; r < k; ++r) mx = fmaxf(mx, lrelu_f(fmaf(a, z[(size_t)r * F1], b), slope));
  for (int r = 0; r < k; ++r) sum += expf(lrelu_f(fmaf(a, z[(size_t)r * F1], b), slope) - mx);
  wmax[tid] = mx;
  wrs[tid] = 1.f / sum;
}

// dm(p,r,c) = sum_o dy[p,o] W2t[r*F1 + c, o] as edge_rank_dgrad_kernel forms it (the same tiling: a lane owns all k ranks of its
// (point, channel) pairs), then with h and s recomputed
//   du = lrelu'(a_h) * dm * s                                  records (sum du, sum du * uhat)
//   g3 = lrelu'(a_3) * s * (dm*h - t),  t = sum_r dm*h*s       records (sum g3, sum g3 * z3hat)        (softmax; else g3 = lrelu'(a_3) * dm*h)
// t needs every rank: pass 0 parks dm in dU and accumulates t in registers, pass 1 reads the lane's own dm back and writes du over it.
template <bool VEC>
__global__ __launch_bounds__(256) void edge_weight_dgrad_kernel(const float* __restrict__ G, int ldg, const float* __restrict__ Wt, int ldwt,
                                                                const float* __restrict__ PQ, int ld, const int32_t* __restrict__ idx, int M, int k,
                                                                int F1, int O, const float* __restrict__ sc, const float* __restrict__ sh,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd, float slope,
                                                                WMod md, const float* __restrict__ mean3, const float* __restrict__ invstd3,
                                                                float* dU, float* __restrict__ G3, float* __restrict__ partU,
                                                                float* __restrict__ part3) {
  const int bx = xcd_block();
  const int p0 = bx * ER_PT;
  if (p0 >= M) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  const bool soft = md.wmax != nullptr;
  const int npass = soft ? 2 : 1;
  for (int cp = 0; cp < F1; cp += 128) {
    const int cw = cp + wave * 32;
    if (cw >= F1) continue;
    float a_[2], s_[2], mu[2], is[2], a3_[2], s3_[2], mu3[2], is3[2];
    float u1[2] = {0.f, 0.f}, u2[2] = {0.f, 0.f}, w1[2] = {0.f, 0.f}, w2[2] = {0.f, 0.f};
    float t[2][4][2], mx[2][4][2], rs[2][4][2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int c = cw + cb * 16 + col;
      const bool ok = c < F1;
      a_[cb] = ok ? sc[c] : 0.f; s_[cb] = ok ? sh[c] : 0.f; mu[cb] = ok ? mean[c] : 0.f; is[cb] = ok ? invstd[c] : 0.f;
      a3_[cb] = ok ? md.sc3[c] : 0.f; s3_[cb] = ok ? md.sh3[c] : 0.f; mu3[cb] = ok ? mean3[c] : 0.f; is3[cb] = ok ? invstd3[c] : 0.f;
#pragma unroll
      for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int p = p0 + pb * 16 + 4 * g + v;
          const bool on = soft && ok && p < M;
          t[pb][v][cb] = 0.f;
          mx[pb][v][cb] = on ? md.wmax[(size_t)p * F1 + c] : 0.f;
          rs[pb][v][cb] = on ? md.wrs[(size_t)p * F1 + c] : 0.f;
        }
    }
    for (int pass = 0; pass < npass; ++pass) {
      const bool last = pass == npass - 1;
      for (int r = 0; r < k; ++r) {
        f32x4 acc[2][2];
        acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (pass == 0) {
          for (int ob = 0; ob < O; ob += 16) {
            const int o = ob + 4 * g;
            f32x4 a[2], b[2];
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
              const int p = p0 + pb * 16 + col;
              a[pb] = ld4<VEC>(G + (size_t)min(p, M - 1) * ldg + o, p < M ? O - o : 0);
            }
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
              const int c = cw + cb * 16 + col;
              b[cb] = ld4<VEC>(Wt + ((size_t)r * F1 + min(c, F1 - 1)) * ldwt + o, c < F1 ? O - o : 0);
            }
#pragma unroll
            for (int pb = 0; pb < 2; ++pb)
#pragma unroll
              for (int cb = 0; cb < 2; ++cb) acc[pb][cb] = mfma4(a[pb], b[cb], acc[pb][cb]);
          }
        }
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int p = p0 + pb * 16 + 4 * g + v;
            if (p >= M) continue;
            const int n = neighbour(idx, p, k, r, M);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
              const int c = cw + cb * 16 + col;
              if (c < F1) {
                const size_t e = ((size_t)p * k + r) * F1 + c;
                const float dm = pass == 0 ? acc[pb][cb][v] : dU[e];
                const float q = PQ[(size_t)p * ld + F1 + c], pv = PQ[(size_t)n * ld + c];
                const float ah = pre_act(q, pv, a_[cb], s_[cb]);
                const float z = md.z3[e];
                const float a3 = fmaf(a3_[cb], z, s3_[cb]);
                const float s = weight_s(lrelu_f(a3, slope), mx[pb][v][cb], rs[pb][v][cb], soft);
                const float ds = dm * lrelu_f(ah, slope);
                if (!last) {
                  dU[e] = dm;
                  t[pb][v][cb] = fmaf(ds, s, t[pb][v][cb]);
                } else {
                  const float du = lrelu_mask(ah, slope) * dm * s;
                  const float g3 = lrelu_mask(a3, slope) * (soft ? s * (ds - t[pb][v][cb]) : ds);
                  dU[e] = du;
                  G3[e] = g3;
                  u1[cb] += du;
                  u2[cb] = fmaf(du, ((q + pv) - mu[cb]) * is[cb], u2[cb]);
                  w1[cb] += g3;
                  w2[cb] = fmaf(g3, (z - mu3[cb]) * is3[cb], w2[cb]);
                }
              }
            }
          }
      }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float a = u1[cb], b = u2[cb], c3 = w1[cb], d3 = w2[cb];
      a += __shfl_xor(a, 16); b += __shfl_xor(b, 16); c3 += __shfl_xor(c3, 16); d3 += __shfl_xor(d3, 16);      // the four point groups, in a fixed order
      a += __shfl_xor(a, 32); b += __shfl_xor(b, 32); c3 += __shfl_xor(c3, 32); d3 += __shfl_xor(d3, 32);
      const int c = cw + cb * 16 + col;
      if (g == 0 && c < F1) {
        float* ru = partU + ((size_t)bx * F1 + c) * 2;
        float* r3 = part3 + ((size_t)bx * F1 + c) * 2;
        ru[0] = a; ru[1] = b;
        r3[0] = c3; r3[1] = d3;
      }
    }
  }
}

// edge_weight_dgrad_kernel for the stored form of h (stored_h4): no graph, a1 = sc[(r & 1)*F1 + c] * U + sh[..], and the h branch's
// records have one column per (rank parity, channel): partU [tiles][2*F1][2].  k is even, so the rank loop runs over pairs and every
// per-parity value stays in a register.  dU receives dm in pass 0 and gU in pass 1: it must not be U.
template <bool VEC>
__global__ __launch_bounds__(256) void edge_stored_dgrad_kernel(const float* __restrict__ G, int ldg, const float* __restrict__ Wt, int ldwt,
                                                                const float* __restrict__ U, int M, int k, int F1, int O,
                                                                const float* __restrict__ sc, const float* __restrict__ sh,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd, float slope,
                                                                WMod md, const float* __restrict__ mean3, const float* __restrict__ invstd3,
                                                                float* __restrict__ dU, float* __restrict__ G3, float* __restrict__ partU,
                                                                float* __restrict__ part3) {
  const int bx = xcd_block();
  const int p0 = bx * ER_PT;
  if (p0 >= M) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  const bool soft = md.wmax != nullptr;
  const int npass = soft ? 2 : 1;
  for (int cp = 0; cp < F1; cp += 128) {
    const int cw = cp + wave * 32;
    if (cw >= F1) continue;
    float a_[2][2], s_[2][2], mu[2][2], is[2][2], a3_[2], s3_[2], mu3[2], is3[2];
    float u1[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, u2[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, w1[2] = {0.f, 0.f}, w2[2] = {0.f, 0.f};
    float t[2][4][2], mx[2][4][2], rs[2][4][2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int c = cw + cb * 16 + col;
      const bool ok = c < F1;
#pragma unroll
      for (int hp = 0; hp < 2; ++hp) {
        const int ch = hp * F1 + c;
        a_[hp][cb] = ok ? sc[ch] : 0.f; s_[hp][cb] = ok ? sh[ch] : 0.f; mu[hp][cb] = ok ? mean[ch] : 0.f; is[hp][cb] = ok ? invstd[ch] : 0.f;
      }
      a3_[cb] = ok ? md.sc3[c] : 0.f; s3_[cb] = ok ? md.sh3[c] : 0.f; mu3[cb] = ok ? mean3[c] : 0.f; is3[cb] = ok ? invstd3[c] : 0.f;
#pragma unroll
      for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int p = p0 + pb * 16 + 4 * g + v;
          const bool on = soft && ok && p < M;
          t[pb][v][cb] = 0.f;
          mx[pb][v][cb] = on ? md.wmax[(size_t)p * F1 + c] : 0.f;
          rs[pb][v][cb] = on ? md.wrs[(size_t)p * F1 + c] : 0.f;
        }
    }
    for (int pass = 0; pass < npass; ++pass) {
      const bool last = pass == npass - 1;
      for (int r2 = 0; r2 < k; r2 += 2) {
#pragma unroll
        for (int hp = 0; hp < 2; ++hp) {
          const int r = r2 + hp;
          f32x4 acc[2][2];
          acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (pass == 0) {
            for (int ob = 0; ob < O; ob += 16) {
              const int o = ob + 4 * g;
              f32x4 a[2], b[2];
#pragma unroll
              for (int pb = 0; pb < 2; ++pb) {
                const int p = p0 + pb * 16 + col;
                a[pb] = ld4<VEC>(G + (size_t)min(p, M - 1) * ldg + o, p < M ? O - o : 0);
              }
#pragma unroll
              for (int cb = 0; cb < 2; ++cb) {
                const int c = cw + cb * 16 + col;
                b[cb] = ld4<VEC>(Wt + ((size_t)r * F1 + min(c, F1 - 1)) * ldwt + o, c < F1 ? O - o : 0);
              }
#pragma unroll
              for (int pb = 0; pb < 2; ++pb)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) acc[pb][cb] = mfma4(a[pb], b[cb], acc[pb][cb]);
            }
          }
#pragma unroll
          for (int pb = 0; pb < 2; ++pb)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int p = p0 + pb * 16 + 4 * g + v;
              if (p >= M) continue;
#pragma unroll
              for (int cb = 0; cb < 2; ++cb) {
                const int c = cw + cb * 16 + col;
                if (c < F1) {
                  const size_t e = ((size_t)p * k + r) * F1 + c;
                  const float dm = pass == 0 ? acc[pb][cb][v] : dU[e];
                  const float u = U[e];
                  const float ah = fmaf(a_[hp][cb], u, s_[hp][cb]);
                  const float z = md.z3[e];
                  const float a3 = fmaf(a3_[cb], z, s3_[cb]);
                  const float s = weight_s(lrelu_f(a3, slope), mx[pb][v][cb], rs[pb][v][cb], soft);
                  const float ds = dm * lrelu_f(ah, slope);
                  if (!last) {
                    dU[e] = dm;
                    t[pb][v][cb] = fmaf(ds, s, t[pb][v][cb]);
                  } else {
                    const float du = lrelu_mask(ah, slope) * dm * s;
                    const float g3 = lrelu_mask(a3, slope) * (soft ? s * (ds - t[pb][v][cb]) : ds);
                    dU[e] = du;
                    G3[e] = g3;
                    u1[hp][cb] += du;
                    u2[hp][cb] = fmaf(du, (u - mu[hp][cb]) * is[hp][cb], u2[hp][cb]);
                    w1[cb] += g3;
                    w2[cb] = fmaf(g3, (z - mu3[cb]) * is3[cb], w2[cb]);
                  }
                }
              }
            }
        }
      }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float c3 = w1[cb], d3 = w2[cb];
      c3 += __shfl_xor(c3, 16); d3 += __shfl_xor(d3, 16);      // the four point groups, in a fixed order
      c3 += __shfl_xor(c3, 32); d3 += __shfl_xor(d3, 32);
      const int c = cw + cb * 16 + col;
      if (g == 0 && c < F1) {
        float* r3 = part3 + ((size_t)bx * F1 + c) * 2;
        r3[0] = c3; r3[1] = d3;
      }
#pragma unroll
      for (int hp = 0; hp < 2; ++hp) {
        float a = u1[hp][cb], b = u2[hp][cb];
        a += __shfl_xor(a, 16); b += __shfl_xor(b, 16);
        a += __shfl_xor(a, 32); b += __shfl_xor(b, 32);
        if (g == 0 && c < F1) {
          float* ru = partU + ((size_t)bx * 2 * F1 + (size_t)hp * F1 + c) * 2;
          ru[0] = a; ru[1] = b;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ the coordinate-guided layer's own passes
// One activated branch value of deform_edgeConv's weight input: both kernels below form it here, so that the a the backward multiplies
// with is the forward's, bit for bit.
struct Branch {
  const float* PQ; int ld; const float* sc; const float* sh; const float* mean; const float* invstd;
};
__device__ __forceinline__ float branch_a(float q, float p, float sc, float sh, float slope) { return lrelu_f(pre_act(q, p, sc, sh), slope); }

// one thread per (edge, V channels): W0 = a_a * a_b
template <int V>
__global__ __launch_bounds__(256) void edge_weight_gather2_kernel(Branch A, Branch B, const int32_t* __restrict__ idx, int M, int k, int F, float slope,
                                                                  float* __restrict__ W0) {
  const int QC = F / V;
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= (size_t)M * k * QC) return;
  const int c = (int)(tid % QC) * V;
  const size_t e = tid / QC;
  const int i = (int)(e / k), r = (int)(e % k);
  const int n = neighbour(idx, i, k, r, M);
  float pa[V], qa[V], pb[V], qb[V], sa[V], ta[V], sb[V], tb[V], w[V];
  ldv<V>(A.PQ + (size_t)n * A.ld + c, pa); ldv<V>(A.PQ + (size_t)i * A.ld + F + c, qa);
  ldv<V>(B.PQ + (size_t)n * B.ld + c, pb); ldv<V>(B.PQ + (size_t)i * B.ld + F + c, qb);
  ldv<V>(A.sc + c, sa); ldv<V>(A.sh + c, ta); ldv<V>(B.sc + c, sb); ldv<V>(B.sh + c, tb);
#pragma unroll
  for (int u = 0; u < V; ++u) w[u] = branch_a(qa[u], pa[u], sa[u], ta[u], slope) * branch_a(qb[u], pb[u], sb[u], tb[u], slope);
  stv<V>(W0 + e * F + c, w);
}

// A workgroup owns the ER_PT points of one record tile: np*k edge rows.  A thread keeps its V channels for the whole tile and walks the
// rows in ascending order (256 / QC rows per sweep), so its four sums per channel (sum GA, sum GA*zhat_a, sum GB, sum GB*zhat_b) have a
// fixed order; the threads of a channel are then combined in a fixed order: by xor shuffles inside a wave where the channel groups divide
// a wave, through LDS in ascending thread order otherwise.
template <int V>
__global__ __launch_bounds__(256) void edge_weight_split_kernel(const float* __restrict__ dW0, Branch A, Branch B, const int32_t* __restrict__ idx, int M,
                                                                int k, int F, float slope, float* __restrict__ GA, float* __restrict__ GB,
                                                                float* __restrict__ partA, float* __restrict__ partB) {
  __shared__ float sm[4 * V * 256];
  const int bx = xcd_block();
  const int p0 = bx * ER_PT;
  if (p0 >= M) return;
  const int ne = min(ER_PT, M - p0) * k;
  const size_t e0 = (size_t)p0 * k;
  const int QC = F / V;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int cb = 0; cb < QC; cb += 256) {
    const int nq = min(256, QC - cb);
    const int rows = 256 / nq;                       // edge rows per sweep; the threads past rows * nq idle
    const bool on = t < rows * nq;
    const bool pow2 = nq <= 64 && (nq & (nq - 1)) == 0;      // uniform
    const int c = (cb + t % nq) * V;
    float sa[V], ta[V], ma[V], ia[V], sb[V], tb[V], mb[V], ib[V], acc[4][V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[0][u] = acc[1][u] = acc[2][u] = acc[3][u] = 0.f;
    if (on) {
      ldv<V>(A.sc + c, sa); ldv<V>(A.sh + c, ta); ldv<V>(A.mean + c, ma); ldv<V>(A.invstd + c, ia);
      ldv<V>(B.sc + c, sb); ldv<V>(B.sh + c, tb); ldv<V>(B.mean + c, mb); ldv<V>(B.invstd + c, ib);
      for (int el = t / nq; el < ne; el += rows) {
        const int i = p0 + el / k;
        const int n = neighbour(idx, i, k, el % k, M);
        const size_t e = e0 + el;
        float d[V], pa[V], qa[V], pb[V], qb[V], ga[V], gb[V];
        ldv<V>(dW0 + e * F + c, d);
        ldv<V>(A.PQ + (size_t)n * A.ld + c, pa); ldv<V>(A.PQ + (size_t)i * A.ld + F + c, qa);
        ldv<V>(B.PQ + (size_t)n * B.ld + c, pb); ldv<V>(B.PQ + (size_t)i * B.ld + F + c, qb);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          const float aa = branch_a(qa[u], pa[u], sa[u], ta[u], slope), ab = branch_a(qb[u], pb[u], sb[u], tb[u], slope);
          ga[u] = lrelu_mask(pre_act(qa[u], pa[u], sa[u], ta[u]), slope) * d[u] * ab;
          gb[u] = lrelu_mask(pre_act(qb[u], pb[u], sb[u], tb[u]), slope) * d[u] * aa;
          acc[0][u] += ga[u];
          acc[1][u] = fmaf(ga[u], ((qa[u] + pa[u]) - ma[u]) * ia[u], acc[1][u]);
          acc[2][u] += gb[u];
          acc[3][u] = fmaf(gb[u], ((qb[u] + pb[u]) - mb[u]) * ib[u], acc[3][u]);
        }
        stv<V>(GA + e * F + c, ga);
        stv<V>(GB + e * F + c, gb);
      }
    }
    int slot = t, groups = rows;
    if (pow2) {                                      // every thread is on: the lanes of a channel group are lane, lane + nq, ...
      for (int off = nq; off < 64; off <<= 1)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int u = 0; u < V; ++u) acc[v][u] += __shfl_xor(acc[v][u], off);
      slot = lane < nq ? wave * nq + lane : -1;
      groups = 4;
    }
    __syncthreads();                                 // the previous channel block's records have been read
    if (slot >= 0)
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int u = 0; u < V; ++u) sm[(v * V + u) * 256 + slot] = on ? acc[v][u] : 0.f;
    __syncthreads();
    for (int o = t; o < nq * 4 * V; o += 256) {
      const int j = o % nq, vu = o / nq;
      float s = 0.f;
      for (int g = 0; g < groups; ++g) s += sm[vu * 256 + g * nq + j];
      const int v = vu / V, ch = (cb + j) * V + vu % V;
      ((v < 2 ? partA : partB) + ((size_t)bx * F + ch) * 2)[v & 1] = s;
    }
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool sizes_ok(int M, int k, int F1, int O) {
  return M > 0 && k >= 1 && k <= ER_KMAX && F1 > 0 && O > 0 && (long)M * k <= 0x7fffffffL && (long)k * F1 <= 0x7fffffffL;
}
inline bool mod_ok(const float* z3, const float* sc3, const float* sh3, const float* wmax, const float* wrs) {
  return z3 && sc3 && sh3 && ((wmax == nullptr) == (wrs == nullptr));
}
inline bool mod_al16(const WMod& m) { return al16(m.z3) && al16(m.sc3) && al16(m.sh3) && al16(m.wmax) && al16(m.wrs); }

// The [1,k] product and its weight gradient, plain (md == nullptr: spgan_edge_rank_*) or with the per-edge weight (spgan_edge_weight_*).
int launch_gemm(const float* PQ, int ld, const int32_t* idx, int M, int k, int F1, const float* scale1, const float* shift1, float slope,
                const float* W2i, int ldw, const float* b2, int O, float* Y, int ldy, float* partials, const WMod* md, hipStream_t st,
                bool stored = false) {
  const bool vec = F1 % 4 == 0 && ld % 4 == 0 && ldw % 4 == 0 && al16(PQ) && al16(W2i) && al16(scale1) && al16(shift1) && (!md || mod_al16(*md));
  const dim3 gr(grid8(cdiv(M, ER_PT))), b(256);
  auto go = [&](auto kernel, const WMod& m) {
    hipLaunchKernelGGL(kernel, gr, b, 0, st, PQ, ld, idx, M, k, F1, scale1, shift1, slope, W2i, ldw, b2, O, Y, ldy, partials, m);
  };
  if (stored && vec) go(edge_rank_gemm_kernel<true, true, true>, *md);
  else if (stored) go(edge_rank_gemm_kernel<false, true, true>, *md);
  else if (md && vec) go(edge_rank_gemm_kernel<true, true>, *md);
  else if (md) go(edge_rank_gemm_kernel<false, true>, *md);
  else if (vec) go(edge_rank_gemm_kernel<true, false>, WMod{});
  else go(edge_rank_gemm_kernel<false, false>, WMod{});
  return spgan_launch_status();
}

int launch_wgrad(const float* PQ, int ld, const int32_t* idx, int M, int k, int F1, const float* scale1, const float* shift1, float slope,
                 const float* dY, int ldg, int O, float* dW2i, int lddw, float* ws, const WMod* md, hipStream_t st, bool stored = false) {
  const RwPlan pl = er_wg_plan(M, k, F1, O);
  const bool vec = F1 % 4 == 0 && ld % 4 == 0 && al16(PQ) && al16(scale1) && al16(shift1) && (!md || mod_al16(*md));
  const dim3 gr(grid8((long)pl.tiles * pl.splits)), b(256);
  auto go = [&](auto kernel, const WMod& m) {
    hipLaunchKernelGGL(kernel, gr, b, 0, st, PQ, ld, idx, M, k, F1, scale1, shift1, slope, dY, ldg, O, ws, pl, m);
  };
  if (stored && vec) go(edge_rank_wgrad_kernel<true, true, true>, *md);
  else if (stored) go(edge_rank_wgrad_kernel<false, true, true>, *md);
  else if (md && vec) go(edge_rank_wgrad_kernel<true, true>, *md);
  else if (md) go(edge_rank_wgrad_kernel<false, true>, *md);
  else if (vec) go(edge_rank_wgrad_kernel<true, false>, WMod{});
  else go(edge_rank_wgrad_kernel<false, false>, WMod{});
  int e = spgan_launch_status();
  if (e) return e;
  hipLaunchKernelGGL(edge_rank_wgrad_reduce_kernel, dim3(cdiv((long)O * k * F1 * 8, 256)), dim3(256), 0, st, ws, pl.splits, O, k * F1, dW2i, lddw);
  return spgan_launch_status();
}

}  // namespace

extern "C" int spgan_edge_rank_tile_points(int k) {
  if (k < 1 || k > ER_KMAX) return 0;
  return ER_PT;
}

extern "C" int spgan_edge_rank_gemm(const float* PQ, int ld, const int32_t* idx, int M, int k, int F1, const float* scale1, const float* shift1,
                                    float slope, const float* W2i, int ldw, const float* b2, int O, float* Y, int ldy, float* partials,
                                    spgan_stream_t s_) {
  SPGAN_CHECK_ARG(PQ && idx && scale1 && shift1 && W2i && Y && sizes_ok(M, k, F1, O) && ld >= 2 * F1 && ldw >= k * F1 && ldy >= O);
  return launch_gemm(PQ, ld, idx, M, k, F1, scale1, shift1, slope, W2i, ldw, b2, O, Y, ldy, partials, nullptr, (hipStream_t)s_);
}

extern "C" size_t spgan_edge_rank_wgrad_ws_bytes(int M, int k, int F1, int O) {
  if (!sizes_ok(M, k, F1, O)) return 0;
  return (size_t)er_wg_plan(M, k, F1, O).splits * O * k * F1 * sizeof(float);
}

extern "C" int spgan_edge_rank_wgrad(const float* PQ, int ld, const int32_t* idx, int M, int k, int F1, const float* scale1, const float* shift1,
                                     float slope, const float* dY, int ldg, int O, float* dW2i, int lddw, float* ws, size_t ws_bytes,
                                     spgan_stream_t s_) {
  SPGAN_CHECK_ARG(PQ && idx && scale1 && shift1 && dY && dW2i && ws && sizes_ok(M, k, F1, O) && ld >= 2 * F1 && ldg >= O && lddw >= k * F1);
  SPGAN_CHECK_ARG(ws_bytes >= spgan_edge_rank_wgrad_ws_bytes(M, k, F1, O));
  return launch_wgrad(PQ, ld, idx, M, k, F1, scale1, shift1, slope, dY, ldg, O, dW2i, lddw, ws, nullptr, (hipStream_t)s_);
}

extern "C" int spgan_edge_rank_dgrad(const float* dY, int ldg, const float* W2t, int ldwt, const float* PQ, int ld, const int32_t* idx, int M, int k,
                                     int F1, int O, const float* scale1, const float* shift1, const float* mean1, const float* invstd1, float slope,
                                     float* dA, float* partials, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dY && W2t && PQ && idx && scale1 && shift1 && mean1 && invstd1 && dA && partials && sizes_ok(M, k, F1, O));
  SPGAN_CHECK_ARG(ldg >= O && ldwt >= O && ld >= 2 * F1);
  const bool vec = O % 4 == 0 && ldg % 4 == 0 && ldwt % 4 == 0 && al16(dY) && al16(W2t);
  const dim3 gr(grid8(cdiv(M, ER_PT))), b(256);
  hipStream_t st = (hipStream_t)s_;
  if (vec)
    hipLaunchKernelGGL(edge_rank_dgrad_kernel<true>, gr, b, 0, st, dY, ldg, W2t, ldwt, PQ, ld, idx, M, k, F1, O, scale1, shift1, mean1, invstd1, slope, dA,
                       partials);
  else
    hipLaunchKernelGGL(edge_rank_dgrad_kernel<false>, gr, b, 0, st, dY, ldg, W2t, ldwt, PQ, ld, idx, M, k, F1, O, scale1, shift1, mean1, invstd1, slope, dA,
                       partials);
  return spgan_launch_status();
}

extern "C" int spgan_edge_rank_scatter(const float* dA, const int32_t* rowptr, const int32_t* src, const float* PQ, int ld, const int32_t* idx, int M,
                                       int k, int F1, const float* scale1, const float* mean1, const float* invstd1, const float* sums, float* dPQ,
                                       int ldd, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dA && rowptr && src && scale1 && dPQ && sizes_ok(M, k, F1, 1) && ldd >= 2 * F1);
  if (sums) SPGAN_CHECK_ARG(PQ && idx && mean1 && invstd1 && ld >= 2 * F1);
  const float inv_e = 1.0f / ((float)M * (float)k);
  const bool v4 = F1 % 4 == 0 && ldd % 4 == 0 && al16(dA) && al16(dPQ) && al16(scale1) &&
                  (!sums || (ld % 4 == 0 && al16(PQ) && al16(mean1) && al16(invstd1) && al16(sums)));
  const long items = (long)M * (v4 ? F1 / 4 : F1);
  hipStream_t st = (hipStream_t)s_;
  if (v4)
    hipLaunchKernelGGL(edge_rank_scatter_kernel<4>, dim3(cdiv(items, 256)), dim3(256), 0, st, dA, rowptr, src, PQ, ld, idx, M, k, F1, scale1, mean1,
                       invstd1, sums, inv_e, dPQ, ldd);
  else
    hipLaunchKernelGGL(edge_rank_scatter_kernel<1>, dim3(cdiv(items, 256)), dim3(256), 0, st, dA, rowptr, src, PQ, ld, idx, M, k, F1, scale1, mean1,
                       invstd1, sums, inv_e, dPQ, ldd);
  return spgan_launch_status();
}

// ------------------------------------------------------------------------------------------ the weighted layer (deform_edgeConv_feat)
extern "C" int spgan_edge_weight_gather(const float* PQ, int ld, const int32_t* idx, int M, int k, int F, float* Z, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(PQ && idx && Z && sizes_ok(M, k, F, 1) && ld >= 2 * F && (long)M * k * F <= 0x7fffffffL * 256L);
  hipLaunchKernelGGL(edge_weight_gather_kernel, dim3(cdiv((long)M * k * F, 256)), dim3(256), 0, (hipStream_t)s_, PQ, ld, idx, M, k, F, Z);
  return spgan_launch_status();
}

extern "C" int spgan_edge_weight_norm(const float* z3, int M, int k, int F1, const float* scale3, const float* shift3, float slope, float* wmax,
                                      float* wrs, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(z3 && scale3 && shift3 && wmax && wrs && sizes_ok(M, k, F1, 1) && (long)M * F1 <= 0x7fffffffL * 256L);
  hipLaunchKernelGGL(edge_weight_norm_kernel, dim3(cdiv((long)M * F1, 256)), dim3(256), 0, (hipStream_t)s_, z3, M, k, F1, scale3, shift3, slope, wmax,
                     wrs);
  return spgan_launch_status();
}

extern "C" int spgan_edge_weight_gemm(const float* PQ, int ld, const int32_t* idx, int M, int k, int F1, const float* scale1, const float* shift1,
                                      float slope, const float* z3, const float* scale3, const float* shift3, const float* wmax, const float* wrs,
                                      const float* W2i, int ldw, const float* b2, int O, float* Y, int ldy, float* partials, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(PQ && idx && scale1 && shift1 && W2i && Y && sizes_ok(M, k, F1, O) && ld >= 2 * F1 && ldw >= k * F1 && ldy >= O);
  SPGAN_CHECK_ARG(mod_ok(z3, scale3, shift3, wmax, wrs));
  const WMod md{z3, scale3, shift3, wmax, wrs};
  return launch_gemm(PQ, ld, idx, M, k, F1, scale1, shift1, slope, W2i, ldw, b2, O, Y, ldy, partials, &md, (hipStream_t)s_);
}

extern "C" int spgan_edge_weight_wgrad(const float* PQ, int ld, const int32_t* idx, int M, int k, int F1, const float* scale1, const float* shift1,
                                       float slope, const float* z3, const float* scale3, const float* shift3, const float* wmax, const float* wrs,
                                       const float* dY, int ldg, int O, float* dW2i, int lddw, float* ws, size_t ws_bytes, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(PQ && idx && scale1 && shift1 && dY && dW2i && ws && sizes_ok(M, k, F1, O) && ld >= 2 * F1 && ldg >= O && lddw >= k * F1);
  SPGAN_CHECK_ARG(mod_ok(z3, scale3, shift3, wmax, wrs) && ws_bytes >= spgan_edge_rank_wgrad_ws_bytes(M, k, F1, O));
  const WMod md{z3, scale3, shift3, wmax, wrs};
  return launch_wgrad(PQ, ld, idx, M, k, F1, scale1, shift1, slope, dY, ldg, O, dW2i, lddw, ws, &md, (hipStream_t)s_);
}

extern "C" int spgan_edge_weight_dgrad(const float* dY, int ldg, const float* W2t, int ldwt, const float* PQ, int ld, const int32_t* idx, int M, int k,
                                       int F1, int O, const float* scale1, const float* shift1, const float* mean1, const float* invstd1, float slope,
                                       const float* z3, const float* scale3, const float* shift3, const float* mean3, const float* invstd3,
                                       const float* wmax, const float* wrs, float* dU, float* G3, float* partials_u, float* partials_3,
                                       spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dY && W2t && PQ && idx && scale1 && shift1 && mean1 && invstd1 && sizes_ok(M, k, F1, O));
  SPGAN_CHECK_ARG(mod_ok(z3, scale3, shift3, wmax, wrs) && mean3 && invstd3 && dU && G3 && dU != G3 && partials_u && partials_3);
  SPGAN_CHECK_ARG(ldg >= O && ldwt >= O && ld >= 2 * F1);
  const WMod md{z3, scale3, shift3, wmax, wrs};
  const bool vec = O % 4 == 0 && ldg % 4 == 0 && ldwt % 4 == 0 && al16(dY) && al16(W2t);
  const dim3 gr(grid8(cdiv(M, ER_PT))), b(256);
  hipStream_t st = (hipStream_t)s_;
  if (vec)
    hipLaunchKernelGGL(edge_weight_dgrad_kernel<true>, gr, b, 0, st, dY, ldg, W2t, ldwt, PQ, ld, idx, M, k, F1, O, scale1, shift1, mean1, invstd1, slope, md,
                       mean3, invstd3, dU, G3, partials_u, partials_3);
  else
    hipLaunchKernelGGL(edge_weight_dgrad_kernel<false>, gr, b, 0, st, dY, ldg, W2t, ldwt, PQ, ld, idx, M, k, F1, O, scale1, shift1, mean1, invstd1, slope, md,
                       mean3, invstd3, dU, G3, partials_u, partials_3);
  return spgan_launch_status();
}

// ------------------------------------------------------------------------------------------ the coordinate-guided layer (deform_edgeConv)
extern "C" int spgan_edge_weight_gather2(const float* PQa, int lda, const float* PQb, int ldb, const int32_t* idx, int M, int k, int F,
                                         const float* scale_a, const float* shift_a, const float* scale_b, const float* shift_b, float slope,
                                         float* W0, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(PQa && PQb && idx && scale_a && shift_a && scale_b && shift_b && W0 && sizes_ok(M, k, F, 1) && lda >= 2 * F && ldb >= 2 * F);
  SPGAN_CHECK_ARG((long)M * k * F <= 0x7fffffffL * 256L);
  const Branch A{PQa, lda, scale_a, shift_a, nullptr, nullptr}, B{PQb, ldb, scale_b, shift_b, nullptr, nullptr};
  const bool v4 = F % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && al16(PQa) && al16(PQb) && al16(scale_a) && al16(shift_a) && al16(scale_b) &&
                  al16(shift_b) && al16(W0);
  const long items = (long)M * k * (v4 ? F / 4 : F);
  if (v4) hipLaunchKernelGGL(edge_weight_gather2_kernel<4>, dim3(cdiv(items, 256)), dim3(256), 0, (hipStream_t)s_, A, B, idx, M, k, F, slope, W0);
  else hipLaunchKernelGGL(edge_weight_gather2_kernel<1>, dim3(cdiv(items, 256)), dim3(256), 0, (hipStream_t)s_, A, B, idx, M, k, F, slope, W0);
  return spgan_launch_status();
}

extern "C" int spgan_edge_weight_split(const float* dW0, const float* PQa, int lda, const float* PQb, int ldb, const int32_t* idx, int M, int k, int F,
                                       const float* scale_a, const float* shift_a, const float* mean_a, const float* invstd_a, const float* scale_b,
                                       const float* shift_b, const float* mean_b, const float* invstd_b, float slope, float* GA, float* GB,
                                       float* partials_a, float* partials_b, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dW0 && PQa && PQb && idx && scale_a && shift_a && mean_a && invstd_a && scale_b && shift_b && mean_b && invstd_b);
  SPGAN_CHECK_ARG(GA && GB && GA != GB && partials_a && partials_b && partials_a != partials_b && sizes_ok(M, k, F, 1) && lda >= 2 * F && ldb >= 2 * F);
  const Branch A{PQa, lda, scale_a, shift_a, mean_a, invstd_a}, B{PQb, ldb, scale_b, shift_b, mean_b, invstd_b};
  const bool v4 = F % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && al16(dW0) && al16(PQa) && al16(PQb) && al16(GA) && al16(GB) && al16(scale_a) &&
                  al16(shift_a) && al16(mean_a) && al16(invstd_a) && al16(scale_b) && al16(shift_b) && al16(mean_b) && al16(invstd_b);
  const dim3 gr(grid8(cdiv(M, ER_PT))), b(256);
  if (v4) hipLaunchKernelGGL(edge_weight_split_kernel<4>, gr, b, 0, (hipStream_t)s_, dW0, A, B, idx, M, k, F, slope, GA, GB, partials_a, partials_b);
  else hipLaunchKernelGGL(edge_weight_split_kernel<1>, gr, b, 0, (hipStream_t)s_, dW0, A, B, idx, M, k, F, slope, GA, GB, partials_a, partials_b);
  return spgan_launch_status();
}

// ------------------------------------------------------------------------------------------ the bilateral layer (bilateral_upsample_edgeConv)
namespace {
inline bool stored_ok(int M, int k, int F1, int O) { return sizes_ok(M, k, F1, O) && k >= 2 && k <= 28 && k % 2 == 0; }
}  // namespace

extern "C" int spgan_edge_stored_gemm(const float* U, int M, int k, int F1, const float* scale1, const float* shift1, float slope, const float* z3,
                                      const float* scale3, const float* shift3, const float* wmax, const float* wrs, const float* W2i, int ldw,
                                      const float* b2, int O, float* Y, int ldy, float* partials, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(U && scale1 && shift1 && W2i && Y && stored_ok(M, k, F1, O) && ldw >= k * F1 && ldy >= O);
  SPGAN_CHECK_ARG(mod_ok(z3, scale3, shift3, wmax, wrs));
  const WMod md{z3, scale3, shift3, wmax, wrs};
  return launch_gemm(U, F1, nullptr, M, k, F1, scale1, shift1, slope, W2i, ldw, b2, O, Y, ldy, partials, &md, (hipStream_t)s_, true);
}

extern "C" int spgan_edge_stored_wgrad(const float* U, int M, int k, int F1, const float* scale1, const float* shift1, float slope, const float* z3,
                                       const float* scale3, const float* shift3, const float* wmax, const float* wrs, const float* dY, int ldg,
                                       int O, float* dW2i, int lddw, float* ws, size_t ws_bytes, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(U && scale1 && shift1 && dY && dW2i && ws && stored_ok(M, k, F1, O) && ldg >= O && lddw >= k * F1);
  SPGAN_CHECK_ARG(mod_ok(z3, scale3, shift3, wmax, wrs) && ws_bytes >= spgan_edge_rank_wgrad_ws_bytes(M, k, F1, O));
  const WMod md{z3, scale3, shift3, wmax, wrs};
  return launch_wgrad(U, F1, nullptr, M, k, F1, scale1, shift1, slope, dY, ldg, O, dW2i, lddw, ws, &md, (hipStream_t)s_, true);
}

extern "C" int spgan_edge_stored_dgrad(const float* dY, int ldg, const float* W2t, int ldwt, const float* U, int M, int k, int F1, int O,
                                       const float* scale1, const float* shift1, const float* mean1, const float* invstd1, float slope,
                                       const float* z3, const float* scale3, const float* shift3, const float* mean3, const float* invstd3,
                                       const float* wmax, const float* wrs, float* dU, float* G3, float* partials_u, float* partials_3,
                                       spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dY && W2t && U && scale1 && shift1 && mean1 && invstd1 && stored_ok(M, k, F1, O));
  SPGAN_CHECK_ARG(mod_ok(z3, scale3, shift3, wmax, wrs) && mean3 && invstd3 && dU && G3 && dU != G3 && dU != U && G3 != U && partials_u && partials_3 &&
                  partials_u != partials_3);
  SPGAN_CHECK_ARG(ldg >= O && ldwt >= O);
  const WMod md{z3, scale3, shift3, wmax, wrs};
  const bool vec = O % 4 == 0 && ldg % 4 == 0 && ldwt % 4 == 0 && al16(dY) && al16(W2t);
  const dim3 gr(grid8(cdiv(M, ER_PT))), b(256);
  hipStream_t st = (hipStream_t)s_;
  if (vec)
    hipLaunchKernelGGL(edge_stored_dgrad_kernel<true>, gr, b, 0, st, dY, ldg, W2t, ldwt, U, M, k, F1, O, scale1, shift1, mean1, invstd1, slope, md, mean3,
                       invstd3, dU, G3, partials_u, partials_3);
  else
    hipLaunchKernelGGL(edge_stored_dgrad_kernel<false>, gr, b, 0, st, dY, ldg, W2t, ldwt, U, M, k, F1, O, scale1, shift1, mean1, invstd1, slope, md, mean3,
                       invstd3, dU, G3, partials_u, partials_3);
  return spgan_launch_status();
}
