// Rank-window edge convolution: the two [1,w] Conv2d layers of the reference's upsample_edgeConv (Generation/modules.py:799-845) as
// products over gathered neighbour rows, without an edge tensor as operand.
//
// With d(i,j) = x_n(i,j) - x_i (j = rank of the neighbour, idx [M,k] global rows) a Conv2d(2C -> O, [1,w]) over get_edge_features(x)
// gives, for the T = k - w + 1 window positions t of point i,
//     u(i,t,:) = Q_i + sum_{r<w} Wd_r d(i,t+r),        Q = (sum_r Wc_r) x + b   (a per-point GEMM, done by spgan_gemm_nt),
// i.e. a GEMM whose A row (i,t) is [d(i,t) | ... | d(i,t+w-1)] (K = w*C): T overlapping slices of the same k gathered rows.
//   spgan_edge_window_gemm    a workgroup stages the k difference rows of its points once per channel chunk in LDS (the centre row is
//                             subtracted while staging: the reference's rounding) and feeds the windows to v_mfma_f32_16x16x4_f32 as
//                             address slices of that staging; output rows (i,t) = [M*T, O] row-major; epilogue: per-point row add,
//                             a second addend of the output's shape, and (sum, centred M2) column records (spgan_colstats_finalize_bn).
//                             (w,T) = (k/2+1, k/2) is inte_conv_hk, (k,1) the first k taps of conv2.
//   spgan_edge_window_wgrad   dW[o, r*C+c] = sum_{i,t} g(i,t,o) d(i,t+r,c): same staging, reduction over the rows, split over point ranges
//                             into a workspace that is summed in split order (no float atomics).
//   spgan_edge_window_dgrad   S(i,j,:) = sum_{t+r=j} g(i,t,:) Wd_r  [M,k,C]: a plain MFMA product per rank j over the valid (t,r) pairs,
//                             both operands straight from global memory / L2 (Wt = the transposed weight image [w*C, O]).
//   spgan_edge_window_scatter dx_i = addends - sum_j S(i,j) + sum_{(i',j)->i} S(i',j) over the in-edge lists of spgan_csr_build in
//                             ascending edge order.
//
// MFMA operand order: a 16-wide K block is held as one 16-byte fragment per lane (lane group g = lane>>4 holds K elements 4g..4g+3) and
// consumed by four MFMA steps (step s takes element s of every group): A and B agree on that order, and every fragment is one
// ds_read_b128 / global_load_dwordx4.  Workgroups are dealt per XCD as in edge.hip, so a shape's gathered rows stay in one L2.
#include "common.hpp"

namespace {

constexpr int EW_KMAX = 28;             // k (padded) ranks x 16 channels of 32 points must fit 64 KB of LDS
constexpr int EW_LDS = 65536;

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

// LDS layout of the forward staging: point p, rank j, channel cc of the chunk at p*pstride + j*CK + cc.  pstride = 4 (mod 32) floats: the
// 16 points of a fragment read spread over all banks.
inline int ew_pstride(int k, int CK) {
  int ps = k * CK;
  while (ps % 32 != 4) ps += 4;
  return ps;
}
// channel chunk: the widest of 64 / 32 / 16 that C needs and PT points fit in LDS with; 0: none fits
inline int ew_chunk(int PT, int k, int C) {
  for (int CK = 64; CK >= 16; CK >>= 1) {
    if (CK >= 32 && CK / 2 >= C) continue;
    if ((long)PT * ew_pstride(k, CK) * 4 <= EW_LDS) return CK;
  }
  return 0;
}
// points per workgroup (= rows of a statistics record / T)
inline int ew_tile_points(int k, int T) {
  if (T > 1) return 32;
  return ew_chunk(64, k, 16) ? 64 : 32;
}

// ------------------------------------------------------------------------------------------ forward
// TB window positions x PB blocks of 16 points x 2 blocks of 16 output columns per wave; the four waves of a workgroup take 128
// consecutive output columns per pass.  T > TB runs several passes over t, each with its own accumulators.
template <int TB, int PB, bool VEC>
__global__ __launch_bounds__(256, 2) void edge_window_gemm_kernel(const float* __restrict__ x, int ldx, const int32_t* __restrict__ idx, int M, int k,
                                                               int C, const float* __restrict__ W, int ldw, int O, int w, int T,
                                                               const float* __restrict__ rowadd, int ldr, const float* __restrict__ add2,
                                                               int lda2, float* __restrict__ Y, int ldy, float* __restrict__ part, int CK,
                                                               int pstride) {
  extern __shared__ float sm[];
  constexpr int PT = PB * 16;
  const int bx = xcd_block();
  const int p0 = bx * PT;
  if (p0 >= M) return;
  const int np = min(PT, M - p0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  const float cnt = (float)np * (float)T;
  for (int ob = 0; ob < O; ob += 128) {
    const int oc0 = ob + wave * 32;
    const bool wave_on = oc0 < O;                 // uniform per wave; idle waves still stage and meet the barriers
    float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f}, y0[2] = {0.f, 0.f};
    for (int t0 = 0; t0 < T; t0 += TB) {
      f32x4 acc[PB][TB][2];
#pragma unroll
      for (int pb = 0; pb < PB; ++pb)
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) acc[pb][tb][0] = acc[pb][tb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int c0 = 0; c0 < C; c0 += CK) {
        __syncthreads();
        if constexpr (VEC) {
          const int q4 = CK >> 2, items = PT * k * q4;
          for (int e = threadIdx.x; e < items; e += 256) {
            const int cc = (e % q4) * 4, pj = e / q4, j = pj % k, p = pj / k;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (p < np && c0 + cc < C) {
              const int i = p0 + p;
              int n = idx[(size_t)i * k + j];
              if ((unsigned)n >= (unsigned)M) n = i;
              const f32x4 xn = *reinterpret_cast<const f32x4*>(x + (size_t)n * ldx + c0 + cc);
              const f32x4 xi = *reinterpret_cast<const f32x4*>(x + (size_t)i * ldx + c0 + cc);
              v = xn - xi;
            }
            *reinterpret_cast<f32x4*>(sm + p * pstride + j * CK + cc) = v;
          }
        } else {
          const int items = PT * k * CK;
          for (int e = threadIdx.x; e < items; e += 256) {
            const int cc = e % CK, pj = e / CK, j = pj % k, p = pj / k;
            float v = 0.f;
            if (p < np && c0 + cc < C) {
              const int i = p0 + p;
              int n = idx[(size_t)i * k + j];
              if ((unsigned)n >= (unsigned)M) n = i;
              v = x[(size_t)n * ldx + c0 + cc] - x[(size_t)i * ldx + c0 + cc];
            }
            sm[p * pstride + j * CK + cc] = v;
          }
        }
        __syncthreads();
        if (!wave_on) continue;
        const int nkb = (min(CK, C - c0) + 15) >> 4;
        for (int r = 0; r < w; ++r) {
          for (int kb = 0; kb < nkb; ++kb) {
            const int cc = kb * 16 + 4 * g;
            f32x4 b[2];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
              const int o = oc0 + cb * 16 + col;
              b[cb] = ld4<VEC>(W + (size_t)min(o, O - 1) * ldw + (size_t)r * C + c0 + cc, o < O ? C - (c0 + cc) : 0);
            }
#pragma unroll
            for (int pb = 0; pb < PB; ++pb)
#pragma unroll
              for (int tb = 0; tb < TB; ++tb) {
                if (t0 + tb < T) {
                  const f32x4 a = *reinterpret_cast<const f32x4*>(sm + (pb * 16 + col) * pstride + (t0 + tb + r) * CK + cc);
                  acc[pb][tb][0] = mfma4(a, b[0], acc[pb][tb][0]);
                  acc[pb][tb][1] = mfma4(a, b[1], acc[pb][tb][1]);
                }
              }
          }
        }
      }
      if (!wave_on) continue;
      // epilogue of this pass: the D fragment of a lane is rows (points) 4g..4g+3 of column col
#pragma unroll
      for (int pb = 0; pb < PB; ++pb)
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) {
          const int t = t0 + tb;
          if (t < T) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
              const int o = oc0 + cb * 16 + col;
#pragma unroll
              for (int v = 0; v < 4; ++v) {
                const int p = pb * 16 + 4 * g + v;
                const bool ok = p < np && o < O;
                const size_t i = (size_t)(p0 + p);
                float val = acc[pb][tb][cb][v];
                if (ok) {
                  if (rowadd) val += rowadd[i * ldr + o];
                  if (add2) val += add2[(i * T + t) * lda2 + o];
                  Y[(i * T + t) * ldy + o] = val;
                }
                if (part) {          // a kernel argument: uniform
                  // shifted sums around the tile's first row of the column (point p0, t = 0: lane `col`, element 0 of the first fragment)
                  if (pb == 0 && tb == 0 && v == 0 && t0 == 0) y0[cb] = __shfl(val, col);
                  if (ok) {
                    const float d = val - y0[cb];
                    s1[cb] += d;
                    s2[cb] = fmaf(d, d, s2[cb]);
                  }
                }
              }
            }
          }
        }
    }
    if (part && wave_on) {
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        float a = s1[cb], b = s2[cb];
        a += __shfl_xor(a, 16); b += __shfl_xor(b, 16);       // the four point groups of a column, in a fixed order
        a += __shfl_xor(a, 32); b += __shfl_xor(b, 32);
        const int o = oc0 + cb * 16 + col;
        if (g == 0 && o < O) {
          float* rec = part + ((size_t)bx * O + o) * 2;
          rec[0] = fmaf(cnt, y0[cb], a);
          rec[1] = fmaxf(b - a * a / cnt, 0.f);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ input side of the backward: slot gradients
// A[p][o] = g(p,t,o), B[o][c] = Wt[(r*C + c), o], D[p][c]: 32 points x 128 channels per workgroup pass, no LDS.
template <bool VEC>
__global__ __launch_bounds__(256) void edge_window_dgrad_kernel(const float* __restrict__ G, int ldg, const float* __restrict__ Wt, int ldwt, int M,
                                                                int k, int C, int O, int w, int T, float* __restrict__ S, int accumulate) {
  const int bx = xcd_block();
  const int p0 = bx * 32;
  if (p0 >= M) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  for (int cp = 0; cp < C; cp += 128) {
    const int cw = cp + wave * 32;
    if (cw >= C) continue;
    for (int j = 0; j < k; ++j) {
      f32x4 acc[2][2];
      acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int tlo = max(0, j - w + 1), thi = min(T - 1, j);
      for (int t = tlo; t <= thi; ++t) {
        const int r = j - t;
        for (int ob = 0; ob < O; ob += 16) {
          const int o = ob + 4 * g;
          f32x4 a[2], b[2];
#pragma unroll
          for (int pb = 0; pb < 2; ++pb) {
            const int p = p0 + pb * 16 + col;
            a[pb] = ld4<VEC>(G + ((size_t)min(p, M - 1) * T + t) * ldg + o, p < M ? O - o : 0);
          }
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            const int c = cw + cb * 16 + col;
            b[cb] = ld4<VEC>(Wt + ((size_t)r * C + min(c, C - 1)) * ldwt + o, c < C ? O - o : 0);
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
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int p = p0 + pb * 16 + 4 * g + v, c = cw + cb * 16 + col;
            if (p < M && c < C) {
              float* d = S + ((size_t)p * k + j) * C + c;
              *d = accumulate ? *d + acc[pb][cb][v] : acc[pb][cb][v];
            }
          }
    }
  }
}

// ------------------------------------------------------------------------------------------ weight gradient
// D[o][c] (one per tap r) += A[o][row] B[row][c]: A = g (global), B = the staged differences; an MFMA step reduces over four
// consecutive points at one window position.  A workgroup owns 128 output channels x 16 input channels x up to RB taps of one point
// range; logical blocks of one range are neighbours, so its gathered rows are fetched into one L2.
constexpr int EW_RB = 6;
inline int ew_wg_pstride(int k) {
  int u = k;
  while (u % 4 != 1) ++u;        // 16 (mod 64) floats between the four points of a fragment
  return u * 16;
}
struct WgPlan {
  int n_ot, n_ct, n_rp, tiles, splits, pps;
};
inline WgPlan ew_wg_plan(int M, int C, int O, int w) {
  WgPlan p;
  p.n_ot = cdiv(O, 128); p.n_ct = cdiv(C, 16); p.n_rp = cdiv(w, EW_RB);
  p.tiles = p.n_ot * p.n_ct * p.n_rp;
  // about 1024 workgroups: a narrow layer (Fin = 3: one tile) is split over up to 512 point ranges, a wide one (32 tiles) over 32
  int s = cdiv(1024, p.tiles);
  s = s < 1 ? 1 : (s > 512 ? 512 : s);
  p.pps = cdiv(cdiv(M, s), 32) * 32;
  p.splits = cdiv(M, p.pps);
  return p;
}

__global__ __launch_bounds__(256) void edge_window_wgrad_kernel(const float* __restrict__ x, int ldx, const int32_t* __restrict__ idx, int M, int k,
                                                                int C, const float* __restrict__ G, int ldg, int O, int w, int T,
                                                                float* __restrict__ ws, WgPlan pl, int pst) {
  extern __shared__ float sm[];
  const int L = xcd_block();
  if (L >= pl.tiles * pl.splits) return;
  const int s = L / pl.tiles, tile = L % pl.tiles;
  const int ot = tile % pl.n_ot, ct = (tile / pl.n_ot) % pl.n_ct, rp = tile / (pl.n_ot * pl.n_ct);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int c0 = ct * 16, r0 = rp * EW_RB, o0 = ot * 128 + wave * 32;
  const int begin = s * pl.pps, end = min(M, begin + pl.pps);
  f32x4 acc[2][EW_RB];
#pragma unroll
  for (int rb = 0; rb < EW_RB; ++rb) acc[0][rb] = acc[1][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int pb = begin; pb < end; pb += 32) {
    __syncthreads();
    for (int e = threadIdx.x; e < 32 * k * 16; e += 256) {
      const int cc = e & 15, pj = e >> 4, j = pj % k, p = pj / k;
      const int i = pb + p;
      float v = 0.f;
      if (i < end && c0 + cc < C) {
        int n = idx[(size_t)i * k + j];
        if ((unsigned)n >= (unsigned)M) n = i;
        v = x[(size_t)n * ldx + c0 + cc] - x[(size_t)i * ldx + c0 + cc];
      }
      sm[p * pst + j * 16 + cc] = v;
    }
    __syncthreads();
    if (o0 >= O) continue;
    for (int q = 0; q < 8; ++q) {
      const int pt = q * 4 + g;
      const int i = pb + pt;
      if (pb + q * 4 >= end) break;                    // uniform
      for (int t = 0; t < T; ++t) {
        float a[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int o = o0 + h * 16 + col;
          a[h] = (i < end && o < O) ? G[((size_t)i * T + t) * ldg + o] : 0.f;
        }
#pragma unroll
        for (int rb = 0; rb < EW_RB; ++rb) {
          if (r0 + rb < w) {
            const float b = sm[pt * pst + (t + r0 + rb) * 16 + col];
            acc[0][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b, acc[0][rb], 0, 0, 0);
            acc[1][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b, acc[1][rb], 0, 0, 0);
          }
        }
      }
    }
  }
  const size_t ldw = (size_t)w * C;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int rb = 0; rb < EW_RB; ++rb)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int o = o0 + h * 16 + 4 * g + v, c = c0 + col;
        if (r0 + rb < w && o < O && c < C) ws[((size_t)s * O + o) * ldw + (size_t)(r0 + rb) * C + c] = acc[h][rb][v];
      }
}

// dW[o, e] = sum_s ws[s][o][e]: eight lanes per element take the splits s = q, q + 8, ... in ascending order and their partial sums are
// combined in a fixed order (a fixed assignment: run-to-run identical, no float atomics)
__global__ __launch_bounds__(256) void edge_window_wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int O, int KW, float* __restrict__ dW,
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

// ------------------------------------------------------------------------------------------ slot gradients -> point gradients
template <int V>
__global__ __launch_bounds__(256) void edge_window_scatter_kernel(const float* __restrict__ S, const int32_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ src, int M, int k, int C,
                                                                  const float* __restrict__ add_a, int lda, const float* __restrict__ add_b, int ldb,
                                                                  float* __restrict__ dx, int lddx) {
  const int QC = C / V;
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= (size_t)M * QC) return;
  const int m = (int)(tid / QC), c = (int)(tid % QC) * V;
  float own[V], in[V], out[V];
#pragma unroll
  for (int u = 0; u < V; ++u) own[u] = in[u] = 0.f;
  for (int j = 0; j < k; ++j) {
    const float* p = S + ((size_t)m * k + j) * C + c;
    if constexpr (V == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p);
      own[0] += v.x; own[1] += v.y; own[2] += v.z; own[3] += v.w;
    } else {
      own[0] += p[0];
    }
  }
  const int t0 = rowptr[m], t1 = rowptr[m + 1];
  for (int t = t0; t < t1; ++t) {            // ascending edge ids: a fixed summation order
    const float* p = S + (size_t)src[t] * C + c;
    if constexpr (V == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p);
      in[0] += v.x; in[1] += v.y; in[2] += v.z; in[3] += v.w;
    } else {
      in[0] += p[0];
    }
  }
#pragma unroll
  for (int u = 0; u < V; ++u) {
    float a = in[u] - own[u];
    if (add_a) a += add_a[(size_t)m * lda + c + u];
    if (add_b) a += add_b[(size_t)m * ldb + c + u];
    out[u] = a;
  }
  float* d = dx + (size_t)m * lddx + c;
  if constexpr (V == 4) *reinterpret_cast<f32x4*>(d) = f32x4{out[0], out[1], out[2], out[3]};
  else d[0] = out[0];
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool sizes_ok(int M, int k, int C, int O, int w) {
  return M > 0 && k >= 1 && k <= EW_KMAX && w >= 1 && w <= k && C > 0 && O > 0 && (long)M * k <= 0x7fffffffL && (long)w * C <= 0x7fffffffL;
}

template <int TB, int PB>
int launch_gemm(bool vec, int CK, const float* x, int ldx, const int32_t* idx, int M, int k, int C, const float* W, int ldw, int O, int w, int T,
                const float* rowadd, int ldr, const float* add2, int lda2, float* Y, int ldy, float* part, hipStream_t st) {
  constexpr int PT = PB * 16;
  const int ps = ew_pstride(k, CK);
  const size_t lds = (size_t)PT * ps * sizeof(float);
  const dim3 gr(grid8(cdiv(M, PT))), b(256);
  if (vec)
    hipLaunchKernelGGL((edge_window_gemm_kernel<TB, PB, true>), gr, b, lds, st, x, ldx, idx, M, k, C, W, ldw, O, w, T, rowadd, ldr, add2, lda2, Y, ldy,
                       part, CK, ps);
  else
    hipLaunchKernelGGL((edge_window_gemm_kernel<TB, PB, false>), gr, b, lds, st, x, ldx, idx, M, k, C, W, ldw, O, w, T, rowadd, ldr, add2, lda2, Y, ldy,
                       part, CK, ps);
  return spgan_launch_status();
}

}  // namespace

extern "C" int spgan_edge_window_tile_points(int k, int T) {
  if (k < 1 || k > EW_KMAX || T < 1 || T > k) return 0;
  return ew_tile_points(k, T);
}

extern "C" int spgan_edge_window_gemm(const float* x, int ldx, const int32_t* idx, int M, int k, int C, const float* W, int ldw, int O, int w,
                                      const float* rowadd, int ld_rowadd, const float* add2, int ld_add2, float* Y, int ldy, float* partials,
                                      spgan_stream_t s_) {
  SPGAN_CHECK_ARG(x && idx && W && Y && sizes_ok(M, k, C, O, w) && ldx >= C && ldw >= w * C && ldy >= O);
  SPGAN_CHECK_ARG((!rowadd || ld_rowadd >= O) && (!add2 || ld_add2 >= O));
  const int T = k - w + 1;
  SPGAN_CHECK_ARG((long)M * T <= 0x7fffffffL);
  const int PT = ew_tile_points(k, T);
  const int CK = ew_chunk(PT, k, C);
  SPGAN_CHECK_ARG(CK > 0);
  const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldw % 4 == 0 && al16(x) && al16(W);
  hipStream_t st = (hipStream_t)s_;
  if (T > 1) return launch_gemm<5, 2>(vec, CK, x, ldx, idx, M, k, C, W, ldw, O, w, T, rowadd, ld_rowadd, add2, ld_add2, Y, ldy, partials, st);
  if (PT == 64) return launch_gemm<1, 4>(vec, CK, x, ldx, idx, M, k, C, W, ldw, O, w, T, rowadd, ld_rowadd, add2, ld_add2, Y, ldy, partials, st);
  return launch_gemm<1, 2>(vec, CK, x, ldx, idx, M, k, C, W, ldw, O, w, T, rowadd, ld_rowadd, add2, ld_add2, Y, ldy, partials, st);
}

extern "C" size_t spgan_edge_window_wgrad_ws_bytes(int M, int k, int C, int O, int w) {
  if (!sizes_ok(M, k, C, O, w)) return 0;
  return (size_t)ew_wg_plan(M, C, O, w).splits * O * w * C * sizeof(float);
}

extern "C" int spgan_edge_window_wgrad(const float* x, int ldx, const int32_t* idx, int M, int k, int C, const float* G, int ldg, int O, int w,
                                       float* dW, int lddw, float* ws, size_t ws_bytes, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(x && idx && G && dW && ws && sizes_ok(M, k, C, O, w) && ldx >= C && ldg >= O && lddw >= w * C);
  const int T = k - w + 1;
  SPGAN_CHECK_ARG((long)M * T <= 0x7fffffffL && ws_bytes >= spgan_edge_window_wgrad_ws_bytes(M, k, C, O, w));
  const WgPlan pl = ew_wg_plan(M, C, O, w);
  const int pst = ew_wg_pstride(k);
  hipStream_t st = (hipStream_t)s_;
  hipLaunchKernelGGL(edge_window_wgrad_kernel, dim3(grid8((long)pl.tiles * pl.splits)), dim3(256), (size_t)32 * pst * sizeof(float), st, x, ldx, idx, M,
                     k, C, G, ldg, O, w, T, ws, pl, pst);
  int e = spgan_launch_status();
  if (e) return e;
  hipLaunchKernelGGL(edge_window_wgrad_reduce_kernel, dim3(cdiv((long)O * w * C * 8, 256)), dim3(256), 0, st, ws, pl.splits, O, w * C, dW, lddw);
  return spgan_launch_status();
}

extern "C" int spgan_edge_window_dgrad(const float* G, int ldg, const float* Wt, int ldwt, int M, int k, int C, int O, int w, float* S,
                                       int accumulate, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(G && Wt && S && sizes_ok(M, k, C, O, w) && ldg >= O && ldwt >= O);
  const int T = k - w + 1;
  SPGAN_CHECK_ARG((long)M * T <= 0x7fffffffL);
  const bool vec = O % 4 == 0 && ldg % 4 == 0 && ldwt % 4 == 0 && al16(G) && al16(Wt);
  const dim3 gr(grid8(cdiv(M, 32))), b(256);
  if (vec) hipLaunchKernelGGL(edge_window_dgrad_kernel<true>, gr, b, 0, (hipStream_t)s_, G, ldg, Wt, ldwt, M, k, C, O, w, T, S, accumulate);
  else hipLaunchKernelGGL(edge_window_dgrad_kernel<false>, gr, b, 0, (hipStream_t)s_, G, ldg, Wt, ldwt, M, k, C, O, w, T, S, accumulate);
  return spgan_launch_status();
}

extern "C" int spgan_edge_window_scatter(const float* S, const int32_t* rowptr, const int32_t* src, int M, int k, int C, const float* add_a,
                                         int ld_a, const float* add_b, int ld_b, float* dx, int lddx, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(S && rowptr && src && dx && M > 0 && k > 0 && C > 0 && (long)M * k <= 0x7fffffffL && lddx >= C);
  SPGAN_CHECK_ARG((!add_a || ld_a >= C) && (!add_b || ld_b >= C));
  const bool v4 = C % 4 == 0 && lddx % 4 == 0 && al16(S) && al16(dx);
  const long items = (long)M * (v4 ? C / 4 : C);
  if (v4)
    hipLaunchKernelGGL(edge_window_scatter_kernel<4>, dim3(cdiv(items, 256)), dim3(256), 0, (hipStream_t)s_, S, rowptr, src, M, k, C, add_a, ld_a, add_b,
                       ld_b, dx, lddx);
  else
    hipLaunchKernelGGL(edge_window_scatter_kernel<1>, dim3(cdiv(items, 256)), dim3(256), 0, (hipStream_t)s_, S, rowptr, src, M, k, C, add_a, ld_a, add_b,
                       ld_b, dx, lddx);
  return spgan_launch_status();
}
