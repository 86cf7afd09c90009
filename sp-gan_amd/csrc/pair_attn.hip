// All-pairs vector attention of PointTransformerLayer (Generation/modules.py:1602-1644) without a per-pair vector in memory.
//
//   r_ij   = relu(W_p1 (pos_i - pos_j) + b_p1)                                [H]
//   sim_ij = w_a2 . relu(Qa_i + c - Ka_j + Wc r_ij)       Wc = W_a1 W_p2      [M = dim * mult rows]
//   a      = softmax_j(sim),  Sv_i = sum_j a_ij v_j,  R_i = sum_j a_ij r_ij
//
// The per-pair product Wc r_ij runs on v_mfma_f32_32x32x2_f32 (exact fp32).  Pairs sit on the 32 MFMA columns (lane & 31), the rows of
// Wc on the MFMA rows, so a lane sums its own 16 accumulator registers into sim and one shuffle joins the two lane halves.  The K index
// of an MFMA is summed over, so its order is free: slot (ht, a, c) of lane half hi holds h = 32 ht + 8 a + 4 hi + c, which is the row
// map of the C/D registers.  An accumulator tile is therefore at once the B operand of the product that contracts over its rows
// (dr = Wc^T dpre), r and dr live in the same lanes, and four consecutive slots are one float4 of a row-major padded operand.
// Swapping the two operands of the same MFMA gives the transposed tile (rows = pairs, lanes = rows of Wc), which is what the sums over
// pairs need (dWc, the row sums of dpre): no tile is transposed through LDS.
//
// Every sum has a fixed order: no float atomics.  Sums over the queries of one key come from a second, key-stationary launch of the
// backward kernel that recomputes (ROLE 1).
#include "common.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define PA_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

namespace {

constexpr int PA_THREADS = 256;      // four waves, each with its own 32-row tiles of Wc
constexpr int PA_TQ = 4;             // queries per forward workgroup (one per wave for the softmax)
constexpr int PA_DCH = 2;            // value columns per thread: dim <= PA_DCH * PA_THREADS
constexpr int PA_BWD_BLOCKS = 512;   // most workgroups (= partial records of dWc, dw_a2) of one backward launch

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float f4c(const float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// relu(w . d + b), one expression everywhere so that every layout of r holds the same bits
__device__ __forceinline__ float pos_unit(const float4& w, float dx, float dy, float dz) {
  return fmaxf(fmaf(w.x, dx, fmaf(w.y, dy, fmaf(w.z, dz, w.w))), 0.f);
}

// r of one pair in the K-slot layout of its lane half
template <int HT>
__device__ __forceinline__ void form_r(const float* __restrict__ Wp1p, float dx, float dy, float dz, int hi, float (&r)[HT * 16]) {
#pragma unroll
  for (int ht = 0; ht < HT; ++ht)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) r[ht * 16 + 4 * a + c] = pos_unit(ld4(Wp1p + 4 * (32 * ht + 8 * a + 4 * hi + c)), dx, dy, dz);
}

__device__ __forceinline__ float half_max(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// MODE 0: online softmax over key tiles -> Sv, R, lse.   MODE 1: P_ij = exp(sim_ij - lse_i) (the backward's recomputation).
template <int HT, int MODE>
__global__ __launch_bounds__(PA_THREADS) void pair_fwd_kernel(const float* __restrict__ pos, const float* __restrict__ Wp1p,
                                                              const float* __restrict__ QaC, const float* __restrict__ Ka,
                                                              const float* __restrict__ Wc, const float* __restrict__ wa2,
                                                              const float* __restrict__ v, int ldv, int n, int D, int Mp,
                                                              const float* __restrict__ lse_in, float* __restrict__ Sv,
                                                              float* __restrict__ R, float* __restrict__ lse_out, float* __restrict__ P) {
  constexpr int Hp = 32 * HT;
  const int MTW = Mp >> 7;                            // row tiles of Wc per wave
  __shared__ float part[4][PA_TQ][32];
  __shared__ float pl[PA_TQ][32];
  __shared__ float al[PA_TQ];
  __shared__ float linv[PA_TQ];                       // its own array: al is still read by the last tile's Sv phase
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 31, hi = lane >> 5;
  const long base = (long)blockIdx.y * n;
  const int i0 = blockIdx.x * PA_TQ;
  int iq[PA_TQ];
  float pq[PA_TQ][3];
#pragma unroll
  for (int q = 0; q < PA_TQ; ++q) {
    iq[q] = min(i0 + q, n - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) pq[q][c] = pos[(base + iq[q]) * 3 + c];
  }
  const bool own_ok = i0 + w < n;                     // wave w runs the softmax of query i0 + w
  const long own = base + min(i0 + w, n - 1);
  float m_run = -INFINITY, l_run = 0.f;
  float Racc[HT * 16];
#pragma unroll
  for (int t = 0; t < HT * 16; ++t) Racc[t] = 0.f;
  float sv[PA_TQ][PA_DCH];
#pragma unroll
  for (int q = 0; q < PA_TQ; ++q)
#pragma unroll
    for (int e = 0; e < PA_DCH; ++e) sv[q][e] = 0.f;
  const float lse_q = MODE == 1 ? lse_in[own] : 0.f;

  for (int j0 = 0; j0 < n; j0 += 32) {
    asm volatile("" ::: "memory");                    // keep the loop's operand loads inside it: hoisted they cost 128 registers
    const int j = j0 + col;
    const long jr = base + min(j, n - 1);
    const float kx = pos[jr * 3], ky = pos[jr * 3 + 1], kz = pos[jr * 3 + 2];
    float r[PA_TQ][HT * 16];
#pragma unroll
    for (int q = 0; q < PA_TQ; ++q) form_r<HT>(Wp1p, pq[q][0] - kx, pq[q][1] - ky, pq[q][2] - kz, hi, r[q]);
    float s[PA_TQ];
#pragma unroll
    for (int q = 0; q < PA_TQ; ++q) s[q] = 0.f;
#pragma unroll 1
    for (int u = 0; u < MTW; ++u) {
      const int m0 = 32 * (w * MTW + u) + 4 * hi;     // + 8 a + c: the accumulator rows of this lane
      f32x16 acc[PA_TQ];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const float4 k4 = ld4(Ka + jr * Mp + m0 + 8 * a);
#pragma unroll
        for (int q = 0; q < PA_TQ; ++q) {
          const float4 q4 = ld4(QaC + (base + iq[q]) * Mp + m0 + 8 * a);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[q][4 * a + c] = f4c(q4, c) - f4c(k4, c);
        }
      }
#pragma unroll
      for (int ht = 0; ht < HT; ++ht)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const float4 wc = ld4(Wc + (long)(32 * (w * MTW + u) + col) * Hp + 32 * ht + 8 * a + 4 * hi);
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < PA_TQ; ++q) acc[q] = PA_MFMA(f4c(wc, c), r[q][ht * 16 + 4 * a + c], acc[q]);
        }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const float4 w2 = ld4(wa2 + m0 + 8 * a);
#pragma unroll
        for (int q = 0; q < PA_TQ; ++q)
#pragma unroll
          for (int c = 0; c < 4; ++c) s[q] = fmaf(f4c(w2, c), fmaxf(acc[q][4 * a + c], 0.f), s[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < PA_TQ; ++q) {
      s[q] += __shfl_xor(s[q], 32);
      if (hi == 0) part[w][q][col] = s[q];
    }
    __syncthreads();
    {
      float sim = ((part[0][w][col] + part[1][w][col]) + part[2][w][col]) + part[3][w][col];
      if (j >= n) sim = -INFINITY;
      if (MODE == 0) {
        const float mn = fmaxf(m_run, half_max(sim));       // finite: key j0 of every tile exists
        const float alpha = expf(m_run - mn);
        const float p = expf(sim - mn);
        l_run = fmaf(l_run, alpha, half_sum(p));
        m_run = mn;
#pragma unroll
        for (int q = 0; q < PA_TQ; ++q)
          if (q == w) {
#pragma unroll
            for (int t = 0; t < HT * 16; ++t) Racc[t] = fmaf(Racc[t], alpha, p * r[q][t]);
          }
        if (hi == 0) pl[w][col] = p;
        if (lane == 0) al[w] = alpha;
      } else if (hi == 0 && j < n && own_ok) {
        P[own * n + j] = expf(sim - lse_q);
      }
    }
    __syncthreads();
    if (MODE == 0) {
#pragma unroll
      for (int e = 0; e < PA_DCH; ++e) {
        const int d = tid + PA_THREADS * e;
        if (d < D) {
#pragma unroll
          for (int q = 0; q < PA_TQ; ++q) sv[q][e] *= al[q];
          for (int jl = 0; jl < 32; ++jl) {
            const float vv = v[(base + min(j0 + jl, n - 1)) * (long)ldv + d];      // a masked key has p = 0
#pragma unroll
            for (int q = 0; q < PA_TQ; ++q) sv[q][e] = fmaf(pl[q][jl], vv, sv[q][e]);
          }
        }
      }
    }
  }
  if (MODE == 0) {
    const float inv = 1.f / l_run;
#pragma unroll
    for (int t = 0; t < HT * 16; ++t) {
      const float tot = half_sum(Racc[t]);
      if (col == 0 && own_ok) R[own * Hp + 32 * (t >> 4) + 8 * ((t >> 2) & 3) + 4 * hi + (t & 3)] = tot * inv;
    }
    if (lane == 0) {
      linv[w] = inv;
      if (own_ok) lse_out[own] = m_run + logf(l_run);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < PA_DCH; ++e) {
      const int d = tid + PA_THREADS * e;
      if (d < D)
#pragma unroll
        for (int q = 0; q < PA_TQ; ++q)
          if (i0 + q < n) Sv[(base + i0 + q) * D + d] = sv[q][e] * linv[q];
    }
  }
}

// dS_ij = P_ij (g_ij - delta_i), g_ij = dout_i . v_j + dR_i . r_ij, delta_i = sum_j P_ij g_ij / sum_j P_ij: one workgroup per query, r
// recomputed.  On entry dS holds dout_i . v_j (a per-cloud GEMM of the caller).  delta equals dout_i . (out_i - b_p2), but taken from the
// same g_ij and P_ij it is subtracted from: under a sharp softmax g_ij - delta_i cancels for the dominant key, and a delta from the
// forward's differently rounded sums would leave that pair's dS with the rounding error of g instead of that of the difference.  g is
// parked in dS between the two passes.
__global__ __launch_bounds__(PA_THREADS) void pair_dsim_kernel(const float* __restrict__ P, const float* __restrict__ dR,
                                                               const float* __restrict__ pos, const float* __restrict__ Wp1p, int n,
                                                               int Hp, float* __restrict__ dS) {
  __shared__ float red[2][PA_THREADS];
  __shared__ float sdR[64];
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.y * n, qi = base + blockIdx.x;
  if (tid < Hp) sdR[tid] = dR[qi * Hp + tid];
  __syncthreads();
  const float qx = pos[qi * 3], qy = pos[qi * 3 + 1], qz = pos[qi * 3 + 2];
  float sp = 0.f, spg = 0.f;
  for (int j = tid; j < n; j += PA_THREADS) {
    const long kj = base + j;
    float g = dS[qi * n + j];
    const float dx = qx - pos[kj * 3], dy = qy - pos[kj * 3 + 1], dz = qz - pos[kj * 3 + 2];
    for (int h = 0; h < Hp; ++h) g = fmaf(pos_unit(ld4(Wp1p + 4 * h), dx, dy, dz), sdR[h], g);
    const float p = P[qi * n + j];
    dS[qi * n + j] = g;
    sp += p;
    spg = fmaf(p, g, spg);
  }
  red[0][tid] = sp;
  red[1][tid] = spg;
  __syncthreads();
  for (int o = PA_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  const float delta = red[1][0] / red[0][0];
  for (int j = tid; j < n; j += PA_THREADS) dS[qi * n + j] = P[qi * n + j] * (dS[qi * n + j] - delta);      // its own g: no fence needed
}

// One stationary point s per outer step, the other point of the pair moves over the lanes.  Wave w of row group blockIdx.z owns the
// 32 rows of Wc of tile mt = 4 blockIdx.z + w; the groups' partial Z are summed by the caller (the mask [r > 0] is linear in dr).
//   ROLE 0: s = query i, St = Qa + c, Mv = Ka.  -> dA = dQa_i, Z_i = sum_j dz_ij, partial dWc and dw_a2 of this workgroup.
//   ROLE 1: s = key j,   St = Ka, Mv = Qa + c.  -> dA = dKa_j, Z_j = sum_i dz_ij.
// dz_ij = [r_ij > 0] (Wc^T dpre_ij + a_ij dR_i);  dpre_ij = dS_ij w_a2 [pre_ij > 0].
template <int HT, int ROLE>
__global__ __launch_bounds__(PA_THREADS) void pair_bwd_kernel(const float* __restrict__ pos, const float* __restrict__ Wp1p,
                                                              const float* __restrict__ St, const float* __restrict__ Mv,
                                                              const float* __restrict__ Wc, const float* __restrict__ WcT,
                                                              const float* __restrict__ wa2, const float* __restrict__ P,
                                                              const float* __restrict__ dS, const float* __restrict__ dR, int n,
                                                              int Mp, float* __restrict__ dA, float* __restrict__ Z, float* __restrict__ ws) {
  constexpr int Hp = 32 * HT;
  __shared__ float zred[4][Hp];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 31, hi = lane >> 5;
  const long base = (long)blockIdx.y * n;
  const int mt = 4 * blockIdx.z + w;
  const bool lead = w == 0 && blockIdx.z == 0;         // the a_ij dR_i term of dz enters once
  const float sg = ROLE == 0 ? 1.f : -1.f;            // d = pos_i - pos_j and pre = .. + Qa_i - Ka_j whichever point is stationary
  f32x16 dW[HT];
  float dw2 = 0.f;
#pragma unroll
  for (int ht = 0; ht < HT; ++ht)
#pragma unroll
    for (int t = 0; t < 16; ++t) dW[ht][t] = 0.f;
  float4 wH[HT];                                      // this lane's hidden unit of every tile, for r in the lanes-are-h layout
#pragma unroll
  for (int ht = 0; ht < HT; ++ht) wH[ht] = ld4(Wp1p + 4 * (32 * ht + col));
  const float w2l = wa2[32 * mt + col];
  float* Zg = Z + (long)blockIdx.z * gridDim.y * n * Hp;

  for (int s = blockIdx.x; s < n; s += gridDim.x) {
    const long sr = base + s;
    const float sx = pos[sr * 3], sy = pos[sr * 3 + 1], sz = pos[sr * 3 + 2];
    const float sT = St[sr * Mp + 32 * mt + col];
    float dAacc = 0.f, Zacc[HT * 16];
#pragma unroll
    for (int t = 0; t < HT * 16; ++t) Zacc[t] = 0.f;

    for (int t0 = 0; t0 < n; t0 += 32) {
      asm volatile("" ::: "memory");                  // keep the loop's operand loads inside it
      const int mv = t0 + col;
      const bool valid = mv < n;
      const long mr = base + min(mv, n - 1);
      float rP[HT * 16];
      form_r<HT>(Wp1p, sg * (sx - pos[mr * 3]), sg * (sy - pos[mr * 3 + 1]), sg * (sz - pos[mr * 3 + 2]), hi, rP);
      const long pair = ROLE == 0 ? sr * n + (mr - base) : mr * n + s;
      const float dSc = valid ? dS[pair] : 0.f, Pc = valid ? P[pair] : 0.f;

      f32x16 a1, a1T;
#pragma unroll
      for (int t = 0; t < 16; ++t) { a1[t] = 0.f; a1T[t] = 0.f; }
#pragma unroll
      for (int ht = 0; ht < HT; ++ht)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const float4 wc = ld4(Wc + (long)(32 * mt + col) * Hp + 32 * ht + 8 * a + 4 * hi);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            a1 = PA_MFMA(f4c(wc, c), rP[ht * 16 + 4 * a + c], a1);       // rows = rows of Wc, lanes = pairs
            a1T = PA_MFMA(rP[ht * 16 + 4 * a + c], f4c(wc, c), a1T);     // rows = pairs, lanes = rows of Wc
          }
        }
      // lanes = pairs: dpre feeds dr = Wc^T dpre as a B operand as it stands
      float dpre[16];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int m0 = 32 * mt + 8 * a + 4 * hi;
        const float4 s4 = ld4(St + sr * Mp + m0), m4 = ld4(Mv + mr * Mp + m0), w4 = ld4(wa2 + m0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float pre = a1[4 * a + c] + sg * (f4c(s4, c) - f4c(m4, c));
          dpre[4 * a + c] = pre > 0.f ? dSc * f4c(w4, c) : 0.f;
        }
      }
      f32x16 acc2[HT];
#pragma unroll
      for (int ht = 0; ht < HT; ++ht) {
#pragma unroll
        for (int t = 0; t < 16; ++t) acc2[ht][t] = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const float4 wt = ld4(WcT + (long)(32 * ht + col) * Mp + 32 * mt + 8 * a + 4 * hi);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc2[ht] = PA_MFMA(f4c(wt, c), dpre[4 * a + c], acc2[ht]);
        }
      }
      const long qrow = ROLE == 0 ? sr : mr;          // the query of this lane's pair
#pragma unroll
      for (int ht = 0; ht < HT; ++ht)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
          if (lead) g4 = ld4(dR + qrow * Hp + 32 * ht + 8 * a + 4 * hi);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int t = ht * 16 + 4 * a + c;
            if (rP[t] > 0.f) Zacc[t] += fmaf(Pc, f4c(g4, c), acc2[ht][4 * a + c]);
          }
        }
      // lanes = rows of Wc: the sums over the pairs of this tile; accumulator row t is the pair t0 + 8 (t / 4) + 4 hi + t % 4
      float dpT[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int p = t0 + 8 * (t >> 2) + 4 * hi + (t & 3);
        const long pr = base + min(p, n - 1);
        const float g = p < n ? dS[ROLE == 0 ? sr * n + p : pr * n + s] : 0.f;
        const float pre = a1T[t] + sg * (sT - Mv[pr * Mp + 32 * mt + col]);
        dpT[t] = pre > 0.f ? g * w2l : 0.f;
        dAacc += dpT[t];
        if (ROLE == 0) {
          dw2 = fmaf(g, fmaxf(pre, 0.f), dw2);
          const float dx = sx - pos[pr * 3], dy = sy - pos[pr * 3 + 1], dz = sz - pos[pr * 3 + 2];
#pragma unroll
          for (int ht = 0; ht < HT; ++ht) dW[ht] = PA_MFMA(pos_unit(wH[ht], dx, dy, dz), dpT[t], dW[ht]);   // dWc^T [h, m] += r^T dpre^T
        }
      }
    }
    {
      const float tot = dAacc + __shfl_xor(dAacc, 32);
      if (hi == 0) dA[sr * Mp + 32 * mt + col] = ROLE == 0 ? tot : -tot;
    }
#pragma unroll
    for (int t = 0; t < HT * 16; ++t) {
      const float tot = half_sum(Zacc[t]);
      if (col == 0) zred[w][32 * (t >> 4) + 8 * ((t >> 2) & 3) + 4 * hi + (t & 3)] = tot;
    }
    __syncthreads();
    if (tid < Hp) Zg[sr * Hp + tid] = ((zred[0][tid] + zred[1][tid]) + zred[2][tid]) + zred[3][tid];
    __syncthreads();
  }
  if (ROLE == 0) {
    float* rec = ws + (long)(blockIdx.y * gridDim.x + blockIdx.x) * ((long)Mp * Hp + Mp);
    const int m = 32 * mt + col;
#pragma unroll
    for (int ht = 0; ht < HT; ++ht)
#pragma unroll
      for (int a = 0; a < 4; ++a)
        *reinterpret_cast<float4*>(rec + (long)m * Hp + 32 * ht + 8 * a + 4 * hi) =
            make_float4(dW[ht][4 * a], dW[ht][4 * a + 1], dW[ht][4 * a + 2], dW[ht][4 * a + 3]);
    const float tot = dw2 + __shfl_xor(dw2, 32);
    if (hi == 0) rec[(long)Mp * Hp + m] = tot;
  }
}

constexpr int PA_MAX_M = 4096;
inline bool pa_domain(int D, int Mp, int Hp) {
  return D >= 1 && D <= PA_DCH * PA_THREADS && Mp >= 128 && Mp <= PA_MAX_M && Mp % 128 == 0 && (Hp == 32 || Hp == 64);
}
inline int pa_bwd_gx(int b, int n) {
  const int per = PA_BWD_BLOCKS / b;
  return per < 1 ? 1 : (per > n ? n : per);
}

}  // namespace

extern "C" {

int spgan_pair_attn_padded_m(int M) { return M < 1 || M > PA_MAX_M ? 0 : (M + 127) / 128 * 128; }
int spgan_pair_attn_padded_h(int H) { return H < 1 || H > 64 ? 0 : H <= 32 ? 32 : 64; }
int spgan_pair_attn_max_dim(void) { return PA_DCH * PA_THREADS; }

int spgan_pair_attn_fwd(const float* pos, const float* Wp1p, const float* QaC, const float* Ka, const float* Wc, const float* wa2,
                        const float* v, int ldv, int b, int n, int D, int Mp, int Hp, const float* lse_in, float* Sv, float* R,
                        float* lse_out, float* P, spgan_stream_t s) {
  SPGAN_CHECK_ARG(pos && Wp1p && QaC && Ka && Wc && wa2);
  SPGAN_CHECK_ARG(b >= 1 && b <= 65535 && n >= 1 && pa_domain(D, Mp, Hp));
  if (lse_in) SPGAN_CHECK_ARG(P != nullptr);
  else SPGAN_CHECK_ARG(v && ldv >= D && Sv && R && lse_out);
  const dim3 grid(cdiv(n, PA_TQ), b);
  hipStream_t st = (hipStream_t)s;
#define PA_FWD(HT, MODE) pair_fwd_kernel<HT, MODE><<<grid, PA_THREADS, 0, st>>>(pos, Wp1p, QaC, Ka, Wc, wa2, v, ldv, n, D, Mp, lse_in, Sv, R, lse_out, P)
  if (Hp == 32) { if (lse_in) PA_FWD(1, 1); else PA_FWD(1, 0); }
  else { if (lse_in) PA_FWD(2, 1); else PA_FWD(2, 0); }
#undef PA_FWD
  return spgan_launch_status();
}

int spgan_pair_attn_dsim(const float* P, const float* dR, const float* pos, const float* Wp1p, int b, int n, int Hp, float* dS,
                         spgan_stream_t s) {
  SPGAN_CHECK_ARG(P && dR && pos && Wp1p && dS);
  SPGAN_CHECK_ARG(b >= 1 && b <= 65535 && n >= 1 && (Hp == 32 || Hp == 64));
  pair_dsim_kernel<<<dim3(n, b), PA_THREADS, 0, (hipStream_t)s>>>(P, dR, pos, Wp1p, n, Hp, dS);
  return spgan_launch_status();
}

int spgan_pair_attn_bwd_records(int b, int n) { return b < 1 || n < 1 ? 0 : b * pa_bwd_gx(b, n); }

size_t spgan_pair_attn_bwd_ws_bytes(int b, int n, int Mp, int Hp) {
  if (b < 1 || n < 1 || !pa_domain(1, Mp, Hp)) return 0;
  return (size_t)spgan_pair_attn_bwd_records(b, n) * ((size_t)Mp * Hp + Mp) * sizeof(float);
}

int spgan_pair_attn_bwd(int role, const float* pos, const float* Wp1p, const float* QaC, const float* Ka, const float* Wc,
                        const float* WcT, const float* wa2, const float* P, const float* dS, const float* dR, int b, int n, int Mp,
                        int Hp, float* dA, float* Z, void* ws, size_t ws_bytes, spgan_stream_t s) {
  SPGAN_CHECK_ARG(role == 0 || role == 1);
  SPGAN_CHECK_ARG(pos && Wp1p && QaC && Ka && Wc && WcT && wa2 && P && dS && dR && dA && Z);
  SPGAN_CHECK_ARG(b >= 1 && b <= 65535 && n >= 1 && pa_domain(1, Mp, Hp));
  if (role == 0) SPGAN_CHECK_ARG(ws && ws_bytes >= spgan_pair_attn_bwd_ws_bytes(b, n, Mp, Hp));
  const dim3 grid(pa_bwd_gx(b, n), b, Mp / 128);
  hipStream_t st = (hipStream_t)s;
  float* wsf = (float*)ws;
#define PA_BWD(HT)                                                                                                              \
  if (role == 0) pair_bwd_kernel<HT, 0><<<grid, PA_THREADS, 0, st>>>(pos, Wp1p, QaC, Ka, Wc, WcT, wa2, P, dS, dR, n, Mp, dA, Z, wsf); \
  else pair_bwd_kernel<HT, 1><<<grid, PA_THREADS, 0, st>>>(pos, Wp1p, Ka, QaC, Wc, WcT, wa2, P, dS, dR, n, Mp, dA, Z, wsf)
  if (Hp == 32) { PA_BWD(1); } else { PA_BWD(2); }
#undef PA_BWD
  return spgan_launch_status();
}

}  // extern "C"
