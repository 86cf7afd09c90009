// Dot-product self-attention over the points of a shape without a [B,N,N] map: the core of spgan.Self_Attn
// (Common/utilities.py:210-245) and of Attention(ch, materialize=False) (Generation/modules.py:534-558).
//
//   S_ij = q_i . k_j,  P = softmax_j(S),  O_i = sum_j P_ij v_j,  lse_i = log sum_j exp(S_ij)          (no 1/sqrt(d): the reference has none)
//
// Every product runs on v_mfma_f32_32x32x2_f32 (exact fp32).  As in pair_attn.hip the tile is computed with the moving points on the
// MFMA rows and the 32 stationary points on the columns (lane & 31): accumulator register t of lane half hi is row 8 (t / 4) + 4 hi + t % 4,
// which is exactly what lane half hi has to supply as the B operand of the product that contracts over the tile's rows.  The S^T tile's
// registers, turned into P^T or dS^T in place, therefore feed O^T = V^T P^T, dQ^T = K^T dS^T, dV^T = dO^T P and dK^T = Q^T dS directly:
// no tile goes through LDS, and a column's softmax statistics are 16 registers and one shuffle across the two lane halves.
// The K index of an MFMA is summed over, so its order is free: lane half hi contracts over the half [hi d/2, (hi + 1) d/2) of a row, two
// consecutive elements (one 8-byte load) per pair of MFMAs.  This needs d % 4 == 0: the host pads dk with zero columns.
//
// The 32 stationary rows are staged once per workgroup in LDS as float2 [d/2][32] (lane-contiguous: no bank conflict); the moving rows
// are read from global memory, 128 bytes per lane half and MFMA for the transposed operands.
//
// forward:  a workgroup owns 4 / NWD blocks of 32 queries; the NWD waves of a block split the value columns (DVT tiles of 32 each) and each
//           computes S^T itself.  Online softmax over the key tiles.
// backward: P = exp(S - lse) recomputed, dP = dO V^T, dS = P (dP - D), D_i = dO_i . O_i = sum_j P_ij dP_ij / sum_j P_ij.
//   role 0 (query-stationary): D (a first walk over the keys), then dQ_i = sum_j dS_ij k_j.   The four waves split the key tiles.
//   role 1 (key-stationary):   dV_j = sum_i P_ij dO_i, dK_j = sum_i dS_ij q_i.   The four waves split the query tiles; more than 320 value
//           columns run as two column passes (blockIdx.z), the second without dP and dK.
//   The waves' partial sums are added by wave 0 through LDS in the order ((w0 + w1) + w2) + w3: no float atomics, results repeat bit for bit.
#include "common.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define PT_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_MAX_DK = 128;
constexpr int PT_MAX_DV = 512;
constexpr int PT_DKT = PT_MAX_DK / 32;      // accumulator tiles of dQ^T / dK^T

__device__ __forceinline__ int acc_row(int t, int hi) { return 8 * (t >> 2) + 4 * hi + (t & 3); }
__device__ __forceinline__ float2 ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }

// 32 rows of X (from row r0 of the shape at `base`, clamped to the shape) -> dst[d/2][32] float2
__device__ __forceinline__ void stage_rows(float2* dst, const float* __restrict__ X, int ld, long base, int r0, int n, int d) {
  const int hp = d >> 1;
  for (int idx = threadIdx.x; idx < 32 * hp; idx += PT_THREADS) {
    const int r = idx & 31, p = idx >> 5;
    dst[idx] = ld2(X + (base + min(r0 + r, n - 1)) * ld + 2 * p);
  }
}

// acc[row = moving point][col = stationary point] = sum_c Mv[row][c] St[col][c]; mrow = this lane's moving row (of lane & 31)
__device__ __forceinline__ f32x16 tile_dot(const float* __restrict__ mrow, const float2* St, int d, int col, int hi) {
  f32x16 acc;
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0.f;
  const int q4 = d >> 2;
  const float* mp = mrow + hi * 2 * q4;
  const float2* sp = St + (hi * q4) * 32 + col;
  for (int u = 0; u < q4; ++u) {
    const float2 a = ld2(mp + 2 * u);
    const float2 b = sp[u * 32];
    acc = PT_MFMA(a.x, b.x, acc);
    acc = PT_MFMA(a.y, b.y, acc);
  }
  return acc;
}

// acc[row = column c0 + (lane & 31) of Mv][col] += sum over the 32 moving rows r of Mv[r][.] w[r][col]; w in accumulator layout
__device__ __forceinline__ void tile_acc(f32x16& acc, const float* __restrict__ Mv, int ld, long base, int r0, int n, int c0, int d,
                                         const float (&w)[16], int col, int hi) {
  const int c = c0 + col;
  const bool ok = c < d;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const long r = base + min(r0 + acc_row(t, hi), n - 1);
    const float a = ok ? Mv[r * ld + c] : 0.f;
    acc = PT_MFMA(a, w[t], acc);
  }
}

// wave 0 ends with ((w0 + w1) + w2) + w3 of the NT tiles; buf holds NT * 16 * 64 floats.  All four waves call it.
template <int NT>
__device__ __forceinline__ void reduce_waves(f32x16 (&acc)[NT], float* buf, int w, int lane) {
  for (int src = 1; src < 4; ++src) {
    __syncthreads();
    if (w == src) {
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int t = 0; t < 16; ++t) buf[(i * 16 + t) * 64 + lane] = acc[i][t];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[i][t] += buf[(i * 16 + t) * 64 + lane];
    }
  }
}

// rows of the stationary block: X[(base + i0 + col)][c0 + 8 a + 4 hi ..] = acc * scale, for the tiles below d
__device__ __forceinline__ void store_tile(const f32x16& acc, float scale, float* __restrict__ X, int ld, long row, int c0, int d, int hi) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int c = c0 + 8 * a + 4 * hi;
    if (c < d)      // d % 4 == 0: the whole float4 is inside
      *reinterpret_cast<float4*>(X + row * ld + c) =
          make_float4(acc[4 * a] * scale, acc[4 * a + 1] * scale, acc[4 * a + 2] * scale, acc[4 * a + 3] * scale);
  }
}

template <int NWD, int DVT>
__global__ __launch_bounds__(PT_THREADS) void point_fwd_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, int ldk,
                                                               const float* __restrict__ v, int ldv, int n, int dk, int dv,
                                                               float* __restrict__ o, int ldo, float* __restrict__ lse) {
  extern __shared__ float2 pt_lds[];
  constexpr int QB = 4 / NWD;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 31, hi = lane >> 5;
  const int qb = w / NWD, wd = w % NWD;
  const long base = (long)blockIdx.y * n;
  const int hp = dk >> 1;
  for (int blk = 0; blk < QB; ++blk) stage_rows(pt_lds + blk * hp * 32, q, ldq, base, (blockIdx.x * QB + blk) * 32, n, dk);
  __syncthreads();
  const int i0 = (blockIdx.x * QB + qb) * 32;
  if (i0 >= n) return;                                 // no barrier below
  const float2* Qs = pt_lds + qb * hp * 32;
  f32x16 oacc[DVT];
#pragma unroll
  for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
    for (int t = 0; t < 16; ++t) oacc[dt][t] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  for (int j0 = 0; j0 < n; j0 += 32) {
    f32x16 s = tile_dot(k + (base + min(j0 + col, n - 1)) * ldk, Qs, dk, col, hi);      // S^T: rows = keys, columns = queries
    float mt = -INFINITY;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      if (j0 + acc_row(t, hi) >= n) s[t] = -INFINITY;                                    // a key past n gets weight exactly 0
      mt = fmaxf(mt, s[t]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float mn = fmaxf(m_run, mt);                 // finite: key j0 of every tile exists
    const float alpha = expf(m_run - mn);
    float p[16], ps = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      p[t] = expf(s[t] - mn);
      ps += p[t];
    }
    ps += __shfl_xor(ps, 32);
    l_run = fmaf(l_run, alpha, ps);
    m_run = mn;
    if (__ballot(alpha != 1.f)) {
#pragma unroll
      for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
        for (int t = 0; t < 16; ++t) oacc[dt][t] *= alpha;
    }
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt) {
      const int d0 = 32 * (wd * DVT + dt);
      if (d0 < dv) tile_acc(oacc[dt], v, ldv, base, j0, n, d0, dv, p, col, hi);         // O^T += V^T P^T
    }
  }
  const int i = i0 + col;
  if (i < n) {
    const float inv = 1.f / l_run;
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt) store_tile(oacc[dt], inv, o, ldo, base + i, 32 * (wd * DVT + dt), dv, hi);
    if (wd == 0 && hi == 0) lse[base + i] = m_run + logf(l_run);
  }
}

// Two walks over the key tiles: the first forms D_i = sum_j P_ij dP_ij / sum_j P_ij (= dO_i . O_i, but from the very numbers it is
// subtracted from: under a sharp softmax dP_ij - D_i cancels for the dominant key, and with one point it is an exact zero), the second
// dS and dQ.
__global__ __launch_bounds__(PT_THREADS) void point_bwd_q_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, int ldk,
                                                                 const float* __restrict__ v, int ldv, const float* __restrict__ dO, int lddo,
                                                                 const float* __restrict__ lse, float* __restrict__ D, int n, int dk,
                                                                 int dv, float* __restrict__ dq, int lddq) {
  extern __shared__ float2 pt_lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 31, hi = lane >> 5;
  const long base = (long)blockIdx.y * n;
  const int i0 = blockIdx.x * 32;
  float2* Qs = pt_lds;
  float2* Gs = pt_lds + (dk >> 1) * 32;
  stage_rows(Qs, q, ldq, base, i0, n, dk);
  stage_rows(Gs, dO, lddo, base, i0, n, dv);
  __syncthreads();
  const long iq = base + min(i0 + col, n - 1);
  const float lse_c = lse[iq];
  float* Dw = reinterpret_cast<float*>(pt_lds + ((dk + dv) >> 1) * 32);     // [2][4][32] behind the operand blocks
  float dpart = 0.f, ppart = 0.f;
  for (int j0 = 32 * w; j0 < n; j0 += 128) {
    const long kr = base + min(j0 + col, n - 1);
    const f32x16 s = tile_dot(k + kr * ldk, Qs, dk, col, hi);
    const f32x16 dp = tile_dot(v + kr * ldv, Gs, dv, col, hi);
#pragma unroll
    for (int t = 0; t < 16; ++t)
      if (j0 + acc_row(t, hi) < n) {
        const float p = expf(s[t] - lse_c);
        dpart = fmaf(p, dp[t], dpart);
        ppart += p;
      }
  }
  dpart += __shfl_xor(dpart, 32);
  ppart += __shfl_xor(ppart, 32);
  if (hi == 0) {
    Dw[w * 32 + col] = dpart;
    Dw[128 + w * 32 + col] = ppart;
  }
  __syncthreads();
  // divided by the recomputed row sum (1 up to the rounding of S - lse): sum_j dS_ij is then zero to rounding, which dQ needs when the
  // keys are large -- a row sum off by 1e-5 would leave D (1 - sum P) k in dQ
  const float D_c = (((Dw[col] + Dw[32 + col]) + Dw[64 + col]) + Dw[96 + col]) /
                    (((Dw[128 + col] + Dw[160 + col]) + Dw[192 + col]) + Dw[224 + col]);
  if (w == 0 && hi == 0 && i0 + col < n) D[iq] = D_c;
  f32x16 acc[PT_DKT];
#pragma unroll
  for (int kt = 0; kt < PT_DKT; ++kt)
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[kt][t] = 0.f;

  for (int j0 = 32 * w; j0 < n; j0 += 128) {
    const long kr = base + min(j0 + col, n - 1);
    const f32x16 s = tile_dot(k + kr * ldk, Qs, dk, col, hi);           // S^T
    const f32x16 dp = tile_dot(v + kr * ldv, Gs, dv, col, hi);          // dP^T[key][query] = v_key . dO_query
    float ds[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const float p = j0 + acc_row(t, hi) < n ? expf(s[t] - lse_c) : 0.f;
      ds[t] = p * (dp[t] - D_c);
    }
#pragma unroll
    for (int kt = 0; kt < PT_DKT; ++kt)
      if (32 * kt < dk) tile_acc(acc[kt], k, ldk, base, j0, n, 32 * kt, dk, ds, col, hi);      // dQ^T += K^T dS^T
  }
  reduce_waves<PT_DKT>(acc, reinterpret_cast<float*>(pt_lds), w, lane);
  if (w == 0 && i0 + col < n) {
#pragma unroll
    for (int kt = 0; kt < PT_DKT; ++kt) store_tile(acc[kt], 1.f, dq, lddq, base + i0 + col, 32 * kt, dk, hi);
  }
}

template <int DVT>
__global__ __launch_bounds__(PT_THREADS) void point_bwd_k_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, int ldk,
                                                                 const float* __restrict__ v, int ldv, const float* __restrict__ dO, int lddo,
                                                                 const float* __restrict__ lse, const float* __restrict__ D, int n, int dk,
                                                                 int dv, float* __restrict__ dkey, int lddk, float* __restrict__ dval, int lddv) {
  extern __shared__ float2 pt_lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 31, hi = lane >> 5;
  const long base = (long)blockIdx.y * n;
  const int j0 = blockIdx.x * 32;
  const bool first = blockIdx.z == 0;                  // the column pass that also forms dK
  const int dvt0 = blockIdx.z * DVT;
  float2* Ks = pt_lds;
  float2* Vs = pt_lds + (dk >> 1) * 32;
  stage_rows(Ks, k, ldk, base, j0, n, dk);
  if (first) stage_rows(Vs, v, ldv, base, j0, n, dv);
  __syncthreads();
  f32x16 acc[DVT + PT_DKT];                            // dV^T tiles, then dK^T tiles
#pragma unroll
  for (int i = 0; i < DVT + PT_DKT; ++i)
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[i][t] = 0.f;

  for (int i0 = 32 * w; i0 < n; i0 += 128) {
    const long qr = base + min(i0 + col, n - 1);
    const f32x16 s = tile_dot(q + qr * ldq, Ks, dk, col, hi);           // S: rows = queries, columns = keys
    float p[16], lr[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int i = i0 + acc_row(t, hi);
      lr[t] = lse[base + min(i, n - 1)];
      p[t] = i < n ? expf(s[t] - lr[t]) : 0.f;         // a query past n enters no sum
    }
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt) {
      const int d0 = 32 * (dvt0 + dt);
      if (d0 < dv) tile_acc(acc[dt], dO, lddo, base, i0, n, d0, dv, p, col, hi);               // dV^T += dO^T P
    }
    if (first) {
      const f32x16 dp = tile_dot(dO + qr * lddo, Vs, dv, col, hi);      // dP[query][key] = dO_query . v_key
      float ds[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) ds[t] = p[t] * (dp[t] - D[base + min(i0 + acc_row(t, hi), n - 1)]);
#pragma unroll
      for (int kt = 0; kt < PT_DKT; ++kt)
        if (32 * kt < dk) tile_acc(acc[DVT + kt], q, ldq, base, i0, n, 32 * kt, dk, ds, col, hi);   // dK^T += Q^T dS
    }
  }
  reduce_waves<DVT + PT_DKT>(acc, reinterpret_cast<float*>(pt_lds), w, lane);
  if (w == 0 && j0 + col < n) {
    const long row = base + j0 + col;
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt) store_tile(acc[dt], 1.f, dval, lddv, row, 32 * (dvt0 + dt), dv, hi);
    if (first) {
#pragma unroll
      for (int kt = 0; kt < PT_DKT; ++kt) store_tile(acc[DVT + kt], 1.f, dkey, lddk, row, 32 * kt, dk, hi);
    }
  }
}

inline bool pt_al(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool pt_ld(int ld, int d) { return ld >= d && ld % 4 == 0; }
inline bool pt_sizes(int b, int n, int dk, int dv) {
  return b >= 1 && b <= 65535 && n >= 1 && dk >= 4 && dk <= PT_MAX_DK && dk % 4 == 0 && dv >= 4 && dv <= PT_MAX_DV && dv % 4 == 0;
}
inline int pt_max(int a, int b) { return a > b ? a : b; }

}  // namespace

extern "C" {

int spgan_point_attn_padded_dk(int dk) { return dk < 1 || dk > PT_MAX_DK ? 0 : (dk + 3) / 4 * 4; }
int spgan_point_attn_max_dv(void) { return PT_MAX_DV; }

int spgan_point_attn_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int b, int n, int dk, int dv, float* o,
                         int ldo, float* lse, spgan_stream_t s) {
  SPGAN_CHECK_ARG(q && k && v && o && lse);
  SPGAN_CHECK_ARG(pt_sizes(b, n, dk, dv) && pt_ld(ldq, dk) && pt_ld(ldk, dk) && pt_ld(ldv, dv) && pt_ld(ldo, dv));
  SPGAN_CHECK_ARG(pt_al(q) && pt_al(k) && pt_al(v) && pt_al(o));
  hipStream_t st = (hipStream_t)s;
#define PT_FWD(NWD, DVT)                                                                                              \
  do {                                                                                                                \
    static LdsOptIn opt;                                                                                              \
    const int lds = (4 / NWD) * dk * 128;                                                                             \
    opt.ensure((const void*)point_fwd_kernel<NWD, DVT>, lds);                                                         \
    point_fwd_kernel<NWD, DVT><<<dim3(cdiv(n, 32 * (4 / NWD)), b), PT_THREADS, lds, st>>>(q, ldq, k, ldk, v, ldv, n, dk, dv, o, ldo, lse); \
  } while (0)
  if (dv <= 160) PT_FWD(1, 5);
  else if (dv <= 320) PT_FWD(2, 5);
  else PT_FWD(4, 4);
#undef PT_FWD
  return spgan_launch_status();
}

int spgan_point_attn_bwd(int role, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* dO, int lddo,
                         const float* lse, float* D, int b, int n, int dk, int dv, float* dq, int lddq, float* dkey, int lddk,
                         float* dval, int lddv, spgan_stream_t s) {
  SPGAN_CHECK_ARG(role == 0 || role == 1);
  SPGAN_CHECK_ARG(q && k && v && dO && lse && D);
  SPGAN_CHECK_ARG(pt_sizes(b, n, dk, dv) && pt_ld(ldq, dk) && pt_ld(ldk, dk) && pt_ld(ldv, dv) && pt_ld(lddo, dv));
  SPGAN_CHECK_ARG(pt_al(q) && pt_al(k) && pt_al(v) && pt_al(dO));
  hipStream_t st = (hipStream_t)s;
  const int opnd = (dk + dv) * 128;                    // the two staged operand blocks
  if (role == 0) {
    SPGAN_CHECK_ARG(dq && pt_ld(lddq, dk) && pt_al(dq));
    static LdsOptIn opt;
    const int lds = pt_max(opnd, PT_DKT * 16 * 64 * 4) + 2 * 4 * 32 * 4;
    opt.ensure((const void*)point_bwd_q_kernel, lds);
    point_bwd_q_kernel<<<dim3(cdiv(n, 32), b), PT_THREADS, lds, st>>>(q, ldq, k, ldk, v, ldv, dO, lddo, lse, D, n, dk, dv, dq, lddq);
    return spgan_launch_status();
  }
  SPGAN_CHECK_ARG(dkey && dval && pt_ld(lddk, dk) && pt_ld(lddv, dv) && pt_al(dkey) && pt_al(dval));
#define PT_BWDK(DVT, PASSES)                                                                                          \
  do {                                                                                                                \
    static LdsOptIn opt;                                                                                              \
    const int lds = pt_max(opnd, (DVT + PT_DKT) * 16 * 64 * 4);                                                       \
    opt.ensure((const void*)point_bwd_k_kernel<DVT>, lds);                                                            \
    point_bwd_k_kernel<DVT><<<dim3(cdiv(n, 32), b, PASSES), PT_THREADS, lds, st>>>(q, ldq, k, ldk, v, ldv, dO, lddo, lse, D, n, dk, dv, \
                                                                                   dkey, lddk, dval, lddv);           \
  } while (0)
  if (dv <= 128) PT_BWDK(4, 1);
  else if (dv <= 256) PT_BWDK(8, 1);
  else if (dv <= 320) PT_BWDK(10, 1);
  else PT_BWDK(8, 2);
#undef PT_BWDK
  return spgan_launch_status();
}

}  // extern "C"
