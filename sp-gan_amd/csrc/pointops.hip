// The pointops extension (metrics/pointops/src/* of the reference): kNN and ball queries from a separate query set, the label
// statistics, feature distribute, channel-major grouping with its gradient, and the channel-major three-point interpolation.  All index
// tensors of this family are int32.  Nothing here uses a float atomic; every sum has a fixed order, so results repeat bit for bit.
//
// Distances.  Every squared distance of this file is d2 = (dx*dx + dy*dy) + dz*dz with dx = query - candidate, each operation rounded on its
// own (the pragma below keeps the compiler from contracting them), so a float32 model reproduces it bit for bit.
//
// kNN (knn_kernel).  One wave per query, KNN_WAVES queries per workgroup, no LDS and no barrier.  Lane l holds the candidates
// i = base + k*64 + l (k < V) as 64-bit keys (float bits of d2) << 32 | i: d2 >= 0, so the unsigned minimum is the least distance and,
// among exact ties, the LOWEST index.  Keys are distinct, so round r's winner is the least key above round r-1's: a round is one masked
// local minimum over the lane's V keys and a six-step DPP minimum; no key is ever rewritten.  The winner of round r stays in the register
// slot r/64 of lane r%64, which is also the layout of the coalesced stores at the end.  A cloud of more than 64*V_MAX points is taken in
// chunks of that size: the winners so far join the next chunk's candidates as T more keys per lane.  Slots past n hold index 0, +inf.
//
// Cloud scans (scan_kernel).  Ball query, the label statistics over a ball, and both at once are one template: one wave per query, 64
// candidates per step, a ballot of the lanes with d2 < r*r (strict), ranks from the ballot's prefix count.  With STOP the scan ends at
// nsample hits and the statistics cover those hits only (labelstat_cuda_kernel.cu:44-46); without it they cover the whole ball.
//
// Grouping (group_cm_kernel).  out[b, c0+c, j, k] = src[b, c, idx[b,j,k]] (- centre[b,j,c]) into a channel slice of a [B,Ctot,m,K]
// buffer.  A workgroup stages CT channel rows of the cloud in LDS (GROUP_LDS_FLOATS / n of them, at most GROUP_CT_MAX), reads each index
// once and writes CT planes, each store coalesced along (j,k).  src is [B,C,n], or [B,n,3] read point-major (transposed while staging).
// Clouds of more than GROUP_LDS_FLOATS points gather from global memory.  Backward: per point, the slots that read it in ascending order
// (spgan_gather_csr), summed by one thread per (b,c,i).
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;
constexpr u64 KEY_NONE = ~0ull;
constexpr int KNN_WAVES = 4;
constexpr int KNN_MAX_NSAMPLE = 200;     // the reference's array size
constexpr int KNN_V_MAX = 32;            // keys per lane: 2048 candidates in registers
constexpr int SCAN_WAVES = 4;
constexpr int STAT_REGS = 4;             // label classes per lane kept in registers: 256; the rest accumulate in the output row
constexpr int GROUP_LDS_FLOATS = 12288;  // 48 KB
constexpr int GROUP_CT_MAX = 8;
constexpr int GROUP_SLOT_CHUNK = 8192;

__device__ __forceinline__ float dist2(float qx, float qy, float qz, float cx, float cy, float cz) {
  const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
  return (dx * dx + dy * dy) + dz * dz;
}

template <int CTRL>
__device__ __forceinline__ u64 dpp_min_step(u64 k) {
  const int lo = (int)(unsigned)k, hi = (int)(unsigned)(k >> 32);
  const unsigned tlo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);   // lanes without a source keep their own
  const unsigned thi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const u64 t = ((u64)thi << 32) | tlo;
  return t < k ? t : k;
}

// Minimum of a 64-bit key over the wave, in registers, returned wave-uniform.  All 64 lanes must be active.  (As in expansion.hip.)
__device__ __forceinline__ u64 wave_min_u64(u64 k) {
  k = dpp_min_step<0xb1>(k);     // quad_perm [1,0,3,2]
  k = dpp_min_step<0x4e>(k);     // quad_perm [2,3,0,1]
  k = dpp_min_step<0x141>(k);    // row_half_mirror
  k = dpp_min_step<0x140>(k);    // row_mirror
  k = dpp_min_step<0x142>(k);    // row_bcast15
  k = dpp_min_step<0x143>(k);    // row_bcast31 -> lane 63 holds the wave's minimum
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
  return ((u64)hi << 32) | lo;
}

// V keys per lane per chunk, T = ceil(nsample/64) result slots per lane, MULTI: the cloud has more than 64*V points.
template <int V, int T, bool MULTI>
__global__ __launch_bounds__(KNN_WAVES * 64) void knn_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz, int n, int m,
                                                             long total, int nsample, int32_t* __restrict__ idx, float* __restrict__ d2out) {
  const int lane = threadIdx.x & 63;
  const long q = (long)blockIdx.x * KNN_WAVES + (threadIdx.x >> 6);
  if (q >= total) return;                              // whole waves leave; there is no barrier
  const long b = q / m;
  const float* cloud = xyz + (size_t)b * n * 3;
  const float qx = new_xyz[q * 3], qy = new_xyz[q * 3 + 1], qz = new_xyz[q * 3 + 2];
  u64 carry[T];
#pragma unroll
  for (int t = 0; t < T; ++t) carry[t] = KEY_NONE;
  for (int base = 0; base < n; base += 64 * V) {
    u64 key[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int i = base + k * 64 + lane;
      key[k] = KEY_NONE;
      if (i < n) {
        const float d = dist2(qx, qy, qz, cloud[(size_t)i * 3], cloud[(size_t)i * 3 + 1], cloud[(size_t)i * 3 + 2]);
        key[k] = ((u64)__float_as_uint(d) << 32) | (unsigned)i;
      }
    }
    u64 res[T];
#pragma unroll
    for (int t = 0; t < T; ++t) res[t] = KEY_NONE;
    u64 lo = 0;                                         // this round takes the least key >= lo
    for (int r = 0; r < nsample; ++r) {
      u64 best = KEY_NONE;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const u64 c = key[k] >= lo ? key[k] : KEY_NONE;
        best = c < best ? c : best;
      }
      if (MULTI) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const u64 c = carry[t] >= lo ? carry[t] : KEY_NONE;
          best = c < best ? c : best;
        }
      }
      const u64 w = wave_min_u64(best);
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (t == (r >> 6) && lane == (r & 63)) res[t] = w;
      lo = w == KEY_NONE ? KEY_NONE : w + 1;
    }
#pragma unroll
    for (int t = 0; t < T; ++t) carry[t] = res[t];
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int s = t * 64 + lane;
    if (s < nsample) {
      const u64 w = carry[t];
      const int i = (int)(unsigned)(w & 0xffffffffu);
      const bool none = w == KEY_NONE || i < 0 || i >= n;
      idx[q * nsample + s] = none ? 0 : i;
      d2out[q * nsample + s] = none ? __builtin_inff() : __uint_as_float((unsigned)(w >> 32));
    }
  }
}

// One wave per query over the cloud in steps of 64 candidates.  IDX: the first nsample hits (ascending), every slot pre-filled with the
// first hit, zeros for an empty ball.  STAT: the sum of the hits' label rows.  STOP: the scan ends at nsample hits.
template <bool IDX, bool STAT, bool STOP>
__global__ __launch_bounds__(SCAN_WAVES * 64) void scan_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                               const int32_t* __restrict__ label, int n, int m, long total, float radius,
                                                               int nsample, int nclass, int32_t* __restrict__ idx, int32_t* __restrict__ stat) {
  const int lane = threadIdx.x & 63;
  const long q = (long)blockIdx.x * SCAN_WAVES + (threadIdx.x >> 6);
  if (q >= total) return;
  const long b = q / m;
  const float* cloud = xyz + (size_t)b * n * 3;
  const int32_t* lab = STAT ? label + (size_t)b * n * nclass : nullptr;
  int32_t* srow = STAT ? stat + (size_t)q * nclass : nullptr;
  int32_t* irow = IDX ? idx + (size_t)q * nsample : nullptr;
  const float qx = new_xyz[q * 3], qy = new_xyz[q * 3 + 1], qz = new_xyz[q * 3 + 2];
  const float r2 = radius * radius;
  int acc[STAT_REGS];
#pragma unroll
  for (int t = 0; t < STAT_REGS; ++t) acc[t] = 0;
  if (STAT)
    for (int c = STAT_REGS * 64 + lane; c < nclass; c += 64) srow[c] = 0;      // the same lane adds to it below
  int cnt = 0, first = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    bool hit = false;
    if (i < n) hit = dist2(qx, qy, qz, cloud[(size_t)i * 3], cloud[(size_t)i * 3 + 1], cloud[(size_t)i * 3 + 2]) < r2;
    u64 mask = __ballot(hit);
    if (mask == 0) continue;
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    if (STOP) {                                         // keep the hits that still fit
      hit = hit && cnt + rank < nsample;
      mask = __ballot(hit);
    }
    if (cnt == 0) first = base + __builtin_ctzll(mask);
    if (IDX && hit && cnt + rank < nsample) irow[cnt + rank] = i;
    if (STAT) {
      u64 rest = mask;
      while (rest) {
        const int k = base + __builtin_ctzll(rest);
        rest &= rest - 1;
        const int32_t* row = lab + (size_t)k * nclass;
#pragma unroll
        for (int t = 0; t < STAT_REGS; ++t) {
          const int c = t * 64 + lane;
          if (c < nclass) acc[t] += row[c];
        }
        for (int c = STAT_REGS * 64 + lane; c < nclass; c += 64) srow[c] += row[c];
      }
    }
    cnt += __popcll(mask);
    if (STOP && cnt >= nsample) break;
  }
  if (IDX) {
    const int fill = cnt == 0 ? 0 : first;
    for (int s = min(cnt, nsample) + lane; s < nsample; s += 64) irow[s] = fill;
  }
  if (STAT) {
#pragma unroll
    for (int t = 0; t < STAT_REGS; ++t) {
      const int c = t * 64 + lane;
      if (c < nclass) srow[c] = acc[t];
    }
  }
}

// out[b,j,c] = sum over k of label[b, idx[b,j,k], c]; an index outside [0,n) adds nothing and sets *bad
__global__ void labelstat_idx_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ idx, int n, int m, int nsample, int nclass,
                                     size_t total, int32_t* __restrict__ out, int* __restrict__ bad) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int c = t % nclass;
  const size_t q = t / nclass;
  const size_t b = q / m;
  const int32_t* lab = label + b * n * nclass;
  int acc = 0;
  for (int k = 0; k < nsample; ++k) {
    const int i = idx[q * nsample + k];
    if (i < 0 || i >= n) {
      if (bad) atomicOr(bad, 1);
      continue;
    }
    acc += lab[(size_t)i * nclass + c];
  }
  out[t] = acc;
}

// the nearest max_xyz of every xyz, the lowest index among equals, -1 when none is nearer than 100000 (squared)
__global__ __launch_bounds__(SCAN_WAVES * 64) void featuredistribute_kernel(const float* __restrict__ max_xyz, const float* __restrict__ xyz,
                                                                            int n, int m, long total, int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long q = (long)blockIdx.x * SCAN_WAVES + (threadIdx.x >> 6);
  if (q >= total) return;
  const long b = q / m;
  const float* cloud = max_xyz + (size_t)b * n * 3;
  const float qx = xyz[q * 3], qy = xyz[q * 3 + 1], qz = xyz[q * 3 + 2];
  u64 best = KEY_NONE;
  for (int i = lane; i < n; i += 64) {
    const float d = dist2(qx, qy, qz, cloud[(size_t)i * 3], cloud[(size_t)i * 3 + 1], cloud[(size_t)i * 3 + 2]);
    const u64 key = ((u64)__float_as_uint(d) << 32) | (unsigned)i;
    best = key < best ? key : best;
  }
  best = wave_min_u64(best);
  if (lane == 0) {
    const int i = (int)(unsigned)(best & 0xffffffffu);
    const float d = __uint_as_float((unsigned)(best >> 32));
    out[q] = (best != KEY_NONE && d < 100000.f && i >= 0 && i < n) ? i : -1;      // a NaN distance compares false
  }
}

// Element (c, i) of the source of shape b sits at srcb[c*sc + i*si]: [C,n] has sc = n, si = 1; [n,3] has sc = 1, si = 3.
// VEC slots per thread: 4 (one 16-byte index load and one 16-byte store per channel; m*K a multiple of 4, 16-byte aligned buffers) or 1.
template <bool STAGE, int VEC>
__global__ __launch_bounds__(256) void group_cm_kernel(const float* __restrict__ src, long sc, long si, const float* __restrict__ center,
                                                       const int32_t* __restrict__ idx, int C, int n, int m, int K, int c0, int Ctot, int CT,
                                                       float* __restrict__ out, int* __restrict__ bad) {
  __shared__ float rows[STAGE ? GROUP_LDS_FLOATS : 1];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int cbase = blockIdx.y * CT;
  const int cn = min(CT, C - cbase);
  const long S = (long)m * K;
  const long s0 = (long)blockIdx.x * GROUP_SLOT_CHUNK;
  const long s1 = min(S, s0 + GROUP_SLOT_CHUNK);
  const float* srcb = src + (size_t)b * C * n;
  if (STAGE) {
    for (int e = tid; e < cn * n; e += 256) {
      const int cl = e / n, i = e - cl * n;
      rows[e] = srcb[(cbase + cl) * sc + i * si];
    }
    __syncthreads();
  }
  const int32_t* ib = idx + (size_t)b * S;
  float* ob = out + ((size_t)b * Ctot + c0 + cbase) * S;
  for (long s = s0 + (long)tid * VEC; s < s1; s += 256 * VEC) {      // VEC == 4: S and the chunk are multiples of 4, so s + 3 < s1
    int i[VEC];
    bool ok[VEC];
    if (VEC == 4) {
      const int4 q = *reinterpret_cast<const int4*>(ib + s);
      i[0] = q.x; i[1 % VEC] = q.y; i[2 % VEC] = q.z; i[3 % VEC] = q.w;
    } else {
      i[0] = ib[s];
    }
    bool all_ok = true;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      ok[e] = i[e] >= 0 && i[e] < n;
      all_ok = all_ok && ok[e];
    }
    if (!all_ok && bad) atomicOr(bad, 1);
    for (int cl = 0; cl < cn; ++cl) {
      float v[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        v[e] = 0.f;
        if (ok[e]) {
          v[e] = STAGE ? rows[cl * n + i[e]] : srcb[(cbase + cl) * sc + i[e] * si];
          if (center) v[e] = v[e] - center[((size_t)b * m + (s + e) / K) * 3 + cbase + cl];
        }
      }
      float* o = ob + (size_t)cl * S + s;
      if (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1 % VEC], v[2 % VEC], v[3 % VEC]);
      else o[0] = v[0];
    }
  }
}

// dsrc[b,c,i] = sum over the slots e of point (b,i) (ascending, spgan_gather_csr) of dout[b, c0+c, e - b*S]; one thread per element
__global__ void group_cm_bwd_kernel(const float* __restrict__ dout, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ slots,
                                    int C, int n, long S, int c0, int Ctot, long sc, long si, size_t total, float* __restrict__ dsrc) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int i = t % n;
  const size_t bc = t / n;
  const int c = bc % C;
  const size_t b = bc / C;
  const size_t row = b * n + i;
  const float* d = dout + (b * Ctot + c0 + c) * S;
  float acc = 0.f;
  for (int e = rowptr[2 * row], e1 = rowptr[2 * row + 1]; e < e1; ++e) {
    const long s = (long)slots[e] - (long)(b * S);
    if (s >= 0 && s < S) acc += d[s];
  }
  dsrc[b * C * n + c * sc + i * si] = acc;
}

// dcenter[b,j,c] = -(sum over k ascending of dout[b, c0+c, j, k]), c < 3
__global__ void group_center_cm_bwd_kernel(const float* __restrict__ dout, int m, int K, int c0, int Ctot, size_t total, float* __restrict__ dcenter) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int c = t % 3;
  const size_t bj = t / 3;
  const size_t b = bj / m, j = bj % m;
  const float* d = dout + ((b * Ctot + c0 + c) * m + j) * K;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc += d[k];
  dcenter[t] = -acc;
}

__global__ void group_int_kernel(const int64_t* __restrict__ feat, const int32_t* __restrict__ idx, int C, int n, long S, size_t total,
                                 int64_t* __restrict__ out, int* __restrict__ bad) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const size_t s = t % S, bc = t / S, b = bc / C;
  const int i = idx[b * S + s];
  if (i < 0 || i >= n) {
    if (bad) atomicOr(bad, 1);
    out[t] = 0;
    return;
  }
  out[t] = feat[bc * n + i];
}

// out[b,c,j] = (w0*f0 + w1*f1) + w2*f2, f_t = feat[b,c,idx[b,j,t]]; a slot whose index lies outside [0,m) contributes 0 and sets *bad
__global__ void interpolate_cm_kernel(const float* __restrict__ feat, const int32_t* __restrict__ idx, const float* __restrict__ weight, int C,
                                      int m, int n, size_t total, float* __restrict__ out, int* __restrict__ bad) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const size_t j = t % n, bc = t / n, b = bc / C;
  const size_t e = (b * n + j) * 3;
  float term[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = idx[e + k];
    if (i < 0 || i >= m) {
      if (bad) atomicOr(bad, 1);
      term[k] = 0.f;
    } else {
      term[k] = weight[e + k] * feat[bc * m + i];
    }
  }
  out[t] = (term[0] + term[1]) + term[2];
}

// dfeat[b,c,i] = sum over the slots e of source point (b,i) (ascending) of weight[e] * dout[b,c,e/3 - b*n]
__global__ void interpolate_cm_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ weight, const int32_t* __restrict__ rowptr,
                                          const int32_t* __restrict__ slots, int C, int m, int n, size_t total, float* __restrict__ dfeat) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int i = t % m;
  const size_t bc = t / m, b = bc / C;
  const size_t row = b * m + i;
  float acc = 0.f;
  for (int e = rowptr[2 * row], e1 = rowptr[2 * row + 1]; e < e1; ++e) {
    const long slot = slots[e];
    const long j = slot / 3 - (long)(b * n);
    if (slot >= 0 && j >= 0 && j < n) acc += weight[slot] * dout[bc * n + j];
  }
  dfeat[t] = acc;
}

template <int V, bool MULTI>
void launch_knn_t(int T, dim3 grid, hipStream_t s, const float* xyz, const float* new_xyz, int n, int m, long total, int nsample, int32_t* idx,
                  float* d2) {
  const dim3 block(KNN_WAVES * 64);
  if (T <= 1) hipLaunchKernelGGL((knn_kernel<V, 1, MULTI>), grid, block, 0, s, xyz, new_xyz, n, m, total, nsample, idx, d2);
  else if (T == 2) hipLaunchKernelGGL((knn_kernel<V, 2, MULTI>), grid, block, 0, s, xyz, new_xyz, n, m, total, nsample, idx, d2);
  else hipLaunchKernelGGL((knn_kernel<V, 4, MULTI>), grid, block, 0, s, xyz, new_xyz, n, m, total, nsample, idx, d2);
}

int launch_knn(const float* xyz, const float* new_xyz, int B, int n, int m, int nsample, int32_t* idx, float* d2, hipStream_t s) {
  SPGAN_CHECK_ARG(xyz && new_xyz && idx && d2);
  SPGAN_CHECK_ARG(B >= 1 && n >= 1 && m >= 1 && nsample >= 1 && nsample <= KNN_MAX_NSAMPLE);
  SPGAN_CHECK_ARG((size_t)B * n < 2147483647u / 3 && (size_t)B * m * nsample < 2147483647u && (size_t)B * m < 2147483647u / 3);
  const long total = (long)B * m;
  const dim3 grid(cdiv(total, KNN_WAVES));
  const int T = (nsample + 63) / 64;                   // 1, 2, 3 (run as 4) or 4
  if (n <= 64) launch_knn_t<1, false>(T, grid, s, xyz, new_xyz, n, m, total, nsample, idx, d2);
  else if (n <= 128) launch_knn_t<2, false>(T, grid, s, xyz, new_xyz, n, m, total, nsample, idx, d2);
  else if (n <= 256) launch_knn_t<4, false>(T, grid, s, xyz, new_xyz, n, m, total, nsample, idx, d2);
  else if (n <= 512) launch_knn_t<8, false>(T, grid, s, xyz, new_xyz, n, m, total, nsample, idx, d2);
  else if (n <= 1024) launch_knn_t<16, false>(T, grid, s, xyz, new_xyz, n, m, total, nsample, idx, d2);
  else if (n <= 64 * KNN_V_MAX) launch_knn_t<KNN_V_MAX, false>(T, grid, s, xyz, new_xyz, n, m, total, nsample, idx, d2);
  else launch_knn_t<KNN_V_MAX, true>(T, grid, s, xyz, new_xyz, n, m, total, nsample, idx, d2);
  return spgan_launch_status();
}

bool scan_sizes_ok(int B, int n, int m, int nsample, int nclass) {
  return B >= 1 && n >= 1 && m >= 1 && nsample >= 1 && nclass >= 1 && (size_t)B * n < 2147483647u / 3 && (size_t)B * m < 2147483647u / 3 &&
         (size_t)B * m * nsample < 2147483647u && (size_t)B * n * nclass < 2147483647u && (size_t)B * m * nclass < 2147483647u;
}

}  // namespace

extern "C" int spgan_pointops_knn_capacity(void) { return 64 * KNN_V_MAX; }
extern "C" int spgan_pointops_group_stage_limit(void) { return GROUP_LDS_FLOATS; }

extern "C" int spgan_pointops_knnquery(const float* xyz, const float* new_xyz, int B, int n, int m, int nsample, int32_t* idx, float* dist2,
                                       spgan_stream_t s_) {
  return launch_knn(xyz, new_xyz, B, n, m, nsample, idx, dist2, (hipStream_t)s_);
}

extern "C" int spgan_pointops_nearestneighbor(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx,
                                              spgan_stream_t s_) {
  return launch_knn(known, unknown, B, m, n, 3, idx, dist2, (hipStream_t)s_);
}

extern "C" int spgan_pointops_ballquery(float radius, int nsample, const float* xyz, const float* new_xyz, int B, int n, int m, int32_t* idx,
                                        spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz && new_xyz && idx && scan_sizes_ok(B, n, m, nsample, 1));
  const long total = (long)B * m;
  hipLaunchKernelGGL((scan_kernel<true, false, true>), dim3(cdiv(total, SCAN_WAVES)), dim3(SCAN_WAVES * 64), 0, (hipStream_t)s_, xyz, new_xyz,
                     (const int32_t*)nullptr, n, m, total, radius, nsample, 1, idx, (int32_t*)nullptr);
  return spgan_launch_status();
}

extern "C" int spgan_pointops_labelstat_ballrange(float radius, const float* xyz, const float* new_xyz, const int32_t* label_stat, int B, int n,
                                                  int m, int nclass, int32_t* new_label_stat, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz && new_xyz && label_stat && new_label_stat && scan_sizes_ok(B, n, m, 1, nclass));
  const long total = (long)B * m;
  hipLaunchKernelGGL((scan_kernel<false, true, false>), dim3(cdiv(total, SCAN_WAVES)), dim3(SCAN_WAVES * 64), 0, (hipStream_t)s_, xyz, new_xyz,
                     label_stat, n, m, total, radius, 1, nclass, (int32_t*)nullptr, new_label_stat);
  return spgan_launch_status();
}

extern "C" int spgan_pointops_labelstat_and_ballquery(float radius, int nsample, const float* xyz, const float* new_xyz, const int32_t* label_stat,
                                                      int B, int n, int m, int nclass, int32_t* idx, int32_t* new_label_stat, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz && new_xyz && label_stat && idx && new_label_stat && scan_sizes_ok(B, n, m, nsample, nclass));
  const long total = (long)B * m;
  hipLaunchKernelGGL((scan_kernel<true, true, true>), dim3(cdiv(total, SCAN_WAVES)), dim3(SCAN_WAVES * 64), 0, (hipStream_t)s_, xyz, new_xyz,
                     label_stat, n, m, total, radius, nsample, nclass, idx, new_label_stat);
  return spgan_launch_status();
}

extern "C" int spgan_pointops_labelstat_idx(const int32_t* label_stat, const int32_t* idx, int B, int n, int m, int nsample, int nclass,
                                            int32_t* new_label_stat, int32_t* bad, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(label_stat && idx && new_label_stat && scan_sizes_ok(B, n, m, nsample, nclass));
  const size_t total = (size_t)B * m * nclass;
  hipLaunchKernelGGL(labelstat_idx_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, label_stat, idx, n, m, nsample, nclass, total,
                     new_label_stat, (int*)bad);
  return spgan_launch_status();
}

extern "C" int spgan_pointops_featuredistribute(const float* max_xyz, const float* xyz, int B, int n, int m, int32_t* distribute_idx,
                                                spgan_stream_t s_) {
  SPGAN_CHECK_ARG(max_xyz && xyz && distribute_idx && scan_sizes_ok(B, n, m, 1, 1));
  const long total = (long)B * m;
  hipLaunchKernelGGL(featuredistribute_kernel, dim3(cdiv(total, SCAN_WAVES)), dim3(SCAN_WAVES * 64), 0, (hipStream_t)s_, max_xyz, xyz, n, m, total,
                     distribute_idx);
  return spgan_launch_status();
}

extern "C" int spgan_pointops_group_cm(const float* src, int point_major, const float* center, const int32_t* idx, int B, int C, int n, int m,
                                       int K, int c0, int Ctot, float* out, int32_t* bad, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(src && idx && out && B >= 1 && C >= 1 && n >= 1 && m >= 1 && K >= 1 && c0 >= 0 && c0 + C <= Ctot);
  SPGAN_CHECK_ARG((!point_major && !center) || C == 3);       // the point-major source and the centre are coordinates
  SPGAN_CHECK_ARG(B <= 65535 && (size_t)m * K < 2147483647u && (size_t)B * C * n < 2147483647u && (size_t)C * n < 2147483647u);
  const long S = (long)m * K;
  const long sc = point_major ? 1 : n, si = point_major ? 3 : 1;
  const int ct_lds = GROUP_LDS_FLOATS / n;
  const int CT = ct_lds >= 1 ? (ct_lds < GROUP_CT_MAX ? ct_lds : GROUP_CT_MAX) : GROUP_CT_MAX;
  SPGAN_CHECK_ARG(cdiv(C, CT) <= 65535);
  const dim3 grid(cdiv(S, GROUP_SLOT_CHUNK), cdiv(C, CT), B), block(256);
  const bool vec = S % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)idx & 15) == 0;
#define SPGAN_GROUP_LAUNCH(STAGE, VEC) \
  hipLaunchKernelGGL((group_cm_kernel<STAGE, VEC>), grid, block, 0, (hipStream_t)s_, src, sc, si, center, idx, C, n, m, K, c0, Ctot, CT, out, (int*)bad)
  if (ct_lds >= 1) {
    if (vec) SPGAN_GROUP_LAUNCH(true, 4); else SPGAN_GROUP_LAUNCH(true, 1);
  } else {
    if (vec) SPGAN_GROUP_LAUNCH(false, 4); else SPGAN_GROUP_LAUNCH(false, 1);
  }
#undef SPGAN_GROUP_LAUNCH
  return spgan_launch_status();
}

extern "C" int spgan_pointops_group_cm_bwd(const float* dout, const int32_t* rowptr, const int32_t* slots, int B, int C, int n, int m, int K, int c0,
                                           int Ctot, int point_major, float* dsrc, float* dcenter, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dout && (dsrc || dcenter) && (!dsrc || (rowptr && slots)));
  SPGAN_CHECK_ARG(B >= 1 && C >= 1 && n >= 1 && m >= 1 && K >= 1 && c0 >= 0 && c0 + C <= Ctot);
  SPGAN_CHECK_ARG((!point_major && !dcenter) || C == 3);
  SPGAN_CHECK_ARG((size_t)B * m * K < 2147483647u && (size_t)B * C * n / 256 < 2147483647u);
  hipStream_t s = (hipStream_t)s_;
  if (dsrc) {
    const size_t total = (size_t)B * C * n;
    const long sc = point_major ? 1 : n, si = point_major ? 3 : 1;
    hipLaunchKernelGGL(group_cm_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, dout, rowptr, slots, C, n, (long)m * K, c0, Ctot, sc, si, total,
                       dsrc);
  }
  if (dcenter) {
    const size_t total = (size_t)B * m * 3;
    hipLaunchKernelGGL(group_center_cm_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, dout, m, K, c0, Ctot, total, dcenter);
  }
  return spgan_launch_status();
}

extern "C" int spgan_pointops_group_int(const int64_t* feat, const int32_t* idx, int B, int C, int n, int m, int K, int64_t* out, int32_t* bad,
                                        spgan_stream_t s_) {
  SPGAN_CHECK_ARG(feat && idx && out && B >= 1 && C >= 1 && n >= 1 && m >= 1 && K >= 1 && (size_t)m * K < 2147483647u);
  const size_t total = (size_t)B * C * m * K;
  SPGAN_CHECK_ARG(total / 256 < 2147483647u);
  hipLaunchKernelGGL(group_int_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, feat, idx, C, n, (long)m * K, total, out, (int*)bad);
  return spgan_launch_status();
}

extern "C" int spgan_pointops_interpolate_cm(const float* feat, const int32_t* idx, const float* weight, int B, int C, int m, int n, float* out,
                                             int32_t* bad, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(feat && idx && weight && out && B >= 1 && C >= 1 && m >= 1 && n >= 1 && (size_t)B * n < 2147483647u / 3);
  const size_t total = (size_t)B * C * n;
  SPGAN_CHECK_ARG(total / 256 < 2147483647u);
  hipLaunchKernelGGL(interpolate_cm_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, feat, idx, weight, C, m, n, total, out, (int*)bad);
  return spgan_launch_status();
}

extern "C" int spgan_pointops_interpolate_cm_bwd(const float* dout, const float* weight, const int32_t* rowptr, const int32_t* slots, int B, int C,
                                                 int m, int n, float* dfeat, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dout && weight && rowptr && slots && dfeat && B >= 1 && C >= 1 && m >= 1 && n >= 1 && (size_t)B * n < 2147483647u / 3);
  const size_t total = (size_t)B * C * m;
  SPGAN_CHECK_ARG(total / 256 < 2147483647u);
  hipLaunchKernelGGL(interpolate_cm_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, dout, weight, rowptr, slots, C, m, n, total,
                     dfeat);
  return spgan_launch_status();
}
