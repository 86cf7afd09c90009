// The point-distribution losses of Common/model_utils.py: get_repulsion_loss, get_repulsion_loss4, get_perulsion_loss and the
// selection under get_uniform_loss_knn.  Each of them groups every point's neighbours (a ball query or kNN of the cloud against itself),
// measures the slots, takes the `keep` smallest and feeds all but the first to a scalar tail.  Here one wave per point does all of it from
// one scan of the cloud; neither the [B,N,nsample] index tensor nor a [B,N,nsample,3] grouped tensor exists in ball mode.
//
// Distances.  dx = p_i - p_j, d2 = (dx*dx + dy*dy) + dz*dz, l1 = (|dx| + |dy|) + |dz|, every operation rounded on its own (the pragma below
// keeps the compiler from contracting them), so a float32 model reproduces every selected index bit for bit.
//
// Forward (nearest_kernel).  One wave per query, PL_WAVES queries per workgroup.
//   Ball mode: the cloud is scanned 64 candidates per step; a ballot of the lanes with d2 < r*r (strict, a float product) ranks the hits,
//   hit `rank` takes slot cnt + rank and writes its 64-bit key (float bits of the slot value) << 32 | slot and its index into the wave's LDS
//   row; the scan ends at nsample hits (spgan_pointops_ballquery's rule with new_xyz = xyz).  Slots past cnt repeat slot 0's value under
//   their own slot number.  An empty ball (NaN coordinates, or r*r rounding to 0) holds point 0 in every slot, as the ball query does.
//   kNN mode: slot s is entry s of an index row written by spgan_pointops_knnquery.
//   Selection: lane l holds the slots l, 64+l, ..; round r is a masked local minimum over the lane's keys at or above round r-1's winner + 1
//   and a six-step DPP minimum (as knn_kernel of pointops.hip).  Slot values are >= +0, so the unsigned order of the keys is the order of
//   the values with ties to the lowest slot.  The `root` metric keys on d2 and takes the square root of the winners only.
//   Tail: lanes 1..keep-1 recompute their winner's value in float64 from the coordinates, form the term and its derivative (coef); the
//   wave adds the terms in ascending slot order, the workgroup adds its waves in ascending order into partial[blockIdx.x] (float64).
//   loss_reduce_kernel adds the partials (thread t of 1024: t, t+1024, .. ascending; then a halving tree) and rounds once to float32.
//
// Backward.  dpred[i] = sum_t c[i,t] * g(p_i - p_idx[i,t])  -  sum over (i',t) with idx[i',t] == i, ascending, of c[i',t] * g(p_i' - p_i),
// g the metric's derivative in the difference (2d; sign(d), 0 at 0; d / sqrt(d2 + 1e-12)), all in float64 with one rounding at the end, no
// atomics.  nearest_bwd_kernel: 64 points per workgroup, four waves; the cloud's [n,keep] index table passes through LDS in chunks and each
// wave walks a quarter of every chunk (a broadcast read and one compare per entry and wave); the order of the sum is fixed: the direct
// terms, then wave 0's entries ascending, wave 1's, ..  With CSR the same terms are added in ascending slot order over spgan_gather_csr's
// per-point lists; that route does only the work the matches need and is the one spgan.model_utils takes (the table walk lost,
// profiles/point_losses_bench.json, and serves clouds beyond spgan_gather_csr's 16384 points).
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;
constexpr u64 KEY_NONE = ~0ull;
constexpr int PL_WAVES = 4;
constexpr int PL_MIN_NSAMPLE = 5;
constexpr int PL_MAX_NSAMPLE = 256;       // four slots per lane
constexpr int PL_KNN_MAX_NSAMPLE = 200;   // spgan_pointops_knnquery's limit
constexpr int PL_MAX_KEEP = 8;
constexpr int PL_BWD_PARTS = 4;           // waves per 64 points in the table walk
constexpr int PL_BWD_CHUNK = 4096;        // table entries staged in LDS per round (16 KB)
constexpr int PL_REDUCE_THREADS = 1024;

enum { METRIC_SQ = 0, METRIC_L1 = 1, METRIC_ROOT = 2 };
enum { TAIL_NONE = 0, TAIL_HINGE = 1, TAIL_REP4 = 2 };

template <int CTRL>
__device__ __forceinline__ u64 dpp_min_step(u64 k) {
  const int lo = (int)(unsigned)k, hi = (int)(unsigned)(k >> 32);
  const unsigned tlo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);   // lanes without a source keep their own
  const unsigned thi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const u64 t = ((u64)thi << 32) | tlo;
  return t < k ? t : k;
}

// Minimum of a 64-bit key over the wave, in registers, returned wave-uniform.  All 64 lanes must be active.  (As in pointops.hip.)
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

// the float whose bits order the slot: the slot value itself, d2 for the root metric
template <int METRIC>
__device__ __forceinline__ float slot_value(float dx, float dy, float dz) {
  if (METRIC == METRIC_L1) return (fabsf(dx) + fabsf(dy)) + fabsf(dz);
  return (dx * dx + dy * dy) + dz * dz;
}

template <int METRIC>
__device__ __forceinline__ double slot_value_d(double dx, double dy, double dz) {
  if (METRIC == METRIC_L1) return (fabs(dx) + fabs(dy)) + fabs(dz);
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  return METRIC == METRIC_ROOT ? sqrt(d2 + 1e-12) : d2;
}

// T key registers per lane: nsample <= 64*T
template <int METRIC, bool KNN, int T>
__global__ __launch_bounds__(PL_WAVES * 64) void nearest_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ group, int n,
                                                                long total, float radius, int nsample, int keep, int tail, double h,
                                                                double rterm, float* __restrict__ val, int32_t* __restrict__ idx,
                                                                float* __restrict__ coef, double* __restrict__ partial) {
  __shared__ u64 skey[KNN ? 1 : PL_WAVES][KNN ? 1 : 64 * T];
  __shared__ int sj[KNN ? 1 : PL_WAVES][KNN ? 1 : 64 * T];
  __shared__ double wsum[PL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long q0 = (long)blockIdx.x * PL_WAVES + wave;
  const bool live = q0 < total;
  const long q = live ? q0 : total - 1;                // a spare wave repeats the last query and stores nothing: the barriers stay whole
  const long b = q / n;
  const float* cloud = xyz + (size_t)b * n * 3;
  const float qx = xyz[q * 3], qy = xyz[q * 3 + 1], qz = xyz[q * 3 + 2];
  const int32_t* grow = KNN ? group + (size_t)q * nsample : nullptr;
  u64 key[T];
  int cnt = 0;
  if (!KNN) {
    const float r2 = radius * radius;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      bool hit = false;
      float m = 0.f;
      if (i < n) {
        const float dx = qx - cloud[(size_t)i * 3], dy = qy - cloud[(size_t)i * 3 + 1], dz = qz - cloud[(size_t)i * 3 + 2];
        hit = (dx * dx + dy * dy) + dz * dz < r2;
        m = slot_value<METRIC>(dx, dy, dz);
      }
      const u64 mask = __ballot(hit);
      if (mask == 0) continue;
      const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
      if (hit && slot < nsample) {                       // nsample <= 64*T: inside the row
        skey[wave][slot] = ((u64)__float_as_uint(m) << 32) | (unsigned)slot;
        sj[wave][slot] = i;
      }
      cnt += __popcll(mask);
      if (cnt >= nsample) break;
    }
    if (cnt == 0 && lane == 0) {                         // the empty ball: point 0
      const float m = slot_value<METRIC>(qx - cloud[0], qy - cloud[1], qz - cloud[2]);
      skey[wave][0] = (u64)__float_as_uint(m) << 32;
      sj[wave][0] = 0;
    }
    cnt = cnt == 0 ? 1 : min(cnt, nsample);
    __syncthreads();
    const u64 pad = skey[wave][0] & 0xffffffff00000000ull;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int s = t * 64 + lane;
      key[t] = s < cnt ? skey[wave][s] : (s < nsample ? (pad | (unsigned)s) : KEY_NONE);
    }
  } else {
    cnt = nsample;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int s = t * 64 + lane;
      key[t] = KEY_NONE;
      if (s < nsample) {
        const int j = min(max(grow[s], 0), n - 1);
        const float m = slot_value<METRIC>(qx - cloud[(size_t)j * 3], qy - cloud[(size_t)j * 3 + 1], qz - cloud[(size_t)j * 3 + 2]);
        key[t] = ((u64)__float_as_uint(m) << 32) | (unsigned)s;
      }
    }
  }
  // `keep` rounds of "the least key at or above the last winner + 1"; keep <= nsample, so a round never comes up empty
  u64 lo = 0, mine = KEY_NONE;
  for (int r = 0; r < keep; ++r) {
    u64 best = KEY_NONE;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const u64 c = key[t] >= lo ? key[t] : KEY_NONE;
      best = c < best ? c : best;
    }
    const u64 w = wave_min_u64(best);
    if (lane == r) mine = w;
    lo = w + 1;
  }
  double term = 0.0;
  if (lane < keep) {
    const int slot = (int)(unsigned)(mine & 0xffffffffu);
    const int src = (slot >= 0 && slot < cnt) ? slot : 0;
    const int j = KNN ? min(max(grow[src], 0), n - 1) : sj[wave][src];
    const float m = __uint_as_float((unsigned)(mine >> 32));
    const float v = METRIC == METRIC_ROOT ? sqrtf(m + 1e-12f) : m;
    if (live) {
      val[q * keep + lane] = v;
      idx[q * keep + lane] = j;
    }
    if (tail != TAIL_NONE) {
      float c = 0.f;
      if (lane > 0) {
        const double dx = (double)qx - (double)cloud[(size_t)j * 3], dy = (double)qy - (double)cloud[(size_t)j * 3 + 1],
                     dz = (double)qz - (double)cloud[(size_t)j * 3 + 2];
        const double vd = slot_value_d<METRIC>(dx, dy, dz);
        if (tail == TAIL_HINGE) {                        // max(0, h - v)
          const double t = h - vd;
          term = t > 0.0 ? t : 0.0;
          c = t > 0.0 ? -1.f : 0.f;
        } else {                                         // rterm - sqrt(w) * exp(-w / h^2), w = max(1e-12, v)
          const double w = vd > 1e-12 ? vd : 1e-12;
          const double s = sqrt(w), e = exp(-w / (h * h));
          term = rterm - s * e;
          c = vd > 1e-12 ? (float)(s * e / (h * h) - e / (2.0 * s)) : 0.f;
        }
      }
      if (live) coef[q * keep + lane] = c;
    }
  }
  if (tail != TAIL_NONE) {                               // wave-uniform
    double tsum = 0.0;
    for (int r = 1; r < keep; ++r) tsum += __shfl(term, r);
    if (lane == 0) wsum[wave] = live ? tsum : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      double a = wsum[0];
#pragma unroll
      for (int w = 1; w < PL_WAVES; ++w) a += wsum[w];
      partial[blockIdx.x] = a;
    }
  }
}

__global__ __launch_bounds__(PL_REDUCE_THREADS) void loss_reduce_kernel(const double* __restrict__ partial, int count, double inv,
                                                                        float* __restrict__ out) {
  __shared__ double sh[PL_REDUCE_THREADS];
  const int t = threadIdx.x;
  double a = 0.0;
#pragma unroll 8
  for (int k = t; k < count; k += PL_REDUCE_THREADS) a += partial[k];
  sh[t] = a;
  __syncthreads();
  for (int o = PL_REDUCE_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) out[0] = (float)(sh[0] * inv);
}

// acc += c * g(d), g the metric's derivative in the difference d
template <int METRIC>
__device__ __forceinline__ void add_term(double& ax, double& ay, double& az, double c, double dx, double dy, double dz) {
  if (METRIC == METRIC_SQ) {
    ax += c * (2.0 * dx); ay += c * (2.0 * dy); az += c * (2.0 * dz);
  } else if (METRIC == METRIC_L1) {
    ax += c * (dx > 0.0 ? 1.0 : (dx < 0.0 ? -1.0 : 0.0));
    ay += c * (dy > 0.0 ? 1.0 : (dy < 0.0 ? -1.0 : 0.0));
    az += c * (dz > 0.0 ? 1.0 : (dz < 0.0 ? -1.0 : 0.0));
  } else {
    const double r = sqrt(((dx * dx + dy * dy) + dz * dz) + 1e-12);
    ax += c * (dx / r); ay += c * (dy / r); az += c * (dz / r);
  }
}

// One table entry that names point i: the term of slot e = (ip, t), the query ip's side negated
template <int METRIC>
__device__ __forceinline__ void add_incoming(double& ax, double& ay, double& az, const float* __restrict__ cloud, const float* __restrict__ ctab,
                                             int e, int keep, double px, double py, double pz) {
  const int ip = e / keep;
  add_term<METRIC>(ax, ay, az, -(double)ctab[e], (double)cloud[(size_t)ip * 3] - px, (double)cloud[(size_t)ip * 3 + 1] - py,
                   (double)cloud[(size_t)ip * 3 + 2] - pz);
}

// 64 points per workgroup.  KEEP > 0: compile-time row length; 0: `keep` at run time.
// CSR: one wave; the incoming terms come from spgan_gather_csr's lists.  Otherwise PL_BWD_PARTS waves, wave w walks part w of the cloud's
// index table, staged in LDS PL_BWD_CHUNK entries at a time, eight entries per step, and the parts are added in ascending order.
template <int METRIC, int KEEP, bool CSR>
__global__ __launch_bounds__(64 * (CSR ? 1 : PL_BWD_PARTS)) void nearest_bwd_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ idx,
                                                                                    const float* __restrict__ coef,
                                                                                    const float* __restrict__ gscale, float scale, int n,
                                                                                    int keep_rt, const int32_t* __restrict__ rowptr,
                                                                                    const int32_t* __restrict__ slots, float* __restrict__ dxyz) {
  __shared__ double part[PL_BWD_PARTS - 1][3][64];
  __shared__ __attribute__((aligned(16))) int stab[CSR ? 8 : PL_BWD_CHUNK];
  const int keep = KEEP > 0 ? KEEP : keep_rt;
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int i0 = blockIdx.x * 64 + lane;
  const bool live = i0 < n;
  const int i = live ? i0 : -1;                          // matches no table entry
  const float* cloud = xyz + (size_t)b * n * 3;
  const int32_t* tab = idx + (size_t)b * n * keep;
  const float* ctab = coef + (size_t)b * n * keep;
  double ax = 0.0, ay = 0.0, az = 0.0;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (live) {
    px = cloud[(size_t)i * 3]; py = cloud[(size_t)i * 3 + 1]; pz = cloud[(size_t)i * 3 + 2];
  }
  if (live && w == 0) {
    for (int t = 0; t < keep; ++t) {
      const int j = min(max(tab[(size_t)i * keep + t], 0), n - 1);
      add_term<METRIC>(ax, ay, az, (double)ctab[(size_t)i * keep + t], px - (double)cloud[(size_t)j * 3], py - (double)cloud[(size_t)j * 3 + 1],
                       pz - (double)cloud[(size_t)j * 3 + 2]);
    }
  }
  if (CSR) {
    if (live) {
      const size_t row = (size_t)b * n + i;
      const long S = (long)n * keep;
      for (int e = rowptr[2 * row], e1 = rowptr[2 * row + 1]; e < e1; ++e) {
        const long s = (long)slots[e] - (long)b * S;
        if (s >= 0 && s < S) add_incoming<METRIC>(ax, ay, az, cloud, ctab, (int)s, keep, px, py, pz);
      }
    }
  } else {
    const int S = n * keep;                              // < 2^31: checked by the launcher
    for (int c0 = 0; c0 < S; c0 += PL_BWD_CHUNK) {       // the table, PL_BWD_CHUNK entries at a time through LDS; wave w takes part w of each
      const int len = min(PL_BWD_CHUNK, S - c0), len8 = (len + 7) & ~7;
      __syncthreads();
      for (int e = threadIdx.x; e < len8; e += 64 * PL_BWD_PARTS) stab[e] = e < len ? tab[c0 + e] : -2;      // -2 names no point
      __syncthreads();
      const int per = ((len8 / 8 + PL_BWD_PARTS - 1) / PL_BWD_PARTS) * 8;
      const int e0 = min(len8, w * per), e1 = min(len8, e0 + per);
      for (int e = e0; e < e1; e += 8) {
        const int4 lo = *reinterpret_cast<const int4*>(&stab[e]), hi = *reinterpret_cast<const int4*>(&stab[e + 4]);
        const int a[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        bool any = false;
#pragma unroll
        for (int u = 0; u < 8; ++u) any = any | (a[u] == i);
        if (!any) continue;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (a[u] == i) add_incoming<METRIC>(ax, ay, az, cloud, ctab, c0 + e + u, keep, px, py, pz);
      }
    }
    if (w > 0) {
      part[w - 1][0][lane] = ax; part[w - 1][1][lane] = ay; part[w - 1][2][lane] = az;
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int k = 0; k < PL_BWD_PARTS - 1; ++k) {
        ax += part[k][0][lane]; ay += part[k][1][lane]; az += part[k][2][lane];
      }
    }
  }
  if (live && w == 0) {
    const double f = (gscale ? (double)gscale[0] : 1.0) * (double)scale;
    float* o = dxyz + ((size_t)b * n + i) * 3;
    o[0] = (float)(ax * f); o[1] = (float)(ay * f); o[2] = (float)(az * f);
  }
}

template <int METRIC, bool KNN>
void launch_nearest_m(hipStream_t s, dim3 grid, const float* xyz, const int32_t* group, int n, long total, float radius, int nsample, int keep,
                      int tail, double h, double rterm, float* val, int32_t* idx, float* coef, double* partial) {
  const dim3 block(PL_WAVES * 64);
  if (nsample <= 64)
    hipLaunchKernelGGL((nearest_kernel<METRIC, KNN, 1>), grid, block, 0, s, xyz, group, n, total, radius, nsample, keep, tail, h, rterm, val, idx,
                       coef, partial);
  else if (nsample <= 128)
    hipLaunchKernelGGL((nearest_kernel<METRIC, KNN, 2>), grid, block, 0, s, xyz, group, n, total, radius, nsample, keep, tail, h, rterm, val, idx,
                       coef, partial);
  else
    hipLaunchKernelGGL((nearest_kernel<METRIC, KNN, 4>), grid, block, 0, s, xyz, group, n, total, radius, nsample, keep, tail, h, rterm, val, idx,
                       coef, partial);
}

template <int METRIC, bool CSR>
void launch_bwd_m(hipStream_t s, dim3 grid, const float* xyz, const int32_t* idx, const float* coef, const float* gscale, float scale, int n,
                  int keep, const int32_t* rowptr, const int32_t* slots, float* dxyz) {
  const dim3 block(64 * (CSR ? 1 : PL_BWD_PARTS));
  if (keep == 5)
    hipLaunchKernelGGL((nearest_bwd_kernel<METRIC, 5, CSR>), grid, block, 0, s, xyz, idx, coef, gscale, scale, n, keep, rowptr, slots, dxyz);
  else if (keep == 6)
    hipLaunchKernelGGL((nearest_bwd_kernel<METRIC, 6, CSR>), grid, block, 0, s, xyz, idx, coef, gscale, scale, n, keep, rowptr, slots, dxyz);
  else
    hipLaunchKernelGGL((nearest_bwd_kernel<METRIC, 0, CSR>), grid, block, 0, s, xyz, idx, coef, gscale, scale, n, keep, rowptr, slots, dxyz);
}

bool sizes_ok(int B, int n, int keep) {
  return B >= 1 && B <= 65535 && n >= 1 && keep >= 2 && keep <= PL_MAX_KEEP && (size_t)B * n < 2147483647u / 8;
}

}  // namespace

extern "C" int spgan_point_losses_partials(int B, int n) {
  if (B < 1 || n < 1) return 0;
  return cdiv((long)B * n, PL_WAVES);
}

extern "C" int spgan_point_losses_fwd(const float* xyz, const int32_t* knn_idx, int B, int n, int nsample, float radius, int metric, int keep,
                                      int tail, double h, double rterm, float* val, int32_t* idx, float* coef, double* partial, float* loss,
                                      spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz && val && idx && sizes_ok(B, n, keep));
  SPGAN_CHECK_ARG(metric >= METRIC_SQ && metric <= METRIC_ROOT && tail >= TAIL_NONE && tail <= TAIL_REP4);
  SPGAN_CHECK_ARG(nsample >= PL_MIN_NSAMPLE && keep <= nsample);
  if (knn_idx) SPGAN_CHECK_ARG(nsample <= PL_KNN_MAX_NSAMPLE && nsample <= n && (size_t)B * n * nsample < 2147483647u);
  else SPGAN_CHECK_ARG(nsample <= PL_MAX_NSAMPLE && radius > 0.f);                  // NaN fails the comparison
  if (tail != TAIL_NONE) SPGAN_CHECK_ARG(coef && partial && loss && h > 0.0);
  hipStream_t s = (hipStream_t)s_;
  const long total = (long)B * n;
  const dim3 grid(cdiv(total, PL_WAVES));
#define SPGAN_PL_LAUNCH(M)                                                                                                              \
  do {                                                                                                                                  \
    if (knn_idx) launch_nearest_m<M, true>(s, grid, xyz, knn_idx, n, total, radius, nsample, keep, tail, h, rterm, val, idx, coef, partial); \
    else launch_nearest_m<M, false>(s, grid, xyz, knn_idx, n, total, radius, nsample, keep, tail, h, rterm, val, idx, coef, partial);       \
  } while (0)
  if (metric == METRIC_SQ) SPGAN_PL_LAUNCH(METRIC_SQ);
  else if (metric == METRIC_L1) SPGAN_PL_LAUNCH(METRIC_L1);
  else SPGAN_PL_LAUNCH(METRIC_ROOT);
#undef SPGAN_PL_LAUNCH
  if (tail != TAIL_NONE)
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(PL_REDUCE_THREADS), 0, s, partial, (int)grid.x,
                       1.0 / ((double)total * (double)(keep - 1)), loss);
  return spgan_launch_status();
}

extern "C" int spgan_point_losses_bwd(const float* xyz, const int32_t* idx, const float* coef, const float* gscale, float scale, int B, int n,
                                      int keep, int metric, const int32_t* rowptr, const int32_t* slots, float* dxyz, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz && idx && coef && dxyz && sizes_ok(B, n, keep) && metric >= METRIC_SQ && metric <= METRIC_ROOT);
  SPGAN_CHECK_ARG((rowptr == nullptr) == (slots == nullptr));
  hipStream_t s = (hipStream_t)s_;
  const dim3 grid(cdiv(n, 64), B);
#define SPGAN_PL_BWD(M)                                                                                              \
  do {                                                                                                               \
    if (rowptr) launch_bwd_m<M, true>(s, grid, xyz, idx, coef, gscale, scale, n, keep, rowptr, slots, dxyz);         \
    else launch_bwd_m<M, false>(s, grid, xyz, idx, coef, gscale, scale, n, keep, rowptr, slots, dxyz);               \
  } while (0)
  if (metric == METRIC_SQ) SPGAN_PL_BWD(METRIC_SQ);
  else if (metric == METRIC_L1) SPGAN_PL_BWD(METRIC_L1);
  else SPGAN_PL_BWD(METRIC_ROOT);
#undef SPGAN_PL_BWD
  return spgan_launch_status();
}
