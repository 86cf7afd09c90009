// MST expansion penalty and minimum-density sampling (metrics/expansion_penalty/expansion_penalty_cuda.cu, metrics/MDS/MDS_cuda.cu of the
// reference).  Both are sequential selections: Prim's algorithm over a primitive of p <= 512 consecutive points, and an iterative
// arg-min over a running density.  Nothing here uses a float atomic or an adjacency workspace, and every sum has a fixed order, so results
// repeat bit for bit.
//
// Expansion penalty.  p <= 256: one wave per primitive, EP_WAVES primitives per workgroup, no workgroup barrier anywhere.  p > 256: Prim's
// algorithm runs on a workgroup per primitive (one vertex per thread, one barrier per step), the rest on that workgroup's first wave.
// The two shapes share arithmetic, key and tie rule; what follows describes the one-wave shape:
//   * lane l owns the local vertices v = k*64 + l (k < V = ceil(p/64) rounded up to 1, 2 or 4) with their coordinates, cur_dis and
//     parent in registers; the coordinates also sit in LDS, so the winner's are one uniform-address read;
//   * a Prim step is the lanes' update, a local arg-min and a six-step DPP reduction over one 64-bit key
//     (float bits of cur_dis) << 32 | (1023 - v): distances are non-negative, so the integer minimum is the least distance and, among
//     exact ties, the HIGHEST vertex index (the reference's reduction tree keeps the higher index on a tie).  A candidate's parent changes
//     only on a strictly smaller distance.  Edge length: sqrtf((dx*dx + dy*dy) + dz*dz), every operation rounded on its own;
//   * order of the primitive's sum of edge lengths (w[v] = length of the edge that attached v, w[0] = 0, absent vertices 0):
//       lane partial s_l = (..((w[l] + w[64+l]) + w[128+l]) + ..) ascending k, then for o = 32, 16, 8, 4, 2, 1: s_l = s_l + s_{l^o};
//     mean = s / (float)(p-1);
//   * mean_mst_length[b] (second launch, one wave per cloud, from prim_mean_ws): lane partial over the primitives j = l, l+64, .. in
//     ascending order, the same butterfly, then / (float)(n/p);
//   * leaf peeling in synchronous rounds on cnt[v] (remaining degree) and xr[v] (XOR of the remaining neighbours' indices) in LDS: a
//     round first reads (every leaf t: u = xr[t], cnt[u]), then updates (LDS integer atomics, which commute).  Leaf t takes its edge when
//     cnt[u] > 1, or cnt[u] == 1 and t > u; the edge's cost is w[t] when u is t's parent, else w[u].
//
// Minimum-density sampling, one 1024-thread workgroup per cloud, one barrier per selected point: thread i owns the points
// k = r*1024 + i with their densities in registers (n <= 16384) and their coordinates in registers (n <= 8192), in LDS (n <= 13600) or
// re-read from global memory; beyond 16384 points the densities live in density_ws.  The arg-min key is (float bits of T) << 32 | k --
// T >= 0, so the minimum is the least density and, among exact ties, the LOWEST index.  Each wave's winner leaves key and coordinates in
// LDS (two buffers, alternating), every thread reduces the 16 records.
#include "common.hpp"

// Every float expression below is evaluated as written.  mul_rn / add_rn are this file's own, defined under the pragma: __fmul_rn and
// __fadd_rn are inline functions of a header compiled with contraction allowed, and once inlined their product and sum fuse into v_fma_f32.
#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

namespace {

constexpr int EP_WAVES = 4;      // primitives per workgroup
constexpr int EP_MAXP = 512;
constexpr int EP_WAVE_MAX_P = 256;   // larger primitives: one workgroup per primitive for Prim's algorithm (measured: DESIGN 31)
typedef unsigned long long u64;

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One step of the wave minimum: every lane takes the smaller of its key and the key of the lane the DPP control names.
template <int CTRL>
__device__ __forceinline__ u64 dpp_min_step(u64 k) {
  const int lo = (int)(unsigned)k, hi = (int)(unsigned)(k >> 32);
  const unsigned tlo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);   // lanes without a source keep their own
  const unsigned thi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const u64 t = ((u64)thi << 32) | tlo;
  return t < k ? t : k;
}

// Minimum of a 64-bit key over the wave, in registers (no LDS round trips), returned wave-uniform.  All 64 lanes must be active.
__device__ __forceinline__ u64 wave_min_u64(u64 k) {
  k = dpp_min_step<0xb1>(k);     // quad_perm [1,0,3,2]: lane ^ 1
  k = dpp_min_step<0x4e>(k);     // quad_perm [2,3,0,1]: lane ^ 2
  k = dpp_min_step<0x141>(k);    // row_half_mirror: the other quad of the 8
  k = dpp_min_step<0x140>(k);    // row_mirror: the other 8 of the row -> every lane holds its row's minimum
  k = dpp_min_step<0x142>(k);    // row_bcast15: rows 1 and 3 take in rows 0 and 2
  k = dpp_min_step<0x143>(k);    // row_bcast31: row 3 takes in rows 0 and 1 -> lane 63 holds the wave's minimum
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
  return ((u64)hi << 32) | lo;
}

// What follows Prim's algorithm, by ONE wave that holds the tree in registers (lane l: vertices k*64 + l with cur[k] = w, par[k]): the mean,
// the synchronous leaf peeling on cnt / xr in LDS, the threshold and the stores.
template <int V>
__device__ __forceinline__ void finish_primitive(const float (&cur)[V], const int (&par)[V], int lane, int p, int prim, int base_in_cloud, size_t base,
                                                 float alpha, float* ws, int* cnt, int* xr, float* __restrict__ dist,
                                                 int32_t* __restrict__ assignment, float* __restrict__ prim_mean) {
  // the primitive's mean edge length, in the order stated at the top of the file
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int v = k * 64 + lane;
    const float w = v < p ? cur[k] : 0.f;
    s = k == 0 ? w : add_rn(s, w);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = add_rn(s, __shfl_xor(s, o));
  const float mean = s / (float)(p - 1);
  if (lane == 0) prim_mean[prim] = mean;
  const float thr = mul_rn(mean, alpha);

  // remaining degree and XOR of the remaining neighbours
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int v = k * 64 + lane;
    if (v < p) {
      ws[v] = cur[k];
      cnt[v] = v > 0 ? 1 : 0;
      xr[v] = v > 0 ? par[k] : 0;
    }
  }
  wave_sync();
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int v = k * 64 + lane;
    if (v < p && v > 0) {
      atomicAdd(&cnt[par[k]], 1);
      atomicXor(&xr[par[k]], v);
    }
  }
  wave_sync();

  float od[V];
  int oa[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { od[k] = 0.f; oa[k] = -1; }
  int remaining = p - 1;
  for (int round = 0; round < p && remaining > 0; ++round) {
    unsigned leaf = 0, take = 0, drop = 0;
    int un[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int v = k * 64 + lane;
      un[k] = 0;
      if (v < p && cnt[v] == 1) {
        const int u = xr[v] & (EP_MAXP - 1);
        const int cu = u < p ? cnt[u] : 0;
        un[k] = u;
        leaf |= 1u << k;
        if (cu > 1) { take |= 1u << k; drop |= 1u << k; }
        else if (cu == 1 && v > u) take |= 1u << k;
      }
    }
    wave_sync();                                      // every read of the round precedes every update
    int taken = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int v = k * 64 + lane;
      if (leaf >> k & 1u) {
        const int u = un[k];
        cnt[v] = 0;
        if (drop >> k & 1u) {
          atomicAdd(&cnt[u], -1);
          atomicXor(&xr[u], v);
        }
        if (take >> k & 1u) {
          const float c = (u == par[k] && v > 0) ? cur[k] : ws[u];
          if (c > thr) { od[k] = c; oa[k] = base_in_cloud + u; }
        }
      }
      taken += __popcll(__ballot((take >> k & 1u) != 0));
    }
    wave_sync();
    remaining -= taken;
    if (taken == 0) break;                            // cannot happen on a tree; ends the loop on anything else
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int v = k * 64 + lane;
    if (v < p) {
      dist[base + v] = od[k];
      assignment[base + v] = oa[k];
    }
  }
}

template <int V>
__global__ __launch_bounds__(EP_WAVES * 64) void expansion_fwd_kernel(const float* __restrict__ xyz, int n, int p, int nprim_total, float alpha,
                                                                      float* __restrict__ dist, int32_t* __restrict__ assignment,
                                                                      float* __restrict__ prim_mean) {
  __shared__ float xs_all[EP_WAVES][V * 64 * 3];
  __shared__ float ws_all[EP_WAVES][V * 64];
  __shared__ int cnt_all[EP_WAVES][V * 64];
  __shared__ int xr_all[EP_WAVES][V * 64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int prim = blockIdx.x * EP_WAVES + wv;       // global primitive: cloud * (n/p) + primitive of the cloud
  if (prim >= nprim_total) return;                    // whole waves leave; no workgroup barrier follows
  float* xs = xs_all[wv];
  float* ws = ws_all[wv];
  int* cnt = cnt_all[wv];
  int* xr = xr_all[wv];
  const size_t base = (size_t)prim * p;               // = b*n + base_in_cloud
  const int base_in_cloud = (prim % (n / p)) * p;
  const float* src = xyz + base * 3;
  for (int e = lane; e < p * 3; e += 64) xs[e] = src[e];
  wave_sync();

  float px[V], py[V], pz[V], cur[V];
  int par[V];
  unsigned vis = 0;                                   // bit k: vertex k*64 + lane is in the tree (or does not exist)
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int v = k * 64 + lane;
    const bool ok = v < p;
    px[k] = ok ? xs[v * 3] : 0.f;
    py[k] = ok ? xs[v * 3 + 1] : 0.f;
    pz[k] = ok ? xs[v * 3 + 2] : 0.f;
    cur[k] = __builtin_inff();
    par[k] = 0;
    if (!ok || v == 0) vis |= 1u << k;
  }
  if (lane == 0) cur[0] = 0.f;                        // w[0] = 0

  int last = 0;
  for (int step = 1; step < p; ++step) {
    const float lx = xs[last * 3], ly = xs[last * 3 + 1], lz = xs[last * 3 + 2];
    u64 best = ~0ull;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (!(vis >> k & 1u)) {
        const int v = k * 64 + lane;
        const float dx = px[k] - lx, dy = py[k] - ly, dz = pz[k] - lz;
        const float d = sqrtf(add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)));
        if (d < cur[k]) { cur[k] = d; par[k] = last; }
        const u64 key = ((u64)__float_as_uint(cur[k]) << 32) | (unsigned)(1023 - v);
        best = key < best ? key : best;
      }
    }
    best = wave_min_u64(best);
    last = 1023 - (int)(unsigned)(best & 0xffffffffu);     // an unvisited vertex of this primitive: p-1 steps, p-1 unvisited vertices
    last = min(max(last, 0), p - 1);
    if ((last & 63) == lane) vis |= 1u << (last >> 6);
  }

  finish_primitive<V>(cur, par, lane, p, prim, base_in_cloud, base, alpha, ws, cnt, xr, dist, assignment, prim_mean);
}

// p > EP_WAVE_MAX_P: one 512-thread workgroup per primitive, one vertex per thread, for Prim's algorithm only -- per step a DPP minimum per
// wave, one record per wave in LDS (two alternating buffers), ONE barrier, every thread reduces the eight records.  The tree then goes
// through LDS to the first wave, which finishes as above while the other waves leave (no barrier follows).  Same arithmetic, key and tie
// rule as the one-wave kernel: the results are bit-identical (tools/exp/expansion_shapes.hip asserts it on the tree).
__global__ __launch_bounds__(512) void expansion_fwd_wg_kernel(const float* __restrict__ xyz, int n, int p, float alpha, float* __restrict__ dist,
                                                               int32_t* __restrict__ assignment, float* __restrict__ prim_mean) {
  __shared__ float xs[EP_MAXP * 3];
  __shared__ float ws[EP_MAXP];
  __shared__ int cnt[EP_MAXP];
  __shared__ int xr[EP_MAXP];
  __shared__ int pars[EP_MAXP];
  __shared__ u64 rec[2][EP_MAXP / 64];
  const int prim = blockIdx.x, v = threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t base = (size_t)prim * p;
  const int base_in_cloud = (prim % (n / p)) * p;
  const float* src = xyz + base * 3;
  for (int e = v; e < p * 3; e += EP_MAXP) xs[e] = src[e];
  __syncthreads();
  const bool ok = v < p;
  const float px = ok ? xs[v * 3] : 0.f, py = ok ? xs[v * 3 + 1] : 0.f, pz = ok ? xs[v * 3 + 2] : 0.f;
  float cur1 = v == 0 ? 0.f : __builtin_inff();
  int par1 = 0;
  bool vis = !ok || v == 0;
  int last = 0;
  for (int step = 1; step < p; ++step) {
    const float lx = xs[last * 3], ly = xs[last * 3 + 1], lz = xs[last * 3 + 2];
    u64 key = ~0ull;
    if (!vis) {
      const float dx = px - lx, dy = py - ly, dz = pz - lz;
      const float d = sqrtf(add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)));
      if (d < cur1) { cur1 = d; par1 = last; }
      key = ((u64)__float_as_uint(cur1) << 32) | (unsigned)(1023 - v);
    }
    const u64 wbest = wave_min_u64(key);
    const int buf = step & 1;
    if (lane == 0) rec[buf][wv] = wbest;
    __syncthreads();
    u64 g = rec[buf][0];
#pragma unroll
    for (int i = 1; i < EP_MAXP / 64; ++i) {
      const u64 o = rec[buf][i];
      g = o < g ? o : g;
    }
    last = min(max(1023 - (int)(unsigned)(g & 0xffffffffu), 0), p - 1);
    if (last == v) vis = true;
  }
  ws[v] = cur1;
  pars[v] = par1;
  __syncthreads();
  if (wv != 0) return;
  constexpr int V = EP_MAXP / 64;
  float cur[V];
  int par[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    cur[k] = ws[k * 64 + lane];
    par[k] = pars[k * 64 + lane];
  }
  wave_sync();
  finish_primitive<V>(cur, par, lane, p, prim, base_in_cloud, base, alpha, ws, cnt, xr, dist, assignment, prim_mean);
}

// mean_mst_length[b] = (sum of the cloud's primitive means, fixed order) / (n/p); one wave per cloud
__global__ __launch_bounds__(64) void expansion_mean_kernel(const float* __restrict__ prim_mean, int nprim, float* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* m = prim_mean + (size_t)b * nprim;
  float s = 0.f;
  for (int j = lane; j < nprim; j += 64) s = j < 64 ? m[j] : add_rn(s, m[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = add_rn(s, __shfl_xor(s, o));
  if (lane == 0) out[b] = s / (float)nprim;
}

// grad_xyz[b,j] = 2 * grad_dist[b,j] * (xyz[b,j] - xyz[b, assignment[b,j]]), 0 where assignment is -1.  One writer per element.
__global__ void expansion_bwd_kernel(const float* __restrict__ xyz, const float* __restrict__ grad_dist, const int32_t* __restrict__ assignment,
                                     int n, size_t total, float* __restrict__ grad_xyz) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int a = assignment[t];
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (a >= 0 && a < n) {
    const size_t o = (t / n) * n + a;
    const float g = grad_dist[t] * 2.f;
    gx = g * (xyz[t * 3] - xyz[o * 3]);
    gy = g * (xyz[t * 3 + 1] - xyz[o * 3 + 1]);
    gz = g * (xyz[t * 3 + 2] - xyz[o * 3 + 2]);
  }
  grad_xyz[t * 3] = gx;
  grad_xyz[t * 3 + 1] = gy;
  grad_xyz[t * 3 + 2] = gz;
}

constexpr int MDS_THREADS = 1024;
constexpr int MDS_WAVES = MDS_THREADS / 64;
constexpr int MDS_LDS_POINTS = (160 * 1024 - 640) / 12;   // 13600

// R > 0: n <= R * 1024 and the densities live in registers; R == 0: any n, densities in `dens_ws` (global).
// COORD 0: the thread's coordinates in registers too (R <= 8); 1: the cloud's coordinates in dynamic LDS (12 n bytes); 2: re-read from global.
template <int R, int COORD>
__global__ __launch_bounds__(MDS_THREADS) void mds_kernel(const float* __restrict__ xyz, int n, int npoint, const float* __restrict__ mean_mst_length,
                                                          int split, int32_t* __restrict__ out, float* __restrict__ dens_ws) {
  __shared__ u64 skey[2][MDS_WAVES];
  __shared__ float sxyz[2][MDS_WAVES][3];
  extern __shared__ float lxyz[];                    // COORD == 1 only
  constexpr int RR = R > 0 ? R : 1;
  constexpr int PR = COORD == 0 ? RR : 1;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* x = xyz + (size_t)b * n * 3;
  float* dens = R > 0 ? nullptr : dens_ws + (size_t)b * n;
  const float L = mean_mst_length[b];
  const float t = (float)(5.0 * (double)L * (double)L);     // the reference evaluates 5.0 * L * L in double and rounds once
  float px[PR], py[PR], pz[PR], T[RR];
  if (COORD == 0) {
#pragma unroll
    for (int r = 0; r < PR; ++r) {
      const int k = r * MDS_THREADS + tid;
      const bool ok = k < n;
      px[r] = ok ? x[(size_t)k * 3] : 0.f;
      py[r] = ok ? x[(size_t)k * 3 + 1] : 0.f;
      pz[r] = ok ? x[(size_t)k * 3 + 2] : 0.f;
    }
  } else if (COORD == 1) {
    for (int e = tid; e < n * 3; e += MDS_THREADS) lxyz[e] = x[e];
    __syncthreads();
  }
  if (R > 0) {
#pragma unroll
    for (int r = 0; r < RR; ++r) T[r] = (r == 0 && tid == 0) ? 1e9f : 0.f;
  } else {
    for (int k = tid; k < n; k += MDS_THREADS) dens[k] = k == 0 ? 1e9f : 0.f;
  }
  if (tid == 0) out[(size_t)b * npoint] = 0;
  float cx = x[0], cy = x[1], cz = x[2];
  for (int j = 1; j < npoint; ++j) {
    u64 best = ~0ull;
    float bx = 0.f, by = 0.f, bz = 0.f;
    const int rounds = R > 0 ? RR : (n + MDS_THREADS - 1) / MDS_THREADS;
#pragma unroll
    for (int r = 0; r < rounds; ++r) {
      const int k = r * MDS_THREADS + tid;
      if (k < n) {
        float qx, qy, qz;
        if (COORD == 0) { qx = px[r % PR]; qy = py[r % PR]; qz = pz[r % PR]; }
        else if (COORD == 1) { qx = lxyz[k * 3]; qy = lxyz[k * 3 + 1]; qz = lxyz[k * 3 + 2]; }
        else { qx = x[(size_t)k * 3]; qy = x[(size_t)k * 3 + 1]; qz = x[(size_t)k * 3 + 2]; }
        const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
        const float d = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
        const float e = expf(-d / t);
        const float v = add_rn(R > 0 ? T[r % RR] : dens[k], k < split ? e : e * 2.0f);
        if (R > 0) T[r % RR] = v; else dens[k] = v;
        const u64 key = ((u64)__float_as_uint(v) << 32) | (unsigned)k;
        if (key < best) { best = key; bx = qx; by = qy; bz = qz; }
      }
    }
    const u64 wbest = wave_min_u64(best);
    const int buf = j & 1;
    if (best == wbest && best != ~0ull) {              // keys are distinct (they carry k): one lane per wave
      skey[buf][wv] = best;
      sxyz[buf][wv][0] = bx; sxyz[buf][wv][1] = by; sxyz[buf][wv][2] = bz;
    } else if (wbest == ~0ull && lane == 0) {
      skey[buf][wv] = ~0ull;
    }
    __syncthreads();
    u64 g = skey[buf][0];
    int gw = 0;
#pragma unroll
    for (int w = 1; w < MDS_WAVES; ++w) {
      const u64 o = skey[buf][w];
      if (o < g) { g = o; gw = w; }
    }
    int sel = (int)(unsigned)(g & 0xffffffffu);
    sel = min(max(sel, 0), n - 1);
    cx = sxyz[buf][gw][0]; cy = sxyz[buf][gw][1]; cz = sxyz[buf][gw][2];
    if (tid == 0) out[(size_t)b * npoint + j] = sel;
    if ((sel & (MDS_THREADS - 1)) == tid) {            // the owner of `sel`, also in the R == 0 sweep
      if (R > 0) {
#pragma unroll
        for (int r = 0; r < RR; ++r)
          if (r == sel / MDS_THREADS) T[r] = 1e9f;
      } else {
        dens[sel] = 1e9f;
      }
    }
  }
}

// out[b,c,j] = feat[b,c,idx[b,j]]; an index outside [0,N) gives 0 and sets *bad
__global__ void gather_points_cm_kernel(const float* __restrict__ feat, const int32_t* __restrict__ idx, int C, int N, int m, size_t total,
                                        float* __restrict__ out, int* __restrict__ bad) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int j = t % m;
  const size_t bc = t / m;
  const size_t b = bc / C;
  const int i = idx[b * m + j];
  if (i < 0 || i >= N) {
    if (bad) atomicOr(bad, 1);
    out[t] = 0.f;
    return;
  }
  out[t] = feat[bc * N + i];
}

// dfeat[b,c,i] = sum over the slots e of point (b,i) (ascending, spgan_gather_csr) of dout[b,c,e - b*m]
__global__ void gather_points_cm_bwd_kernel(const float* __restrict__ dout, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                            int C, int N, int m, size_t total, float* __restrict__ dfeat) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int i = t % N;
  const size_t bc = t / N;
  const size_t b = bc / C;
  const size_t row = b * N + i;
  float acc = 0.f;
  for (int e = rowptr[2 * row], e1 = rowptr[2 * row + 1]; e < e1; ++e) {
    const long j = (long)src[e] - (long)(b * m);
    if (j >= 0 && j < m) acc += dout[bc * m + j];
  }
  dfeat[t] = acc;
}

}  // namespace

extern "C" int spgan_expansion_penalty_fwd(const float* xyz, int B, int n, int primitive_size, float alpha, float* dist, int32_t* assignment,
                                           float* mean_mst_length, float* prim_mean_ws, spgan_stream_t s_) {
  const int p = primitive_size;
  SPGAN_CHECK_ARG(xyz && dist && assignment && mean_mst_length && prim_mean_ws);
  SPGAN_CHECK_ARG(B >= 1 && n >= 1 && p >= 2 && p <= EP_MAXP && n % p == 0 && (size_t)B * n < 2147483647u / 3);
  const int nprim = n / p, total = B * nprim;
  const dim3 grid(cdiv(total, EP_WAVES)), block(EP_WAVES * 64);
  hipStream_t s = (hipStream_t)s_;
  if (p <= 64) hipLaunchKernelGGL((expansion_fwd_kernel<1>), grid, block, 0, s, xyz, n, p, total, alpha, dist, assignment, prim_mean_ws);
  else if (p <= 128) hipLaunchKernelGGL((expansion_fwd_kernel<2>), grid, block, 0, s, xyz, n, p, total, alpha, dist, assignment, prim_mean_ws);
  else if (p <= EP_WAVE_MAX_P) hipLaunchKernelGGL((expansion_fwd_kernel<4>), grid, block, 0, s, xyz, n, p, total, alpha, dist, assignment, prim_mean_ws);
  else hipLaunchKernelGGL(expansion_fwd_wg_kernel, dim3(total), dim3(EP_MAXP), 0, s, xyz, n, p, alpha, dist, assignment, prim_mean_ws);
  hipLaunchKernelGGL(expansion_mean_kernel, dim3(B), dim3(64), 0, s, prim_mean_ws, nprim, mean_mst_length);
  return spgan_launch_status();
}

extern "C" int spgan_expansion_penalty_bwd(const float* xyz, const float* grad_dist, const int32_t* assignment, int B, int n, float* grad_xyz,
                                           spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz && grad_dist && assignment && grad_xyz && B >= 1 && n >= 1 && (size_t)B * n < 2147483647u / 3);
  const size_t total = (size_t)B * n;
  hipLaunchKernelGGL(expansion_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, xyz, grad_dist, assignment, n, total, grad_xyz);
  return spgan_launch_status();
}

extern "C" int spgan_minimum_density_sample_needs_ws(int n) { return n > 16 * MDS_THREADS ? 1 : 0; }

extern "C" int spgan_minimum_density_sample(const float* xyz, int B, int n, int npoint, const float* mean_mst_length, int split, int32_t* out,
                                            float* density_ws, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz && mean_mst_length && out && B >= 1 && n >= 1 && npoint >= 1 && npoint <= n && (size_t)B * n < 2147483647u / 3);
  SPGAN_CHECK_ARG(density_ws || !spgan_minimum_density_sample_needs_ws(n));
  hipStream_t s = (hipStream_t)s_;
  const dim3 grid(B), block(MDS_THREADS);
#define SPGAN_MDS_LAUNCH(R, COORD, LDS) \
  hipLaunchKernelGGL((mds_kernel<R, COORD>), grid, block, LDS, s, xyz, n, npoint, mean_mst_length, split, out, density_ws)
  const size_t lds = (size_t)n * 3 * sizeof(float);
  if (n <= 1 * MDS_THREADS) SPGAN_MDS_LAUNCH(1, 0, 0);
  else if (n <= 2 * MDS_THREADS) SPGAN_MDS_LAUNCH(2, 0, 0);
  else if (n <= 4 * MDS_THREADS) SPGAN_MDS_LAUNCH(4, 0, 0);
  else if (n <= 8 * MDS_THREADS) SPGAN_MDS_LAUNCH(8, 0, 0);
  else if (n <= MDS_LDS_POINTS) {                    // densities in registers, coordinates in LDS: 12 n + 640 bytes <= 160 KB
    static LdsOptIn opt;
    opt.ensure(reinterpret_cast<const void*>(&mds_kernel<16, 1>), 160 * 1024 - 640);
    SPGAN_MDS_LAUNCH(16, 1, lds);
  } else if (n <= 16 * MDS_THREADS) SPGAN_MDS_LAUNCH(16, 2, 0);
  else SPGAN_MDS_LAUNCH(0, 2, 0);
#undef SPGAN_MDS_LAUNCH
  return spgan_launch_status();
}

extern "C" int spgan_gather_points_cm(const float* feat, const int32_t* idx, int B, int C, int N, int m, float* out, int32_t* bad,
                                      spgan_stream_t s_) {
  SPGAN_CHECK_ARG(feat && idx && out && B >= 1 && C >= 1 && N >= 1 && m >= 1);
  const size_t total = (size_t)B * C * m;
  SPGAN_CHECK_ARG(cdiv(total, 256) > 0 && total / 256 < 2147483647u);
  hipLaunchKernelGGL(gather_points_cm_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, feat, idx, C, N, m, total, out, (int*)bad);
  return spgan_launch_status();
}

extern "C" int spgan_gather_points_cm_bwd(const float* dout, const int32_t* rowptr, const int32_t* src, int B, int C, int N, int m, float* dfeat,
                                          spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dout && rowptr && src && dfeat && B >= 1 && C >= 1 && N >= 1 && m >= 1);
  const size_t total = (size_t)B * C * N;
  SPGAN_CHECK_ARG(total / 256 < 2147483647u);
  hipLaunchKernelGGL(gather_points_cm_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)s_, dout, rowptr, src, C, N, m, total, dfeat);
  return spgan_launch_status();
}
