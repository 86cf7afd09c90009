// Experiment for DESIGN 31: Prim's algorithm of the expansion penalty in two kernel shapes, the tree only (edge length and parent per vertex).
//   exp_prim_wave: one wave per primitive, up to 8 vertices per lane -- the shape csrc/expansion.hip uses
//   exp_prim_wg:   one workgroup per primitive, one vertex per thread; per step a DPP minimum per wave, one record per wave in LDS
//                  (two alternating buffers), one barrier, every thread reduces the records
// Same arithmetic, key and tie rule in both, so w and parent must come out identical.  Built and timed by tools/exp/run_expansion_shapes.py.
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

typedef unsigned long long u64;

template <int CTRL>
__device__ __forceinline__ u64 dpp_min_step(u64 k) {
  const int lo = (int)(unsigned)k, hi = (int)(unsigned)(k >> 32);
  const unsigned tlo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const unsigned thi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const u64 t = ((u64)thi << 32) | tlo;
  return t < k ? t : k;
}

__device__ __forceinline__ u64 wave_min_u64(u64 k) {
  k = dpp_min_step<0xb1>(k);
  k = dpp_min_step<0x4e>(k);
  k = dpp_min_step<0x141>(k);
  k = dpp_min_step<0x140>(k);
  k = dpp_min_step<0x142>(k);
  k = dpp_min_step<0x143>(k);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ float edge_len(float dx, float dy, float dz) {
  return sqrtf(add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)));
}

template <int V>
__global__ __launch_bounds__(256) void prim_wave_kernel(const float* __restrict__ xyz, int p, int P, float* __restrict__ w, int* __restrict__ parent) {
  __shared__ float xs_all[4][V * 64 * 3];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int prim = blockIdx.x * 4 + wv;
  if (prim >= P) return;
  float* xs = xs_all[wv];
  const float* src = xyz + (size_t)prim * p * 3;
  for (int e = lane; e < p * 3; e += 64) xs[e] = src[e];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float px[V], py[V], pz[V], cur[V];
  int par[V];
  unsigned vis = 0;
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
  if (lane == 0) cur[0] = 0.f;
  int last = 0;
  for (int step = 1; step < p; ++step) {
    const float lx = xs[last * 3], ly = xs[last * 3 + 1], lz = xs[last * 3 + 2];
    u64 best = ~0ull;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (!(vis >> k & 1u)) {
        const int v = k * 64 + lane;
        const float d = edge_len(px[k] - lx, py[k] - ly, pz[k] - lz);
        if (d < cur[k]) { cur[k] = d; par[k] = last; }
        const u64 key = ((u64)__float_as_uint(cur[k]) << 32) | (unsigned)(1023 - v);
        best = key < best ? key : best;
      }
    }
    best = wave_min_u64(best);
    last = min(max(1023 - (int)(unsigned)(best & 0xffffffffu), 0), p - 1);
    if ((last & 63) == lane) vis |= 1u << (last >> 6);
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int v = k * 64 + lane;
    if (v < p) { w[(size_t)prim * p + v] = cur[k]; parent[(size_t)prim * p + v] = par[k]; }
  }
}

// blockDim.x = p rounded up to a multiple of 64 (<= 512)
__global__ __launch_bounds__(512) void prim_wg_kernel(const float* __restrict__ xyz, int p, float* __restrict__ w, int* __restrict__ parent) {
  __shared__ float xs[512 * 3];
  __shared__ u64 rec[2][8];
  const int prim = blockIdx.x, v = threadIdx.x, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const float* src = xyz + (size_t)prim * p * 3;
  for (int e = v; e < p * 3; e += blockDim.x) xs[e] = src[e];
  __syncthreads();
  const bool ok = v < p;
  const float px = ok ? xs[v * 3] : 0.f, py = ok ? xs[v * 3 + 1] : 0.f, pz = ok ? xs[v * 3 + 2] : 0.f;
  float cur = v == 0 ? 0.f : __builtin_inff();
  int par = 0;
  bool vis = !ok || v == 0;
  int last = 0;
  for (int step = 1; step < p; ++step) {
    const float lx = xs[last * 3], ly = xs[last * 3 + 1], lz = xs[last * 3 + 2];
    u64 key = ~0ull;
    if (!vis) {
      const float d = edge_len(px - lx, py - ly, pz - lz);
      if (d < cur) { cur = d; par = last; }
      key = ((u64)__float_as_uint(cur) << 32) | (unsigned)(1023 - v);
    }
    const u64 wbest = wave_min_u64(key);
    const int buf = step & 1;
    if ((v & 63) == 0) rec[buf][wv] = wbest;
    __syncthreads();
    u64 g = rec[buf][0];
    for (int i = 1; i < nw; ++i) {
      const u64 o = rec[buf][i];
      g = o < g ? o : g;
    }
    last = min(max(1023 - (int)(unsigned)(g & 0xffffffffu), 0), p - 1);
    if (last == v) vis = true;
  }
  if (ok) { w[(size_t)prim * p + v] = cur; parent[(size_t)prim * p + v] = par; }
}

extern "C" int exp_prim_wave(const float* xyz, int P, int p, float* w, int* parent, void* s_) {
  if (!xyz || !w || !parent || P < 1 || p < 2 || p > 512) return -22;
  const dim3 grid((P + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)s_;
  if (p <= 64) hipLaunchKernelGGL((prim_wave_kernel<1>), grid, block, 0, s, xyz, p, P, w, parent);
  else if (p <= 128) hipLaunchKernelGGL((prim_wave_kernel<2>), grid, block, 0, s, xyz, p, P, w, parent);
  else if (p <= 256) hipLaunchKernelGGL((prim_wave_kernel<4>), grid, block, 0, s, xyz, p, P, w, parent);
  else hipLaunchKernelGGL((prim_wave_kernel<8>), grid, block, 0, s, xyz, p, P, w, parent);
  return (int)hipGetLastError();
}

extern "C" int exp_prim_wg(const float* xyz, int P, int p, float* w, int* parent, void* s_) {
  if (!xyz || !w || !parent || P < 1 || p < 2 || p > 512) return -22;
  hipLaunchKernelGGL(prim_wg_kernel, dim3(P), dim3((p + 63) / 64 * 64), 0, (hipStream_t)s_, xyz, p, w, parent);
  return (int)hipGetLastError();
}
