// The tail of the bilateral / deform blocks (Generation/modules.py:928-1391) behind an edge convolution: BatchNorm1d + LeakyReLU over the
// layer's channel-major output Y [B,C,L] and the concatenation with the broadcast global vectors, as one pass over Y.
//   spgan_cm_stats              (sum, centred M2) of every row (b, c) of Y: records [B][C][2] for spgan_colstats_finalize_bn (tile_rows = L)
//   spgan_block_tail_fwd        out_x = cat[xs broadcast, a], out_g = cat[g broadcast, a], a = lrelu(scale * Y + shift): Y read once
//   spgan_block_tail_bwd_reduce (sum gact, sum gact * yhat) per row and the row sums of the broadcast channels' cotangents
//   spgan_block_tail_bwd_apply  dY from gact, recomputed from the cotangents by the same device function: the masked gradient is never stored
// All four are HBM-bound streams without reuse: no LDS.  One wave owns one row (the L floats of one (b, c)) at a time and loops over it,
// the waves of the grid stride over the rows; a row's sum is its lanes' partial sums combined by a butterfly, so results do not depend
// on the grid and repeat bit for bit.  Rows that start 16-byte aligned with L % 4 == 0 move as 16-byte pieces, anything else by scalars:
// decided once per launch (template parameter).  No float atomics.
#include "common.hpp"

namespace {

constexpr int WAVES = 4;          // per 256-thread workgroup
constexpr int MAX_BLOCKS = 2048;  // 256 CUs x 8 workgroups: the rest is grid-stride

template <bool VEC> struct Elem { typedef float type; };
template <> struct Elem<true> { typedef f32x4 type; };

__device__ __forceinline__ float hsum(float v) { return v; }
__device__ __forceinline__ float hsum(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ __forceinline__ float splat(float, float v) { return v; }
__device__ __forceinline__ f32x4 splat(f32x4, float v) { return f32x4{v, v, v, v}; }

__device__ __forceinline__ float act(float y, float sc, float sh, float slope) { return lrelu_f(fmaf(sc, y, sh), slope); }
__device__ __forceinline__ f32x4 act(f32x4 y, float sc, float sh, float slope) {
  return f32x4{act(y[0], sc, sh, slope), act(y[1], sc, sh, slope), act(y[2], sc, sh, slope), act(y[3], sc, sh, slope)};
}

// the cotangent of the BatchNorm output: the (up to three) cotangents of the activated tensor, summed in one order, times lrelu'
__device__ __forceinline__ float gact(float y, float dx, float dg, float ex, float sc, float sh, float slope) {
  return ((dx + dg) + ex) * lrelu_mask(fmaf(sc, y, sh), slope);
}
__device__ __forceinline__ f32x4 gact(f32x4 y, f32x4 dx, f32x4 dg, f32x4 ex, float sc, float sh, float slope) {
  return f32x4{gact(y[0], dx[0], dg[0], ex[0], sc, sh, slope), gact(y[1], dx[1], dg[1], ex[1], sc, sh, slope),
               gact(y[2], dx[2], dg[2], ex[2], sc, sh, slope), gact(y[3], dx[3], dg[3], ex[3], sc, sh, slope)};
}

// the row (b, c) of a [B, Ctot, L] tensor at channel offset c0 (NULL stays NULL)
template <class V>
__device__ __forceinline__ const V* row_of(const float* p, int b, int Ctot, int c, int L) {
  return p ? reinterpret_cast<const V*>(p + ((size_t)b * Ctot + c) * L) : nullptr;
}
template <class V>
__device__ __forceinline__ V* row_of(float* p, int b, int Ctot, int c, int L) {
  return p ? reinterpret_cast<V*>(p + ((size_t)b * Ctot + c) * L) : nullptr;
}

template <class V>
__device__ __forceinline__ float row_sum(const V* __restrict__ r, int n, int lane) {
  V a = splat(V{}, 0.f);
  for (int i = lane; i < n; i += 64) a += r[i];
  return wave_sum(hsum(a));
}

template <class V>
__device__ __forceinline__ void row_fill(V* __restrict__ r, int n, int lane, float v) {
  const V q = splat(V{}, v);
  for (int i = lane; i < n; i += 64) r[i] = q;
}

template <bool VEC>
__global__ __launch_bounds__(256) void cm_stats_kernel(const float* __restrict__ Y, int rows, int L, float* __restrict__ part) {
  typedef typename Elem<VEC>::type V;
  const int lane = threadIdx.x & 63, n = VEC ? L >> 2 : L;
  for (int t = blockIdx.x * WAVES + (threadIdx.x >> 6); t < rows; t += gridDim.x * WAVES) {
    const V* r = reinterpret_cast<const V*>(Y + (size_t)t * L);
    const float s = row_sum(r, n, lane);
    const V mean = splat(V{}, s / (float)L);
    V m2 = splat(V{}, 0.f);
    for (int i = lane; i < n; i += 64) {  // the row was just read: this pass is served by the cache
      const V d = r[i] - mean;
      m2 += d * d;
    }
    const float q = wave_sum(hsum(m2));
    if (lane == 0) {
      part[(size_t)t * 2] = s;
      part[(size_t)t * 2 + 1] = q;
    }
  }
}

// tasks per b: C data rows, then Csx fill rows of out_x, then Cgx fill rows of out_g
template <bool VEC>
__global__ __launch_bounds__(256) void block_tail_fwd_kernel(const float* __restrict__ Y, const float* __restrict__ xs, const float* __restrict__ g,
                                                             int B, int C, int L, int Cs, int Cg, int Csx, int Cgx, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, float slope, float* __restrict__ out_x,
                                                             float* __restrict__ out_g) {
  typedef typename Elem<VEC>::type V;
  const int lane = threadIdx.x & 63, n = VEC ? L >> 2 : L;
  const int per_b = C + Csx + Cgx, tasks = B * per_b;
  for (int t = blockIdx.x * WAVES + (threadIdx.x >> 6); t < tasks; t += gridDim.x * WAVES) {
    const int b = t / per_b, r = t - b * per_b;
    if (r < C) {
      const V* y = row_of<V>(Y, b, C, r, L);
      V* ox = row_of<V>(out_x, b, Cs + C, Cs + r, L);
      V* og = row_of<V>(out_g, b, Cg + C, Cg + r, L);
      const float sc = scale[r], sh = shift[r];
      for (int i = lane; i < n; i += 64) {
        const V a = act(y[i], sc, sh, slope);
        if (ox) ox[i] = a;
        if (og) og[i] = a;
      }
    } else if (r < C + Csx) {
      const int c = r - C;
      row_fill(row_of<V>(out_x, b, Cs + C, c, L), n, lane, xs[(size_t)b * Cs + c]);
    } else {
      const int c = r - C - Csx;
      row_fill(row_of<V>(out_g, b, Cg + C, c, L), n, lane, g[(size_t)b * Cg + c]);
    }
  }
}

// tasks per b: C data rows, then Csx rows of dout_x's broadcast channels, then Cgx rows of dout_g's
template <bool VEC>
__global__ __launch_bounds__(256) void block_tail_bwd_reduce_kernel(const float* __restrict__ Y, const float* __restrict__ dout_x,
                                                                    const float* __restrict__ dout_g, const float* __restrict__ extra, int B, int C,
                                                                    int L, int Cs, int Cg, int Csx, int Cgx, const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, float slope, const float* __restrict__ mean,
                                                                    const float* __restrict__ invstd, float* __restrict__ part,
                                                                    float* __restrict__ dxs, float* __restrict__ dg) {
  typedef typename Elem<VEC>::type V;
  const int lane = threadIdx.x & 63, n = VEC ? L >> 2 : L;
  const int per_b = C + Csx + Cgx, tasks = B * per_b;
  const V zero = splat(V{}, 0.f);
  for (int t = blockIdx.x * WAVES + (threadIdx.x >> 6); t < tasks; t += gridDim.x * WAVES) {
    const int b = t / per_b, r = t - b * per_b;
    if (r < C) {
      const V* y = row_of<V>(Y, b, C, r, L);
      const V* dx = row_of<V>(dout_x, b, Cs + C, Cs + r, L);
      const V* dgr = row_of<V>(dout_g, b, Cg + C, Cg + r, L);
      const V* ex = row_of<V>(extra, b, C, r, L);
      const float sc = scale[r], sh = shift[r], inv = invstd[r];
      const V mu = splat(V{}, mean[r]);
      V s0 = zero, s1 = zero;
      for (int i = lane; i < n; i += 64) {
        const V yv = y[i];
        const V ga = gact(yv, dx ? dx[i] : zero, dgr ? dgr[i] : zero, ex ? ex[i] : zero, sc, sh, slope);
        s0 += ga;
        s1 += ga * ((yv - mu) * inv);
      }
      const float t0 = wave_sum(hsum(s0)), t1 = wave_sum(hsum(s1));
      if (lane == 0) {
        float* o = part + ((size_t)b * C + r) * 2;
        o[0] = t0;
        o[1] = t1;
      }
    } else if (r < C + Csx) {
      const int c = r - C;
      const float s = dout_x ? row_sum(row_of<V>(dout_x, b, Cs + C, c, L), n, lane) : 0.f;
      if (lane == 0) dxs[(size_t)b * Cs + c] = s;
    } else {
      const int c = r - C - Csx;
      const float s = dout_g ? row_sum(row_of<V>(dout_g, b, Cg + C, c, L), n, lane) : 0.f;
      if (lane == 0) dg[(size_t)b * Cg + c] = s;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void block_tail_bwd_apply_kernel(const float* __restrict__ Y, const float* __restrict__ dout_x,
                                                                   const float* __restrict__ dout_g, const float* __restrict__ extra, int B, int C,
                                                                   int L, int Cs, int Cg, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, float slope, const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                   const float* __restrict__ sums, float rcount, float* __restrict__ dY) {
  typedef typename Elem<VEC>::type V;
  const int lane = threadIdx.x & 63, n = VEC ? L >> 2 : L;
  const int tasks = B * C;
  const V zero = splat(V{}, 0.f);
  for (int t = blockIdx.x * WAVES + (threadIdx.x >> 6); t < tasks; t += gridDim.x * WAVES) {
    const int b = t / C, r = t - b * C;
    const V* y = row_of<V>(Y, b, C, r, L);
    const V* dx = row_of<V>(dout_x, b, Cs + C, Cs + r, L);
    const V* dgr = row_of<V>(dout_g, b, Cg + C, Cg + r, L);
    const V* ex = row_of<V>(extra, b, C, r, L);
    V* o = row_of<V>(dY, b, C, r, L);
    const float sc = scale[r], sh = shift[r];
    if (sums) {  // train mode: the batch statistics depend on Y
      const float inv = invstd[r], p = (gamma ? gamma[r] : 1.f) * inv;
      const V mu = splat(V{}, mean[r]), m0 = splat(V{}, sums[r] * rcount), m1 = splat(V{}, sums[C + r] * rcount);
      for (int i = lane; i < n; i += 64) {
        const V yv = y[i];
        const V ga = gact(yv, dx ? dx[i] : zero, dgr ? dgr[i] : zero, ex ? ex[i] : zero, sc, sh, slope);
        o[i] = p * ((ga - m0) - ((yv - mu) * inv) * m1);
      }
    } else {
      for (int i = lane; i < n; i += 64)
        o[i] = sc * gact(y[i], dx ? dx[i] : zero, dgr ? dgr[i] : zero, ex ? ex[i] : zero, sc, sh, slope);
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }  // NULL counts as aligned
inline int grid_for(long tasks) { return (int)(tasks < (long)MAX_BLOCKS * WAVES ? (tasks + WAVES - 1) / WAVES : MAX_BLOCKS); }
inline bool sizes_ok(int B, int C, int L, int Cs, int Cg) {
  return B > 0 && C > 0 && L > 0 && Cs >= 0 && Cg >= 0 && (long)B * ((long)C + Cs + Cg) < (1L << 31) - MAX_BLOCKS * WAVES;
}

}  // namespace

extern "C" int spgan_cm_stats(const float* Y, int B, int C, int L, float* partials, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(Y && partials && sizes_ok(B, C, L, 0, 0));
  const int rows = B * C;
  if (L % 4 == 0 && aligned16(Y))
    hipLaunchKernelGGL(cm_stats_kernel<true>, dim3(grid_for(rows)), dim3(256), 0, (hipStream_t)s_, Y, rows, L, partials);
  else
    hipLaunchKernelGGL(cm_stats_kernel<false>, dim3(grid_for(rows)), dim3(256), 0, (hipStream_t)s_, Y, rows, L, partials);
  return spgan_launch_status();
}

extern "C" int spgan_block_tail_fwd(const float* Y, const float* xs, const float* g, int B, int C, int L, int Cs, int Cg, const float* scale,
                                    const float* shift, float slope, float* out_x, float* out_g, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(Y && scale && shift && (out_x || out_g) && sizes_ok(B, C, L, Cs, Cg));
  SPGAN_CHECK_ARG((!out_x || Cs == 0 || xs) && (!out_g || Cg == 0 || g));
  const int Csx = out_x ? Cs : 0, Cgx = out_g ? Cg : 0;
  const int grid = grid_for((long)B * (C + Csx + Cgx));
  if (L % 4 == 0 && aligned16(Y) && aligned16(out_x) && aligned16(out_g))
    hipLaunchKernelGGL(block_tail_fwd_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)s_, Y, xs, g, B, C, L, Cs, Cg, Csx, Cgx, scale, shift,
                       slope, out_x, out_g);
  else
    hipLaunchKernelGGL(block_tail_fwd_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)s_, Y, xs, g, B, C, L, Cs, Cg, Csx, Cgx, scale, shift,
                       slope, out_x, out_g);
  return spgan_launch_status();
}

extern "C" int spgan_block_tail_bwd_reduce(const float* Y, const float* dout_x, const float* dout_g, const float* extra, int B, int C, int L, int Cs,
                                           int Cg, const float* scale, const float* shift, float slope, const float* mean, const float* invstd,
                                           float* partials, float* dxs, float* dg, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(Y && scale && shift && mean && invstd && partials && sizes_ok(B, C, L, Cs, Cg));
  const int Csx = dxs ? Cs : 0, Cgx = dg ? Cg : 0;
  const int grid = grid_for((long)B * (C + Csx + Cgx));
  if (L % 4 == 0 && aligned16(Y) && aligned16(dout_x) && aligned16(dout_g) && aligned16(extra))
    hipLaunchKernelGGL(block_tail_bwd_reduce_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)s_, Y, dout_x, dout_g, extra, B, C, L, Cs, Cg,
                       Csx, Cgx, scale, shift, slope, mean, invstd, partials, dxs, dg);
  else
    hipLaunchKernelGGL(block_tail_bwd_reduce_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)s_, Y, dout_x, dout_g, extra, B, C, L, Cs, Cg,
                       Csx, Cgx, scale, shift, slope, mean, invstd, partials, dxs, dg);
  return spgan_launch_status();
}

extern "C" int spgan_block_tail_bwd_apply(const float* Y, const float* dout_x, const float* dout_g, const float* extra, int B, int C, int L, int Cs,
                                          int Cg, const float* scale, const float* shift, float slope, const float* mean, const float* invstd,
                                          const float* gamma, const float* sums, float count, float* dY, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(Y && scale && shift && dY && sizes_ok(B, C, L, Cs, Cg));
  SPGAN_CHECK_ARG(!sums || (mean && invstd && count > 0.f));
  const int grid = grid_for((long)B * C);
  const float rcount = sums ? 1.0f / count : 0.f;
  if (L % 4 == 0 && aligned16(Y) && aligned16(dout_x) && aligned16(dout_g) && aligned16(extra) && aligned16(dY))
    hipLaunchKernelGGL(block_tail_bwd_apply_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)s_, Y, dout_x, dout_g, extra, B, C, L, Cs, Cg, scale,
                       shift, slope, mean, invstd, gamma, sums, rcount, dY);
  else
    hipLaunchKernelGGL(block_tail_bwd_apply_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)s_, Y, dout_x, dout_g, extra, B, C, L, Cs, Cg, scale,
                       shift, slope, mean, invstd, gamma, sums, rcount, dY);
  return spgan_launch_status();
}
