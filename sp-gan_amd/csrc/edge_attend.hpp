// Shared by the EdgeBlock attention-backward kernels (edge.hip: dT read from memory; edge_dt.hip: dT formed in the launch's MFMA
// accumulators): the XCD-aware block order and the per-element arithmetic.  Both kernels compile the SAME expressions, so their g2, gy
// and statistics records agree bit for bit.
#pragma once
#include "common.hpp"

// XCD-aware workgroup order for the gather kernels: the hardware deals consecutive workgroup ids round-robin to the 8 XCDs, each with its own
// 4 MB L2.  In launch order, neighbouring point chunks -- which gather the same rows of the [B*N, H+2F] point tensor, 2.6 MB per shape at
// F = 128 -- would sit on eight different L2s and every shape's rows would be fetched eight times.  Logical block xcd * per + t runs on XCD
// xcd: an XCD works through a CONTIGUOUS eighth of the points (4 shapes at B = 32), whose rows it fetches once.  Grids are rounded up to a
// multiple of 8; logical blocks past the end find no points.
// Measured in the replayed step (profiles/r04_step_sequence.txt): edge_stats 65 -> 43-51 us, edge_attend_bwd 280 -> 272, edge_scatter 237 -> 228
// (9.24 -> 9.18-9.20 ms/step on one box); the same order changed nothing for the kNN scan and the per-edge-operand GEMM (not kept there).
__device__ __forceinline__ int xcd_block() {
  const int per = gridDim.x >> 3;
  return (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
}
inline int grid8(long n) { return (int)((n + 7) / 8 * 8); }

// One (point, channel) of the attention backward over the point's K edges: channel q of the lane's VEC.
//   hp[r][q] = h2pre, d[r][q] = dT, yp[r][q] = Q_j on entry (left as the pre-activation (R_i + Q_j) + bx), Ri = R_i;
//   a2/c2, ax/cx: BatchNorm scale/shift of conv_w.4 / conv_x.1; m2/i2, mxm/ixv: their mean / inverse standard deviation.
//   o2[r][q] / oy[r][q]: gradients w.r.t. the two BatchNorm outputs; s0..s3 += (g2, g2*xhat2, gy, gy*xhaty) in edge order.
//   FUSED_SUMS: the plain sums s0 / s2 take the last product of g2 / gy unrounded (one fma) instead of adding the stored value.  That is
//   how the one-channel-per-lane kernels of edge.hip (VEC = 1) have always been compiled, while the two-channel kernel (VEC = 2) adds the
//   rounded product; each keeps its rounding, and edge_dt.hip follows the two-channel kernel it replaces.
template <int K, int VEC, bool FUSED_SUMS>
__device__ __forceinline__ void edge_attend_bwd_elem(int q, const float (&hp)[K][VEC], const float (&d)[K][VEC], float (&yp)[K][VEC],
                                                     const float (&Ri)[VEC], const float (&a2)[VEC], const float (&c2)[VEC], const float (&ax)[VEC],
                                                     const float (&cx)[VEC], const float (&bb)[VEC], const float (&m2)[VEC], const float (&i2)[VEC],
                                                     const float (&mxm)[VEC], const float (&ixv)[VEC], float slope, float (&o2)[K][VEC],
                                                     float (&oy)[K][VEC], float (&s0)[VEC], float (&s1)[VEC], float (&s2)[VEC], float (&s3)[VEC]) {
  // Every fused multiply-add is written out and the compiler forms no other: which products it would fuse depends on how the code around
  // the call vectorises, and kernels that share a route must round alike.
#pragma clang fp contract(off)
  float e[K], mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < K; ++r) {
    e[r] = lrelu_f(fmaf(hp[r][q], a2[q], c2[q]), slope);
    mx = fmaxf(mx, e[r]);
  }
  float den = 0.f;
#pragma unroll
  for (int r = 0; r < K; ++r) {
    e[r] = expf(e[r] - mx);
    den += e[r];
  }
  const float rden = 1.0f / den;
  float dot = 0.f;
#pragma unroll
  for (int r = 0; r < K; ++r) {
    yp[r][q] = (Ri[q] + yp[r][q]) + bb[q];
    e[r] *= rden;
    const float yv = lrelu_f(fmaf(yp[r][q], ax[q], cx[q]), slope);
    dot = fmaf(d[r][q] * yv, e[r], dot);
  }
#pragma unroll
  for (int r = 0; r < K; ++r) {
    const float z2 = fmaf(hp[r][q], a2[q], c2[q]);
    const float zy = fmaf(yp[r][q], ax[q], cx[q]);
    const float yv = lrelu_f(zy, slope);
    const float ds = e[r] * fmaf(d[r][q], yv, -dot);
    const float k2 = lrelu_mask(z2, slope), ky = lrelu_mask(zy, slope), de = d[r][q] * e[r];
    const float v2 = ds * k2;
    const float vy = de * ky;
    o2[r][q] = v2; oy[r][q] = vy;
    s0[q] = FUSED_SUMS ? fmaf(ds, k2, s0[q]) : s0[q] + v2;
    s1[q] = fmaf(v2, (hp[r][q] - m2[q]) * i2[q], s1[q]);
    s2[q] = FUSED_SUMS ? fmaf(de, ky, s2[q]) : s2[q] + vy;
    s3[q] = fmaf(vy, (yp[r][q] - mxm[q]) * ixv[q], s3[q]);
  }
}
