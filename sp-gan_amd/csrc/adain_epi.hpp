// SPGAN_EPI_ADAIN: AdaptivePointNorm applied in the epilogue of the style GEMM (gemm.hip's 128-row kernel in its 128-column
// configuration, gemm_wide.hip's 256 x 256-tile kernel).  The weight tile is staged so that a wave's two 32-column accumulator tiles
// hold gamma (j = 0) and beta (j = 1) of the SAME 32 channels: lane l of the wave has gamma[row, c] and beta[row, c] in the same
// register slot, and the epilogue is element-wise -- no exchange, [M, 2C] never reaches memory.  The expressions are those of the
// GEMM's bias add and of adain_fwd_kernel (pointwise.hip), so the bits are those of the three-launch chain.
#pragma once
#include "common.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// One wave's rows [wrow0, wrow0 + 32*TI) of channel c (this lane's column); on return acc[i][0] holds the stored output (what the
// pooling records are taken from).  GUARD: the tile may reach past row M or channel C (nothing is loaded or stored there).
template <int TI, bool GUARD>
__device__ __forceinline__ void adain_wave_epilogue(const spgan_gemm_nt_args& p, float* __restrict__ Y, f32x16 (&acc)[TI][2], int wrow0, int lh, int c) {
  const int C = p.N >> 1, N = p.ad_rows;
  const bool cok = !GUARD || c < C;
  const int cc = cok ? c : 0;
  const int rlast = GUARD ? min(wrow0 + TI * 32, p.M) - 1 : wrow0 + TI * 32 - 1;
  if (GUARD && rlast < wrow0) return;
  const float bg = p.bias ? p.bias[cc] : 0.f, bb = p.bias ? p.bias[C + cc] : 0.f;
  const float sl = p.ad_slope, eps = p.ad_eps;
  const int rbase = wrow0 + 4 * lh;
  const int b0 = wrow0 / N;
  const int g0 = p.ad_gamma ? p.ad_gamma_row0 : 0x7fffffff;   // gamma is stored for rows >= g0
  const bool gany = rlast >= g0;
  const unsigned ldy = (unsigned)p.ldy, ldx = (unsigned)p.ad_ldx, ldg = (unsigned)p.ad_ld_gamma;
  float* yb = Y + (size_t)rbase * ldy + cc;
#define AD_ROFF(r) (((r) & 3) + 8 * ((r) >> 2))   // C/D layout of v_mfma_f32_32x32x*: register r of lane l holds row AD_ROFF(r) + 4*(l >> 5)
  auto finish = [&](int i, int r, float xv, float mu, float rs) {
    const int row = rbase + i * 32 + AD_ROFF(r);
    const float gamma = acc[i][0][r] + bg, beta = acc[i][1][r] + bb;
    const float xh = (lrelu_f(xv, sl) - mu) * rs;
    const float o = fmaf(gamma, xh, beta);
    acc[i][0][r] = o;
    if (!GUARD || (cok && row <= rlast)) {
      if (gany && row >= g0) p.ad_gamma[(size_t)(row - g0) * ldg + cc] = gamma;
      yb[(size_t)((unsigned)(i * 32 + AD_ROFF(r)) * ldy)] = o;
    }
  };
  if (rlast < (b0 + 1) * N) {   // the wave's rows lie in one shape (always when ad_rows % 128 == 0): one (mean, var) pair per lane
    const float mu = p.ad_mean[(size_t)b0 * C + cc], rs = rsqrtf(p.ad_var[(size_t)b0 * C + cc] + eps);
    const float* xb = p.ad_x + (size_t)b0 * (size_t)p.ad_x_shape_stride + (size_t)(rbase - b0 * N) * ldx + cc;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      float xv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        xv[r] = (!GUARD || rbase + i * 32 + AD_ROFF(r) <= rlast) ? xb[(size_t)((unsigned)(i * 32 + AD_ROFF(r)) * ldx)] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) finish(i, r, xv[r], mu, rs);
    }
  } else {
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = min(rbase + i * 32 + AD_ROFF(r), rlast);   // (rows past the end repeat the last one: computed, not stored)
        const int b = row / N;
        const float xv = p.ad_x[(size_t)b * (size_t)p.ad_x_shape_stride + (size_t)(row - b * N) * ldx + cc];
        finish(i, r, xv, p.ad_mean[(size_t)b * C + cc], rsqrtf(p.ad_var[(size_t)b * C + cc] + eps));
      }
  }
}

// (max, min) and their rows over this lane's 16*TI rows of acc[.][0], merged with the other lane half: the record of the wave's rows.
// Rows ascend with (i, r) and strict compares keep the first; the lane halves merge by value, then by the lower row.
template <int TI>
__device__ __forceinline__ void adain_wave_extrema(const f32x16 (&acc)[TI][2], int rbase, float& vx, int& ax, float& vn, int& an) {
  vx = -INFINITY; vn = INFINITY;
  ax = 0x7fffffff; an = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = acc[i][0][r];
      const int row = rbase + i * 32 + AD_ROFF(r);
      if (v > vx) { vx = v; ax = row; }
      if (v < vn) { vn = v; an = row; }
    }
  const float ovx = __shfl_xor(vx, 32), ovn = __shfl_xor(vn, 32);
  const int oax = __shfl_xor(ax, 32), oan = __shfl_xor(an, 32);
  if (ovx > vx || (ovx == vx && oax < ax)) { vx = ovx; ax = oax; }
  if (ovn < vn || (ovn == vn && oan < an)) { vn = ovn; an = oan; }
}
