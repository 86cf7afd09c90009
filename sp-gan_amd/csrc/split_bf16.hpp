// Exact split of fp32 values into three bfloat16 terms x = hi + mid + lo, and the 8-byte-per-plane LDS store of four consecutive k-values --
// shared by the split-bf16 kernels (gemm.hip's 128-row kernel, gemm_wide3.hip with W's split image, gemm_tn_wide3.hip).
// The contract (tests/kernel_model.py::_split_bf16x3 is its model):
//   finite x:  hi = RN(clamp(x, +-BF16_MAX)), mid = RN(x - hi), lo = x - hi - mid (round to nearest at each level, every residual exact).
//              Without the clamp a finite x at or above the bf16 overflow point (0x7f7f8000 .. FLT_MAX) would round hi to +-inf and leave a
//              residual of -+inf: NaN in the cross products.  x and the clamped hi share a binade, so the residual still fits mid + lo.
//              Where hi does not overflow the clamp changes nothing: those planes are what plain rounding gives.
//   x = +-inf: (+0, +0, +-inf); x = NaN: (+0, +0, NaN).  A non-finite value sits in lo, the one plane that meets only the partner's hi in the
//              six cross terms (lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi): inf * b is then +-inf * b_hi -- +-inf for every finite non-zero
//              b (the six terms never form inf * 0 from a zero mid or lo plane of b), NaN for b = 0 or NaN, as in fp32.  The one product fp32
//              gives and the split cannot: inf * inf, which meets only hi * lo and lo * hi = inf * 0 -> NaN.
// The kNN kernels' own copies of the plain split (graph.hip, knn_pipe.hip) keep the unclamped form: their distances square the features, so
// an input in the affected range overflows in fp32 as well.
#pragma once
#include "common.hpp"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

constexpr float BF16_MAX = 0x1.fep127f;   // the largest finite bfloat16 (0x7f7f)

// two fp32 values -> (hi, mid, lo) as packed bf16 pairs
__device__ __forceinline__ void split2(float x, float y, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
  // a non-finite value rounds to hi = mid = 0 and passes on through the residuals into lo (one class test per value serves both selects)
  const bool fx = __builtin_isfinite(x), fy = __builtin_isfinite(y);
  const f32x2v v = {fx ? __builtin_amdgcn_fmed3f(x, -BF16_MAX, BF16_MAX) : 0.f, fy ? __builtin_amdgcn_fmed3f(y, -BF16_MAX, BF16_MAX) : 0.f};
  const bf16x2 h = __builtin_convertvector(v, bf16x2);
  hi = *reinterpret_cast<const uint32_t*>(&h);
  const float rx = x - __uint_as_float(hi << 16), ry = y - __uint_as_float(hi & 0xffff0000u);
  const f32x2v r = {fx ? rx : 0.f, fy ? ry : 0.f};
  const bf16x2 m = __builtin_convertvector(r, bf16x2);
  mid = *reinterpret_cast<const uint32_t*>(&m);
  const f32x2v q = {rx - __uint_as_float(mid << 16), ry - __uint_as_float(mid & 0xffff0000u)};
  const bf16x2 l = __builtin_convertvector(q, bf16x2);
  lo = *reinterpret_cast<const uint32_t*>(&l);
}

// 4 consecutive k-values -> 8 bytes in each of the three planes (p points at the hi plane's slot, `plane` words between planes)
__device__ __forceinline__ void st_split4(uint32_t* p, int plane, float4 v) {
  uint32_t h0, m0, l0, h1, m1, l1;
  split2(v.x, v.y, h0, m0, l0);
  split2(v.z, v.w, h1, m1, l1);
  *reinterpret_cast<uint2*>(p) = make_uint2(h0, h1);
  *reinterpret_cast<uint2*>(p + plane) = make_uint2(m0, m1);
  *reinterpret_cast<uint2*>(p + 2 * plane) = make_uint2(l0, l1);
}

