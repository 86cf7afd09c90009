// The reference's square_distance arithmetic (Common/pointnet_util.py:19-40), shared by every kernel that must land on the same
// float32 value as its `-2ab + |a|^2 + |b|^2` form (golden G9): ball query, kNN, three_nn.
#pragma once
#include "common.hpp"

// ((-2*<a,b>) + |a|^2) + |b|^2 in fp32, products and sums rounded separately like torch's matmul/sum on 3-vectors.
template <int C>
__device__ __forceinline__ float sqdist_expanded(const float (&a)[C], float an, const float* __restrict__ b, float bn) {
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) dot = fmaf(a[c], b[c], dot);
  return (-2.f * dot + an) + bn;
}

__device__ __forceinline__ float norm2(const float* __restrict__ p, int C) {
  float s = 0.f;
  for (int c = 0; c < C; ++c) s = fmaf(p[c], p[c], s);
  return s;
}

// The same expanded form evaluated in float64 from the float32 coordinates (the products are then exact).  For consumers that divide the
// distance by a small number inside an exponent (the kernel density, pointconv_util.py:205-206): there the float32 form's cancellation
// error, about 2^-24 * (|a|^2 + |b|^2), is amplified by 1 / (2 h^2) and dominates everything computed from the result.
template <int C>
__device__ __forceinline__ double sqdist_expanded_f64(const float (&a)[C], double an, const double* __restrict__ b, double bn) {
  double dot = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) dot = fma((double)a[c], b[c], dot);
  return (-2.0 * dot + an) + bn;
}
