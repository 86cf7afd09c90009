// EXPERIMENT: what a register-only loop of v_mfma_f64_16x16x4_f64 reaches -- the ceiling csrc/frechet.hip's product is quoted against.
// Every wave keeps ACC independent accumulators and issues `iters` rounds of ACC MFMAs on loop-invariant operands: no LDS, no memory.
#include <hip/hip_runtime.h>

typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int ACC>
__global__ __launch_bounds__(256) void peak_kernel(double* __restrict__ out, int iters, double a0, double b0) {
  f64x4 acc[ACC];
#pragma unroll
  for (int j = 0; j < ACC; ++j) acc[j] = f64x4{0., 0., 0., 0.};
  const double a = a0 + 1e-9 * threadIdx.x, b = b0 - 1e-9 * threadIdx.x;
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int j = 0; j < ACC; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
  }
  double s = 0.;
#pragma unroll
  for (int j = 0; j < ACC; ++j) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  out[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}

// flop per launch = blocks * 4 waves * iters * acc * 2 * 16 * 16 * 4
extern "C" int exp_mfma_f64_peak(double* out, int blocks, int iters, int acc, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (acc == 1) hipLaunchKernelGGL(peak_kernel<1>, dim3(blocks), dim3(256), 0, s, out, iters, 1.0, 0.5);
  else if (acc == 2) hipLaunchKernelGGL(peak_kernel<2>, dim3(blocks), dim3(256), 0, s, out, iters, 1.0, 0.5);
  else if (acc == 4) hipLaunchKernelGGL(peak_kernel<4>, dim3(blocks), dim3(256), 0, s, out, iters, 1.0, 0.5);
  else return -22;
  return (int)hipGetLastError();
}
