// EXPERIMENT: what a register-only loop of expf reaches -- the ceiling csrc/approxmatch.hip's sweeps are quoted against.
// Every lane keeps ACC independent chains x <- expf(-x) (values stay in (0.36, 1]): no LDS, no memory.  fast != 0 uses __expf (the bare
// v_exp_f32 after one multiply), which the kernels do not use: its argument's rounding grows with |level * d2|.
#include <hip/hip_runtime.h>

template <int ACC, bool FAST>
__global__ __launch_bounds__(256) void exp_peak_kernel(float* __restrict__ out, int iters, float x0) {
  float x[ACC];
#pragma unroll
  for (int j = 0; j < ACC; ++j) x[j] = x0 + 1e-3f * (float)((threadIdx.x + 7 * j) & 255);
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int j = 0; j < ACC; ++j) x[j] = FAST ? __expf(-x[j]) : expf(-x[j]);
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < ACC; ++j) s += x[j];
  out[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}

// exp evaluations per launch = blocks * 256 * iters * acc
extern "C" int exp_exp_peak(float* out, int blocks, int iters, int acc, int fast, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (acc == 4 && !fast) hipLaunchKernelGGL((exp_peak_kernel<4, false>), dim3(blocks), dim3(256), 0, s, out, iters, 0.5f);
  else if (acc == 8 && !fast) hipLaunchKernelGGL((exp_peak_kernel<8, false>), dim3(blocks), dim3(256), 0, s, out, iters, 0.5f);
  else if (acc == 4 && fast) hipLaunchKernelGGL((exp_peak_kernel<4, true>), dim3(blocks), dim3(256), 0, s, out, iters, 0.5f);
  else if (acc == 8 && fast) hipLaunchKernelGGL((exp_peak_kernel<8, true>), dim3(blocks), dim3(256), 0, s, out, iters, 0.5f);
  else return -22;
  return (int)hipGetLastError();
}
