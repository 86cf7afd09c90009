// Device-side batch augmentation (include/spgan_hip.h, "Device-side batch augmentation").
// Launch 1, one workgroup per cloud: the cloud's parameter record and, with the permutation on, a bitonic sort of its 64-bit keys in LDS.
// Launch 2, one thread per output row: gather, xyz A + t, jitter, dropout, store in either layout; its first thread advances the counter.
#include "common.hpp"

namespace {

constexpr int AUG_MAX_N = 8192;          // 8192 keys x 8 B = 64 KB of LDS: what a workgroup gets without opting in
constexpr int AUG_APPLY_THREADS = 256;
constexpr float TWO_PI_F = 6.2831853f;

struct Philox4 { uint32_t x[4]; };

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

struct Stream {           // seed, step and the batch slot: everything of a Philox call but purpose and element
  uint32_t k0, k1, s0, s1, b;
  __device__ Philox4 at(uint32_t purpose, uint32_t e) const { return philox4x32_10(e, (purpose << 24) | b, s0, s1, k0, k1); }
  __device__ uint32_t word(uint32_t purpose, uint32_t w) const {          // selects, not an indexed array: that would live in scratch / LDS
    const Philox4 d = at(purpose, w >> 2);
    const uint32_t q = w & 3;
    return q == 0 ? d.x[0] : q == 1 ? d.x[1] : q == 2 ? d.x[2] : d.x[3];
  }
};

__device__ __forceinline__ float uni(uint32_t x) { return (float)(x >> 8) * 0x1p-24f; }
// Box-Muller: (r cos th, r sin th)
__device__ __forceinline__ void normal2(uint32_t xa, uint32_t xb, float& g0, float& g1) {
  const float u1 = (float)((xa >> 8) + 1u) * 0x1p-24f;
  const float r = sqrtf(-2.f * logf(u1));
  float s, c;
  sincosf(TWO_PI_F * uni(xb), &s, &c);
  g0 = r * c; g1 = r * s;
}
__device__ __forceinline__ float clipf(float v, float c) { return fminf(fmaxf(v, -c), c); }

struct M3 { float m[9]; };
__device__ inline M3 m3_identity() { return M3{{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}}; }
__device__ inline M3 m3_mul(const M3& a, const M3& b) {
  M3 o;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o.m[3 * r + c] = a.m[3 * r] * b.m[c] + a.m[3 * r + 1] * b.m[3 + c] + a.m[3 * r + 2] * b.m[6 + c];
  return o;
}
__device__ inline M3 m3_t(const M3& a) { return M3{{a.m[0], a.m[3], a.m[6], a.m[1], a.m[4], a.m[7], a.m[2], a.m[5], a.m[8]}}; }
// Rz Ry Rx of the angles about x, y, z (provider.py's matrices)
__device__ inline M3 m3_euler(float ax, float ay, float az) {
  float sx, cx, sy, cy, sz, cz;
  sincosf(ax, &sx, &cx); sincosf(ay, &sy, &cy); sincosf(az, &sz, &cz);
  const M3 rx{{1.f, 0.f, 0.f, 0.f, cx, -sx, 0.f, sx, cx}};
  const M3 ry{{cy, 0.f, sy, 0.f, 1.f, 0.f, -sy, 0.f, cy}};
  const M3 rz{{cz, -sz, 0.f, sz, cz, 0.f, 0.f, 0.f, 1.f}};
  return m3_mul(rz, m3_mul(ry, rx));
}
// data_utils.angle_axis: c I + s [u]x + (1 - c) u u^T
__device__ inline M3 m3_axis(float a, const float* u) {
  float s, c;
  sincosf(a, &s, &c);
  const float k = 1.f - c;
  return M3{{c + k * u[0] * u[0], -s * u[2] + k * u[0] * u[1], s * u[1] + k * u[0] * u[2],
             s * u[2] + k * u[1] * u[0], c + k * u[1] * u[1], -s * u[0] + k * u[1] * u[2],
             -s * u[1] + k * u[2] * u[0], s * u[0] + k * u[2] * u[1], c + k * u[2] * u[2]}};
}

// ---------------------------------------------------------------------------------------- launch 1
__global__ void augment_prepare_kernel(spgan_augment_cfg cfg, int N, int npad, uint32_t k0, uint32_t k1, const unsigned long long* step,
                                       const uint32_t* __restrict__ keys, const float* __restrict__ params, int32_t* __restrict__ perm,
                                       float* __restrict__ rec) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long skey[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned long long st = *step;
  const Stream rng{k0, k1, (uint32_t)st, (uint32_t)(st >> 32), (uint32_t)b};

  if (tid == 0) {
    float* r = rec + (size_t)b * 16;
    const Philox4 d0 = rng.at(0, 0);
    float a[9], t[3] = {0.f, 0.f, 0.f};
    if (params) {
      const float* p = params + (size_t)b * 16;
      for (int i = 0; i < 9; ++i) a[i] = p[i];
      for (int i = 0; i < 3; ++i) t[i] = p[9 + i];
    } else {
      M3 m = m3_identity();
      if (cfg.rotate) {
        const M3 rm = cfg.rotate == 1 ? m3_axis(TWO_PI_F * uni(d0.x[0]), cfg.axis)
                                      : m3_euler(TWO_PI_F * uni(d0.x[0]), TWO_PI_F * uni(d0.x[1]), TWO_PI_F * uni(d0.x[2]));
        m = cfg.transpose ? m3_t(rm) : rm;
      }
      if (cfg.perturb) {
        const Philox4 d1 = rng.at(0, 1);
        float g0, g1, g2, g3;
        normal2(d1.x[0], d1.x[1], g0, g1);
        normal2(d1.x[2], d1.x[3], g2, g3);
        const M3 pm = m3_euler(clipf(cfg.perturb_sigma * g0, cfg.perturb_clip), clipf(cfg.perturb_sigma * g1, cfg.perturb_clip),
                               clipf(cfg.perturb_sigma * g2, cfg.perturb_clip));
        m = m3_mul(m, cfg.transpose ? m3_t(pm) : pm);
      }
      float sc[3] = {1.f, 1.f, 1.f};
      if (cfg.scale) {
        const Philox4 d2 = rng.at(0, 2);
        const float w = cfg.scale_hi - cfg.scale_lo;
        sc[0] = cfg.scale_lo + w * uni(d2.x[0]);
        sc[1] = cfg.scale == 2 ? cfg.scale_lo + w * uni(d2.x[1]) : sc[0];
        sc[2] = cfg.scale == 2 ? cfg.scale_lo + w * uni(d2.x[2]) : sc[0];
      }
      for (int i = 0; i < 9; ++i) a[i] = m.m[i] * sc[i % 3];
      if (cfg.translate) {
        const Philox4 d3 = rng.at(0, 3);
        t[0] = (2.f * uni(d3.x[0]) - 1.f) * cfg.translate_range;
        t[1] = cfg.translate == 1 ? (2.f * uni(d3.x[1]) - 1.f) * cfg.translate_range : t[0];
        t[2] = cfg.translate == 1 ? (2.f * uni(d3.x[2]) - 1.f) * cfg.translate_range : t[0];
      }
    }
    for (int i = 0; i < 9; ++i) r[i] = a[i];
    for (int i = 0; i < 3; ++i) r[9 + i] = t[i];
    r[12] = cfg.dropout ? uni(d0.x[3]) * cfg.dropout_max : 0.f;
    r[13] = __uint_as_float((uint32_t)st);
    r[14] = __uint_as_float((uint32_t)(st >> 32));
    r[15] = 0.f;
  }
  if (!cfg.permute) return;          // uniform over the grid

  // keys (draw << 32) | index are distinct, so the network's order is the stable order; the padding sorts behind every key
  for (int i = tid; i < npad; i += blockDim.x) {
    unsigned long long k = ~0ull;
    if (i < N) {
      const uint32_t d = keys ? keys[(size_t)b * N + i] : rng.word(1, (uint32_t)i);
      k = ((unsigned long long)d << 32) | (uint32_t)i;
    }
    skey[i] = k;
  }
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (npad >> 1); t += blockDim.x) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;          // the t-th pair at distance j
        const unsigned long long x = skey[lo], y = skey[hi];
        const bool up = (lo & k) == 0;
        if ((x > y) == up) { skey[lo] = y; skey[hi] = x; }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < N; i += blockDim.x) perm[(size_t)b * N + i] = (int32_t)(uint32_t)skey[i];
}

// ---------------------------------------------------------------------------------------- launch 2
struct Row { float v[6]; };

template <int C>
__device__ __forceinline__ Row final_row(const spgan_augment_cfg& cfg, const Stream& rng, const float* __restrict__ cloud, int src, int i,
                                         bool affine, const float* a, const float* t, const float* an) {
  Row o;
  if (cloud) {
#pragma unroll
    for (int c = 0; c < C; ++c) o.v[c] = cloud[(size_t)src * C + c];
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) o.v[c] = __uint_as_float(0x7fc00000u);
  }
  if (affine) {
    const float x = o.v[0], y = o.v[1], z = o.v[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) o.v[c] = x * a[c] + y * a[3 + c] + z * a[6 + c] + t[c];
    if (C == 6) {
      const float nx = o.v[3], ny = o.v[4], nz = o.v[5];
#pragma unroll
      for (int c = 0; c < 3; ++c) o.v[3 + c] = nx * an[c] + ny * an[3 + c] + nz * an[6 + c];
    }
  }
  if (cfg.jitter) {
    const Philox4 d = rng.at(2, (uint32_t)i);
    float j0, j1, j2, j3;
    normal2(d.x[0], d.x[1], j0, j1);
    normal2(d.x[2], d.x[3], j2, j3);
    o.v[0] += clipf(cfg.jitter_sigma * j0, cfg.jitter_clip);
    o.v[1] += clipf(cfg.jitter_sigma * j1, cfg.jitter_clip);
    o.v[2] += clipf(cfg.jitter_sigma * j2, cfg.jitter_clip);
  }
  return o;
}

template <int C>
__global__ void __launch_bounds__(AUG_APPLY_THREADS)
augment_apply_kernel(spgan_augment_cfg cfg, const float* __restrict__ data, long S, int P, const int64_t* __restrict__ index, int N,
                     int layout, int affine, uint32_t k0, uint32_t k1, unsigned long long* step, int advance,
                     const int32_t* __restrict__ perm, const float* __restrict__ rec, float* __restrict__ out) {
  const int b = blockIdx.y, i = blockIdx.x * AUG_APPLY_THREADS + threadIdx.x;
  const float* r = rec + (size_t)b * 16;
  const uint32_t s0 = __float_as_uint(r[13]), s1 = __float_as_uint(r[14]);
  if (advance && b == 0 && i == 0) *step = (((unsigned long long)s1 << 32) | s0) + 1ull;       // no thread of this launch reads *step
  if (i >= N) return;
  const Stream rng{k0, k1, s0, s1, (uint32_t)b};
  float a[9], t[3], an[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) a[q] = r[q];
#pragma unroll
  for (int q = 0; q < 3; ++q) t[q] = r[9 + q];
  if (C == 6 && affine) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float inv = 1.f / sqrtf(a[c] * a[c] + a[3 + c] * a[3 + c] + a[6 + c] * a[6 + c]);
      an[c] = a[c] * inv; an[3 + c] = a[3 + c] * inv; an[6 + c] = a[6 + c] * inv;
    }
  }
  const int64_t ci = index[b];
  const float* cloud = (ci >= 0 && ci < (int64_t)S) ? data + (size_t)ci * P * C : nullptr;
  int row = i;
  if (cfg.dropout && uni(rng.word(3, (uint32_t)i)) <= r[12]) row = 0;
  int src = cfg.permute ? perm[(size_t)b * N + row] : row;
  src = min(max(src, 0), N - 1);
  const Row o = final_row<C>(cfg, rng, cloud, src, row, affine != 0, a, t, an);
  if (layout == 0) {
    float* dst = out + ((size_t)b * N + i) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c] = o.v[c];
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) out[((size_t)b * C + c) * N + i] = o.v[c];
  }
}

__global__ void philox_fill_kernel(uint32_t k0, uint32_t k1, uint32_t c1, uint32_t s0, uint32_t s1, long n_words, uint32_t* __restrict__ out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e * 4 >= n_words) return;
  const Philox4 d = philox4x32_10((uint32_t)e, c1, s0, s1, k0, k1);
  for (int q = 0; q < 4 && e * 4 + q < n_words; ++q) out[e * 4 + q] = d.x[q];
}

}  // namespace

extern "C" int spgan_augment_max_points(void) { return AUG_MAX_N; }

extern "C" int spgan_augment_batch(const float* data, long S, int P, int C, const int64_t* index, int B, int N, int layout,
                                   const spgan_augment_cfg* cfg, unsigned long long seed, unsigned long long* step, int advance,
                                   const uint32_t* keys, const float* params, int32_t* perm_ws, float* out, float* rec, spgan_stream_t s) {
  SPGAN_CHECK_ARG(data && index && cfg && step && out && rec);
  SPGAN_CHECK_ARG(S >= 1 && P >= 1 && (C == 3 || C == 6) && B >= 1 && B < (1 << 24) && B <= 65535);
  SPGAN_CHECK_ARG(N >= 1 && N <= P && N <= AUG_MAX_N && (layout == 0 || layout == 1));
  SPGAN_CHECK_ARG(cfg->rotate >= 0 && cfg->rotate <= 2 && cfg->scale >= 0 && cfg->scale <= 2 && cfg->translate >= 0 && cfg->translate <= 2);
  SPGAN_CHECK_ARG(!cfg->permute || perm_ws);
  SPGAN_CHECK_ARG(!keys || cfg->permute);
  hipStream_t st = (hipStream_t)s;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  int npad = 2;
  while (npad < N) npad <<= 1;
  const int threads = cfg->permute ? (npad / 2 < 64 ? 64 : (npad / 2 > 1024 ? 1024 : npad / 2)) : 64;
  const size_t lds = cfg->permute ? (size_t)npad * sizeof(unsigned long long) : 0;
  hipLaunchKernelGGL(augment_prepare_kernel, dim3(B), dim3(threads), lds, st, *cfg, N, npad, k0, k1, step, keys, params, perm_ws, rec);
  const int affine = (params || cfg->rotate || cfg->perturb || cfg->scale || cfg->translate) ? 1 : 0;
  const dim3 grid(cdiv(N, AUG_APPLY_THREADS), B);
  if (C == 3)
    hipLaunchKernelGGL(augment_apply_kernel<3>, grid, dim3(AUG_APPLY_THREADS), 0, st, *cfg, data, S, P, index, N, layout, affine, k0, k1, step,
                       advance, perm_ws, rec, out);
  else
    hipLaunchKernelGGL(augment_apply_kernel<6>, grid, dim3(AUG_APPLY_THREADS), 0, st, *cfg, data, S, P, index, N, layout, affine, k0, k1, step,
                       advance, perm_ws, rec, out);
  return spgan_launch_status();
}

extern "C" int spgan_philox_fill(unsigned long long seed, int purpose, int slot, unsigned long long step, long n_words, uint32_t* out,
                                 spgan_stream_t s) {
  SPGAN_CHECK_ARG(out && n_words >= 1 && purpose >= 0 && purpose < 256 && slot >= 0 && slot < (1 << 24));
  const long calls = (n_words + 3) / 4;
  SPGAN_CHECK_ARG(calls <= 0xffffffffL);
  hipLaunchKernelGGL(philox_fill_kernel, dim3(cdiv(calls, 256)), dim3(256), 0, (hipStream_t)s, (uint32_t)seed, (uint32_t)(seed >> 32),
                     ((uint32_t)purpose << 24) | (uint32_t)slot, (uint32_t)step, (uint32_t)(step >> 32), n_words, out);
  return spgan_launch_status();
}
