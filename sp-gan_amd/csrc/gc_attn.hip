// Global-context attention (GC_attn, Common/utilities.py:357-426) in two passes over x per direction.  Per sample b
// over its L positions, x_n in R^C:
//   m_n = w . x_n + bias,  p = softmax_n(m)  (or p_n = 1/L: w == NULL),  ctx = sum_n p_n x_n,
//   add = branch(ctx),  mul = sigmoid(branch(ctx)),  branch = Conv1d(C,O) -> LayerNorm(O) -> ReLU -> Conv1d(O,C),  out_n = x_n * mul + add
//   spgan_gc_attn_pool_fwd     logits, an online softmax and the weighted sum from one read of x: one record (max, sum, ctx partial) per
//                              workgroup, combined in ascending chunk order by a second small launch
//   spgan_gc_attn_channel_fwd  both branches for every sample, one launch;  spgan_gc_attn_channel_bwd: their backward, one launch
//   spgan_gc_attn_apply_fwd    out = x * mul[b] + add[b]
//   spgan_gc_attn_bwd_reduce   dmul = sum_n g_n * x_n, dadd = sum_n g_n
//   spgan_gc_attn_bwd_apply    dx_n = g_n * mul + p_n dctx + s_n w,  s_n = p_n (dctx . x_n - dctx . ctx), and one record sum_n s_n x_n per workgroup
// Two layouts.  Channel-major [B,C,L] (layout 0): a workgroup owns CHUNK_CM consecutive positions of a sample.  pool_fwd and bwd_apply need
// a position's sum over all channels before any channel of it can be used: up to C = 484 they stage [C, 64] (or [C, 32]) tiles of x in
// LDS and read x from memory ONCE (pool_cm_lds_kernel, bwd_apply_cm_lds_kernel).  Wider C (485..1024) takes the two-walk kernels, in which
// the four waves split the channels, a lane holds four positions and the slab [C, CHUNK_CM] is loaded TWICE: there pool_fwd moves 2|x|
// and bwd_apply 4|x|.  Point-major rows [B*L, C] with a row stride >= C (layout 1): TPR = a power of two of lanes
// spans a row (16-byte pieces when C % 4 == 0, the strides are multiples of 4 and the bases aligned), 64 / TPR rows per wave step; a
// lane keeps its channels of the running sums in registers and a row is read once.  Every sum has a fixed order (lanes by butterfly,
// waves and row slots through LDS in ascending order, records in ascending chunk order): no float atomics, results repeat bit for bit.
#include <math.h>

#include "common.hpp"

namespace {

constexpr int WAVES = 4;          // per 256-thread workgroup
constexpr int CHUNK_CM = 256;     // positions per workgroup, channel-major: 64 lanes x 4
constexpr int CHUNK_PM = 128;     // rows per workgroup, point-major
constexpr int MAX_DIM = 1024;     // C and O
constexpr int MAX_BLOCKS = 2048;  // the wave-per-row kernels: 256 CUs x 8 workgroups, the rest is grid-stride
constexpr int MAXK_VEC = 4;       // pieces of a row one lane holds: 1024 / (4 * 64)
constexpr int MAXK_SCL = 16;      // 1024 / 64

template <bool VEC> struct Elem { typedef float type; };
template <> struct Elem<true> { typedef f32x4 type; };

__device__ __forceinline__ float hsum(float v) { return v; }
__device__ __forceinline__ float hsum(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ __forceinline__ float splat(float, float v) { return v; }
__device__ __forceinline__ f32x4 splat(f32x4, float v) { return f32x4{v, v, v, v}; }
__device__ __forceinline__ float hmax(f32x4 v) { return fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// the sum over the `tpr` lanes (a power of two) that share a row
__device__ __forceinline__ float group_sum(float v, int tpr) {
  for (int o = tpr >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ------------------------------------------------------------------------------------------------- channel-major: four positions per lane
// position (within the chunk) of element j of a lane
template <bool VEC> __device__ __forceinline__ int cm_pos(int lane, int j) { return VEC ? 4 * lane + j : lane + 64 * j; }

// row = the chunk's first position of one channel; valid = positions of the chunk inside the sample (a multiple of 4 when VEC)
template <bool VEC> __device__ __forceinline__ f32x4 cm_load(const float* __restrict__ row, int lane, int valid) {
  if (VEC) return 4 * lane < valid ? *reinterpret_cast<const f32x4*>(row + 4 * lane) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = lane + 64 * j < valid ? row[lane + 64 * j] : 0.f;
  return v;
}
template <bool VEC> __device__ __forceinline__ void cm_store(float* __restrict__ row, int lane, int valid, f32x4 v) {
  if (VEC) {
    if (4 * lane < valid) *reinterpret_cast<f32x4*>(row + 4 * lane) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lane + 64 * j < valid) row[lane + 64 * j] = v[j];
  }
}

// sum over the channels of coef[c] * x[c, positions of the lane]: each wave sums its channels, the four partial sums meet in LDS and
// every wave adds them in the same order, so all four hold the same values
template <bool VEC>
__device__ __forceinline__ f32x4 cm_channel_dot(const float* __restrict__ xb, size_t L, int C, const float* __restrict__ coef, int lane, int wave,
                                                int valid, float (*sp)[CHUNK_CM]) {
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int c = wave; c < C; c += WAVES) a += coef[c] * cm_load<VEC>(xb + (size_t)c * L, lane, valid);
#pragma unroll
  for (int j = 0; j < 4; ++j) sp[wave][4 * lane + j] = a[j];
  __syncthreads();
  f32x4 t;
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = (sp[0][4 * lane + j] + sp[1][4 * lane + j]) + (sp[2][4 * lane + j] + sp[3][4 * lane + j]);
  return t;
}

// record of a chunk: [0] = max logit, [1] = sum exp(m - max), [2 + c] = sum_n exp(m_n - max) x[c, n]   (average: max 0, weights 1)
template <bool VEC>
__global__ __launch_bounds__(256) void pool_cm_kernel(const float* __restrict__ x, int C, size_t L, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ part, float* __restrict__ m_out) {
  __shared__ float sp[WAVES][CHUNK_CM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t b = blockIdx.y, n0 = (size_t)blockIdx.x * CHUNK_CM;
  const int valid = (int)(L - n0 < (size_t)CHUNK_CM ? L - n0 : (size_t)CHUNK_CM);
  const float* xb = x + b * C * L + n0;
  float* rec = part + (b * gridDim.x + blockIdx.x) * (size_t)(C + 2);
  f32x4 p;
  float mx = 0.f, sum;
  if (w) {
    f32x4 m = cm_channel_dot<VEC>(xb, L, C, w, lane, wave, valid, sp);
    const float bs = bias ? bias[0] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = cm_pos<VEC>(lane, j) < valid;
      m[j] = in ? m[j] + bs : -INFINITY;
      if (in && wave == 0) m_out[b * L + n0 + cm_pos<VEC>(lane, j)] = m[j];
    }
    mx = wave_max(hmax(m));
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = expf(m[j] - mx);  // exp(-inf) = 0 outside the sample
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = cm_pos<VEC>(lane, j) < valid ? 1.f : 0.f;
  }
  sum = wave_sum(hsum(p));
  for (int c = wave; c < C; c += WAVES) {
    const f32x4 v = cm_load<VEC>(xb + (size_t)c * L, lane, valid);
    const float t = wave_sum(hsum(p * v));
    if (lane == 0) rec[2 + c] = t;
  }
  if (threadIdx.x == 0) {
    rec[0] = mx;
    rec[1] = sum;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void bwd_apply_cm_kernel(const float* __restrict__ x, const float* __restrict__ g, int C, size_t L,
                                                           const float* __restrict__ mul, const float* __restrict__ dctx,
                                                           const float* __restrict__ ctx, const float* __restrict__ w,
                                                           const float* __restrict__ m_in, const float* __restrict__ stat,
                                                           float* __restrict__ dx, float* __restrict__ dwpart) {
  __shared__ float sp[WAVES][CHUNK_CM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t b = blockIdx.y, n0 = (size_t)blockIdx.x * CHUNK_CM;
  const int valid = (int)(L - n0 < (size_t)CHUNK_CM ? L - n0 : (size_t)CHUNK_CM);
  const size_t base = b * C * L + n0;
  const float* dcb = dctx + b * C;
  const float* mub = mul ? mul + b * C : nullptr;
  f32x4 p, s = {0.f, 0.f, 0.f, 0.f};
  if (w) {
    float dc = 0.f;
    for (int c = lane; c < C; c += 64) dc = fmaf(dcb[c], ctx[b * C + c], dc);
    dc = wave_sum(dc);
    const f32x4 t = cm_channel_dot<VEC>(x + base, L, C, dcb, lane, wave, valid, sp);
    const float M = stat[2 * b], rS = 1.0f / stat[2 * b + 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = cm_pos<VEC>(lane, j);
      p[j] = q < valid ? expf(m_in[b * L + n0 + q] - M) * rS : 0.f;
      s[j] = p[j] * (t[j] - dc);
    }
  } else {
    const float r = 1.0f / (float)L;
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = r;
  }
  float* rec = dwpart ? dwpart + (b * gridDim.x + blockIdx.x) * (size_t)C : nullptr;
  for (int c = wave; c < C; c += WAVES) {
    const f32x4 xv = cm_load<VEC>(x + base + (size_t)c * L, lane, valid);
    const f32x4 gv = cm_load<VEC>(g + base + (size_t)c * L, lane, valid);
    const float mu = mub ? mub[c] : 1.f, dcc = dcb[c];
    f32x4 o = gv * mu + p * dcc;
    if (w) o += s * w[c];
    cm_store<VEC>(dx + base + (size_t)c * L, lane, valid, o);
    if (w) {
      const float t = wave_sum(hsum(s * xv));
      if (lane == 0) rec[c] = t;
    }
  }
}

// one wave per row (b, c), the waves of the grid stride over the rows
template <bool VEC>
__global__ __launch_bounds__(256) void apply_cm_kernel(const float* __restrict__ x, size_t rows, size_t L, const float* __restrict__ mul,
                                                       const float* __restrict__ add, float* __restrict__ out) {
  typedef typename Elem<VEC>::type V;
  const int lane = threadIdx.x & 63;
  const size_t n = VEC ? L >> 2 : L;
  for (size_t t = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < rows; t += (size_t)gridDim.x * WAVES) {
    const V* r = reinterpret_cast<const V*>(x + t * L);
    V* o = reinterpret_cast<V*>(out + t * L);
    const V mu = splat(V{}, mul ? mul[t] : 1.f), ad = splat(V{}, add ? add[t] : 0.f);
    for (size_t i = lane; i < n; i += 64) o[i] = r[i] * mu + ad;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void bwd_reduce_cm_kernel(const float* __restrict__ x, const float* __restrict__ g, size_t rows, size_t L,
                                                            float* __restrict__ dmul, float* __restrict__ dadd) {
  typedef typename Elem<VEC>::type V;
  const int lane = threadIdx.x & 63;
  const size_t n = VEC ? L >> 2 : L;
  for (size_t t = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < rows; t += (size_t)gridDim.x * WAVES) {
    const V* xr = reinterpret_cast<const V*>(x + t * L);
    const V* gr = reinterpret_cast<const V*>(g + t * L);
    V s0 = splat(V{}, 0.f), s1 = splat(V{}, 0.f);
    for (size_t i = lane; i < n; i += 64) {
      const V gv = gr[i];
      s0 += gv;
      if (dmul) s1 += gv * xr[i];
    }
    const float a = wave_sum(hsum(s0)), m = wave_sum(hsum(s1));
    if (lane == 0) {
      if (dadd) dadd[t] = a;
      if (dmul) dmul[t] = m;
    }
  }
}

// ------------------------------------------------------------------------------------------------- point-major: lanes along the channels
// The row geometry every point-major kernel shares: lane `sub` of a row's tpr lanes holds the pieces sub + k * tpr, k < MAXK, of the row
// (a piece = 4 channels or 1); slot = wave * (64 / tpr) + lane / tpr walks the chunk's rows slot, slot + nslots, ...
template <bool VEC> struct Pm {
  typedef typename Elem<VEC>::type V;
  static constexpr int MAXK = VEC ? MAXK_VEC : MAXK_SCL;
  static constexpr int W = VEC ? 4 : 1;
  int sub, slot, nslots, tpr, pieces;
  __device__ __forceinline__ Pm(int C, int tpr_) {
    const int lane = threadIdx.x & 63, rw = 64 / tpr_;
    tpr = tpr_;
    sub = lane & (tpr_ - 1);
    slot = (threadIdx.x >> 6) * rw + lane / tpr_;
    nslots = WAVES * rw;
    pieces = C / W;
  }
  __device__ __forceinline__ bool has(int k) const { return sub + k * tpr < pieces; }
  __device__ __forceinline__ int chan(int k) const { return (sub + k * tpr) * W; }
  __device__ __forceinline__ void load(const float* __restrict__ row, V (&v)[MAXK]) const {  // NULL: zeros
#pragma unroll
    for (int k = 0; k < MAXK; ++k) v[k] = row && has(k) ? *reinterpret_cast<const V*>(row + chan(k)) : splat(V{}, 0.f);
  }
  __device__ __forceinline__ void fill(V (&v)[MAXK], float f) const {
#pragma unroll
    for (int k = 0; k < MAXK; ++k) v[k] = splat(V{}, f);
  }
  __device__ __forceinline__ void store(float* __restrict__ row, const V (&v)[MAXK]) const {
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
      if (has(k)) *reinterpret_cast<V*>(row + chan(k)) = v[k];
  }
  __device__ __forceinline__ float dot(const V (&a)[MAXK], const V (&b)[MAXK]) const {  // over the whole row, in every lane of the row
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) d += hsum(a[k] * b[k]);
    return group_sum(d, tpr);
  }
  // the lane's channels of its slot's sums -> s[slot * C + c]
  __device__ __forceinline__ void to_lds(float* __restrict__ s, int C, const V (&v)[MAXK]) const { store(s + (size_t)slot * C, v); }
};

constexpr int PM_BATCH = 4;           // rows of a slot per step of pool_pm (the sums below are written for 4)
constexpr int PM_LDS = WAVES * MAX_DIM;  // nslots * C <= 4096 floats: tpr < 64 means one piece per lane, C <= 4 * tpr

template <bool VEC>
__global__ __launch_bounds__(256) void pool_pm_kernel(const float* __restrict__ x, size_t ld, int C, size_t L, int tpr, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ part, float* __restrict__ m_out) {
  typedef Pm<VEC> G;
  typedef typename G::V V;
  __shared__ __attribute__((aligned(16))) float sacc[PM_LDS];
  __shared__ float smx[256], ssm[256];
  const G pm(C, tpr);
  const size_t b = blockIdx.y, r0 = (size_t)blockIdx.x * CHUNK_PM;
  const int valid = (int)(L - r0 < (size_t)CHUNK_PM ? L - r0 : (size_t)CHUNK_PM);
  V wv[G::MAXK], acc[G::MAXK];
  pm.load(w, wv);
  pm.fill(acc, 0.f);
  const float bs = (w && bias) ? bias[0] : 0.f;
  float mx = w ? -INFINITY : 0.f, sm = 0.f;
  // PM_BATCH rows of a slot per step: their loads and dot products are independent, and the running maximum, the two expf of the
  // rescale and the rescale of the sums are paid once per step instead of once per row
  for (int r = pm.slot; r < valid; r += PM_BATCH * pm.nslots) {
    V xv[PM_BATCH][G::MAXK];
    bool ok[PM_BATCH];
#pragma unroll
    for (int i = 0; i < PM_BATCH; ++i) {
      const int ri = r + i * pm.nslots;
      ok[i] = ri < valid;  // the same in every lane of a row
      pm.load(ok[i] ? x + (b * L + r0 + ri) * ld : nullptr, xv[i]);
    }
    if (w) {
      float m[PM_BATCH], mn = mx;
#pragma unroll
      for (int i = 0; i < PM_BATCH; ++i) {
        const float d = pm.dot(wv, xv[i]) + bs;
        m[i] = ok[i] ? d : -INFINITY;
        if (ok[i] && pm.sub == 0) m_out[b * L + r0 + r + i * pm.nslots] = d;
        mn = fmaxf(mn, m[i]);
      }
      const float sc = expf(mx - mn);  // row r exists: mn is finite
      float pr[PM_BATCH];
#pragma unroll
      for (int i = 0; i < PM_BATCH; ++i) pr[i] = expf(m[i] - mn);  // exp(-inf) = 0 for a row outside the chunk
      sm = fmaf(sm, sc, (pr[0] + pr[1]) + (pr[2] + pr[3]));
#pragma unroll
      for (int k = 0; k < G::MAXK; ++k) acc[k] = acc[k] * sc + ((pr[0] * xv[0][k] + pr[1] * xv[1][k]) + (pr[2] * xv[2][k] + pr[3] * xv[3][k]));
      mx = mn;
    } else {
#pragma unroll
      for (int i = 0; i < PM_BATCH; ++i) sm += ok[i] ? 1.f : 0.f;
#pragma unroll
      for (int k = 0; k < G::MAXK; ++k) acc[k] += (xv[0][k] + xv[1][k]) + (xv[2][k] + xv[3][k]);
    }
  }
  pm.to_lds(sacc, C, acc);
  if (pm.sub == 0) {
    smx[pm.slot] = mx;
    ssm[pm.slot] = sm;
  }
  __syncthreads();
  float M = smx[0];
  for (int s = 1; s < pm.nslots; ++s) M = fmaxf(M, smx[s]);  // finite: slot 0 always has a row
  float* rec = part + (b * gridDim.x + blockIdx.x) * (size_t)(C + 2);
  for (int c = threadIdx.x; c < C; c += 256) {
    float a = 0.f;
    for (int s = 0; s < pm.nslots; ++s) a = fmaf(expf(smx[s] - M), sacc[s * C + c], a);  // an empty slot: exp(-inf) = 0
    rec[2 + c] = a;
  }
  if (threadIdx.x == 0) {
    float S = 0.f;
    for (int s = 0; s < pm.nslots; ++s) S = fmaf(expf(smx[s] - M), ssm[s], S);
    rec[0] = M;
    rec[1] = S;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void apply_pm_kernel(const float* __restrict__ x, size_t ldx, int C, size_t L, int tpr, const float* __restrict__ mul,
                                                       const float* __restrict__ add, float* __restrict__ out, size_t ldo) {
  typedef Pm<VEC> G;
  typedef typename G::V V;
  const G pm(C, tpr);
  const size_t b = blockIdx.y, r0 = (size_t)blockIdx.x * CHUNK_PM;
  const int valid = (int)(L - r0 < (size_t)CHUNK_PM ? L - r0 : (size_t)CHUNK_PM);
  V mu[G::MAXK], ad[G::MAXK];
  if (mul) pm.load(mul + b * C, mu); else pm.fill(mu, 1.f);
  pm.load(add ? add + b * C : nullptr, ad);
  for (int r = pm.slot; r < valid; r += pm.nslots) {
    V xv[G::MAXK];
    pm.load(x + (b * L + r0 + r) * ldx, xv);
#pragma unroll
    for (int k = 0; k < G::MAXK; ++k) xv[k] = xv[k] * mu[k] + ad[k];
    pm.store(out + (b * L + r0 + r) * ldo, xv);
  }
}

// record of a chunk: [c] = sum g x, [C + c] = sum g
template <bool VEC>
__global__ __launch_bounds__(256) void bwd_reduce_pm_kernel(const float* __restrict__ x, size_t ldx, const float* __restrict__ g, size_t ldg, int C,
                                                            size_t L, int tpr, float* __restrict__ part) {
  typedef Pm<VEC> G;
  typedef typename G::V V;
  __shared__ __attribute__((aligned(16))) float s0[PM_LDS];
  __shared__ __attribute__((aligned(16))) float s1[PM_LDS];
  const G pm(C, tpr);
  const size_t b = blockIdx.y, r0 = (size_t)blockIdx.x * CHUNK_PM;
  const int valid = (int)(L - r0 < (size_t)CHUNK_PM ? L - r0 : (size_t)CHUNK_PM);
  V a0[G::MAXK], a1[G::MAXK];
  pm.fill(a0, 0.f);
  pm.fill(a1, 0.f);
  for (int r = pm.slot; r < valid; r += pm.nslots) {
    V xv[G::MAXK], gv[G::MAXK];
    pm.load(x + (b * L + r0 + r) * ldx, xv);
    pm.load(g + (b * L + r0 + r) * ldg, gv);
#pragma unroll
    for (int k = 0; k < G::MAXK; ++k) {
      a0[k] += gv[k] * xv[k];
      a1[k] += gv[k];
    }
  }
  pm.to_lds(s0, C, a0);
  pm.to_lds(s1, C, a1);
  __syncthreads();
  float* rec = part + (b * gridDim.x + blockIdx.x) * (size_t)(2 * C);
  for (int c = threadIdx.x; c < C; c += 256) {
    float u = 0.f, v = 0.f;
    for (int s = 0; s < pm.nslots; ++s) {
      u += s0[s * C + c];
      v += s1[s * C + c];
    }
    rec[c] = u;
    rec[C + c] = v;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void bwd_apply_pm_kernel(const float* __restrict__ x, size_t ldx, const float* __restrict__ g, size_t ldg, int C,
                                                           size_t L, int tpr, const float* __restrict__ mul, const float* __restrict__ dctx,
                                                           const float* __restrict__ ctx, const float* __restrict__ w,
                                                           const float* __restrict__ m_in, const float* __restrict__ stat,
                                                           float* __restrict__ dx, size_t lddx, float* __restrict__ dwpart) {
  typedef Pm<VEC> G;
  typedef typename G::V V;
  __shared__ __attribute__((aligned(16))) float sacc[PM_LDS];
  const G pm(C, tpr);
  const size_t b = blockIdx.y, r0 = (size_t)blockIdx.x * CHUNK_PM;
  const int valid = (int)(L - r0 < (size_t)CHUNK_PM ? L - r0 : (size_t)CHUNK_PM);
  V mu[G::MAXK], dc[G::MAXK], wv[G::MAXK], acc[G::MAXK];
  if (mul) pm.load(mul + b * C, mu); else pm.fill(mu, 1.f);
  pm.load(dctx + b * C, dc);
  pm.load(w, wv);
  pm.fill(acc, 0.f);
  float dcc = 0.f, M = 0.f, rS = 0.f;
  if (w) {
    V cv[G::MAXK];
    pm.load(ctx + b * C, cv);
    dcc = pm.dot(dc, cv);
    M = stat[2 * b];
    rS = 1.0f / stat[2 * b + 1];
  }
  const float pavg = 1.0f / (float)L;
  for (int r = pm.slot; r < valid; r += pm.nslots) {
    V xv[G::MAXK], gv[G::MAXK];
    pm.load(x + (b * L + r0 + r) * ldx, xv);
    pm.load(g + (b * L + r0 + r) * ldg, gv);
    float p = pavg, s = 0.f;
    if (w) {
      p = expf(m_in[b * L + r0 + r] - M) * rS;
      s = p * (pm.dot(dc, xv) - dcc);
    }
#pragma unroll
    for (int k = 0; k < G::MAXK; ++k) {
      gv[k] = gv[k] * mu[k] + p * dc[k] + s * wv[k];
      acc[k] += s * xv[k];
    }
    pm.store(dx + (b * L + r0 + r) * lddx, gv);
  }
  if (!w) return;
  pm.to_lds(sacc, C, acc);
  __syncthreads();
  float* rec = dwpart + (b * gridDim.x + blockIdx.x) * (size_t)C;
  for (int c = threadIdx.x; c < C; c += 256) {
    float u = 0.f;
    for (int s = 0; s < pm.nslots; ++s) u += sacc[s * C + c];
    rec[c] = u;
  }
}

// ------------------------------------------------------------------------------------------------- the records of a sample, in chunk order
// the sum / max of v over the workgroup's threads, in every thread (wave butterflies, then the four waves in order)
__device__ __forceinline__ float block_sum(float v, float* s4) {
  v = wave_sum(v);
  __syncthreads();  // s4 may still be read from the previous call
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}
__device__ __forceinline__ float block_max(float v, float* s4) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s4[0], s4[1]), fmaxf(s4[2], s4[3]));
}

// grid (B, ceil(C / 64)).  Every workgroup forms the sample's (M, S) from the heads of the records, its threads striding over the chunks;
// then a lane owns one of the workgroup's 64 channels, wave w sums the chunks j = w (mod 4) -- independent, coalesced loads -- and the
// four partial sums meet in LDS in wave order.
__global__ __launch_bounds__(256) void pool_combine_kernel(const float* __restrict__ part, int nch, int C, float* __restrict__ ctx,
                                                           float* __restrict__ lse, float* __restrict__ stat) {
  __shared__ float s4[WAVES], sp[WAVES][64];
  const size_t b = blockIdx.x, W = (size_t)C + 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* rec = part + b * nch * W;
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < nch; j += 256) mx = fmaxf(mx, rec[j * W]);
  const float M = block_max(mx, s4);
  float s = 0.f;
  for (int j = threadIdx.x; j < nch; j += 256) s = fmaf(expf(rec[j * W] - M), rec[j * W + 1], s);
  const float S = block_sum(s, s4);
  const int c = blockIdx.y * 64 + lane;
  float a = 0.f;
  if (c < C) {
#pragma unroll 4
    for (int j = wave; j < nch; j += WAVES) a = fmaf(expf(rec[j * W] - M), rec[j * W + 2 + c], a);
  }
  sp[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && c < C) ctx[b * C + c] = ((sp[0][lane] + sp[1][lane]) + (sp[2][lane] + sp[3][lane])) / S;
  if (threadIdx.x == 0 && blockIdx.y == 0) {
    lse[b] = M + logf(S);
    stat[2 * b] = M;
    stat[2 * b + 1] = S;
  }
}

// grid (B, ceil(2C / 64)): the same split of the chunks over the waves
__global__ __launch_bounds__(256) void reduce_combine_kernel(const float* __restrict__ part, int nch, int C, float* __restrict__ dmul,
                                                             float* __restrict__ dadd) {
  __shared__ float sp[WAVES][64];
  const size_t b = blockIdx.x, W = 2 * (size_t)C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* rec = part + b * nch * W;
  const int c = blockIdx.y * 64 + lane;
  float a = 0.f;
  if (c < 2 * C) {
#pragma unroll 4
    for (int j = wave; j < nch; j += WAVES) a += rec[j * W + c];
  }
  sp[wave][lane] = a;
  __syncthreads();
  if (wave != 0 || c >= 2 * C) return;
  a = (sp[0][lane] + sp[1][lane]) + (sp[2][lane] + sp[3][lane]);
  if (c < C) {
    if (dmul) dmul[b * C + c] = a;
  } else if (dadd) {
    dadd[b * C + c - C] = a;
  }
}

// ------------------------------------------------------------------------------------------------- channel-major through LDS: one read of x
// pool_fwd and bwd_apply need a position's sum over ALL channels before they can use any channel of it.  While a [C, tp] tile of x fits in
// 64 KB of LDS (tp = 64 positions up to C = 246, 32 up to C = 484) the workgroup stages it once, forms the sums from LDS with the threads
// along the positions, and then walks the tile again from LDS with one thread per channel: x comes from memory once.  A chunk of CHUNK_CM
// positions is CHUNK_CM / tp tiles with an online softmax across them.  Rows of the tile are tp + 1 floats apart: the per-channel walk
// (thread c reads xs[c][n]) and the per-position walk (thread n reads xs[c][n]) are both free of bank conflicts.  Wider C takes the
// two-walk kernels above.
constexpr int CM_ACC = 2;  // channels per thread: C <= 484 < 2 * 256

struct CmTile {
  float *xs, *spart, *sp, *ss, *misc;
  int ld;
  __device__ __forceinline__ CmTile(float* base, int C, int tp) {
    ld = tp + 1;
    xs = base;
    spart = xs + (size_t)C * ld;
    sp = spart + 256;
    ss = sp + 64;
    misc = ss + 64;
  }
};
inline size_t cm_tile_bytes(int C, int tp) { return ((size_t)C * (tp + 1) + 256 + 64 + 64 + 8) * sizeof(float); }

// the tile [C, tp] at position t0 of the chunk -> xs; positions outside the sample read as 0
template <bool VEC>
__device__ __forceinline__ void cm_tile_load(const float* __restrict__ xb, size_t L, int C, int tp, int t0, int valid, const CmTile& t) {
  if (VEC) {
    const int q4 = tp >> 2, total = C * q4;
    for (int e = threadIdx.x; e < total; e += 256) {
      const int c = e / q4, q = e - c * q4, n = t0 + 4 * q;
      const f32x4 v = n < valid ? *reinterpret_cast<const f32x4*>(xb + (size_t)c * L + n) : f32x4{0.f, 0.f, 0.f, 0.f};
      float* d = t.xs + c * t.ld + 4 * q;
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
  } else {
    const int total = C * tp;
    for (int e = threadIdx.x; e < total; e += 256) {
      const int c = e / tp, q = e - c * tp, n = t0 + q;
      t.xs[c * t.ld + q] = n < valid ? xb[(size_t)c * L + n] : 0.f;
    }
  }
}

// sum_c coef[c] * xs[c][n] for the tile's positions: thread (group = tid / tp, n = tid % tp) sums the channels c = group (mod 256 / tp),
// the partial sums meet in spart and are added in group order; valid in the threads tid < tp after the call (which ends in a barrier)
__device__ __forceinline__ float cm_tile_dot(const float* __restrict__ coef, int C, int tp, const CmTile& t) {
  const int groups = 256 / tp, n = threadIdx.x % tp, gq = threadIdx.x / tp;
  float a = 0.f;
  for (int c = gq; c < C; c += groups) a = fmaf(coef[c], t.xs[c * t.ld + n], a);
  t.spart[gq * tp + n] = a;
  __syncthreads();
  float d = 0.f;
  if (threadIdx.x < tp)
    for (int q = 0; q < groups; ++q) d += t.spart[q * tp + n];
  return d;
}

template <bool VEC>
__global__ __launch_bounds__(256) void pool_cm_lds_kernel(const float* __restrict__ x, int C, size_t L, int tp, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ part, float* __restrict__ m_out) {
  extern __shared__ __attribute__((aligned(16))) float cm_smem[];
  const CmTile t(cm_smem, C, tp);
  const size_t b = blockIdx.y, n0 = (size_t)blockIdx.x * CHUNK_CM;
  const int valid = (int)(L - n0 < (size_t)CHUNK_CM ? L - n0 : (size_t)CHUNK_CM);
  const float* xb = x + b * C * L + n0;
  const float bs = (w && bias) ? bias[0] : 0.f;
  float acc[CM_ACC] = {0.f, 0.f};
  float mx = w ? -INFINITY : 0.f, sum = 0.f;  // kept by the first wave
  for (int t0 = 0; t0 < valid; t0 += tp) {
    __syncthreads();  // the previous tile is done with
    cm_tile_load<VEC>(xb, L, C, tp, t0, valid, t);
    __syncthreads();
    float m = 0.f;
    if (w) m = cm_tile_dot(w, C, tp, t) + bs;
    if (threadIdx.x < 64) {  // tp <= 64: the first wave holds the tile's logits, a lane per position
      const bool in = (int)threadIdx.x < tp && t0 + (int)threadIdx.x < valid;
      float p, sc = 1.f;
      if (w) {
        if (in) m_out[b * L + n0 + t0 + threadIdx.x] = m;
        const float mi = in ? m : -INFINITY;
        const float mn = fmaxf(mx, wave_max(mi));  // position t0 is inside the sample: finite
        sc = expf(mx - mn);
        p = expf(mi - mn);
        mx = mn;
      } else {
        p = in ? 1.f : 0.f;
      }
      sum = fmaf(sum, sc, wave_sum(p));
      if ((int)threadIdx.x < tp) t.sp[threadIdx.x] = p;
      if (threadIdx.x == 0) t.misc[0] = sc;
    }
    __syncthreads();
    const float sc = t.misc[0];
#pragma unroll
    for (int k = 0; k < CM_ACC; ++k) {
      const int c = threadIdx.x + 256 * k;
      if (c < C) {
        const float* row = t.xs + c * t.ld;
        float a = 0.f;
        for (int n = 0; n < tp; ++n) a = fmaf(t.sp[n], row[n], a);
        acc[k] = fmaf(acc[k], sc, a);
      }
    }
  }
  float* rec = part + (b * gridDim.x + blockIdx.x) * (size_t)(C + 2);
#pragma unroll
  for (int k = 0; k < CM_ACC; ++k)
    if (threadIdx.x + 256 * k < C) rec[2 + threadIdx.x + 256 * k] = acc[k];
  if (threadIdx.x == 0) {
    rec[0] = mx;
    rec[1] = sum;
  }
}

// attention pooling only (w != NULL): average pooling needs no sum over the channels and stays on bwd_apply_cm_kernel
template <bool VEC>
__global__ __launch_bounds__(256) void bwd_apply_cm_lds_kernel(const float* __restrict__ x, const float* __restrict__ g, int C, size_t L, int tp,
                                                               const float* __restrict__ mul, const float* __restrict__ dctx,
                                                               const float* __restrict__ ctx, const float* __restrict__ w,
                                                               const float* __restrict__ m_in, const float* __restrict__ stat,
                                                               float* __restrict__ dx, float* __restrict__ dwpart) {
  extern __shared__ __attribute__((aligned(16))) float cm_smem[];
  const CmTile t(cm_smem, C, tp);
  const size_t b = blockIdx.y, n0 = (size_t)blockIdx.x * CHUNK_CM;
  const int valid = (int)(L - n0 < (size_t)CHUNK_CM ? L - n0 : (size_t)CHUNK_CM);
  const size_t base = b * C * L + n0;
  const float* dcb = dctx + b * C;
  const float* mub = mul ? mul + b * C : nullptr;
  float dc = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) dc = fmaf(dcb[c], ctx[b * C + c], dc);
  dc = block_sum(dc, t.misc + 4);
  const float M = stat[2 * b], rS = 1.0f / stat[2 * b + 1];
  float acc[CM_ACC] = {0.f, 0.f};
  for (int t0 = 0; t0 < valid; t0 += tp) {
    __syncthreads();
    cm_tile_load<VEC>(x + base, L, C, tp, t0, valid, t);
    __syncthreads();
    const float d = cm_tile_dot(dcb, C, tp, t);
    if ((int)threadIdx.x < tp) {
      const bool in = t0 + (int)threadIdx.x < valid;
      const float p = in ? expf(m_in[b * L + n0 + t0 + threadIdx.x] - M) * rS : 0.f;
      t.sp[threadIdx.x] = p;
      t.ss[threadIdx.x] = p * (d - dc);
    }
    __syncthreads();
    if (VEC) {
      const int q4 = tp >> 2, total = C * q4;
      for (int e = threadIdx.x; e < total; e += 256) {
        const int c = e / q4, q = e - c * q4, n = t0 + 4 * q;
        if (n < valid) {
          const size_t at = base + (size_t)c * L + n;
          const f32x4 gv = *reinterpret_cast<const f32x4*>(g + at);
          const float mu = mub ? mub[c] : 1.f, dcc = dcb[c], wc = w[c];
          f32x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = gv[j] * mu + t.sp[4 * q + j] * dcc + t.ss[4 * q + j] * wc;
          *reinterpret_cast<f32x4*>(dx + at) = o;
        }
      }
    } else {
      const int total = C * tp;
      for (int e = threadIdx.x; e < total; e += 256) {
        const int c = e / tp, q = e - c * tp, n = t0 + q;
        if (n < valid) {
          const size_t at = base + (size_t)c * L + n;
          dx[at] = g[at] * (mub ? mub[c] : 1.f) + t.sp[q] * dcb[c] + t.ss[q] * w[c];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < CM_ACC; ++k) {
      const int c = threadIdx.x + 256 * k;
      if (c < C) {
        const float* row = t.xs + c * t.ld;
        float a = 0.f;
        for (int n = 0; n < tp; ++n) a = fmaf(t.ss[n], row[n], a);
        acc[k] += a;
      }
    }
  }
  float* rec = dwpart + (b * gridDim.x + blockIdx.x) * (size_t)C;
#pragma unroll
  for (int k = 0; k < CM_ACC; ++k)
    if (threadIdx.x + 256 * k < C) rec[threadIdx.x + 256 * k] = acc[k];
}

// ------------------------------------------------------------------------------------------------- the two branches on the context vector
struct Branch {
  const float *W1, *b1, *lnw, *lnb, *W2, *b2;
};

__device__ __forceinline__ float ln_out(float h, float mean, float rstd, float lw, float lb) { return fmaf((h - mean) * rstd, lw, lb); }

constexpr int MV_ROWS = 8;  // rows of a matrix-vector product a wave has in flight

// out[r] = Wm[r, :] . v + bias[r], r < rows: a wave owns MV_ROWS rows at a time, its lanes stride over the columns (coalesced), the
// loads of the rows are independent; v in LDS
__device__ __forceinline__ void matvec_rows(const float* __restrict__ Wm, const float* __restrict__ bias, const float* v, int rows, int cols,
                                            float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r0 = wave * MV_ROWS; r0 < rows; r0 += WAVES * MV_ROWS) {
    float d[MV_ROWS];
#pragma unroll
    for (int u = 0; u < MV_ROWS; ++u) d[u] = 0.f;
    for (int c = lane; c < cols; c += 64) {
      const float vc = v[c];
#pragma unroll
      for (int u = 0; u < MV_ROWS; ++u)
        if (r0 + u < rows) d[u] = fmaf(Wm[(size_t)(r0 + u) * cols + c], vc, d[u]);
    }
#pragma unroll
    for (int u = 0; u < MV_ROWS; ++u) d[u] = wave_sum(d[u]);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < MV_ROWS; ++u)
        if (r0 + u < rows) out[r0 + u] = d[u] + bias[r0 + u];
    }
  }
}

// part[wave][c] = sum over the rows r = wave (mod 4) of Wm[r, c] * v[r], c < cols: lanes along the columns (coalesced), the rows split
// over the waves; the caller adds the four partial sums in wave order
__device__ __forceinline__ void vecmat_partial(const float* __restrict__ Wm, const float* v, int rows, int cols, float (*part)[MAX_DIM]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = lane; c < cols; c += 64) {
    float a = 0.f;
#pragma unroll 8
    for (int r = wave; r < rows; r += WAVES) a = fmaf(Wm[(size_t)r * cols + c], v[r], a);
    part[wave][c] = a;
  }
}

// grid (B, 2): branch 0 = add, 1 = mul.  hid [2,B,O] = the first convolution's output, lnstat [2,B,2] = (mean, rstd) of its LayerNorm
__global__ __launch_bounds__(256) void channel_fwd_kernel(const float* __restrict__ ctx, int B, int C, int O, Branch badd, Branch bmul, float eps,
                                                          float* __restrict__ hid, float* __restrict__ lnstat, float* __restrict__ add,
                                                          float* __restrict__ mul) {
  __shared__ float sctx[MAX_DIM], sh[MAX_DIM], s4[WAVES];
  const int br = blockIdx.y;
  const Branch p = br ? bmul : badd;
  if (!p.W1) return;
  const size_t b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += 256) sctx[c] = ctx[b * C + c];
  __syncthreads();
  matvec_rows(p.W1, p.b1, sctx, O, C, sh);
  __syncthreads();
  float t = 0.f;
  for (int o = threadIdx.x; o < O; o += 256) t += sh[o];
  const float mean = block_sum(t, s4) / (float)O;
  t = 0.f;
  for (int o = threadIdx.x; o < O; o += 256) t += (sh[o] - mean) * (sh[o] - mean);
  const float rstd = 1.0f / sqrtf(block_sum(t, s4) / (float)O + eps);
  float* hb = hid + ((size_t)br * B + b) * O;
  for (int o = threadIdx.x; o < O; o += 256) {
    hb[o] = sh[o];
    sctx[o] = fmaxf(ln_out(sh[o], mean, rstd, p.lnw[o], p.lnb[o]), 0.f);  // sctx is free: every thread is past the first product
  }
  if (threadIdx.x == 0) {
    lnstat[((size_t)br * B + b) * 2] = mean;
    lnstat[((size_t)br * B + b) * 2 + 1] = rstd;
  }
  __syncthreads();
  matvec_rows(p.W2, p.b2, sctx, C, O, sh);  // sh is free: hid holds it
  __syncthreads();
  float* dst = (br ? mul : add) + b * C;
  for (int c = threadIdx.x; c < C; c += 256) dst[c] = br ? 1.0f / (1.0f + expf(-sh[c])) : sh[c];
}

// grid B.  Per branch, G row b holds at the branch's offset [dt (C) | dh (O) | dhn * xhat (O) | dhn (O) | r (O)]: the per-sample factors
// of the cross-sample parameter gradients (dt: the cotangent of the second convolution's output, dh: of the first one's, dhn: of the
// LayerNorm's, r: the ReLU's output).  dctx [B,C] = the sum of both branches' W1^T dh.
__global__ __launch_bounds__(256) void channel_bwd_kernel(const float* __restrict__ dadd, const float* __restrict__ dmul, const float* __restrict__ mul,
                                                          const float* __restrict__ hid, const float* __restrict__ lnstat, int B, int C, int O,
                                                          Branch badd, Branch bmul, float* __restrict__ G, int ldg, int off_add, int off_mul,
                                                          float* __restrict__ dctx) {
  __shared__ float sdt[MAX_DIM], sxh[MAX_DIM], sdx[MAX_DIM], s4[WAVES], spart[WAVES][MAX_DIM];
  const size_t b = blockIdx.x;
  float dacc[MAX_DIM / 256] = {0.f, 0.f, 0.f, 0.f};
  for (int br = 0; br < 2; ++br) {
    const Branch p = br ? bmul : badd;
    if (!p.W1) continue;  // uniform over the workgroup
    float* gr = G + b * ldg + (br ? off_mul : off_add);
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      float dt;
      if (br) {
        const float mu = mul[b * C + c];
        dt = dmul[b * C + c] * mu * (1.f - mu);
      } else {
        dt = dadd[b * C + c];
      }
      sdt[c] = dt;
      gr[c] = dt;
    }
    __syncthreads();
    vecmat_partial(p.W2, sdt, C, O, spart);  // dr = W2^T dt
    __syncthreads();
    const float mean = lnstat[((size_t)br * B + b) * 2], rstd = lnstat[((size_t)br * B + b) * 2 + 1];
    const float* hb = hid + ((size_t)br * B + b) * O;
    float t1 = 0.f, t2 = 0.f;
    for (int o = threadIdx.x; o < O; o += 256) {
      const float xh = (hb[o] - mean) * rstd, hn = fmaf(xh, p.lnw[o], p.lnb[o]);
      const float dr = (spart[0][o] + spart[1][o]) + (spart[2][o] + spart[3][o]);
      const float dhn = hn > 0.f ? dr : 0.f, dxh = dhn * p.lnw[o];
      gr[C + O + o] = dhn * xh;
      gr[C + 2 * O + o] = dhn;
      gr[C + 3 * O + o] = fmaxf(hn, 0.f);
      sxh[o] = xh;
      sdx[o] = dxh;
      t1 += dxh;
      t2 += dxh * xh;
    }
    const float m1 = block_sum(t1, s4) / (float)O;
    const float m2 = block_sum(t2, s4) / (float)O;
    for (int o = threadIdx.x; o < O; o += 256) {  // each thread rewrites the entries it wrote
      const float dh = rstd * (sdx[o] - m1 - sxh[o] * m2);
      sdx[o] = dh;
      gr[C + o] = dh;
    }
    __syncthreads();
    vecmat_partial(p.W1, sdx, O, C, spart);  // W1^T dh
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MAX_DIM / 256; ++k) {
      const int c = threadIdx.x + 256 * k;
      if (c < C) dacc[k] += (spart[0][c] + spart[1][c]) + (spart[2][c] + spart[3][c]);
    }
  }
#pragma unroll
  for (int k = 0; k < MAX_DIM / 256; ++k)
    if (threadIdx.x + 256 * k < C) dctx[b * C + threadIdx.x + 256 * k] = dacc[k];
}

// ------------------------------------------------------------------------------------------------- host side
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }  // NULL counts as aligned
inline bool dims_ok(int layout, int B, int C, long L) {
  return (layout == 0 || layout == 1) && B >= 1 && B <= 65535 && C >= 1 && C <= MAX_DIM && L >= 1 && (L + CHUNK_PM - 1) / CHUNK_PM < (1L << 31);
}
inline unsigned chunks_of(int layout, long L) { return (unsigned)((L + (layout ? CHUNK_PM : CHUNK_CM) - 1) / (layout ? CHUNK_PM : CHUNK_CM)); }
inline int rows_grid(size_t rows) { return (int)(rows < (size_t)MAX_BLOCKS * WAVES ? (rows + WAVES - 1) / WAVES : MAX_BLOCKS); }
// lanes per row: the smallest power of two that covers the row's pieces, at most a wave
inline int tpr_of(int C, bool vec) {
  const int pieces = vec ? C / 4 : C;
  int t = 1;
  while (t < pieces && t < 64) t <<= 1;
  return t;
}
// positions per LDS tile of the one-read channel-major kernels; 0: the tile does not fit, the two-walk kernels serve
inline int cm_tile_positions(int C) {
  for (int tp = 64; tp >= 32; tp >>= 1)
    if (C <= CM_ACC * 256 && cm_tile_bytes(C, tp) <= 65536) return tp;
  return 0;
}
inline bool pm_vec(int C, long ld) { return C % 4 == 0 && ld % 4 == 0; }
inline bool branch_ok(const spgan_gc_branch_t* p) { return !p || (p->W1 && p->b1 && p->lnw && p->lnb && p->W2 && p->b2); }
inline Branch branch_of(const spgan_gc_branch_t* p) {
  return p ? Branch{p->W1, p->b1, p->lnw, p->lnb, p->W2, p->b2} : Branch{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
}

}  // namespace

#define GC_LAUNCH(kernel, vec, grid, ...)                                                             \
  do {                                                                                                \
    if (vec)                                                                                          \
      hipLaunchKernelGGL(kernel<true>, grid, dim3(256), 0, (hipStream_t)s_, __VA_ARGS__);             \
    else                                                                                              \
      hipLaunchKernelGGL(kernel<false>, grid, dim3(256), 0, (hipStream_t)s_, __VA_ARGS__);            \
  } while (0)

extern "C" int spgan_gc_attn_chunk_points(int layout) { return layout == 0 ? CHUNK_CM : (layout == 1 ? CHUNK_PM : 0); }

extern "C" int spgan_gc_attn_pool_fwd(const float* x, int layout, long ld, int B, int C, long L, const float* w, const float* bias, float* part,
                                      float* m, float* ctx, float* lse, float* stat, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(x && part && ctx && lse && stat && dims_ok(layout, B, C, L) && (!w || m) && (layout == 0 || ld >= C));
  const unsigned nch = chunks_of(layout, L);
  const dim3 grid(nch, B);
  if (layout == 0) {
    const bool vec = L % 4 == 0 && aligned16(x);
    const int tp = cm_tile_positions(C);
    if (tp) {
      if (vec)
        hipLaunchKernelGGL(pool_cm_lds_kernel<true>, grid, dim3(256), cm_tile_bytes(C, tp), (hipStream_t)s_, x, C, (size_t)L, tp, w, bias, part, m);
      else
        hipLaunchKernelGGL(pool_cm_lds_kernel<false>, grid, dim3(256), cm_tile_bytes(C, tp), (hipStream_t)s_, x, C, (size_t)L, tp, w, bias, part, m);
    } else {
      GC_LAUNCH(pool_cm_kernel, vec, grid, x, C, (size_t)L, w, bias, part, m);
    }
  } else {
    const bool vec = pm_vec(C, ld) && aligned16(x) && aligned16(w);
    GC_LAUNCH(pool_pm_kernel, vec, grid, x, (size_t)ld, C, (size_t)L, tpr_of(C, vec), w, bias, part, m);
  }
  hipLaunchKernelGGL(pool_combine_kernel, dim3(B, (C + 63) / 64), dim3(256), 0, (hipStream_t)s_, part, (int)nch, C, ctx, lse, stat);
  return spgan_launch_status();
}

extern "C" int spgan_gc_attn_channel_fwd(const float* ctx, int B, int C, int O, const spgan_gc_branch_t* add_p, const spgan_gc_branch_t* mul_p,
                                         float eps, float* hid, float* lnstat, float* add, float* mul, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(ctx && hid && lnstat && B >= 1 && B <= 65535 && C >= 1 && C <= MAX_DIM && O >= 1 && O <= MAX_DIM && eps > 0.f);
  SPGAN_CHECK_ARG((add_p || mul_p) && branch_ok(add_p) && branch_ok(mul_p) && (!add_p || add) && (!mul_p || mul));
  hipLaunchKernelGGL(channel_fwd_kernel, dim3(B, 2), dim3(256), 0, (hipStream_t)s_, ctx, B, C, O, branch_of(add_p), branch_of(mul_p), eps, hid,
                     lnstat, add, mul);
  return spgan_launch_status();
}

extern "C" int spgan_gc_attn_channel_bwd(const float* dadd, const float* dmul, const float* mul, const float* hid, const float* lnstat, int B, int C,
                                         int O, const spgan_gc_branch_t* add_p, const spgan_gc_branch_t* mul_p, float* G, float* dctx,
                                         spgan_stream_t s_) {
  SPGAN_CHECK_ARG(hid && lnstat && G && dctx && B >= 1 && B <= 65535 && C >= 1 && C <= MAX_DIM && O >= 1 && O <= MAX_DIM);
  SPGAN_CHECK_ARG((add_p || mul_p) && branch_ok(add_p) && branch_ok(mul_p) && (!add_p || dadd) && (!mul_p || (dmul && mul)));
  const int W = C + 4 * O, ldg = W * ((add_p ? 1 : 0) + (mul_p ? 1 : 0));
  hipLaunchKernelGGL(channel_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)s_, dadd, dmul, mul, hid, lnstat, B, C, O, branch_of(add_p),
                     branch_of(mul_p), G, ldg, 0, add_p ? W : 0, dctx);
  return spgan_launch_status();
}

extern "C" int spgan_gc_attn_apply_fwd(const float* x, int layout, long ldx, int B, int C, long L, const float* mul, const float* add, float* out,
                                       long ldo, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(x && out && (mul || add) && dims_ok(layout, B, C, L) && (layout == 0 || (ldx >= C && ldo >= C)));
  if (layout == 0) {
    const size_t rows = (size_t)B * C;
    GC_LAUNCH(apply_cm_kernel, L % 4 == 0 && aligned16(x) && aligned16(out), dim3(rows_grid(rows)), x, rows, (size_t)L, mul, add, out);
  } else {
    const bool vec = pm_vec(C, ldx) && ldo % 4 == 0 && aligned16(x) && aligned16(out) && aligned16(mul) && aligned16(add);
    GC_LAUNCH(apply_pm_kernel, vec, dim3(chunks_of(1, L), B), x, (size_t)ldx, C, (size_t)L, tpr_of(C, vec), mul, add, out, (size_t)ldo);
  }
  return spgan_launch_status();
}

extern "C" int spgan_gc_attn_bwd_reduce(const float* x, long ldx, const float* g, long ldg, int layout, int B, int C, long L, float* part,
                                        float* dmul, float* dadd, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(x && g && (dmul || dadd) && dims_ok(layout, B, C, L) && (layout == 0 || (part && ldx >= C && ldg >= C)));
  if (layout == 0) {
    const size_t rows = (size_t)B * C;
    GC_LAUNCH(bwd_reduce_cm_kernel, L % 4 == 0 && aligned16(x) && aligned16(g), dim3(rows_grid(rows)), x, g, rows, (size_t)L, dmul, dadd);
  } else {
    const bool vec = pm_vec(C, ldx) && ldg % 4 == 0 && aligned16(x) && aligned16(g);
    const unsigned nch = chunks_of(1, L);
    GC_LAUNCH(bwd_reduce_pm_kernel, vec, dim3(nch, B), x, (size_t)ldx, g, (size_t)ldg, C, (size_t)L, tpr_of(C, vec), part);
    hipLaunchKernelGGL(reduce_combine_kernel, dim3(B, (2 * C + 63) / 64), dim3(256), 0, (hipStream_t)s_, part, (int)nch, C, dmul, dadd);
  }
  return spgan_launch_status();
}

extern "C" int spgan_gc_attn_bwd_apply(const float* x, long ldx, const float* g, long ldg, int layout, int B, int C, long L, const float* mul,
                                       const float* dctx, const float* ctx, const float* w, const float* m, const float* stat, float* dx,
                                       long lddx, float* dwpart, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(x && g && dctx && dx && dims_ok(layout, B, C, L) && (!w || (ctx && m && stat && dwpart)));
  SPGAN_CHECK_ARG(layout == 0 || (ldx >= C && ldg >= C && lddx >= C));
  const dim3 grid(chunks_of(layout, L), B);
  if (layout == 0) {
    const bool vec = L % 4 == 0 && aligned16(x) && aligned16(g) && aligned16(dx);
    const int tp = w ? cm_tile_positions(C) : 0;
    if (tp) {
      if (vec)
        hipLaunchKernelGGL(bwd_apply_cm_lds_kernel<true>, grid, dim3(256), cm_tile_bytes(C, tp), (hipStream_t)s_, x, g, C, (size_t)L, tp, mul, dctx,
                           ctx, w, m, stat, dx, dwpart);
      else
        hipLaunchKernelGGL(bwd_apply_cm_lds_kernel<false>, grid, dim3(256), cm_tile_bytes(C, tp), (hipStream_t)s_, x, g, C, (size_t)L, tp, mul, dctx,
                           ctx, w, m, stat, dx, dwpart);
    } else {
      GC_LAUNCH(bwd_apply_cm_kernel, vec, grid, x, g, C, (size_t)L, mul, dctx, ctx, w, m, stat, dx, dwpart);
    }
  } else {
    const bool vec = pm_vec(C, ldx) && ldg % 4 == 0 && lddx % 4 == 0 && aligned16(x) && aligned16(g) && aligned16(dx) && aligned16(mul) &&
                     aligned16(dctx) && aligned16(ctx) && aligned16(w);
    GC_LAUNCH(bwd_apply_pm_kernel, vec, grid, x, (size_t)ldx, g, (size_t)ldg, C, (size_t)L, tpr_of(C, vec), mul, dctx, ctx, w, m, stat, dx,
              (size_t)lddx, dwpart);
  }
  return spgan_launch_status();
}
