// GAN-stabiliser and StyleGAN-style layers (Generation/modules.py:32-390, 437-496 of the reference): grouped spectral normalisation,
// the minibatch-stddev channel, and the fused layer epilogue  y = gamma * IN(PN(act(x + w*noise))) + beta  (DESIGN 36).
// fp32 tensors, no float atomics: every sum is a fixed tree (per-thread ascending loop, wave butterfly, ascending merge of the partial
// records), so results repeat bit for bit and a problem gives the same bits alone and inside a group.
#include "common.hpp"

namespace {

constexpr int WG = 256;

// sum over the 256 threads of a workgroup, the same value returned to all of them: wave butterfly, then the 4 wave sums in ascending order
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                                  // red may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ int find_problem(const int* start, int count, int tile) {
  int p = 0;
  while (p + 1 < count && tile >= start[p + 1]) ++p;
  return p;
}

// ------------------------------------------------------------------------------------------------ spectral normalisation
constexpr int SN_ROWS = 16;       // rows of W per workgroup of the W^T u pass (one partial vector per chunk)
constexpr int SN_MV_ROWS = 4;     // rows per workgroup of the W v pass: one wave per row
constexpr int SN_TILE = 2048;     // elements per workgroup of the element-wise passes

struct SnTiles { int start[SPGAN_SN_MAX + 1]; };

// workspace of one problem (floats): [chunks*w partial W^T u | h raw W v | dot partials]
__host__ __device__ inline int sn_chunks(int h) { return (h + SN_ROWS - 1) / SN_ROWS; }
__host__ __device__ inline long sn_ws_uraw(int h, int w) { return (long)sn_chunks(h) * w; }
__host__ __device__ inline long sn_ws_dot(int h, int w) { return sn_ws_uraw(h, w) + h; }
__host__ __device__ inline int sn_elem_tiles(int h, int w) { return (int)(((long)h * w + SN_TILE - 1) / SN_TILE); }

// part[chunk, j] = sum_{i in chunk} W[i, j] * u[i]: thread per column, rows ascending
__global__ __launch_bounds__(WG) void sn_mvt_kernel(const spgan_sn_args a, const SnTiles t) {
  const int p = find_problem(t.start, a.count, blockIdx.x);
  const int h = a.h[p], w = a.w[p];
  const int cb = (w + WG - 1) / WG;
  const int lt = blockIdx.x - t.start[p];
  const int chunk = lt / cb, j = (lt % cb) * WG + threadIdx.x;
  if (j >= w) return;
  const float* __restrict__ W = a.W[p];
  const float* __restrict__ u = a.u[p];
  const int i0 = chunk * SN_ROWS, i1 = min(h, i0 + SN_ROWS);
  float acc = 0.f;
#pragma unroll 4
  for (int i = i0; i < i1; ++i) acc += W[(long)i * w + j] * u[i];
  a.ws[p][(long)chunk * w + j] = acc;
}

// uraw[i] = sum_j W[i, j] * v[j]: one wave per row, lanes over columns, butterfly
__global__ __launch_bounds__(WG) void sn_mv_kernel(const spgan_sn_args a, const SnTiles t) {
  const int p = find_problem(t.start, a.count, blockIdx.x);
  const int h = a.h[p], w = a.w[p];
  const int i = (blockIdx.x - t.start[p]) * SN_MV_ROWS + (threadIdx.x >> 6);
  if (i >= h) return;                                // whole wave leaves together
  const float* __restrict__ W = a.W[p] + (long)i * w;
  const float* __restrict__ v = a.v[p];
  float acc = 0.f;
  for (int j = threadIdx.x & 63; j < w; j += 64) acc += W[j] * v[j];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) a.ws[p][sn_ws_uraw(h, w) + i] = acc;
}

__device__ __forceinline__ float sn_norm_scale(float sumsq, int rule, float eps) {
  const float nrm = sqrtf(sumsq);
  return rule == 0 ? nrm + eps : fmaxf(nrm, eps);    // rule 0: x / (|x| + eps) (l2normalize); rule 1: x / max(|x|, eps) (F.normalize)
}

// One workgroup per problem.  which = 0: v <- norm(sum of the W^T u partials);  which = 1: u <- norm(uraw) when `normalise`, and when
// `last`: sigma = u . uraw and the copies of u, v for the backward.  save = [sigma | u (h) | v (w)].
__global__ __launch_bounds__(WG) void sn_fin_kernel(const spgan_sn_args a, int which, int normalise, int last, int rule, float eps) {
  __shared__ float red[4];
  const int p = blockIdx.x;
  const int h = a.h[p], w = a.w[p];
  if (which == 0) {
    const float* __restrict__ part = a.ws[p];
    float* __restrict__ v = a.v[p];
    const int chunks = sn_chunks(h);
    float ss = 0.f;
    for (int j = threadIdx.x; j < w; j += WG) {
      float x = 0.f;
      int c = 0;
      for (; c + 8 <= chunks; c += 8) {               // eight loads in flight, added in ascending order
        float t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = part[(long)(c + q) * w + j];
#pragma unroll
        for (int q = 0; q < 8; ++q) x += t[q];
      }
      for (; c < chunks; ++c) x += part[(long)c * w + j];
      v[j] = x;
      ss += x * x;
    }
    const float d = sn_norm_scale(block_sum(ss, red), rule, eps);
    for (int j = threadIdx.x; j < w; j += WG) v[j] = v[j] / d;        // the thread's own elements
    return;
  }
  const float* __restrict__ uraw = a.ws[p] + sn_ws_uraw(h, w);
  float* __restrict__ u = a.u[p];
  if (normalise) {
    float ss = 0.f;
    for (int i = threadIdx.x; i < h; i += WG) ss += uraw[i] * uraw[i];
    const float d = sn_norm_scale(block_sum(ss, red), rule, eps);
    for (int i = threadIdx.x; i < h; i += WG) u[i] = uraw[i] / d;
  }
  if (!last) return;
  float* __restrict__ save = a.save[p];
  float dot = 0.f;
  for (int i = threadIdx.x; i < h; i += WG) {
    const float ui = u[i];
    dot += ui * uraw[i];
    save[1 + i] = ui;
  }
  const float* __restrict__ v = a.v[p];
  for (int j = threadIdx.x; j < w; j += WG) save[1 + h + j] = v[j];
  dot = block_sum(dot, red);
  if (threadIdx.x == 0) save[0] = dot;
}

// out = W / sigma
__global__ __launch_bounds__(WG) void sn_apply_kernel(const spgan_sn_args a, const SnTiles t) {
  const int p = find_problem(t.start, a.count, blockIdx.x);
  const long n = (long)a.h[p] * a.w[p];
  const long e0 = (long)(blockIdx.x - t.start[p]) * SN_TILE;
  const float sigma = a.save[p][0];
  const float* __restrict__ W = a.W[p];
  float* __restrict__ out = a.out[p];
#pragma unroll
  for (int k = 0; k < SN_TILE / WG; ++k) {
    const long e = e0 + k * WG + threadIdx.x;
    if (e < n) out[e] = W[e] / sigma;
  }
}

// partial <G, W> of one tile
__global__ __launch_bounds__(WG) void sn_dot_kernel(const spgan_sn_args a, const SnTiles t) {
  __shared__ float red[4];
  const int p = find_problem(t.start, a.count, blockIdx.x);
  const int h = a.h[p], w = a.w[p];
  const long n = (long)h * w;
  const int lt = blockIdx.x - t.start[p];
  const long e0 = (long)lt * SN_TILE;
  const float* __restrict__ W = a.W[p];
  const float* __restrict__ G = a.G[p];
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < SN_TILE / WG; ++k) {
    const long e = e0 + k * WG + threadIdx.x;
    if (e < n) acc += G[e] * W[e];
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) a.ws[p][sn_ws_dot(h, w) + lt] = acc;
}

// dW = G / sigma - (<G,W> / sigma^2) u v^T; every workgroup sums its problem's dot partials in the same order
__global__ __launch_bounds__(WG) void sn_bwd_apply_kernel(const spgan_sn_args a, const SnTiles t) {
  __shared__ float red[4];
  const int p = find_problem(t.start, a.count, blockIdx.x);
  const int h = a.h[p], w = a.w[p];
  const long n = (long)h * w;
  const int tiles = sn_elem_tiles(h, w);
  const float* __restrict__ part = a.ws[p] + sn_ws_dot(h, w);
  float acc = 0.f;
  for (int i = threadIdx.x; i < tiles; i += WG) acc += part[i];
  const float dot = block_sum(acc, red);
  const float* __restrict__ save = a.save[p];
  const float sigma = save[0];
  const float coef = dot / (sigma * sigma);
  const float* __restrict__ u = save + 1;
  const float* __restrict__ v = save + 1 + h;
  const float* __restrict__ G = a.G[p];
  float* __restrict__ dW = a.dW[p];
  const long e0 = (long)(blockIdx.x - t.start[p]) * SN_TILE;
#pragma unroll
  for (int k = 0; k < SN_TILE / WG; ++k) {
    const long e = e0 + k * WG + threadIdx.x;
    if (e < n) {
      const unsigned eu = (unsigned)e, i = eu / (unsigned)w, j = eu - i * (unsigned)w;      // n < 2^31
      dW[e] = G[e] / sigma - coef * (u[i] * v[j]);
    }
  }
}

int sn_check(const spgan_sn_args* a, bool fwd) {
  SPGAN_CHECK_ARG(a && a->count > 0 && a->count <= SPGAN_SN_MAX);
  for (int p = 0; p < a->count; ++p) {
    SPGAN_CHECK_ARG(a->h[p] > 0 && a->w[p] > 0 && (long)a->h[p] * a->w[p] < (1l << 31));
    SPGAN_CHECK_ARG(a->W[p] && a->save[p] && a->ws[p]);
    if (fwd) SPGAN_CHECK_ARG(a->u[p] && a->v[p] && a->out[p]);
    else SPGAN_CHECK_ARG(a->G[p] && a->dW[p]);
  }
  return SPGAN_OK;
}

template <class F>
bool sn_tiles(const spgan_sn_args* a, SnTiles* t, F per_problem) {
  long total = 0;
  for (int p = 0; p < a->count; ++p) {
    t->start[p] = (int)total;
    total += per_problem(a->h[p], a->w[p]);
    if (total >= (1l << 30)) return false;
  }
  t->start[a->count] = (int)total;
  return true;
}

// ------------------------------------------------------------------------------------------------ minibatch stddev
constexpr int MB_TILE = 1024;     // points per workgroup: 4 per thread, stride 256
constexpr int MB_REG = 16;        // group sizes up to this are held in registers; larger ones are read again (from cache)

// grid: (m, c, tile).  Copies x into out[:, :C] and writes the tile's sum of std over its points to part[(m*C + c)*tiles + tile].
template <int GREG>
__global__ __launch_bounds__(WG) void mbstd_fwd_kernel(const float* __restrict__ x, int M, int G, int C, int F, int N, float alpha,
                                                       float* __restrict__ out, float* __restrict__ part) {
  __shared__ float red[4];
  const int tiles = (N + MB_TILE - 1) / MB_TILE;
  const int tile = blockIdx.x % tiles;
  const int mc = blockIdx.x / tiles, c = mc % C, m = mc / C;
  const long xs = (long)M * C * N, os = (long)M * (C + F) * N;       // stride of g
  const float* __restrict__ xp = x + ((long)m * C + c) * N;
  float* __restrict__ op = out + ((long)m * (C + F) + c) * N;
  float acc = 0.f;
  for (int k = 0; k < MB_TILE / WG; ++k) {
    const int n = tile * MB_TILE + k * WG + threadIdx.x;
    if (n >= N) break;
    float xv[GREG > 0 ? GREG : 1];
    float s = 0.f;
    if (GREG > 0) {
#pragma unroll
      for (int g = 0; g < GREG; ++g)
        if (g < G) {
          xv[g] = xp[g * xs + n];
          op[g * os + n] = xv[g];
          s += xv[g];
        }
    } else {
      for (int g = 0; g < G; ++g) {
        const float v = xp[g * xs + n];
        op[g * os + n] = v;
        s += v;
      }
    }
    const float mean = s / (float)G;
    float q = 0.f;
    if (GREG > 0) {
#pragma unroll
      for (int g = 0; g < GREG; ++g)
        if (g < G) q += (xv[g] - mean) * (xv[g] - mean);
    } else {
      for (int g = 0; g < G; ++g) {
        const float d = xp[g * xs + n] - mean;
        q += d * d;
      }
    }
    acc += sqrtf(q / (float)G + alpha);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// grid: (b, f, tile).  stat[m, f] = mean of the partials of the feature group's channels; fills out[b, C + f, tile]
__global__ __launch_bounds__(WG) void mbstd_fill_kernel(const float* __restrict__ part, int M, int G, int C, int F, int N,
                                                        float* __restrict__ out) {
  __shared__ float red[4];
  const int tiles = (N + MB_TILE - 1) / MB_TILE;
  const int tile = blockIdx.x % tiles;
  const int bf = blockIdx.x / tiles, f = bf % F, b = bf / F, m = b % M;
  const int Cp = C / F, cnt = Cp * tiles;
  const float* __restrict__ pp = part + ((long)m * C + (long)f * Cp) * tiles;
  float acc = 0.f;
  for (int i = threadIdx.x; i < cnt; i += WG) acc += pp[i];
  const float stat = block_sum(acc, red) / ((float)Cp * (float)N);
  float* __restrict__ op = out + ((long)b * (C + F) + C + f) * N;
  for (int k = 0; k < MB_TILE / WG; ++k) {
    const int n = tile * MB_TILE + k * WG + threadIdx.x;
    if (n < N) op[n] = stat;
  }
}

// S[m, f] = sum over g (ascending) and n of dout[g*M + m, C + f, n]: one workgroup per (m, f)
__global__ __launch_bounds__(WG) void mbstd_bwd_sum_kernel(const float* __restrict__ dout, int M, int G, int C, int F, int N,
                                                           float* __restrict__ S) {
  __shared__ float red[4];
  const int f = blockIdx.x % F, m = blockIdx.x / F;
  float acc = 0.f;
  for (int g = 0; g < G; ++g) {
    const float* __restrict__ dp = dout + ((long)(g * M + m) * (C + F) + C + f) * N;
    for (int n = threadIdx.x; n < N; n += WG) acc += dp[n];
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) S[blockIdx.x] = acc;
}

// dx = dout[:, :C] + S (x - mean) / (G std C' N)
template <int GREG>
__global__ __launch_bounds__(WG) void mbstd_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                       const float* __restrict__ S, int M, int G, int C, int F, int N, float alpha,
                                                       float* __restrict__ dx) {
  const int tiles = (N + MB_TILE - 1) / MB_TILE;
  const int tile = blockIdx.x % tiles;
  const int mc = blockIdx.x / tiles, c = mc % C, m = mc / C;
  const int Cp = C / F;
  const long xs = (long)M * C * N, os = (long)M * (C + F) * N;
  const float* __restrict__ xp = x + ((long)m * C + c) * N;
  const float* __restrict__ dp = dout + ((long)m * (C + F) + c) * N;
  float* __restrict__ gp = dx + ((long)m * C + c) * N;
  const float coef = S[m * F + c / Cp] / ((float)G * (float)Cp * (float)N);
  for (int k = 0; k < MB_TILE / WG; ++k) {
    const int n = tile * MB_TILE + k * WG + threadIdx.x;
    if (n >= N) break;
    float xv[GREG > 0 ? GREG : 1];
    float s = 0.f;
    if (GREG > 0) {
#pragma unroll
      for (int g = 0; g < GREG; ++g)
        if (g < G) {
          xv[g] = xp[g * xs + n];
          s += xv[g];
        }
    } else {
      for (int g = 0; g < G; ++g) s += xp[g * xs + n];
    }
    const float mean = s / (float)G;
    float q = 0.f;
    if (GREG > 0) {
#pragma unroll
      for (int g = 0; g < GREG; ++g)
        if (g < G) q += (xv[g] - mean) * (xv[g] - mean);
    } else {
      for (int g = 0; g < G; ++g) {
        const float d = xp[g * xs + n] - mean;
        q += d * d;
      }
    }
    const float k2 = coef / sqrtf(q / (float)G + alpha);
    if (GREG > 0) {
#pragma unroll
      for (int g = 0; g < GREG; ++g)
        if (g < G) gp[g * xs + n] = dp[g * os + n] + k2 * (xv[g] - mean);
    } else {
      for (int g = 0; g < G; ++g) gp[g * xs + n] = dp[g * os + n] + k2 * (xp[g * xs + n] - mean);
    }
  }
}

// ------------------------------------------------------------------------------------------------ layer epilogue
constexpr int EP_K = 4;               // points per lane of the column passes
constexpr int EP_L = 64 * EP_K;       // points per workgroup: lane i owns the points i, 64 + i, ...
constexpr int EP_WAVES = 8;           // wave k owns the channels c = k (mod EP_WAVES) of these points
constexpr int EP_WG = 64 * EP_WAVES;

struct Epi {                       // the device-side view of spgan_epilogue_args
  const float* x; const float* noise; const float* w; const float* gamma; const float* beta; int ld_gb;
  int B, C, L, act, pn, stats; float slope, pn_eps, in_eps;
};

__device__ __forceinline__ float epi_act(const Epi& e, float z) { return e.act == 0 ? z : (e.act == 1 ? fmaxf(z, 0.f) : lrelu_f(z, e.slope)); }
__device__ __forceinline__ float epi_dact(const Epi& e, float z) { return e.act == 0 ? 1.f : (z > 0.f ? 1.f : (e.act == 1 ? 0.f : e.slope)); }
// rs[b,l]: form 1 (PixelNorm) holds rsqrt(mean + eps) and t = a * rs; form 2 (PixelwiseNorm) holds sqrt(mean + eps) and t = a / rs
__device__ __forceinline__ float epi_pn(const Epi& e, float a, float rs) { return e.pn == 0 ? a : (e.pn == 1 ? a * rs : a / rs); }
__device__ __forceinline__ float epi_rs(const Epi& e, float meansq) {
  return e.pn == 1 ? 1.f / sqrtf(meansq + e.pn_eps) : sqrtf(meansq + e.pn_eps);
}

// sum over the waves (ascending) of the per-lane values of each owned point: every thread gets the totals of its points
__device__ __forceinline__ void point_sum(float (&v)[EP_K], float (*buf)[EP_L]) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EP_K; ++k) buf[wv][k * 64 + lane] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EP_K; ++k) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < EP_WAVES; ++q) s += buf[q][k * 64 + lane];
    v[k] = s;
  }
}

// the points of a lane: index, validity, noise value, pixel-norm factor
struct EpiPts {
  int l[EP_K]; bool ok[EP_K]; float nz[EP_K]; float r[EP_K];
  __device__ __forceinline__ EpiPts(const Epi& e, int b, int tile, const float* rs) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < EP_K; ++k) {
      l[k] = tile * EP_L + k * 64 + lane;
      ok[k] = l[k] < e.L;
      nz[k] = (e.noise && ok[k]) ? e.noise[(long)b * e.L + l[k]] : 0.f;
      r[k] = (rs && ok[k]) ? rs[(long)b * e.L + l[k]] : 1.f;
    }
  }
};

// The channel loop of the column passes: wave wv visits c = wv, wv + EP_WAVES, ...; the x (and dy) values of EP_U channels are loaded
// before the first of them is used, so that EP_U * EP_K loads per lane are in flight.  body(c, x[EP_K], dy[EP_K]) runs in ascending c.
constexpr int EP_U = 4;
template <class F>
__device__ __forceinline__ void for_channels(const Epi& e, const EpiPts& pt, int b, const float* __restrict__ dy, F body) {
  const float* __restrict__ xb = e.x + (long)b * e.C * e.L;
  const float* __restrict__ db = dy ? dy + (long)b * e.C * e.L : nullptr;
  for (int c0 = threadIdx.x >> 6; c0 < e.C; c0 += EP_U * EP_WAVES) {
    float xv[EP_U][EP_K], dv[EP_U][EP_K];
#pragma unroll
    for (int q = 0; q < EP_U; ++q) {
      const int c = c0 + q * EP_WAVES;
#pragma unroll
      for (int k = 0; k < EP_K; ++k) {
        const bool ok = c < e.C && pt.ok[k];
        xv[q][k] = ok ? xb[(long)c * e.L + pt.l[k]] : 0.f;
        dv[q][k] = (ok && db) ? db[(long)c * e.L + pt.l[k]] : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < EP_U; ++q) {
      const int c = c0 + q * EP_WAVES;
      if (c < e.C) body(c, xv[q], dv[q]);
    }
  }
}

// Forward column pass, grid (b, tile of EP_L points).  Writes rs[b,l] (pn) and, with statistics on, the per-(b, c, tile) record
// (sum of t, centred M2 of t) over the tile's points: shifted sums around the tile's first value of the channel, M2 = S2 - S1^2 / n.
// With statistics off (pn only) it writes y = PN(act(..)) directly.
__global__ __launch_bounds__(EP_WG) void epi_fwd_col_kernel(const Epi e, float* __restrict__ rs_out, float* __restrict__ rec,
                                                            float* __restrict__ y) {
  __shared__ float buf[EP_WAVES][EP_L];
  const int tiles = (e.L + EP_L - 1) / EP_L;
  const int tile = blockIdx.x % tiles, b = blockIdx.x / tiles;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cnt = min(EP_L, e.L - tile * EP_L);
  EpiPts pt(e, b, tile, nullptr);
  if (e.pn) {
    float ss[EP_K] = {};
    for_channels(e, pt, b, nullptr, [&](int c, const float (&x)[EP_K], const float (&)[EP_K]) {
      const float wc = e.noise ? e.w[c] : 0.f;
#pragma unroll
      for (int k = 0; k < EP_K; ++k)
        if (pt.ok[k]) {
          const float a = epi_act(e, x[k] + wc * pt.nz[k]);
          ss[k] += a * a;
        }
    });
    point_sum(ss, buf);
#pragma unroll
    for (int k = 0; k < EP_K; ++k) {
      pt.r[k] = epi_rs(e, ss[k] / (float)e.C);
      if (pt.ok[k] && wv == 0) rs_out[(long)b * e.L + pt.l[k]] = pt.r[k];
    }
  }
  for_channels(e, pt, b, nullptr, [&](int c, const float (&x)[EP_K], const float (&)[EP_K]) {
    const float wc = e.noise ? e.w[c] : 0.f;
    float t[EP_K];
#pragma unroll
    for (int k = 0; k < EP_K; ++k) t[k] = pt.ok[k] ? epi_pn(e, epi_act(e, x[k] + wc * pt.nz[k]), pt.r[k]) : 0.f;
    if (!e.stats) {
#pragma unroll
      for (int k = 0; k < EP_K; ++k)
        if (pt.ok[k]) y[((long)b * e.C + c) * e.L + pt.l[k]] = t[k];
      return;
    }
    const float pivot = __shfl(t[0], 0);             // the tile's first point: always inside
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < EP_K; ++k) {
      const float d = pt.ok[k] ? t[k] - pivot : 0.f;
      s1 += d;
      s2 += d * d;
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
      float* r = rec + (((long)b * e.C + c) * tiles + tile) * 2;
      r[0] = (float)cnt * pivot + s1;
      r[1] = fmaxf(s2 - s1 * s1 / (float)cnt, 0.f);
    }
  });
}

// Chan's merge of (n, mean, M2) records in double; the order of the merges is fixed by the caller
struct Mom { double n, mean, m2; };
__device__ __forceinline__ void mom_merge(Mom& a, double n, double mean, double m2) {
  if (n == 0.0) return;
  const double tot = a.n + n, d = mean - a.mean;
  a.mean += d * (n / tot);
  a.m2 += m2 + d * d * (a.n * n / tot);
  a.n = tot;
}

// One workgroup per b: the tile records of a channel merged in ascending tile order by one thread; stats 1: stat[b, c] = (mean, invstd);
// stats 2 (joint over C*L): a thread's channels merged in ascending order, the threads' records by a fixed binary tree, stat[b] = (mean, invstd).
__global__ __launch_bounds__(WG) void epi_fwd_fin_kernel(const float* __restrict__ rec, int C, int L, int stats, float eps,
                                                         float* __restrict__ stat) {
  __shared__ double sh[WG][3];
  const int tiles = (L + EP_L - 1) / EP_L;
  const int b = blockIdx.x;
  Mom mine = {0.0, 0.0, 0.0};
  for (int c = threadIdx.x; c < C; c += WG) {
    Mom ch = {0.0, 0.0, 0.0};
    const float* r = rec + ((long)b * C + c) * tiles * 2;
    for (int t = 0; t < tiles; ++t) {
      const double n = (double)min(EP_L, L - t * EP_L);
      mom_merge(ch, n, (double)r[2 * t] / n, (double)r[2 * t + 1]);
    }
    if (stats == 1) {
      stat[((long)b * C + c) * 2] = (float)ch.mean;
      stat[((long)b * C + c) * 2 + 1] = (float)(1.0 / sqrt(ch.m2 / ch.n + (double)eps));
    } else {
      mom_merge(mine, ch.n, ch.mean, ch.m2);
    }
  }
  if (stats != 2) return;
  sh[threadIdx.x][0] = mine.n; sh[threadIdx.x][1] = mine.mean; sh[threadIdx.x][2] = mine.m2;
  for (int stride = 1; stride < WG; stride <<= 1) {           // a fixed binary tree over the threads' records: left operand first
    __syncthreads();
    if ((threadIdx.x & (2 * stride - 1)) == 0) {
      Mom m = {sh[threadIdx.x][0], sh[threadIdx.x][1], sh[threadIdx.x][2]};
      mom_merge(m, sh[threadIdx.x + stride][0], sh[threadIdx.x + stride][1], sh[threadIdx.x + stride][2]);
      sh[threadIdx.x][0] = m.n; sh[threadIdx.x][1] = m.mean; sh[threadIdx.x][2] = m.m2;
    }
  }
  if (threadIdx.x == 0) {
    stat[(long)b * 2] = (float)sh[0][1];
    stat[(long)b * 2 + 1] = (float)(1.0 / sqrt(sh[0][2] / sh[0][0] + (double)eps));
  }
}

// Element-wise forward, grid (row b*C + c, chunk of EA_L points): y = gamma * (t - mean) * invstd + beta with t recomputed from x, noise
// and rs.  Also the whole layer when there is neither pixel norm nor statistics.
constexpr int EA_L = 4 * WG;
__global__ __launch_bounds__(WG) void epi_fwd_apply_kernel(const Epi e, const float* __restrict__ rs, const float* __restrict__ stat,
                                                           float* __restrict__ y) {
  const unsigned chunks = (unsigned)(e.L + EA_L - 1) / EA_L;
  const unsigned bc = blockIdx.x / chunks, chunk = blockIdx.x - bc * chunks;
  const unsigned b = bc / (unsigned)e.C, c = bc - b * (unsigned)e.C;
  const float wc = e.noise ? e.w[c] : 0.f;
  float mean = 0.f, is = 1.f, gm = 1.f, bt = 0.f;
  if (e.stats) {
    const float* st = stat + (e.stats == 1 ? (long)bc : (long)b) * 2;
    mean = st[0];
    is = st[1];
  }
  if (e.gamma) {
    gm = e.gamma[(long)b * e.ld_gb + c];
    bt = e.beta[(long)b * e.ld_gb + c];
  }
  const float* __restrict__ xr = e.x + (long)bc * e.L;
  const float* __restrict__ nr = e.noise ? e.noise + (long)b * e.L : nullptr;
  const float* __restrict__ rr = e.pn ? rs + (long)b * e.L : nullptr;
  float* __restrict__ yr = y + (long)bc * e.L;
#pragma unroll
  for (int k = 0; k < EA_L / WG; ++k) {
    const int l = chunk * EA_L + k * WG + threadIdx.x;
    if (l < e.L) {
      float z = xr[l];
      if (nr) z += wc * nr[l];
      float t = epi_pn(e, epi_act(e, z), rr ? rr[l] : 1.f);
      if (e.stats) t = (t - mean) * is;
      if (e.gamma) t = gm * t + bt;
      yr[l] = t;
    }
  }
}

// Backward reduction, grid (b, tile): per-(b, c, tile) sums of dy and dy * yhat (yhat = (t - mean) * invstd; t when statistics are off)
__global__ __launch_bounds__(EP_WG) void epi_bwd_red_kernel(const Epi e, const float* __restrict__ dy, const float* __restrict__ rs,
                                                            const float* __restrict__ stat, float* __restrict__ rec) {
  const int tiles = (e.L + EP_L - 1) / EP_L;
  const int tile = blockIdx.x % tiles, b = blockIdx.x / tiles;
  const int lane = threadIdx.x & 63;
  EpiPts pt(e, b, tile, e.pn ? rs : nullptr);
  for_channels(e, pt, b, dy, [&](int c, const float (&x)[EP_K], const float (&d)[EP_K]) {
    const float wc = e.noise ? e.w[c] : 0.f;
    float mean = 0.f, is = 1.f;
    if (e.stats) {
      const float* st = stat + (e.stats == 1 ? (long)b * e.C + c : (long)b) * 2;
      mean = st[0];
      is = st[1];
    }
    float g = 0.f, gy = 0.f;
#pragma unroll
    for (int k = 0; k < EP_K; ++k)
      if (pt.ok[k]) {
        float t = epi_pn(e, epi_act(e, x[k] + wc * pt.nz[k]), pt.r[k]);
        if (e.stats) t = (t - mean) * is;
        g += d[k];
        gy += d[k] * t;
      }
    g = wave_sum(g);
    gy = wave_sum(gy);
    if (lane == 0) {
      float* o = rec + (((long)b * e.C + c) * tiles + tile) * 2;
      o[0] = g;
      o[1] = gy;
    }
  });
}

// One workgroup per b: sums[b, c] = (sum dy, sum dy*yhat) over the tiles in ascending order -> dbeta, dgamma (rows of ld_d floats);
// grp[b, c] (stats 1) or grp[b] (stats 2) = (mean of g1, mean of g1*yhat) with g1 = gamma * dy, the two means the statistics' backward needs.
__global__ __launch_bounds__(WG) void epi_bwd_fin_kernel(const float* __restrict__ rec, const float* __restrict__ gamma, int ld_gb, int C,
                                                         int L, int stats, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                         int ld_d, float* __restrict__ grp) {
  __shared__ float sh[WG][2];
  const int tiles = (L + EP_L - 1) / EP_L;
  const int b = blockIdx.x;
  float ja = 0.f, jb = 0.f;
  for (int c = threadIdx.x; c < C; c += WG) {
    const float* r = rec + ((long)b * C + c) * tiles * 2;
    float s0 = 0.f, s1 = 0.f;
    for (int t = 0; t < tiles; ++t) {
      s0 += r[2 * t];
      s1 += r[2 * t + 1];
    }
    if (dgamma) {
      dbeta[(long)b * ld_d + c] = s0;
      dgamma[(long)b * ld_d + c] = s1;
    }
    const float gm = gamma ? gamma[(long)b * ld_gb + c] : 1.f;
    if (stats == 1) {
      grp[((long)b * C + c) * 2] = gm * s0 / (float)L;
      grp[((long)b * C + c) * 2 + 1] = gm * s1 / (float)L;
    } else {
      ja += gm * s0;
      jb += gm * s1;
    }
  }
  if (stats != 2) return;
  sh[threadIdx.x][0] = ja; sh[threadIdx.x][1] = jb;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, bb = 0.f;
    for (int i = 0; i < WG; ++i) {
      a += sh[i][0];
      bb += sh[i][1];
    }
    const float n = (float)C * (float)L;
    grp[(long)b * 2] = a / n;
    grp[(long)b * 2 + 1] = bb / n;
  }
}

// the cotangent of t at one element: the affine, then the statistics' backward
__device__ __forceinline__ float epi_dt(const Epi& e, float g, float t, int b, int c, const float* stat, const float* grp) {
  if (e.gamma) g *= e.gamma[(long)b * e.ld_gb + c];
  if (!e.stats) return g;
  const long s = (e.stats == 1 ? (long)b * e.C + c : (long)b) * 2;
  const float yh = (t - stat[s]) * stat[s + 1];
  return stat[s + 1] * (g - grp[s] - yh * grp[s + 1]);
}

// Backward column pass, grid (b, tile): dx, dnoise[b, l] = sum_c dz * w[c], and the per-(b, c, tile) sums of dz * noise (-> dw)
__global__ __launch_bounds__(EP_WG) void epi_bwd_col_kernel(const Epi e, const float* __restrict__ dy, const float* __restrict__ rs,
                                                            const float* __restrict__ stat, const float* __restrict__ grp,
                                                            float* __restrict__ dx, float* __restrict__ dnoise, float* __restrict__ wrec) {
  __shared__ float buf[EP_WAVES][EP_L];
  const int tiles = (e.L + EP_L - 1) / EP_L;
  const int tile = blockIdx.x % tiles, b = blockIdx.x / tiles;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  EpiPts pt(e, b, tile, e.pn ? rs : nullptr);
  float rinv[EP_K], pk[EP_K];                         // d t / d a at fixed norm;  sum_c (dt * a) * rinv^3 / C
#pragma unroll
  for (int k = 0; k < EP_K; ++k) {
    rinv[k] = e.pn == 2 ? 1.f / pt.r[k] : pt.r[k];
    pk[k] = 0.f;
  }
  if (e.pn) {
    for_channels(e, pt, b, dy, [&](int c, const float (&x)[EP_K], const float (&d)[EP_K]) {
      const float wc = e.noise ? e.w[c] : 0.f;
#pragma unroll
      for (int k = 0; k < EP_K; ++k)
        if (pt.ok[k]) {
          const float a = epi_act(e, x[k] + wc * pt.nz[k]);
          pk[k] += epi_dt(e, d[k], epi_pn(e, a, pt.r[k]), b, c, stat, grp) * a;
        }
    });
    point_sum(pk, buf);
#pragma unroll
    for (int k = 0; k < EP_K; ++k) pk[k] = pk[k] * rinv[k] * rinv[k] * rinv[k] / (float)e.C;
  }
  float dn[EP_K] = {};
  for_channels(e, pt, b, dy, [&](int c, const float (&x)[EP_K], const float (&d)[EP_K]) {
    const float wc = e.noise ? e.w[c] : 0.f;
    float dzn = 0.f;
#pragma unroll
    for (int k = 0; k < EP_K; ++k)
      if (pt.ok[k]) {
        const float z = x[k] + wc * pt.nz[k];
        const float a = epi_act(e, z);
        const float dt = epi_dt(e, d[k], epi_pn(e, a, pt.r[k]), b, c, stat, grp);
        const float da = e.pn ? dt * rinv[k] - a * pk[k] : dt;
        const float dz = da * epi_dact(e, z);
        if (dx) dx[((long)b * e.C + c) * e.L + pt.l[k]] = dz;
        dn[k] += dz * wc;
        dzn += dz * pt.nz[k];
      }
    if (wrec) {
      dzn = wave_sum(dzn);
      if (lane == 0) wrec[((long)b * e.C + c) * tiles + tile] = dzn;
    }
  });
  if (dnoise) {
    point_sum(dn, buf);
#pragma unroll
    for (int k = 0; k < EP_K; ++k)
      if (pt.ok[k] && wv == 0) dnoise[(long)b * e.L + pt.l[k]] = dn[k];
  }
}

// dw[c] = sum over b and tiles (ascending) of wrec: one thread per channel
__global__ __launch_bounds__(WG) void epi_dw_kernel(const float* __restrict__ wrec, int B, int C, int tiles, float* __restrict__ dw) {
  const int c = blockIdx.x * WG + threadIdx.x;
  if (c >= C) return;
  float acc = 0.f;
  const int n = B * tiles;                            // record i = b * tiles + t, ascending
  int i = 0;
  for (; i + 8 <= n; i += 8) {                        // eight loads in flight, added in ascending order
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int b = (i + q) / tiles, t = (i + q) - b * tiles;
      v[q] = wrec[((long)b * C + c) * tiles + t];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) acc += v[q];
  }
  for (; i < n; ++i) {
    const int b = i / tiles, t = i - b * tiles;
    acc += wrec[((long)b * C + c) * tiles + t];
  }
  dw[c] = acc;
}

int epi_make(const spgan_epilogue_args* a, Epi* e) {
  SPGAN_CHECK_ARG(a && a->x && a->B > 0 && a->C > 0 && a->C <= SPGAN_EPILOGUE_MAX_C && a->L > 0);
  SPGAN_CHECK_ARG((long)a->B * a->C * a->L < (1l << 31));
  SPGAN_CHECK_ARG(a->act >= 0 && a->act <= 2 && a->pn >= 0 && a->pn <= 2 && a->stats >= 0 && a->stats <= 2);
  SPGAN_CHECK_ARG((a->noise != nullptr) == (a->w != nullptr));
  SPGAN_CHECK_ARG((a->gamma != nullptr) == (a->beta != nullptr) && (!a->gamma || a->ld_gb >= a->C));
  SPGAN_CHECK_ARG(!a->pn || (a->rs && a->pn_eps >= 0.f));
  SPGAN_CHECK_ARG(!a->stats || (a->stat && a->rec && a->in_eps >= 0.f && (long)a->C * a->L > 1));
  *e = Epi{a->x, a->noise, a->w, a->gamma, a->beta, a->ld_gb, a->B, a->C, a->L, a->act, a->pn, a->stats, a->slope, a->pn_eps, a->in_eps};
  return SPGAN_OK;
}

int elem_blocks(long total) {
  long b = (total + WG * 4 - 1) / (WG * 4);
  return (int)(b > 4096 ? 4096 : b);
}

// ------------------------------------------------------------------------------------------------ truncation
// out[b, l, d] = l < max_layer ? lerp(avg[l or 0, d], x, thr) : x   (torch.lerp's two-sided formula);  backward: dx = dout * (thr | 1)
__global__ __launch_bounds__(WG) void truncation_kernel(const float* __restrict__ x, const float* __restrict__ avg, long avg_stride, int Lr,
                                                        int D, long total, int max_layer, float thr, int bwd, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * WG + threadIdx.x; i < total; i += (long)gridDim.x * WG) {
    const int d = (int)(i % D), l = (int)((i / D) % Lr);
    const float v = x[i];
    if (l >= max_layer) {
      out[i] = v;
    } else if (bwd) {
      out[i] = v * thr;
    } else {
      const float a = avg[l * avg_stride + d];
      out[i] = thr < 0.5f ? a + thr * (v - a) : v - (v - a) * (1.f - thr);
    }
  }
}

}  // namespace

extern "C" size_t spgan_sn_ws_floats(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  return (size_t)(sn_ws_dot(h, w) + sn_elem_tiles(h, w));
}

extern "C" int spgan_sn_forward(const spgan_sn_args* a, int n_iter, int rule, float eps, spgan_stream_t s_) {
  if (int st = sn_check(a, true)) return st;
  SPGAN_CHECK_ARG(n_iter >= 0 && n_iter <= 1024 && (rule == 0 || rule == 1) && eps >= 0.f);
  SnTiles tv, tu, te;
  SPGAN_CHECK_ARG(sn_tiles(a, &tv, [](int h, int w) { return (long)sn_chunks(h) * ((w + WG - 1) / WG); }));
  SPGAN_CHECK_ARG(sn_tiles(a, &tu, [](int h, int) { return (long)((h + SN_MV_ROWS - 1) / SN_MV_ROWS); }));
  SPGAN_CHECK_ARG(sn_tiles(a, &te, [](int h, int w) { return (long)sn_elem_tiles(h, w); }));
  hipStream_t s = (hipStream_t)s_;
  for (int it = 0; it < n_iter; ++it) {
    hipLaunchKernelGGL(sn_mvt_kernel, dim3(tv.start[a->count]), dim3(WG), 0, s, *a, tv);
    hipLaunchKernelGGL(sn_fin_kernel, dim3(a->count), dim3(WG), 0, s, *a, 0, 1, 0, rule, eps);
    hipLaunchKernelGGL(sn_mv_kernel, dim3(tu.start[a->count]), dim3(WG), 0, s, *a, tu);
    hipLaunchKernelGGL(sn_fin_kernel, dim3(a->count), dim3(WG), 0, s, *a, 1, 1, it == n_iter - 1 ? 1 : 0, rule, eps);
  }
  if (n_iter == 0) {                                 // eval mode of the hook form: sigma from the stored u, v
    hipLaunchKernelGGL(sn_mv_kernel, dim3(tu.start[a->count]), dim3(WG), 0, s, *a, tu);
    hipLaunchKernelGGL(sn_fin_kernel, dim3(a->count), dim3(WG), 0, s, *a, 1, 0, 1, rule, eps);
  }
  hipLaunchKernelGGL(sn_apply_kernel, dim3(te.start[a->count]), dim3(WG), 0, s, *a, te);
  return spgan_launch_status();
}

extern "C" int spgan_sn_backward(const spgan_sn_args* a, spgan_stream_t s_) {
  if (int st = sn_check(a, false)) return st;
  SnTiles te;
  SPGAN_CHECK_ARG(sn_tiles(a, &te, [](int h, int w) { return (long)sn_elem_tiles(h, w); }));
  hipStream_t s = (hipStream_t)s_;
  hipLaunchKernelGGL(sn_dot_kernel, dim3(te.start[a->count]), dim3(WG), 0, s, *a, te);
  hipLaunchKernelGGL(sn_bwd_apply_kernel, dim3(te.start[a->count]), dim3(WG), 0, s, *a, te);
  return spgan_launch_status();
}

static int mbstd_check(int B, int C, int N, int G, int F) {
  SPGAN_CHECK_ARG(B > 0 && C > 0 && N > 0 && G > 0 && F > 0 && B % G == 0 && C % F == 0);
  SPGAN_CHECK_ARG((long)B * (C + F) * N < (1l << 31));
  const long tiles = (N + MB_TILE - 1) / MB_TILE;
  SPGAN_CHECK_ARG((long)(B / G) * C * tiles < (1l << 30) && (long)B * F * tiles < (1l << 30));
  return SPGAN_OK;
}

extern "C" size_t spgan_mbstd_ws_floats(int B, int C, int N, int G) {
  if (B <= 0 || C <= 0 || N <= 0 || G <= 0 || B % G) return 0;
  return (size_t)(B / G) * C * ((N + MB_TILE - 1) / MB_TILE);
}

extern "C" int spgan_mbstd_forward(const float* x, int B, int C, int N, int G, int F, float alpha, float* out, float* ws, spgan_stream_t s_) {
  if (int st = mbstd_check(B, C, N, G, F)) return st;
  SPGAN_CHECK_ARG(x && out && ws && alpha >= 0.f);
  const int M = B / G, tiles = (N + MB_TILE - 1) / MB_TILE;
  hipStream_t s = (hipStream_t)s_;
  if (G <= 4) hipLaunchKernelGGL(mbstd_fwd_kernel<4>, dim3(M * C * tiles), dim3(WG), 0, s, x, M, G, C, F, N, alpha, out, ws);
  else if (G <= MB_REG) hipLaunchKernelGGL(mbstd_fwd_kernel<MB_REG>, dim3(M * C * tiles), dim3(WG), 0, s, x, M, G, C, F, N, alpha, out, ws);
  else hipLaunchKernelGGL(mbstd_fwd_kernel<0>, dim3(M * C * tiles), dim3(WG), 0, s, x, M, G, C, F, N, alpha, out, ws);
  hipLaunchKernelGGL(mbstd_fill_kernel, dim3(B * F * tiles), dim3(WG), 0, s, ws, M, G, C, F, N, out);
  return spgan_launch_status();
}

extern "C" int spgan_mbstd_backward(const float* x, const float* dout, int B, int C, int N, int G, int F, float alpha, float* dx, float* S,
                                    spgan_stream_t s_) {
  if (int st = mbstd_check(B, C, N, G, F)) return st;
  SPGAN_CHECK_ARG(x && dout && dx && S && alpha >= 0.f);
  const int M = B / G, tiles = (N + MB_TILE - 1) / MB_TILE;
  hipStream_t s = (hipStream_t)s_;
  hipLaunchKernelGGL(mbstd_bwd_sum_kernel, dim3(M * F), dim3(WG), 0, s, dout, M, G, C, F, N, S);
  if (G <= 4) hipLaunchKernelGGL(mbstd_bwd_kernel<4>, dim3(M * C * tiles), dim3(WG), 0, s, x, dout, S, M, G, C, F, N, alpha, dx);
  else if (G <= MB_REG) hipLaunchKernelGGL(mbstd_bwd_kernel<MB_REG>, dim3(M * C * tiles), dim3(WG), 0, s, x, dout, S, M, G, C, F, N, alpha, dx);
  else hipLaunchKernelGGL(mbstd_bwd_kernel<0>, dim3(M * C * tiles), dim3(WG), 0, s, x, dout, S, M, G, C, F, N, alpha, dx);
  return spgan_launch_status();
}

extern "C" size_t spgan_epilogue_rec_floats(int B, int C, int L) {
  if (B <= 0 || C <= 0 || L <= 0) return 0;
  return (size_t)B * C * ((L + EP_L - 1) / EP_L) * 2;
}

extern "C" int spgan_epilogue_forward(const spgan_epilogue_args* a, float* y, spgan_stream_t s_) {
  Epi e;
  if (int st = epi_make(a, &e)) return st;
  SPGAN_CHECK_ARG(y);
  hipStream_t s = (hipStream_t)s_;
  const int tiles = (e.L + EP_L - 1) / EP_L;
  SPGAN_CHECK_ARG((long)e.B * tiles < (1l << 30));
  if (e.pn || e.stats) hipLaunchKernelGGL(epi_fwd_col_kernel, dim3(e.B * tiles), dim3(EP_WG), 0, s, e, a->rs, a->rec, y);
  if (e.stats) hipLaunchKernelGGL(epi_fwd_fin_kernel, dim3(e.B), dim3(WG), 0, s, (const float*)a->rec, e.C, e.L, e.stats, e.in_eps, a->stat);
  if (e.stats || !e.pn || e.gamma)
    hipLaunchKernelGGL(epi_fwd_apply_kernel, dim3(e.B * e.C * ((e.L + EA_L - 1) / EA_L)), dim3(WG), 0, s, e, (const float*)a->rs,
                       (const float*)a->stat, y);
  return spgan_launch_status();
}

extern "C" int spgan_epilogue_backward(const spgan_epilogue_args* a, const float* dy, float* dx, float* dnoise, float* dw, float* dgamma,
                                       float* dbeta, int ld_d, float* grp, spgan_stream_t s_) {
  Epi e;
  if (int st = epi_make(a, &e)) return st;
  SPGAN_CHECK_ARG(dy && (dx || dnoise || dw || dgamma));
  SPGAN_CHECK_ARG((dgamma != nullptr) == (dbeta != nullptr) && (!dgamma || (e.gamma && ld_d >= e.C)));
  SPGAN_CHECK_ARG((!dnoise && !dw) || e.noise);
  const bool red = e.stats || dgamma;
  SPGAN_CHECK_ARG(!red || a->rec);
  SPGAN_CHECK_ARG(!e.stats || grp);
  SPGAN_CHECK_ARG(!dw || a->rec);
  hipStream_t s = (hipStream_t)s_;
  const int tiles = (e.L + EP_L - 1) / EP_L;
  SPGAN_CHECK_ARG((long)e.B * tiles < (1l << 30));
  if (red) {
    hipLaunchKernelGGL(epi_bwd_red_kernel, dim3(e.B * tiles), dim3(EP_WG), 0, s, e, dy, (const float*)a->rs, (const float*)a->stat, a->rec);
    hipLaunchKernelGGL(epi_bwd_fin_kernel, dim3(e.B), dim3(WG), 0, s, (const float*)a->rec, e.gamma, e.ld_gb, e.C, e.L, e.stats, dgamma, dbeta,
                       ld_d, grp);
  }
  if (dx || dnoise || dw) {
    // the dw records reuse rec: its (sum, sum*yhat) records were consumed by the finalising launch above
    hipLaunchKernelGGL(epi_bwd_col_kernel, dim3(e.B * tiles), dim3(EP_WG), 0, s, e, dy, (const float*)a->rs, (const float*)a->stat,
                       (const float*)grp, dx, dnoise, dw ? a->rec : nullptr);
    if (dw) hipLaunchKernelGGL(epi_dw_kernel, dim3((e.C + WG - 1) / WG), dim3(WG), 0, s, (const float*)a->rec, e.B, e.C, tiles, dw);
  }
  return spgan_launch_status();
}

extern "C" int spgan_truncation(const float* x, const float* avg, int avg_per_layer, int B, int Lr, int D, int max_layer, float thr, int bwd,
                                float* out, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(x && out && (bwd || avg) && B > 0 && Lr > 0 && D > 0 && (long)B * Lr * D < (1l << 31));
  const long total = (long)B * Lr * D;
  hipLaunchKernelGGL(truncation_kernel, dim3(elem_blocks(total)), dim3(WG), 0, (hipStream_t)s_, x, avg, avg_per_layer ? (long)D : 0l, Lr, D, total,
                     max_layer, thr, bwd, out);
  return spgan_launch_status();
}
