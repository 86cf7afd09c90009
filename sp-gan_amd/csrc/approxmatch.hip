// The approxmatch earth mover's distance (StructuralLosses.match_cost / tf_approxmatch; Fan, Su and Guibas' soft multi-level transport
// plan), chip-wide and without the [n,m] match matrix.  xyz1 [B,n,3], xyz2 [B,m,3]; k indexes xyz1 (rows), l xyz2 (columns).
//
//   remainL = multiL, remainR = multiR                       multiL = max(n,m)/n, multiR = max(n,m)/m
//   for j = 7 .. -2, level = -(4^j), level(-2) = 0,  E(k,l) = exp(level * d2(k,l)):
//     sweep 1 (row-stationary)     ratioL[k] = remainL[k] / (1e-9 + sum_l E * remainR[l])
//     sweep 2 (column-stationary)  sumr[l] = remainR[l] * sum_k E * ratioL[k];  ratioR[l] = min(remainR / (sumr + 1e-9), 1) * remainR;
//                                  remainR[l] = max(0, remainR - sumr)
//     sweep 3 (row-stationary)     w = E * ratioL[k] * ratioR[l];  remainL[k] = max(0, remainL - sum_l w);  cost += sum_l w * sqrt(d2)
//
// Launch structure: the sweeps are grid-wide launches over (64-point blocks of the stationary cloud) x pairs, ordered by the stream alone.
// Sweep 3 of level j and sweep 1 of level j-1 walk the same columns and need only the remainR that sweep 2 of level j left: they share
// one launch and one d2.  1 (init) + 1 (sweep 1 of level 7) + 10 (sweep 2) + 10 (sweep 3 [+ sweep 1]) + 1 (cost) = 23 launches.
// What the forward keeps is ratioL [B,10,n] and ratioR [B,10,m]; the backward and the dense-plan writer recompute
//   match(k,l) = sum_j E_j(k,l) * ratioL_j[k] * ratioR_j[l]           (plan_entry below: one order for every consumer).
//
// Work placement: one thread per stationary point, the walked cloud staged in LDS tiles that every lane reads at the same address (a
// broadcast, no bank conflicts), so the inner loop is VALU and transcendental issue only.  A block owns 64 stationary points and `WAVES`
// waves; wave w walks the w-th part of every tile, a lane adds its terms into four interleaved accumulators in ascending column order,
// and the waves' partial sums are added in ascending w.  Every order is fixed: no atomics, results repeat bit for bit.
// E and d2 are float32; the sums and the state between the sweeps are float64 (AmState below says why).
#include "common.hpp"

namespace {

constexpr int AM_LEVELS = 10;   // j = 7 .. -2
constexpr int AM_ROWS = 64;     // stationary points per block (one per lane)
constexpr int AM_TILE = 1024;   // walked points per LDS tile of the sweeps
constexpr int AM_GTILE = 256;   // walked points per LDS tile of the backward (16 floats each)

__host__ __device__ __forceinline__ float am_level(int i) {  // i = 0 .. 9  <->  j = 7 .. -2
  return i == AM_LEVELS - 1 ? 0.f : -ldexpf(1.f, 2 * (7 - i));
}

__device__ __forceinline__ float am_d2(float ax, float ay, float az, float bx, float by, float bz, float& dx, float& dy, float& dz) {
  dx = ax - bx; dy = ay - by; dz = az - bz;
  return dx * dx + dy * dy + dz * dz;
}

// The state that crosses the sweeps -- remainL, remainR, the current level's ratioL and ratioR, the per-row cost -- and every sum over
// the walked cloud are float64: remainL - ratioL * sum_l E * ratioR cancels to about 1e-9 of remainL at every row whose columns are not
// oversubscribed, the next level divides that remainder by (1e-9 + a sum that may be 0), and a float32 cancellation (6e-8) would decide the
// result.  E itself is float32 (expf), the same bits in every sweep that meets the pair, so the cancellation is exact where it must be.
struct AmState {
  double* remainL;   // [B,n]
  double* cost_row;  // [B,n]
  double* curL;      // [B,n]  ratioL of the level in flight
  double* remainR;   // [B,m]
  double* curR;      // [B,m]  ratioR of the level in flight
};

__global__ void am_init_kernel(AmState st, size_t bn, size_t bm, double multiL, double multiR) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < bn) { st.remainL[i] = multiL; st.cost_row[i] = 0.; }
  if (i < bm) st.remainR[i] = multiR;
}

// MODE 1: sweep 1 of level `lv`   own = xyz1 row k, walked = xyz2 with remainR;          writes curL and the record ratioL[lv]
// MODE 2: sweep 2 of level `lv`   own = xyz2 column l, walked = xyz1 with curL;          writes curR and ratioR[lv], updates remainR
// MODE 3: sweep 3 of level `lv` and, if lv + 1 < 10, sweep 1 of level lv + 1
//                                 own = xyz1 row k, walked = xyz2 with curR and remainR; updates remainL and cost_row, writes curL, ratioL[lv+1]
template <int MODE, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void am_sweep_kernel(const float* __restrict__ own, long own_stride, int n_own,
                                                              const float* __restrict__ oth, long oth_stride, int n_oth, int lv,
                                                              float* __restrict__ ratioL, float* __restrict__ ratioR, AmState st) {
  constexpr int NT = 64 * WAVES, PART = AM_TILE / WAVES;
  __shared__ float4 tile[AM_TILE];                       // x, y, z, unused
  __shared__ double tw[AM_TILE];                         // the walked point's weight
  __shared__ double tw2[MODE == 3 ? AM_TILE : 1];        // MODE 3: remainR (sweep 1 of the next level)
  __shared__ double part[3][WAVES][AM_ROWS];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * AM_ROWS + lane;
  const bool valid = p < n_own;
  const float* o = own + (size_t)b * own_stride;
  const float* q = oth + (size_t)b * oth_stride;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (valid) { px = o[(size_t)p * 3 + 0]; py = o[(size_t)p * 3 + 1]; pz = o[(size_t)p * 3 + 2]; }
  const double* wgt = (MODE == 1 ? st.remainR : MODE == 2 ? st.curL : st.curR) + (size_t)b * n_oth;
  const double* wgt2 = st.remainR + (size_t)b * n_oth;
  const float level = am_level(lv), level2 = am_level(min(lv + 1, AM_LEVELS - 1));
  double a0[4] = {0., 0., 0., 0.}, a1[4] = {0., 0., 0., 0.}, a2[4] = {0., 0., 0., 0.};
  for (int t0 = 0; t0 < n_oth; t0 += AM_TILE) {
    const int cnt = min(AM_TILE, n_oth - t0);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += NT) {
      const size_t g = (size_t)(t0 + i);
      tile[i] = make_float4(q[g * 3 + 0], q[g * 3 + 1], q[g * 3 + 2], 0.f);
      tw[i] = wgt[g];
      if (MODE == 3) tw2[i] = wgt2[g];
    }
    __syncthreads();
    const int lo = wave * PART, hi = min(cnt, lo + PART);
    auto term = [&](int i, double& s0, double& s1, double& s2) {
      const float4 c = tile[i];
      float dx, dy, dz;
      const float d2 = am_d2(px, py, pz, c.x, c.y, c.z, dx, dy, dz);
      const double e = (double)expf(level * d2);
      if (MODE == 3) {
        const double t = e * tw[i];
        s0 += t;
        s1 = fma(t, (double)sqrtf(d2), s1);
        s2 = fma((double)expf(level2 * d2), tw2[i], s2);
      } else {
        s0 = fma(e, tw[i], s0);
      }
    };
    int i = lo;
    for (; i + 4 <= hi; i += 4) {                          // point i of the part goes to accumulator (i - lo) % 4
#pragma unroll
      for (int u = 0; u < 4; ++u) term(i + u, a0[u], a1[u], a2[u]);
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (i + u < hi) term(i + u, a0[u], a1[u], a2[u]);
  }
  part[0][wave][lane] = (a0[0] + a0[1]) + (a0[2] + a0[3]);
  if (MODE == 3) {
    part[1][wave][lane] = (a1[0] + a1[1]) + (a1[2] + a1[3]);
    part[2][wave][lane] = (a2[0] + a2[1]) + (a2[2] + a2[3]);
  }
  __syncthreads();
  if (wave != 0 || !valid) return;
  double s0 = part[0][0][lane], s1 = 0., s2 = 0.;
  if (MODE == 3) { s1 = part[1][0][lane]; s2 = part[2][0][lane]; }
#pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    s0 += part[0][w][lane];
    if (MODE == 3) { s1 += part[1][w][lane]; s2 += part[2][w][lane]; }
  }
  const size_t row = (size_t)b * n_own + p;
  const size_t rec = ((size_t)b * AM_LEVELS + lv) * n_own + p;
  if (MODE == 1) {
    const double rl = st.remainL[row] / (1e-9 + s0);
    st.curL[row] = rl;
    ratioL[rec] = (float)rl;
  } else if (MODE == 2) {
    const double r = st.remainR[row];
    const double sumr = r * s0;
    const double rr = fmin(r / (sumr + 1e-9), 1.) * r;
    st.curR[row] = rr;
    ratioR[rec] = (float)rr;
    st.remainR[row] = fmax(0., r - sumr);
  } else {
    const double rl = st.curL[row];
    const double rem = fmax(0., st.remainL[row] - rl * s0);
    st.remainL[row] = rem;
    st.cost_row[row] = fma(rl, s1, st.cost_row[row]);
    if (lv + 1 < AM_LEVELS) {
      const double nl = rem / (1e-9 + s2);
      st.curL[row] = nl;
      ratioL[rec + n_own] = (float)nl;
    }
  }
}

// out[b] = the sum of rows[b, 0..len): thread t adds t, t+256, .. in float64, then a halving tree; rounded once.
__global__ __launch_bounds__(256) void am_reduce_kernel(const double* __restrict__ rows, int len, float* __restrict__ out) {
  __shared__ double sh[256];
  const double* r = rows + (size_t)blockIdx.x * len;
  double acc = 0.;
  for (int i = threadIdx.x; i < len; i += 256) acc += r[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = (float)sh[0];
}

// match(k,l) from the records, levels in the forward's order (j = 7 first)
__device__ __forceinline__ float plan_entry(float d2, const float* ro, const float* rq) {
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < AM_LEVELS - 1; ++i) m = fmaf(expf(am_level(i) * d2) * ro[i], rq[i], m);
  return fmaf(ro[AM_LEVELS - 1], rq[AM_LEVELS - 1], m);      // level 0: E = 1
}

// grad_own[p] = g[b] * sum_q match(p,q) * (own[p] - oth[q]) / max(|own[p] - oth[q]|, 1e-20): grad_xyz1 with (own, oth) = (xyz1, xyz2) and
// grad_xyz2 with the roles swapped (the sign comes with the swap).  rec_own [B,10,n_own], rec_oth [B,10,n_oth].
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void am_grad_kernel(const float* __restrict__ own, long own_stride, int n_own,
                                                             const float* __restrict__ oth, long oth_stride, int n_oth,
                                                             const float* __restrict__ rec_own, const float* __restrict__ rec_oth,
                                                             const float* __restrict__ gcost, float* __restrict__ grad) {
  constexpr int NT = 64 * WAVES, PART = AM_GTILE / WAVES;
  __shared__ __attribute__((aligned(16))) float tile[AM_GTILE][16];      // x, y, z, the ten records, 3 unused
  __shared__ double part[3][WAVES][AM_ROWS];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * AM_ROWS + lane;
  const bool valid = p < n_own;
  const float* o = own + (size_t)b * own_stride;
  const float* q = oth + (size_t)b * oth_stride;
  const float* rq = rec_oth + (size_t)b * AM_LEVELS * n_oth;
  float px = 0.f, py = 0.f, pz = 0.f, ro[AM_LEVELS];
#pragma unroll
  for (int i = 0; i < AM_LEVELS; ++i) ro[i] = valid ? rec_own[((size_t)b * AM_LEVELS + i) * n_own + p] : 0.f;
  if (valid) { px = o[(size_t)p * 3 + 0]; py = o[(size_t)p * 3 + 1]; pz = o[(size_t)p * 3 + 2]; }
  double gx[2] = {0., 0.}, gy[2] = {0., 0.}, gz[2] = {0., 0.};      // float64 sums: a row adds up to 2048 terms of either sign
  for (int t0 = 0; t0 < n_oth; t0 += AM_GTILE) {
    const int cnt = min(AM_GTILE, n_oth - t0);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * 13; e += NT) {      // e = field * cnt + point: the records' loads are contiguous
      const int f = e / cnt, i = e - f * cnt;
      const size_t g = (size_t)(t0 + i);
      tile[i][f] = f < 3 ? q[g * 3 + f] : rq[(size_t)(f - 3) * n_oth + g];
    }
    __syncthreads();
    const int lo = wave * PART, hi = min(cnt, lo + PART);
    for (int i = lo; i < hi; ++i) {
      const int u = (i - lo) & 1;
      const float4 c0 = *reinterpret_cast<const float4*>(&tile[i][0]);
      const float4 c1 = *reinterpret_cast<const float4*>(&tile[i][4]);
      const float4 c2 = *reinterpret_cast<const float4*>(&tile[i][8]);
      const float c3 = tile[i][12];
      const float r[AM_LEVELS] = {c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3};
      float dx, dy, dz;
      const float d2 = am_d2(px, py, pz, c0.x, c0.y, c0.z, dx, dy, dz);
      const double t = (double)(plan_entry(d2, ro, r) / fmaxf(sqrtf(d2), 1e-20f));
      gx[u] = fma(t, (double)dx, gx[u]); gy[u] = fma(t, (double)dy, gy[u]); gz[u] = fma(t, (double)dz, gz[u]);
    }
  }
  part[0][wave][lane] = gx[0] + gx[1]; part[1][wave][lane] = gy[0] + gy[1]; part[2][wave][lane] = gz[0] + gz[1];
  __syncthreads();
  if (wave != 0 || !valid) return;
  const double gc = (double)gcost[b];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double s = part[c][0][lane];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += part[c][w][lane];
    grad[((size_t)b * n_own + p) * 3 + c] = (float)(gc * s);
  }
}

// match[b,l,k] (tf_approxmatch's layout) from the records; one thread per entry, k fastest.
__global__ __launch_bounds__(256) void am_plan_kernel(const float* __restrict__ xyz1, long stride1, const float* __restrict__ xyz2, int n, int m,
                                                      const float* __restrict__ ratioL, const float* __restrict__ ratioR,
                                                      float* __restrict__ match) {
  const int k = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y, b = blockIdx.z;
  if (k >= n) return;
  const float* a = xyz1 + (size_t)b * stride1 + (size_t)k * 3;
  const float* c = xyz2 + ((size_t)b * m + l) * 3;
  float rl[AM_LEVELS], rr[AM_LEVELS];
#pragma unroll
  for (int i = 0; i < AM_LEVELS; ++i) {
    rl[i] = ratioL[((size_t)b * AM_LEVELS + i) * n + k];
    rr[i] = ratioR[((size_t)b * AM_LEVELS + i) * m + l];
  }
  float dx, dy, dz;
  const float d2 = am_d2(a[0], a[1], a[2], c[0], c[1], c[2], dx, dy, dz);
  match[((size_t)b * m + l) * n + k] = plan_entry(d2, rl, rr);
}

// dense match_cost: rowcost[b,l] = sum_k match[b,l,k] * |xyz1[k] - xyz2[l]|; thread t adds k = t, t+256, .. then a halving tree
__global__ __launch_bounds__(256) void am_dense_rows_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                            const float* __restrict__ match, int n, int m, double* __restrict__ rowcost) {
  __shared__ double sh[256];
  const int l = blockIdx.x, b = blockIdx.y;
  const float* c = xyz2 + ((size_t)b * m + l) * 3;
  const float cx = c[0], cy = c[1], cz = c[2];
  const float* mr = match + ((size_t)b * m + l) * n;
  double acc = 0.;
  for (int k = threadIdx.x; k < n; k += 256) {
    const float* a = xyz1 + ((size_t)b * n + k) * 3;
    float dx, dy, dz;
    acc = fma((double)mr[k], (double)sqrtf(am_d2(a[0], a[1], a[2], cx, cy, cz, dx, dy, dz)), acc);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) rowcost[(size_t)b * m + l] = sh[0];
}

// grad_xyz1[k] = g[b] * sum_l match[b,l,k] * (xyz1[k] - xyz2[l]) / max(d, 1e-20): one thread per k, l ascending (reads coalesced over k)
__global__ __launch_bounds__(256) void am_dense_grad1_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                             const float* __restrict__ match, int n, int m, const float* __restrict__ gcost,
                                                             float* __restrict__ grad1) {
  const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (k >= n) return;
  const float* a = xyz1 + ((size_t)b * n + k) * 3;
  const float ax = a[0], ay = a[1], az = a[2];
  double gx = 0., gy = 0., gz = 0.;
  for (int l = 0; l < m; ++l) {
    const float* c = xyz2 + ((size_t)b * m + l) * 3;
    float dx, dy, dz;
    const float d2 = am_d2(ax, ay, az, c[0], c[1], c[2], dx, dy, dz);
    const double t = (double)(match[((size_t)b * m + l) * n + k] / fmaxf(sqrtf(d2), 1e-20f));
    gx = fma(t, (double)dx, gx); gy = fma(t, (double)dy, gy); gz = fma(t, (double)dz, gz);
  }
  const double gc = (double)gcost[b];
  float* g = grad1 + ((size_t)b * n + k) * 3;
  g[0] = (float)(gc * gx); g[1] = (float)(gc * gy); g[2] = (float)(gc * gz);
}

// grad_xyz2[l] = -g[b] * sum_k match[b,l,k] * (xyz1[k] - xyz2[l]) / max(d, 1e-20): one wave per l, lane t adds k = t, t+64, .., then the
// wave's butterfly
__global__ __launch_bounds__(256) void am_dense_grad2_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                             const float* __restrict__ match, int n, int m, const float* __restrict__ gcost,
                                                             float* __restrict__ grad2) {
  const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (l >= m) return;                                       // whole waves leave: no barrier below
  const float* c = xyz2 + ((size_t)b * m + l) * 3;
  const float cx = c[0], cy = c[1], cz = c[2];
  const float* mr = match + ((size_t)b * m + l) * n;
  double gx = 0., gy = 0., gz = 0.;
  for (int k = lane; k < n; k += 64) {
    const float* a = xyz1 + ((size_t)b * n + k) * 3;
    float dx, dy, dz;
    const float d2 = am_d2(a[0], a[1], a[2], cx, cy, cz, dx, dy, dz);
    const double t = (double)(mr[k] / fmaxf(sqrtf(d2), 1e-20f));
    gx = fma(t, (double)dx, gx); gy = fma(t, (double)dy, gy); gz = fma(t, (double)dz, gz);
  }
  gx = wave_sum_d(gx); gy = wave_sum_d(gy); gz = wave_sum_d(gz);
  if (lane == 0) {
    const double gc = -(double)gcost[b];
    float* g = grad2 + ((size_t)b * m + l) * 3;
    g[0] = (float)(gc * gx); g[1] = (float)(gc * gy); g[2] = (float)(gc * gz);
  }
}

bool am_sizes_ok(int B, int n, int m) {
  if (B <= 0 || n <= 0 || m <= 0 || B > 65535 || n > (1 << 24) || m > (1 << 24)) return false;
  return n >= m ? n % m == 0 : m % n == 0;                 // the original's integer n/m must be the real ratio
}

template <int WAVES>
void am_forward(const float* xyz1, long stride1, const float* xyz2, int B, int n, int m, float* cost, float* ratioL, float* ratioR, double* ws,
                hipStream_t s) {
  const size_t bn = (size_t)B * n, bm = (size_t)B * m;
  const AmState st{ws, ws + bn, ws + 2 * bn, ws + 3 * bn, ws + 3 * bn + bm};
  const int big = n > m ? n : m;
  const size_t top = bn > bm ? bn : bm;
  hipLaunchKernelGGL(am_init_kernel, dim3(cdiv((long)top, 256)), dim3(256), 0, s, st, bn, bm, (double)big / n, (double)big / m);
  const dim3 rows(cdiv(n, AM_ROWS), B), cols(cdiv(m, AM_ROWS), B), blk(64 * WAVES);
  const long stride2 = (long)m * 3;
  hipLaunchKernelGGL((am_sweep_kernel<1, WAVES>), rows, blk, 0, s, xyz1, stride1, n, xyz2, stride2, m, 0, ratioL, ratioR, st);
  for (int lv = 0; lv < AM_LEVELS; ++lv) {
    hipLaunchKernelGGL((am_sweep_kernel<2, WAVES>), cols, blk, 0, s, xyz2, stride2, m, xyz1, stride1, n, lv, ratioL, ratioR, st);
    hipLaunchKernelGGL((am_sweep_kernel<3, WAVES>), rows, blk, 0, s, xyz1, stride1, n, xyz2, stride2, m, lv, ratioL, ratioR, st);
  }
  hipLaunchKernelGGL(am_reduce_kernel, dim3(B), dim3(256), 0, s, (const double*)st.cost_row, n, cost);
}

}  // namespace

extern "C" int spgan_approxmatch_levels(void) { return AM_LEVELS; }
extern "C" int spgan_approxmatch_tile(void) { return AM_TILE; }

extern "C" size_t spgan_approxmatch_ws_bytes(int B, int n, int m) {
  if (B <= 0 || n <= 0 || m <= 0) return 0;
  return ((size_t)B * n * 3 + (size_t)B * m * 2) * sizeof(double);      // remainL, cost_row, curL [B,n] | remainR, curR [B,m]
}

extern "C" int spgan_approxmatch_fwd(const float* xyz1, long stride1, const float* xyz2, int B, int n, int m, int waves, float* cost,
                                     float* ratioL, float* ratioR, void* ws, size_t ws_bytes, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz1 && xyz2 && cost && ratioL && ratioR && ws && am_sizes_ok(B, n, m));
  SPGAN_CHECK_ARG(stride1 == 0 || stride1 == (long)n * 3);
  SPGAN_CHECK_ARG(ws_bytes >= spgan_approxmatch_ws_bytes(B, n, m) && ((uintptr_t)ws & 7) == 0);
  hipStream_t s = (hipStream_t)s_;
  if (waves == 0 || waves == 4) am_forward<4>(xyz1, stride1, xyz2, B, n, m, cost, ratioL, ratioR, (double*)ws, s);
  else if (waves == 1) am_forward<1>(xyz1, stride1, xyz2, B, n, m, cost, ratioL, ratioR, (double*)ws, s);
  else return SPGAN_EINVAL;
  return spgan_launch_status();
}

extern "C" int spgan_approxmatch_bwd(const float* xyz1, long stride1, const float* xyz2, int B, int n, int m, const float* ratioL,
                                     const float* ratioR, const float* grad_cost, float* grad_xyz1, float* grad_xyz2, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz1 && xyz2 && ratioL && ratioR && grad_cost && (grad_xyz1 || grad_xyz2) && am_sizes_ok(B, n, m));
  SPGAN_CHECK_ARG(stride1 == 0 || stride1 == (long)n * 3);
  hipStream_t s = (hipStream_t)s_;
  const long stride2 = (long)m * 3;
  if (grad_xyz1)
    hipLaunchKernelGGL((am_grad_kernel<4>), dim3(cdiv(n, AM_ROWS), B), dim3(256), 0, s, xyz1, stride1, n, xyz2, stride2, m, ratioL, ratioR,
                       grad_cost, grad_xyz1);
  if (grad_xyz2)
    hipLaunchKernelGGL((am_grad_kernel<4>), dim3(cdiv(m, AM_ROWS), B), dim3(256), 0, s, xyz2, stride2, m, xyz1, stride1, n, ratioR, ratioL,
                       grad_cost, grad_xyz2);
  return spgan_launch_status();
}

extern "C" int spgan_approxmatch_plan(const float* xyz1, long stride1, const float* xyz2, int B, int n, int m, const float* ratioL,
                                      const float* ratioR, float* match, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz1 && xyz2 && ratioL && ratioR && match && am_sizes_ok(B, n, m) && m <= 65535);
  SPGAN_CHECK_ARG(stride1 == 0 || stride1 == (long)n * 3);
  hipLaunchKernelGGL(am_plan_kernel, dim3(cdiv(n, 256), m, B), dim3(256), 0, (hipStream_t)s_, xyz1, stride1, xyz2, n, m, ratioL, ratioR, match);
  return spgan_launch_status();
}

extern "C" int spgan_match_cost_dense_fwd(const float* xyz1, const float* xyz2, const float* match, int B, int n, int m, float* cost, void* ws,
                                          size_t ws_bytes, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz1 && xyz2 && match && cost && ws && am_sizes_ok(B, n, m));
  SPGAN_CHECK_ARG(ws_bytes >= (size_t)B * m * sizeof(double) && ((uintptr_t)ws & 7) == 0);
  hipStream_t s = (hipStream_t)s_;
  hipLaunchKernelGGL(am_dense_rows_kernel, dim3(m, B), dim3(256), 0, s, xyz1, xyz2, match, n, m, (double*)ws);
  hipLaunchKernelGGL(am_reduce_kernel, dim3(B), dim3(256), 0, s, (const double*)ws, m, cost);
  return spgan_launch_status();
}

extern "C" int spgan_match_cost_dense_bwd(const float* xyz1, const float* xyz2, const float* match, int B, int n, int m, const float* grad_cost,
                                          float* grad_xyz1, float* grad_xyz2, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(xyz1 && xyz2 && match && grad_cost && (grad_xyz1 || grad_xyz2) && am_sizes_ok(B, n, m));
  hipStream_t s = (hipStream_t)s_;
  if (grad_xyz1) hipLaunchKernelGGL(am_dense_grad1_kernel, dim3(cdiv(n, 256), B), dim3(256), 0, s, xyz1, xyz2, match, n, m, grad_cost, grad_xyz1);
  if (grad_xyz2) hipLaunchKernelGGL(am_dense_grad2_kernel, dim3(cdiv(m, 4), B), dim3(256), 0, s, xyz1, xyz2, match, n, m, grad_cost, grad_xyz2);
  return spgan_launch_status();
}
