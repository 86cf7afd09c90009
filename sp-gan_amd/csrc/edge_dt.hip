// EdgeConv2's attention backward with dT = dout . WoT formed in the launch's MFMA accumulators (k = 10, F = 128, fp32).
//
// The chain  dT = gemm_nt(dout, WoT)  ->  edge_attend_bwd(dT, ...)  writes the [M, k*F] tensor dT (336 MB in the train step) and reads it
// back once; nothing else reads it.  Here a workgroup of four waves takes 32 points as the rows of 32 x 32 MFMA tiles; wave w owns the
// channels f in [32w, 32w + 32) for all ten neighbours r: ten accumulator tiles (tile r = columns r*F + 32w .. of dT), 160 registers per
// lane.  In the v_mfma_f32_32x32x2_f32 output layout a lane then holds, for ONE channel, sixteen points x all ten r: the softmax's max,
// its denominator and the `dot` of its backward are in-lane reductions over the ten tiles at one register index -- no LDS exchange, no
// second pass over dT.
//
// Bits.  Every result equals the chain's (tests/test_edge_dt_gpu.py compares with torch.equal):
//   * dT: one accumulator per output tile, from zero, over K = 128 in the order of gemm_nt_wide_kernel's compute() (gemm_wide.hip): k-tiles
//     of 32 ascending; inside a tile, for kk = 0..7, the MFMA on the pair {4kk, 4kk+2} (lane half lh supplies 4kk + 2 lh), then the one on
//     {4kk+1, 4kk+3}.  The route is taken only where the chain's product would run that kernel (spgan_edge_attend_bwd_dt_selected).
//   * g2, gy: the expressions of edge_attend_bwd_k_kernel, shared through edge_attend.hpp.
//   * statistics records [tiles][2F][2], 32 points each: the chain's wave c sums the points 4 pp + c, pp = 0..7, each over r = 0..9, and
//     the record is (c0 + c1) + (c2 + c3).  Which point an MFMA row holds is free -- it is only the order in which dout's rows are put
//     into LDS: accumulator register v of lane half lh holds point 4 (v/2) + 2 lh + (v%2).  A lane then owns the two complete classes
//     c = 2 lh and 2 lh + 1 with pp ascending: four running sums per class as in-lane chains in the chain's order, (c0 + c1) in lane half
//     0, (c2 + c3) in half 1, one cross-half add.
//
// Staging.  The workgroup's 32 x 128 block of dout stays in LDS (row pitch 130 words == 2 mod 64: conflict-free 8-byte fragment reads).  WoT
// [1280,128] (640 KB, L2-resident) goes through LDS in 40 double-buffered stages of 128 rows x 32 k (one r, one k-tile; row pitch 34 as
// gemm_wide.hip), coalesced 16-byte loads issued one stage ahead.  256 threads, 32 points, 52 KB of LDS, two workgroups per CU (254
// registers per lane): one's MFMA phase runs beside the other's memory phase.  No atomics, nothing shared between workgroups.
// A 512-thread form (two groups of 32 points sharing each staged WoT tile: half the L2 -> LDS traffic, one workgroup per CU) measured
// 361 us against this form's 356 us in the train step on one machine and was not kept.
#include <stdlib.h>
#include "edge_attend.hpp"
#include "gemm_nt_plan.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int DK = 10, DF = 128;           // neighbours per point, channels
constexpr int DP = 32;                     // points per workgroup = one statistics record (EB_PT of edge.hip)
constexpr int DKT = 32, DLW = DKT + 2;     // k-tile and row pitch of a staged WoT tile
constexpr int DLA = DF + 2;                // row pitch of the dout block
constexpr int DNKT = DF / DKT;             // k-tiles
constexpr size_t DT_LDS = ((size_t)DP * DLA + 2 * DF * DLW + DP * DK) * sizeof(float);   // 52,736 bytes

// the point (of the workgroup's 32) whose dout row is MFMA row i: row i = 8 (v/4) + 4 lh + v%4 is register v of lane half lh
__device__ __forceinline__ int row_point(int i) {
  const int lh = (i >> 2) & 1, v = (i & 3) + 4 * (i >> 3);
  return 4 * (v >> 1) + 2 * lh + (v & 1);
}

__global__ __launch_bounds__(256, 2) void edge_attend_bwd_dt_kernel(
    const float* __restrict__ dout, int ldo, const float* __restrict__ WoT, int ldw, const float* __restrict__ h2,
    const float* __restrict__ sc2, const float* __restrict__ sh2, const float* __restrict__ mean2, const float* __restrict__ inv2,
    const float* __restrict__ PQR, int ld, int H, const int32_t* __restrict__ idx, int M, const float* __restrict__ bx,
    const float* __restrict__ scx, const float* __restrict__ shx, const float* __restrict__ meanx, const float* __restrict__ invx, float slope,
    float* __restrict__ g2, float* __restrict__ gy, float* __restrict__ part) {
  constexpr int THREADS = 256, SLOTS = 4, RPP = 32;   // WoT stage: 128 rows x 8 float4 over the workgroup
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                                  // [32][DLA]     dout rows in MFMA row order
  float* Bs = smem + DP * DLA;                       // [2][128*DLW]  WoT rows r*F .. r*F+127, one k-tile
  int* sidx = reinterpret_cast<int*>(Bs + 2 * DF * DLW);   // [32][10]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int bxid = xcd_block();
  const int i0 = bxid * DP;                          // the workgroup's first point (host: M % 32 == 0)
  if (i0 >= M) return;

#pragma unroll
  for (int s = 0; s < 4; ++s) {                      // dout block: 32 rows x 32 float4
    const int q = tid + s * THREADS, row = q >> 5, c4 = (q & 31) * 4;
    const int i = i0 + row_point(row);
    const float4 v = *reinterpret_cast<const float4*>(dout + (size_t)i * ldo + c4);
    float* a = As + row * DLA + c4;
    *reinterpret_cast<float2*>(a) = make_float2(v.x, v.y);
    *reinterpret_cast<float2*>(a + 2) = make_float2(v.z, v.w);
  }
  for (int t = tid; t < DP * DK; t += THREADS) sidx[t] = idx[(size_t)i0 * DK + t];

  f32x16 acc[DK];
#pragma unroll
  for (int r = 0; r < DK; ++r)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[r][v] = 0.f;

  float4 rb[SLOTS];
  const int lrow = tid >> 3, lc4 = (tid & 7) * 4;
  auto gload = [&](int r, int kt) {
#pragma unroll
    for (int i = 0; i < SLOTS; ++i)
      rb[i] = *reinterpret_cast<const float4*>(WoT + (size_t)(r * DF + lrow + RPP * i) * ldw + kt * DKT + lc4);
  };
  auto sstore = [&](int buf) {
    float* b = Bs + buf * DF * DLW + lrow * DLW + lc4;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      *reinterpret_cast<float2*>(b + i * RPP * DLW) = make_float2(rb[i].x, rb[i].y);
      *reinterpret_cast<float2*>(b + i * RPP * DLW + 2) = make_float2(rb[i].z, rb[i].w);
    }
  };
  const float* afrag = As + l31 * DLA + 2 * lh;
  const float* bfrag = Bs + (w * 32 + l31) * DLW + 2 * lh;

  // the lane's channel; sixteen points (register v), all ten r in acc[0..9][v]
  const int f = w * 32 + l31;
  // A point row's ten h2pre loads, ten Q_j gathers and R_i are issued together, one row AHEAD of the arithmetic (two register sets): the
  // phase is bound by how many bytes a wave keeps in flight, not by its instruction count.  Row 0 is fetched under the last MFMA stages.
  float hp[2][DK][1], yp[2][DK][1], Ri[2][1];
  auto fetch = [&](int v) {
    const int p = 4 * (v >> 1) + 2 * lh + (v & 1);
    const size_t i = (size_t)(i0 + p);
    Ri[v & 1][0] = PQR[i * ld + H + DF + f];
#pragma unroll
    for (int r = 0; r < DK; ++r) {
      const int j = sidx[p * DK + r];
      hp[v & 1][r][0] = h2[(i * DK + r) * DF + f];
      yp[v & 1][r][0] = PQR[(size_t)j * ld + H + f];
    }
  };

  gload(0, 0);
  sstore(0);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < DK; ++r) {
#pragma unroll
    for (int kt = 0; kt < DNKT; ++kt) {
      const int s = r * DNKT + kt, buf = s & 1;
      if (s + 1 < DK * DNKT) gload((s + 1) / DNKT, (s + 1) % DNKT);   // next stage's loads fly under this stage's MFMAs
      if (s == DK * DNKT - 2) fetch(0);
      float2 af[DKT / 4], bf[DKT / 4];
#pragma unroll
      for (int kk = 0; kk < DKT / 4; ++kk) {
        af[kk] = *reinterpret_cast<const float2*>(afrag + kt * DKT + kk * 4);
        bf[kk] = *reinterpret_cast<const float2*>(bfrag + buf * DF * DLW + kk * 4);
      }
#pragma unroll
      for (int kk = 0; kk < DKT / 4; ++kk) {
        acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk].x, bf[kk].x, acc[r], 0, 0, 0);
        acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk].y, bf[kk].y, acc[r], 0, 0, 0);
      }
      // issue order of the stage: global loads, fragment reads, MFMAs (the scheduler otherwise sinks the loads behind the MFMAs to shorten
      // live ranges and the stage waits a whole L2 round trip at its end)
      __builtin_amdgcn_sched_group_barrier(0x020, 32, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (s + 1 < DK * DNKT) sstore(buf ^ 1);   // the other buffer: its last readers passed the previous barrier
      __syncthreads();
    }
  }

  const float a2[1] = {sc2[f]}, c2[1] = {sh2[f]}, ax[1] = {scx[f]}, cx[1] = {shx[f]}, bb[1] = {bx[f]}, m2[1] = {mean2[f]}, i2[1] = {inv2[f]},
              mxm[1] = {meanx[f]}, ixv[1] = {invx[f]};
  float sums[2][4][1] = {};   // the lane's two classes c = 2 lh + (v & 1): (g2, g2*xhat2, gy, gy*xhaty)
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    if (v + 1 < 16) fetch(v + 1);
    __builtin_amdgcn_sched_barrier(0);
    const int p = 4 * (v >> 1) + 2 * lh + (v & 1);
    const size_t e0 = ((size_t)(i0 + p) * DK) * DF + f;
    float d[DK][1], o2[DK][1], oy[DK][1];
#pragma unroll
    for (int r = 0; r < DK; ++r) d[r][0] = acc[r][v];
    auto& s = sums[v & 1];
    edge_attend_bwd_elem<DK, 1, false>(0, hp[v & 1], d, yp[v & 1], Ri[v & 1], a2, c2, ax, cx, bb, m2, i2, mxm, ixv, slope, o2, oy, s[0], s[1], s[2],
                                       s[3]);
#pragma unroll
    for (int r = 0; r < DK; ++r) {
      g2[e0 + (size_t)r * DF] = o2[r][0];
      gy[e0 + (size_t)r * DF] = oy[r][0];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  float tot[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const float t = sums[0][n][0] + sums[1][n][0];   // (c0 + c1) in lane half 0, (c2 + c3) in half 1
    tot[n] = t + __shfl_xor(t, 32);
  }
  if (lh == 0) {
    float* o = part + (size_t)bxid * (2 * DF) * 2;
    o[(size_t)f * 2 + 0] = tot[0];
    o[(size_t)f * 2 + 1] = tot[2];
    o[(size_t)(DF + f) * 2 + 0] = tot[1];
    o[(size_t)(DF + f) * 2 + 1] = tot[3];
  }
}

inline bool al(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

}  // namespace

extern "C" int spgan_edge_attend_bwd_dt_selected(const float* dout, int ldo, const float* WoT, int ldw, int M, int k, int F, int tile_hint) {
  if (!dout || !WoT || k != DK || F != DF || M <= 0 || M % DP) return 0;
  spgan_gemm_nt_args a = {};   // the chain's product dT = gemm_nt(dout, WoT) as spgan_gemm_nt would see it
  a.A = dout; a.lda = ldo; a.W = WoT; a.ldw = ldw;
  a.Y = const_cast<float*>(dout); a.ldy = k * F;   // any non-null address: the selection never reads through it
  a.M = M; a.N = k * F; a.K = F;
  a.a_mode = SPGAN_A_PLAIN; a.epi_mode = SPGAN_EPI_LINEAR; a.mfma_f16 = 0; a.tile_hint = tile_hint;
  return nt_plan(a).kernel == NT_WIDE ? 1 : 0;
}

extern "C" int spgan_edge_attend_bwd_dt(const float* dout, int ldo, const float* WoT, int ldw, const float* h2pre, const float* sc2,
                                        const float* sh2, const float* mean2, const float* inv2, const float* PQR, int ld, int H, int F,
                                        const int32_t* idx, int M, int k, const float* bx, const float* scx, const float* shx, const float* meanx,
                                        const float* invx, float slope, float* g2, float* gy, float* partials, spgan_stream_t s_) {
  SPGAN_CHECK_ARG(dout && WoT && h2pre && sc2 && sh2 && mean2 && inv2 && PQR && idx && bx && scx && shx && meanx && invx && g2 && gy && partials);
  SPGAN_CHECK_ARG(k == DK && F == DF && M > 0 && M % DP == 0 && H >= 0 && ld >= H + 2 * F);
  SPGAN_CHECK_ARG(ldo >= F && ldo % 4 == 0 && ldw >= F && ldw % 4 == 0 && al(dout, 16) && al(WoT, 16));
  SPGAN_CHECK_ARG(al(h2pre, 4) && al(sc2, 4) && al(sh2, 4) && al(mean2, 4) && al(inv2, 4) && al(PQR, 4) && al(idx, 4) && al(bx, 4) && al(scx, 4) &&
                  al(shx, 4) && al(meanx, 4) && al(invx, 4) && al(g2, 4) && al(gy, 4) && al(partials, 4));
  hipLaunchKernelGGL(edge_attend_bwd_dt_kernel, dim3(grid8(M / DP)), dim3(256), DT_LDS, (hipStream_t)s_, dout, ldo, WoT, ldw, h2pre, sc2, sh2, mean2,
                     inv2, PQR, ld, H, idx, M, bx, scx, shx, meanx, invx, slope, g2, gy, partials);
  return spgan_launch_status();
}
