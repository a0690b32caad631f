// Fused MLP step (mlp_step.hip): the factor engines (sufficient-factor exchange) --
// mlp_fwdapply_factor_kernel and mlp_wgrad_factor_kernel.
#pragma once
#include "mlp_step_3launch.h"

namespace dtfx {
namespace mlp {

// ---------------------------------------------------------------------------
// Pipelined FACTOR engine (world XW, 2 launches per data-parallel step): the
// mlp_fwdapply_kernel structure with the W1 update formed from EVERY rank's factors:
//   g = sum_q dz1A[q][jt]^T . x_q(t-1)   (K = XW * BP, the all-gathered factors of step
//   t-1 and every rank's resident batch), W1new = W1old - lr * g,
// then step t's forward on W1new.  The single-GPU step's 28-feature K slices (196 W1
// blocks): 1024-thread blocks, wave (c, s) owns column group c (16 + 12 live features) and
// K split s of fx_kspl = 8 (generic batches: 512 threads, 4 splits); the partial slices are
// added in split order through LDS
// (identical order on every rank: bit-identical replicas).  At 8 ranks the global W1 gradient
// is 8 x the 1-GPU step's MFMA work (K = 800), so it must be spread over the chip and issue
// all of its loads in ONE round trip: a wave's K share (XW * 7 / 8 batch groups of 16 rows, 7
// at 8 ranks) is requested at once (CH groups per round), and the seven hidden tiles of a K slice
// -- which read the same x columns of every rank's batch, the one large fresh read -- run on
// one XCD (block b on XCD b % 8; speed only), so each XCD's L2 fetches its slices' x once.
// The first version (14 slices, 98 blocks, 4 load rounds, slices scattered over the XCDs)
// cost 21.2 us per step at 8 ranks against 7.3 for the 1-GPU step (round-4 local cost).
// Measured and not kept (round 5): the block's x slab of all ranks staged in LDS with 16-byte
// loads instead of per-lane 4-byte gathers (first launch + plain head 10.9-11.1 -> 11.8-12.1
// us at 8 ranks: the staging round trip then sits in front of every MFMA).
// Small-parameter blocks exchange dW2/db1/db2 partials of step t-1 as in the 3-launch factor
// engine (waves 0..3 of the block).  The head of step t all-gathers dz1 into dz1A
// (mlp_head_kernel<.., XW, KS3>).
constexpr int FX_SLOTS = (KS3 + 7) / 8 * HT;  // block slots per XCD (4 slice rows x 7 tiles)
// phase-A K splits: 8 (1024-thread blocks, 16 waves, 4 per SIMD) for the batch <= 112
// instantiations; the generic ones keep 4 (512 threads: their small-parameter waves hold
// 16 batch groups of operands, which 4 waves per SIMD would spill)
template <int NGT> constexpr int fx_kspl() { return NGT > 0 ? 8 : 4; }
// Phase A of mlp_fwdapply_factor_kernel in row-quad form (DTFX_XG_SPLIT bit 5, round 6): each
// of the block's 16 waves covers ALL 28 features of the slice for its 1/16 of the K = XW x BP
// rows.  Per quad of 4 rows a lane loads ONE float2 of x (features 2r, 2r + 1 of row base + q;
// lanes r >= 14 are dead) and ONE dz1A value (hidden r of row base + q), and feeds two
// 16x16x4 MFMAs (accumulator e: features 2r + e).  The column-group form loads four scalar x
// and four dz1A values per 16 rows and column group -- twice the load instructions per
// element, the one cost that grows with K = XW x BP (the global W1 gradient is 8x the 1-GPU
// step's MFMA work at 8 ranks).  The 16 partials are added in split order (the same bits on
// every rank); wave e in {0, 1} applies accumulator e.
template <int XW, int NGT>
__device__ __forceinline__ void fx_phase_a_quads(
    const float* __restrict__ p_old, float* __restrict__ p_new, float lr,
    const float* __restrict__ x_prev, long long xstride, const float* __restrict__ dz1A, int B,
    int BP, int jt, int f0, int me, int wave, int lane, float (&Wt)[16][D / KS3 + 4],
    f32x4* red) {
  constexpr int KWX = D / KS3;         // 28 features
  constexpr int NQ = NGT * 4;          // row quads per rank
  constexpr int GQ = XW * NQ;          // row quads in all
  constexpr int QPW = (GQ + 15) / 16;  // per wave (14 at 8 ranks x 112 rows)
  const int r = lane & 15, q = lane >> 4;
  const bool lv = r < KWX / 2;
  const int fo = 2 * (lv ? r : KWX / 2 - 1);
  float pw[4];
  if (wave < 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = jt * 16 + q * 4 + i;
      pw[i] = p_old[OFF_W1 + (size_t)(j < H ? j : H - 1) * D + f0 + fo + wave];
    }
  }
  float av[QPW];
  float2 xv[QPW];
  const int u0 = wave * QPW;
#pragma unroll
  for (int u = 0; u < QPW; ++u) {
    const int g = u0 + u;
    if (g < GQ) {  // wave-uniform
      const int qq = g / NQ, row = (g - qq * NQ) * 4 + q;
      av[u] = dz1A[((size_t)qq * BP + row) * HP + jt * 16 + r];  // rows >= B: zero
      xv[u] = *reinterpret_cast<const float2*>(
          x_prev + (long long)(qq - me) * xstride + (size_t)(row < B ? row : B - 1) * D + f0 + fo);
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // the wave's loads in flight together
  f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < QPW; ++u) {
    if (u0 + u < GQ) {
      a0 = mfma16x16x4(av[u], xv[u].x, a0);
      a1 = mfma16x16x4(av[u], xv[u].y, a1);
    }
  }
  red[(wave * 2 + 0) * 64 + lane] = a0;
  red[(wave * 2 + 1) * 64 + lane] = a1;
  __syncthreads();
  if (wave < 2) {
    f32x4 part = red[wave * 64 + lane];
#pragma unroll
    for (int k = 1; k < 16; ++k) {  // split order: the same bits on every rank
      const f32x4 o = red[(k * 2 + wave) * 64 + lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) part[i] += o[i];
    }
    const int fl = fo + wave;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int hl = q * 4 + i, j = jt * 16 + hl;
      const float v = pw[i] - lr * part[i];
      if (lv) {
        Wt[hl][fl] = j < H ? v : 0.f;
        if (j < H) p_new[OFF_W1 + (size_t)j * D + f0 + fl] = v;
      }
    }
  }
}

template <int XW, int NGT>
__global__ __launch_bounds__(128 * fx_kspl<NGT>()) void mlp_fwdapply_factor_kernel(
    const float* __restrict__ p_old, float* __restrict__ p_new, float lr,
    const float* __restrict__ x_prev, const float* __restrict__ x, long long xstride,
    const float* __restrict__ dz1A, Bufs w, int* __restrict__ ctr, float* __restrict__ stats,
    int stats_ring, int B, int stats_on, MlpXg xg) {
  constexpr int FX_KSPL = fx_kspl<NGT>();
  const int BP = NGT > 0 ? NGT * 16 : ((B + 15) >> 4) * 16;
  const int NG = NGT > 0 ? NGT : BP / 16;
  const int RT = (B + 15) >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int bid = blockIdx.x;
  if (bid >= 8 * FX_SLOTS) {
    const int jt = bid - 8 * FX_SLOTS;
    if (wave < 4)
      wgrad_small<true, NGT, XW>(jt, wave, lane, MLP_XG_SMALL_EPOCH + jt * 4 + wave, p_new, lr,
                                 nullptr, w, ctr, stats, stats_ring, B, xg, p_old, stats_on);
    return;
  }
  // block -> (hidden tile jt, K slice ks) with ks % 8 == the block's XCD
  const int xcd = bid & 7, s8 = bid >> 3;
  const int jt = s8 % HT, ks = (s8 / HT) * 8 + xcd;
  if (ks >= KS3) return;  // (whole block: the slots past the 28 slices)
  constexpr int KWX = D / KS3;  // 28 features
  constexpr int LW = KWX + 4;
  __shared__ float Wt[16][LW];
  // K-split partials: [c][k][lane] (column-group form) or [s][e][lane] (row-quad form)
  __shared__ f32x4 red[32 * 64];
  const int f0 = ks * KWX;
  const int me = xgll::uniform(xg.rank);
  // phase B's x rows (wave w < RT owns row tile w; B <= 128): requested first
  float4 xa[2];
  const int rowB = wave * 16 + r;
  const float rmB = rowB < B ? 1.f : 0.f;
  if (wave < RT) {
    const float* xr = x + (size_t)(rowB < B ? rowB : B - 1) * D + f0;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int k = 16 * g + 4 * q;
      xa[g] = f4(xr + (k < KWX ? k : 0));
    }
  }
  if (NGT > 0 && (xg.split & 32)) {
    if constexpr (NGT > 0)
      fx_phase_a_quads<XW, NGT>(p_old, p_new, lr, x_prev, xstride, dz1A, B, BP, jt, f0, me,
                                wave, lane, Wt, red);
  } else {
  // ---- phase A: column group c, K split sp (FX_KSPL splits) ------------------------------
  const int c = wave & 1, sp = wave >> 1;
  const int fl = c * 16 + r;
  const bool cv = fl < KWX;
  const int fc = f0 + (cv ? fl : KWX - 1);
  const int G = XW * NG, per = (G + FX_KSPL - 1) / FX_KSPL;
  const int g0 = sp * per, g1 = min(G, g0 + per);
  float pw[4];
  if (sp == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = jt * 16 + q * 4 + i;
      pw[i] = p_old[OFF_W1 + (size_t)(j < H ? j : H - 1) * D + fc];
    }
  }
  f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  // one round at 8 ranks x 7 groups (7 per split); more only for batches > 112 rows
  constexpr int CH = (XW * (NGT > 0 ? NGT : 7) + FX_KSPL - 1) / FX_KSPL;
  for (int c0 = g0; c0 < g1; c0 += CH) {
    float4 av[CH];
    float xv[CH][4];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int g = c0 + i;
      if (g < g1) {  // wave-uniform
        const int qq = g / NG, gg = g - qq * NG;
        const float* a = dz1A + ((size_t)qq * BP + gg * 16 + q * 4) * HP + jt * 16 + r;
        av[i] = make_float4(a[0], a[HP], a[2 * HP], a[3 * HP]);
        const float* xq = x_prev + (long long)(qq - me) * xstride + fc;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int b = gg * 16 + q * 4 + e;  // rows >= B: dz1A is zero there
          xv[i][e] = xq[(size_t)(b < B ? b : B - 1) * D];
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // the round's loads in flight together
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      if (c0 + i < g1) {
        acc0 = mfma16x16x4(av[i].x, xv[i][0], acc0);
        acc1 = mfma16x16x4(av[i].y, xv[i][1], acc1);
        acc0 = mfma16x16x4(av[i].z, xv[i][2], acc0);
        acc1 = mfma16x16x4(av[i].w, xv[i][3], acc1);
      }
    }
  }
  f32x4 part;
#pragma unroll
  for (int i = 0; i < 4; ++i) part[i] = acc0[i] + acc1[i];
  if (sp > 0) red[(c * (FX_KSPL - 1) + sp - 1) * 64 + lane] = part;
  __syncthreads();
  if (sp == 0) {
#pragma unroll
    for (int k = 0; k < FX_KSPL - 1; ++k) {  // split order: the same bits on every rank
      const f32x4 o = red[(c * (FX_KSPL - 1) + k) * 64 + lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) part[i] += o[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int hl = q * 4 + i, j = jt * 16 + hl;
      const float v = pw[i] - lr * part[i];
      if (cv) {
        Wt[hl][fl] = j < H ? v : 0.f;
        if (j < H) p_new[OFF_W1 + (size_t)j * D + f0 + fl] = v;
      }
    }
  }
  }
  __syncthreads();
  // ---- phase B: z1 partial of row tile `wave` over the block's 28 features -------------
  if (wave >= RT) return;
  float4 wb[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int k = 16 * g + 4 * q;
    wb[g] = k < KWX ? *reinterpret_cast<const float4*>(&Wt[r][k]) : float4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 o0 = {0, 0, 0, 0}, o1 = {0, 0, 0, 0};
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    // (wb is zero for the dead part of the last group, so no mask is needed on xa there)
    o0 = mfma16x16x4(xa[g].x * rmB, wb[g].x, o0);
    o1 = mfma16x16x4(xa[g].y * rmB, wb[g].y, o1);
    o0 = mfma16x16x4(xa[g].z * rmB, wb[g].z, o0);
    o1 = mfma16x16x4(xa[g].w * rmB, wb[g].w, o1);
  }
  float* out = w.slab + ((size_t)ks * BP + wave * 16 + q * 4) * HP + jt * 16 + r;
#pragma unroll
  for (int i = 0; i < 4; ++i) out[(size_t)i * HP] = o0[i] + o1[i];
}

// ---------------------------------------------------------------------------
// K3, factor engine (sufficient-factor exchange, world XW): the backprop factors dz1 of
// every rank were all-gathered by mlp_head_kernel<.., XW> into dz1A [XW][BP][HP], and every
// rank holds every rank's (deterministic, device-resident) batch, so each rank computes the
// GLOBAL dW1^T = sum_q dz1_q^T . x_q itself (K = XW * BP) and applies it -- the 313 KB W1
// gradient never crosses xGMI; only the 1,110 small-parameter gradients are exchanged
// (wgrad_small, LL push).  Identical inputs + a fixed summation order keep the replicas
// bit-identical.
//   blocks [0, 8 * FT): one 16x16 dW1^T tile per block, the K range split over 4 waves and
//     the 4 partial tiles added in wave order through LDS.  Block b runs on XCD b % 8
//     (round-robin dispatch; speed only): feature tile kt = 8 * s + b % 8 keeps each
//     XCD's x columns to ~1/8 of every rank's batch (x is the one large fresh read).
//   blocks [8 * FT, 8 * FT + HT): wgrad_small (dW2 / db1 / db2 partials exchanged).
// xstride: elements between consecutive ranks' datasets (x of rank q = x + (q - me) * xstride).
template <int XW, int NGT>
__global__ __launch_bounds__(256) void mlp_wgrad_factor_kernel(
    float* __restrict__ p, float lr, const float* __restrict__ x, long long xstride,
    const float* __restrict__ dz1A, Bufs w, int* __restrict__ ctr, float* __restrict__ stats,
    int stats_ring, int B, MlpXg xg) {
  const int BP = NGT > 0 ? NGT * 16 : ((B + 15) >> 4) * 16;
  const int NG = NGT > 0 ? NGT : BP / 16;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, r = lane & 15, q4 = lane >> 4;
  const int bid = blockIdx.x;
  constexpr int NSLOT = (FT + 7) / 8;  // 7 feature-tile slots per XCD
  if (bid >= 8 * HT * NSLOT) {
    const int jt = bid - 8 * HT * NSLOT;
    wgrad_small<true, NGT, XW>(jt, wave, lane, MLP_XG_SMALL_EPOCH + jt * 4 + wave, p, lr,
                               nullptr, w, ctr, stats, stats_ring, B, xg);
    return;
  }
  const int xcd = bid & 7, s = bid >> 3;
  const int jt = s / NSLOT, kt = (s % NSLOT) * 8 + xcd;
  if (kt >= FT) return;  // whole block: uniform
  __shared__ f32x4 red[3][64];
  const int G = XW * NG, per = (G + 3) / 4;
  const int g0 = wave * per, g1 = min(G, g0 + per);
  const int me = xgll::uniform(xg.rank);
  float pw[4];
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = jt * 16 + q4 * 4 + i;
      pw[i] = p[OFF_W1 + (size_t)(j < H ? j : H - 1) * D + kt * 16 + r];
    }
  }
  f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  constexpr int CH = 7;  // groups of 16 batch rows per load round (all in flight together)
  for (int c0 = g0; c0 < g1; c0 += CH) {
    float4 av[CH];
    float xv[CH][4];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int g = c0 + i;
      if (g < g1) {  // wave-uniform
        const int qq = g / NG, gg = g - qq * NG;
        const float* a = dz1A + ((size_t)qq * BP + gg * 16 + q4 * 4) * HP + jt * 16 + r;
        av[i] = make_float4(a[0], a[HP], a[2 * HP], a[3 * HP]);
        const float* xq = x + (long long)(qq - me) * xstride + kt * 16 + r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int b = gg * 16 + q4 * 4 + e;  // rows >= B: dz1A is zero there
          xv[i][e] = xq[(size_t)(b < B ? b : B - 1) * D];
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // the round's loads in flight together
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      if (c0 + i < g1) {
        acc0 = mfma16x16x4(av[i].x, xv[i][0], acc0);
        acc1 = mfma16x16x4(av[i].y, xv[i][1], acc1);
        acc0 = mfma16x16x4(av[i].z, xv[i][2], acc0);
        acc1 = mfma16x16x4(av[i].w, xv[i][3], acc1);
      }
    }
  }
  f32x4 part;
#pragma unroll
  for (int i = 0; i < 4; ++i) part[i] = acc0[i] + acc1[i];
  if (wave > 0) red[wave - 1][lane] = part;
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const f32x4 o = red[k][lane];
#pragma unroll
    for (int i = 0; i < 4; ++i) part[i] += o[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = jt * 16 + q4 * 4 + i;
    if (j < H) p[OFF_W1 + (size_t)j * D + kt * 16 + r] = pw[i] - lr * part[i];
  }
}

}  // namespace mlp
}  // namespace dtfx
