// Fused MLP step (mlp_step.hip): the two-launch step -- fwdapply_block / mlp_fwdapply_kernel,
// the lean single-GPU entry points with their optimizer, schedule and trace forms, and the
// fused flush (mlp_head_flush_kernel).
//
// The single-GPU two-launch step (bench.py's default workload) runs through LEAN entry points,
// mlp_lean_fwdapply_kernel / mlp_lean_head_kernel: the fwdapply_block<.., 0, .., KS3> /
// head_row<.., RM> bodies behind kernel arguments of scalars and pointers only (at most 16
// dwords; the workspace regions derived from one base pointer through ws_layout), preloaded
// into user SGPRs at wave launch, and with phase A's own operands (dz1R / x_prev, then W1)
// requested before phase B's cold x rows, so the first MFMA does not wait for those
// (profiles/lean_step/: -0.56 us per step, bit-identical results).  mlp_fwdapply_launch /
// mlp_head2_launch, the data-parallel engines and the opt-in fused flush keep
// mlp_fwdapply_kernel / mlp_head_kernel.  Measured and not kept there: tile-major z1 slabs.
// The lean first launch also applies W1 in 16-byte accesses (fwdapply_block<.., A16>,
// profiles/wide_wt_stores/: -0.21 us per step, bit-identical results): one float4 of p_old,
// p_new and Wt per live lane on all four waves, the p_old load issued by every lane without a
// branch, so phase A's vmcnt waits are the exact ones.  Measured and not kept there:
//   phase B with swapped MFMA operands and one float4 slab store per lane: within the noise;
//   those slab stores written through (sc1): the boundary to the head shrinks by what the
//     stores' own drain adds to the launch's tail, no gain per step;
//   p_new written through as well: slower in the driver-sized run.
// The lean head reads its 28 slab planes through ONE buffer descriptor (head_row<.., SB>,
// profiles/lean_prologue/: -0.24 us per step, bit-identical results): lane offset in the vector
// offset, plane and row in the scalar one, so the one in-order wave issues 28 loads with a scalar
// add each where the pointer form rebuilt a 64-bit per-lane address for every plane (48 VALU
// adds and 24 s_nop between the first and the last slab load).  Measured and not kept there:
//   b1 / W2 / b2 through a descriptor as well (no VALU ahead of the last operand load at all)
//     and 1 / B computed behind the head's operand loads instead of ahead of them: within the
//     noise;
//   the first launch's dz1R / x_prev loads through descriptors with 32-bit offsets (no 64-bit
//     multiply-add ahead of the last phase-A operand): within the noise.
#pragma once
#include "mlp_step_3launch.h"

namespace dtfx {
namespace mlp {

// ---------------------------------------------------------------------------
// Pipelined single-GPU step (2 launches): K1' applies step t-1's SGD update and runs
// step t's forward in ONE launch, then mlp_head_kernel<.., KS2> finishes step t.
//   blocks [0, HT*KS2): block (jt, ks) OWNS the W1 tile [16 hidden][56 features]:
//     wave w forms dW1^T[jt][ks*56 + 16w .. +16) = dz1T[jt] . x_prev (f32 MFMA,
//     K = batch; wave 3 has 8 live columns), W1new = W1old - lr * g -> LDS + p_new;
//     barrier; then z1 partial of row tiles rt = w, w+4, .. over the block's 56 features
//     with W1new from LDS -> slab[ks].  No tile is computed twice and no W1 gradient is
//     ever stored.
//   blocks [HT*KS2, +HT): wgrad_small (dW2 / db1 / db2 of step t-1, p_old -> p_new; the
//     loss/accuracy record and global_step += 1 of step t-1).
// lr = 0 / stats_on = 0 (the first step after a flush): a pure copy p_old -> p_new.
// Removes one dependent kernel boundary and one cold-load phase per step vs the 3-launch
// step (fwd / head / wgrad).
// XW > 0 (pipelined FUSED data-parallel engine, launched with KSX = KS3): each 16x16 local
// gradient slice (summed over the two K-split waves) is exchanged by its K-split-0 wave in LL
// words with the XW - 1 peers (xg_exchange, epoch slot bid * NCG + column group) and summed
// in rank order before the apply -- the all-reduce of the 3-launch fused engine,
// moved into the next step's first launch (2 launches per data-parallel step).
// TRACE (probe builds, tools/probes/mlp_pipelined_trace.py): per wave, s_memrealtime stamps
// 0 entry, 1 phase-A operands landed, 2 W1 tile applied (after the barrier), 3 slab stored;
// small-parameter blocks: 0 entry, 3 done.  tr: [blocks * 4 waves][4].
// KSX: K slices (blocks per hidden tile).  KS2 = 14 (56 features, 105 blocks: the factor
// engine's layout); KS3 = 28 for the single-GPU step and the fused engines: 203 blocks on the 256 CUs instead of
// 105, phase A's K (the batch) split over two waves per 16-column group (partials added
// through LDS) and phase B's z1 partial over 28 features -- per wave 14 + 8..16 f32 MFMAs
// instead of 28 + 16..32.  f32 MFMAs issue at 32 cycles each on one SIMD, so with one wave
// per SIMD the MFMA issue itself set the two phases' length (profiles/r3/mlp_trace/pmc.md:
// 41 % of the waves' cycles were issue stalls).
// XW == 0 with KSX = KS3 (the single-GPU step): the factors are ROW-major (dz1R / dlR, written
// by head_row<.., RM>) and phase A runs in row-quad form instead -- wave w takes a quarter of
// the batch's quads of 4 rows for all 28 features, the four partials are added in wave order
// through LDS and waves 0 / 1 apply one accumulator each (profiles/rowmajor_factors/).
// FWD = false (mlp_apply_launch: the pending update of the last pipelined step, the flush):
// phase A and the small parameters only -- no forward, no x loads.
// (the body of block `bid`: mlp_fwdapply_kernel runs it with bid = blockIdx.x, the terminal
// head + apply kernel of a launched region with FWD = false on its apply blocks)
// ORD (the lean step, row-quad form): phase A's own operands are requested FIRST -- dz1R / x_prev,
// then the W1 values pw, then phase B's rows xa.  Vector loads return in order, so the first
// MFMA's vmcnt then leaves pw and the cold xa rows in flight instead of waiting for them.
// trs (TRACE, NGT > 0, optional): [blocks * 4 waves][2] split stamps -- 0: the first-issued operand
// class has landed (ORD: factors + x_prev; else the xa rows), 1: unused.
// A16 (the lean step only, on top of ORD; profiles/wide_wt_stores/): the W1 apply runs on all
// four waves over items of (hidden row, four adjacent features), 28 per wave -- one float4 of
// p_old per live lane, requested by every lane of every wave at the pw position (no branch: the
// first MFMA's vmcnt leaves pw and xa in flight, the apply waits for pw alone), the four
// partials read back from LDS as one float4 per wave and added in wave order, one float4 store
// each to p_new and Wt -- instead of waves 0 / 1 moving four dwords at stride D each.
// OPT (momentum / adam, on top of A16; see OptArgs): the item's slot float4s are requested at
// the pw position, right after pw4 (same clamped address in the slot planes), so the first
// MFMA's vmcnt still waits for phase A's operands only and the apply waits for pw4 and the
// slots; the new slot values go back through the p_new store's predicate.  The update is
// computed by every lane and selected by oa.apply (no branch around the loads' uses, which
// would let the compiler sink them below the barrier).
// WD (weight decay / Nesterov; see OptArgs): the same item with opt_update<OPT, WD> -- pw4 is the
// decayed value, so no load is added; apply == 0 stays the copy.
// EMA (the moving average of the parameters; see EmaOptArgs): the item's shadow float4 is requested
// at the slot position, after pw4 and the slots at the same clamped address; once v is selected
// the item stores ema_update(shadow, v) under the p_new store's predicate and oa.apply.
template <int NGT, int XW = 0, bool TRACE = false, bool TWO = false, int KSX = KS2, bool FWD = true,
          bool ORD = false, bool A16 = false, int OPT = OPT_SGD, bool SCHED = false,
          bool WD = false, bool EMA = false>
__device__ __forceinline__ void fwdapply_block(
    const int bid, const float* __restrict__ p_old, float* __restrict__ p_new, float lr,
    const float* __restrict__ x_prev, const float* __restrict__ x, const Bufs& w,
    int* __restrict__ ctr, float* __restrict__ stats, int stats_ring, int B, int stats_on,
    const MlpXg& xg, unsigned long long* __restrict__ tr,
    unsigned long long* __restrict__ trs = nullptr,
    const OptArgsOf<EMA>& oa = OptArgsOf<EMA>{}) {
  static_assert(!ORD || (XW == 0 && KSX == KS3), "load order of the row-quad form");
  static_assert(!A16 || ORD, "the 16-byte apply belongs to the lean step");
  constexpr bool OX = OPT != OPT_SGD || SCHED || WD || EMA;  // the OptArgs path (sgd: no slots)
  static_assert(!OX || (A16 && !TRACE), "optimizer variants: the lean step only");
  // stamps per wave: 0 entry, 1 phase-A operands landed, 2 W1 tile applied + barrier, 3 slab
  // stored; with XW > 0 also 4 local gradient slice ready (exchange starts), 5 two-shot: the
  // owned sums done (first hop), 6 exchange done -- 8 slots per wave then
  constexpr int TRN = XW > 0 ? 8 : 4;
  unsigned long long* trw = TRACE ? tr + (size_t)(bid * 4 + (threadIdx.x >> 6)) * TRN : nullptr;
  if (TRACE) trace_stamp(trw, 0);
  const int BP = NGT > 0 ? NGT * 16 : ((B + 15) >> 4) * 16;
  const int NG = NGT > 0 ? NGT : BP / 16;
  const int RT = (B + 15) >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  constexpr int MAXG = NGT > 0 ? NGT : MAXB / 16;
  constexpr int KWX = D / KSX;            // features per block
  constexpr int NCG = (KWX + 15) / 16;     // 16-column groups of the W1 tile (4 or 2)
  constexpr int KSP = 4 / NCG;             // phase-A K splits (waves per column group)
  constexpr int G2 = (KWX + 15) / 16;      // phase-B 16-feature groups
  static_assert(KSX * KWX == D && KWX % 4 == 0 && NCG * KSP == 4, "K slicing");
  // the single-GPU step's factors are row-major (head_row<.., RM>): phase A in row-quad form
  constexpr bool RM = XW == 0 && KSX == KS3;
  if (bid >= HT * KSX) {
    const int jt = bid - HT * KSX;
    if constexpr (OX)
      wgrad_small<true, NGT, XW, RM, OPT, SCHED, WD, EMA>(jt, wave, lane, 0, p_new, lr, nullptr, w,
                                                          ctr, stats, stats_ring, B, xg, p_old,
                                                          stats_on, oa);
    else
    wgrad_small<true, NGT, XW, RM>(jt, wave, lane, MLP_XG_SMALL_EPOCH + jt * 4 + wave, p_new, lr,
                               nullptr, w, ctr, stats, stats_ring, B, xg, p_old, stats_on);
    if (TRACE) trace_stamp(trw, 3);
    return;
  }
  constexpr int LW = KWX + 4;  // LDS row pitch (floats)
  __shared__ float Wt[16][LW];
  __shared__ float Kred[!RM && KSP > 1 ? NCG : 1][64][4];  // phase-A K-split partials
  __shared__ f32x4 red[RM && !A16 ? 4 * 2 * 64 : 1];       // row-quad form: (wave, accumulator)
  // A16: the four partial tiles as [wave][hidden row][feature]
  __shared__ __attribute__((aligned(16))) float redw[A16 ? 4 : 1][A16 ? 16 : 1][KWX];
  const int jt = bid / KSX, ks = bid % KSX;
  const int f0 = ks * KWX;
  // phase B's x rows are independent of phase A: requested first, so the whole launch
  // makes one memory round trip (B <= 128 -> at most 2 row tiles per wave held here)
  constexpr int RTW = 2;
  float4 xa[RTW][G2];
  float rmv[RTW];
  auto load_xa = [&]() {
#pragma unroll
    for (int t = 0; t < (FWD ? RTW : 0); ++t) {
      const int row = (wave + 4 * t) * 16 + r;
      const float* xr = x + (size_t)(row < B ? row : B - 1) * D + f0;
      rmv[t] = row < B ? 1.f : 0.f;
#pragma unroll
      for (int g = 0; g < G2; ++g) {
        const int k = 16 * g + 4 * q;
        xa[t][g] = f4(xr + (k < KWX ? k : 0));
      }
    }
  };
  if constexpr (!ORD) load_xa();

  if constexpr (RM) {
    // ---- phase A, row-quad form (after fx_phase_a_quads): wave w covers ALL 28 features of
    // the slice for its quarter of the batch's row quads (NG each).  Per quad of 4 rows a lane
    // loads ONE dz1R value (hidden r of row base + q: a 64-B run per row) and ONE float2 of x
    // (features 2r, 2r + 1; lanes r >= 14 are dead) and feeds two MFMAs (accumulator e:
    // features 2r + e): at 112 rows 14 operand loads and 14 MFMAs per wave where the
    // column-group form has 20 and 16, and the slice is not padded to 32 features.  Rows >= B
    // read a clamped x row and a zero factor.  The four partials are added in wave order
    // through LDS; wave e in {0, 1} applies accumulator e.
    const bool lv = r < KWX / 2;
    const int fo = 2 * (lv ? r : KWX / 2 - 1);
    float pw[4] = {0.f, 0.f, 0.f, 0.f};
    // (the wave-uniform branch also keeps the loads HERE: issued unconditionally, the compiler
    // sinks them into the apply branch after the barrier -- a serial round trip)
    // A16: item (hidden row hw, feature quad mw) of this lane; lanes >= IPW repeat the
    // wave's last item (same addresses, same values), so nothing before the p_new store branches
    constexpr int MQ = KWX / 4, IPW = 16 * MQ / 4;
    static_assert(!A16 || (16 * MQ) % 4 == 0, "items per wave");
    const int item = wave * IPW + (lane < IPW ? lane : IPW - 1);
    const int hw = item / MQ, mw = item % MQ, jw = jt * 16 + hw;
    float4 pw4 = {0.f, 0.f, 0.f, 0.f};
    float4 sa4 = {0.f, 0.f, 0.f, 0.f}, sb4 = {0.f, 0.f, 0.f, 0.f};  // OPT: the item's slot values
    [[maybe_unused]] EmaRegs<EMA, float4> em;  // EMA: its shadow values and 1 - d_t
    auto load_pw = [&]() {
      if constexpr (A16) {
        pw4 = f4(p_old + OFF_W1 + (size_t)(jw < H ? jw : H - 1) * D + f0 + 4 * mw);
        if constexpr (OPT != OPT_SGD)
          sa4 = f4(oa.s0 + OFF_W1 + (size_t)(jw < H ? jw : H - 1) * D + f0 + 4 * mw);
        if constexpr (OPT == OPT_ADAM)
          sb4 = f4(oa.s1 + OFF_W1 + (size_t)(jw < H ? jw : H - 1) * D + f0 + 4 * mw);
        if constexpr (EMA)
          em.e = f4(oa.se + OFF_W1 + (size_t)(jw < H ? jw : H - 1) * D + f0 + 4 * mw);
      } else if (wave < 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = jt * 16 + q * 4 + i;
          pw[i] = p_old[OFF_W1 + (size_t)(j < H ? j : H - 1) * D + f0 + fo + wave];
        }
      }
    };
    if constexpr (!ORD) load_pw();
    float av[MAXG];
    float2 xv[MAXG];
    const int u0 = wave * NG;
#pragma unroll
    for (int u = 0; u < MAXG; ++u) {
      if (u < NG) {
        const int row = (u0 + u) * 4 + q;  // < 16 NG = BP
        av[u] = w.dz1R[(size_t)row * HP + jt * 16 + r];
        xv[u] = *reinterpret_cast<const float2*>(x_prev + (size_t)(row < B ? row : B - 1) * D +
                                                 f0 + fo);
      }
    }
    if constexpr (ORD) {  // (the fences pin the issue order of the three operand classes)
      __builtin_amdgcn_sched_barrier(0);
      load_pw();
      __builtin_amdgcn_sched_barrier(0);
      load_xa();
    }
    __builtin_amdgcn_sched_barrier(0);  // all loads in flight together
    // (OPT: adam's b1^t / b2^t while the loads are in flight, not between the sum and the store)
    [[maybe_unused]] OptCoef oc = {};
    if constexpr (OX) oc = opt_coef<OPT, SCHED, WD>(lr, oa);
    if constexpr (EMA) em.om = ema_omd(oa);  // (1 - d_t of the step applied, once per wave)
    if constexpr (TRACE && NGT > 0 && FWD) {
      if (trs) {  // loads issued after the first class: ORD pw + xa, else pw + the factors
        unsigned long long* t2 = trs + (size_t)(bid * 4 + wave) * 2;
        constexpr int NLATE = ORD ? RTW * G2 : 2 * NGT;
        if constexpr (A16) trace_stamp_vm<NLATE + 1>(t2, 0);
        else if (wave < 2) trace_stamp_vm<NLATE + 4>(t2, 0);
        else trace_stamp_vm<NLATE>(t2, 0);
      }
    }
    if (TRACE) trace_stamp(trw, 1);
    f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < MAXG; ++u) {
      if (u < NG) {
        a0 = mfma16x16x4(av[u], xv[u].x, a0);
        a1 = mfma16x16x4(av[u], xv[u].y, a1);
      }
    }
    if constexpr (A16) {
      if (lv) {
#pragma unroll
        for (int i = 0; i < 4; ++i)  // features 2r, 2r + 1 of hidden row 4q + i
          *reinterpret_cast<float2*>(&redw[wave][q * 4 + i][2 * r]) = float2{a0[i], a1[i]};
      }
      __syncthreads();
      float4 part = *reinterpret_cast<const float4*>(&redw[0][hw][4 * mw]);
#pragma unroll
      for (int k = 1; k < 4; ++k) {  // wave order
        const float4 o = *reinterpret_cast<const float4*>(&redw[k][hw][4 * mw]);
        part.x += o.x, part.y += o.y, part.z += o.z, part.w += o.w;
      }
      const bool live = jw < H;
      float4 v;
      if constexpr (OX) {
        v.x = opt_update<OPT, WD>(pw4.x, part.x, sa4.x, sb4.x, oc);
        v.y = opt_update<OPT, WD>(pw4.y, part.y, sa4.y, sb4.y, oc);
        v.z = opt_update<OPT, WD>(pw4.z, part.z, sa4.z, sb4.z, oc);
        v.w = opt_update<OPT, WD>(pw4.w, part.w, sa4.w, sb4.w, oc);
        if (!oa.apply) v = pw4;  // nothing pending: a copy, and no slot byte is written
        if constexpr (OPT != OPT_SGD) {
          if (oa.apply && lane < IPW && live) {
            float* so = oa.s0 + OFF_W1 + (size_t)jw * D + f0 + 4 * mw;
            *reinterpret_cast<float4*>(so) = sa4;
            if constexpr (OPT == OPT_ADAM)
              *reinterpret_cast<float4*>(oa.s1 + (so - oa.s0)) = sb4;
          }
        }
        if constexpr (EMA) {  // (after the select: v is the value the p_new store writes)
          if (oa.apply && lane < IPW && live) {
            const float4 e = {ema_update(em.e.x, v.x, em.om), ema_update(em.e.y, v.y, em.om),
                              ema_update(em.e.z, v.z, em.om), ema_update(em.e.w, v.w, em.om)};
            *reinterpret_cast<float4*>(oa.se + OFF_W1 + (size_t)jw * D + f0 + 4 * mw) = e;
          }
        }
      } else {
      v.x = pw4.x - lr * part.x, v.y = pw4.y - lr * part.y;
      v.z = pw4.z - lr * part.z, v.w = pw4.w - lr * part.w;
      }
      // (every lane: the LDS store also keeps the pw load above the barrier, where it was issued)
      if (FWD)  // padded hidden rows contribute exact zeros
        *reinterpret_cast<float4*>(&Wt[hw][4 * mw]) = live ? v : float4{0.f, 0.f, 0.f, 0.f};
      if (lane < IPW && live)
        *reinterpret_cast<float4*>(p_new + OFF_W1 + (size_t)jw * D + f0 + 4 * mw) = v;
    } else {
    red[(wave * 2 + 0) * 64 + lane] = a0;
    red[(wave * 2 + 1) * 64 + lane] = a1;
    __syncthreads();
    if (wave < 2) {
      f32x4 part = red[wave * 64 + lane];
#pragma unroll
      for (int k = 1; k < 4; ++k) {  // wave order
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
          if (FWD) Wt[hl][fl] = j < H ? v : 0.f;  // padded hidden rows contribute exact zeros
          if (j < H) p_new[OFF_W1 + (size_t)j * D + f0 + fl] = v;
        }
      }
    }
    }  // !A16
  } else {
    // ---- phase A: this wave's 16 x 16 slice of the updated W1 tile (K split sp of KSP) -----
    const int cgp = wave % NCG, sp = wave / NCG;
    const int fl = cgp * 16 + r;            // feature within the block's slice
    const bool cv = fl < KWX;               // (14 slices: wave 3 has 8 live columns)
    const int fc = f0 + (cv ? fl : KWX - 1);
    const float* a = w.dz1T + (size_t)(jt * 16 + r) * BP + q * 4;
    const float* xc = x_prev + fc;
    constexpr int GPS = (MAXG + KSP - 1) / KSP;  // batch groups per K split
    const int g0 = sp * GPS;
    float4 av[GPS];
    float xv[GPS][4];
    float pw[4] = {0.f, 0.f, 0.f, 0.f};
    // exchange-epoch slot of this 16 x 16 slice (the K split 0 wave exchanges the summed tile)
    const int eslot = bid * NCG + cgp;
    const unsigned ep = XW > 0 ? xg.epochs[eslot] + 1 : 0u;
#pragma unroll
    for (int gg = 0; gg < GPS; ++gg) {
      const int g = g0 + gg;
      if (g < NG) {
        av[gg] = f4(a + g * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int b = g * 16 + q * 4 + e;  // rows >= B: dz1T is zero there
          xv[gg][e] = xc[(size_t)(b < B ? b : B - 1) * D];
        }
      }
    }
    // SPLITX (exchange engines, two K-split waves per column group): BOTH waves finish half of
    // the slice -- wave sp joins, exchanges and applies elements 2 sp, 2 sp + 1 of each lane --
    // so the exchange's uncached-memory transactions are spread over all 4 waves of the block
    // (the exchange bounds the phase at 4-8 ranks, tools/probes/engine_trace.py)
    const bool SPLITX = XW > 0 && KSP == 2 && (xg.split & 1);
    if (SPLITX || sp == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (SPLITX && (i >> 1) != sp) continue;
        const int j = jt * 16 + q * 4 + i;
        pw[i] = p_old[OFF_W1 + (size_t)(j < H ? j : H - 1) * D + fc];
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // all loads in flight together
    if (TRACE) trace_stamp(trw, 1);
    f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
    for (int gg = 0; gg < GPS; ++gg) {
      if (g0 + gg < NG) {
        acc0 = mfma16x16x4(av[gg].x, xv[gg][0], acc0);
        acc1 = mfma16x16x4(av[gg].y, xv[gg][1], acc1);
        acc0 = mfma16x16x4(av[gg].z, xv[gg][2], acc0);
        acc1 = mfma16x16x4(av[gg].w, xv[gg][3], acc1);
      }
    }
    float gv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) gv[i] = acc0[i] + acc1[i];
    if (SPLITX) {  // hand the other wave its half: element i goes to wave i / 2
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((i >> 1) != sp) Kred[cgp][lane][i] = gv[i];
      __syncthreads();
      // split 0 + split 1 either way (IEEE addition commutes: the same bits on every rank)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((i >> 1) == sp) gv[i] += Kred[cgp][lane][i];
    } else if constexpr (KSP > 1) {  // the later K split's partial joins split 0 (fixed order)
      if (sp > 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) Kred[cgp][lane][i] = gv[i];
      __syncthreads();
      if (sp == 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) gv[i] += Kred[cgp][lane][i];
    }
    bool fail = false;
    if constexpr (XW > 0) {
    if (SPLITX) {
      size_t offw[2];
      bool okw[2];
      float g2[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = 2 * sp + e;
        const int j = jt * 16 + q * 4 + i;
        okw[e] = cv && j < H;
        offw[e] = OFF_W1 + (size_t)(j < H ? j : 0) * D + fc;
        g2[e] = sp == 0 ? gv[e] : gv[2 + e];
      }
      if (TRACE) trace_stamp(trw, 4);
      // the pair's two hidden rows j, j + 1 (j even, H even: both live or both padding)
      const bool plive = cv && jt * 16 + q * 4 + 2 * sp < H;
      if constexpr (TWO) {
        if (xg.split & 4)  // (DTFX_XG_SPLIT bit 2: the round-4 per-element owners, A/B runs)
          xg_exchange2<XW, 2>(xg, ep, offw, okw, g2, fail, lane, TRACE ? trw : nullptr, 2 * sp);
        else if (xg.split & 16)
          xg_exchange2p<XW, true>(xg, ep, XG_W1_BASE + ((long long)(eslot * 2 + sp) * 64 + lane) * 2,
                                  g2, fail, lane, sp, TRACE ? trw : nullptr, plive);
        else
          xg_exchange2p<XW>(xg, ep, XG_W1_BASE + ((long long)(eslot * 2 + sp) * 64 + lane) * 2,
                            g2, fail, lane, sp, TRACE ? trw : nullptr, plive);
      } else if (xg.split & 16)
        xg_exchange16<XW, true>(xg, ep, XG_W1_BASE + ((long long)(eslot * 2 + sp) * 64 + lane) * 2,
                                g2, fail, plive);
      else
        xg_exchange16<XW>(xg, ep, XG_W1_BASE + ((long long)(eslot * 2 + sp) * 64 + lane) * 2,
                          g2, fail, plive);
      if (TRACE) trace_stamp(trw, 6);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = 2 * sp + e;
        const int hl = q * 4 + i, j = jt * 16 + hl;
        const float pv = sp == 0 ? pw[e] : pw[2 + e];
        const float v = fail ? pv : pv - lr * g2[e];  // timed out: keep W1 (err raised)
        if (cv) {
          if (FWD) Wt[hl][fl] = j < H ? v : 0.f;  // padded hidden rows contribute exact zeros
          if (j < H) p_new[OFF_W1 + (size_t)j * D + f0 + fl] = v;
        }
      }
      if (sp == 0 && lane == 0) xg.epochs[eslot] = ep;
      if (fail) atomicExch(xg.err, 1);
    } else if (sp == 0) {
      size_t offw[4];
      bool okw[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = jt * 16 + q * 4 + i;
        okw[i] = cv && j < H;
        offw[i] = OFF_W1 + (size_t)(j < H ? j : 0) * D + fc;
      }
      if (TRACE) trace_stamp(trw, 4);
      if constexpr (TWO) xg_exchange2<XW>(xg, ep, offw, okw, gv, fail, lane, TRACE ? trw : nullptr);
      else xg_exchange<XW>(xg, ep, offw, okw, gv, fail);
      if (TRACE) trace_stamp(trw, 6);
    }
    }  // XW > 0
    if (!SPLITX && sp == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int hl = q * 4 + i, j = jt * 16 + hl;
        const float v = fail ? pw[i] : pw[i] - lr * gv[i];  // timed out: keep W1 (err raised)
        if (cv) {
          if (FWD) Wt[hl][fl] = j < H ? v : 0.f;  // padded hidden rows contribute exact zeros
          if (j < H) p_new[OFF_W1 + (size_t)j * D + f0 + fl] = v;
        }
      }
    }
    if (XW > 0 && !SPLITX && sp == 0) {
      if (lane == 0) xg.epochs[eslot] = ep;
      if (fail) atomicExch(xg.err, 1);
    }
  }
  if constexpr (!FWD) return;
  __syncthreads();
  if (TRACE) trace_stamp(trw, 2);

  // ---- phase B: z1 partial over the block's KWX features, row tiles rt = wave, wave + 4,
  // ..  lane (r, q): A = x[rt*16 + r][f0 + 16g + 4q + e], B = Wt[r][16g + 4q + e]; the last
  // group is partly live (14 slices: 8 features, q < 2; 28 slices: 12, q < 3)
  float4 wb[G2];
#pragma unroll
  for (int g = 0; g < G2; ++g) {
    const int k = 16 * g + 4 * q;
    wb[g] = k < KWX ? *reinterpret_cast<const float4*>(&Wt[r][k]) : float4{0.f, 0.f, 0.f, 0.f};
  }
  for (int rt = wave, t = 0; rt < RT; rt += 4, ++t) {
    float4 xg[G2];
    float rm;
    if (t < RTW) {  // prefetched (wave-uniform)
#pragma unroll
      for (int g = 0; g < G2; ++g) xg[g] = t == 0 ? xa[0][g] : xa[1][g];
      rm = t == 0 ? rmv[0] : rmv[1];
    } else {        // B > 128: later row tiles load here
      const int row = rt * 16 + r;
      const float* xr = x + (size_t)(row < B ? row : B - 1) * D + f0;
      rm = row < B ? 1.f : 0.f;
#pragma unroll
      for (int g = 0; g < G2; ++g) {
        const int k = 16 * g + 4 * q;
        xg[g] = f4(xr + (k < KWX ? k : 0));
      }
    }
    f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < G2; ++g) {
      // (wb is zero for the dead part of the last group, so no mask is needed on xg there)
      acc0 = mfma16x16x4(xg[g].x * rm, wb[g].x, acc0);
      acc1 = mfma16x16x4(xg[g].y * rm, wb[g].y, acc1);
      acc0 = mfma16x16x4(xg[g].z * rm, wb[g].z, acc0);
      acc1 = mfma16x16x4(xg[g].w * rm, wb[g].w, acc1);
    }
    float* out = w.slab + ((size_t)ks * BP + rt * 16 + q * 4) * HP + jt * 16 + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) out[(size_t)i * HP] = acc0[i] + acc1[i];
  }
  if (TRACE) trace_stamp(trw, 3);
}

template <int NGT, int XW = 0, bool TRACE = false, bool TWO = false, int KSX = KS2, bool FWD = true>
__global__ __launch_bounds__(256) void mlp_fwdapply_kernel(
    const float* __restrict__ p_old, float* __restrict__ p_new, float lr,
    const float* __restrict__ x_prev, const float* __restrict__ x, Bufs w, int* __restrict__ ctr,
    float* __restrict__ stats, int stats_ring, int B, int stats_on, MlpXg xg,
    unsigned long long* __restrict__ tr = nullptr) {
  fwdapply_block<NGT, XW, TRACE, TWO, KSX, FWD>(blockIdx.x, p_old, p_new, lr, x_prev, x, w, ctr,
                                                stats, stats_ring, B, stats_on, xg, tr);
}

// ---------------------------------------------------------------------------
// Lean entry points of the single-GPU two-launch step (28 K slices, row-major factors): the
// bodies above (fwdapply_block<.., 0, .., KS3> / head_row<.., RM>) behind kernel arguments of
// scalars and pointers only -- 16 dwords for the first launch, 7 for the head -- which the file
// is built to PRELOAD into user SGPRs at wave launch (-amdgpu-kernarg-preload-count=16; by-value
// structs such as Bufs / MlpXg are never preloaded).  14 dwords fit beside the kernarg segment
// pointer, so `stats` (read by one wave of one block) comes last and is fetched the usual way.  The workspace regions come from the base
// pointer through ws_layout, the host launchers' own offsets.
//   flags = B | stats_on << 9 | stats_ring << 10 (lean_flags)
// The data-parallel engines, mlp_fwdapply_launch / mlp_head2_launch and the opt-in fused flush
// keep mlp_fwdapply_kernel / mlp_head_kernel.

template <int NGT, bool TRACE, bool FWD, int OPT = OPT_SGD, bool SCHED = false, bool WD = false,
          bool EMA = false>
__device__ __forceinline__ void lean_fwdapply_body(
    const float* __restrict__ p_old, float* __restrict__ p_new, const float* __restrict__ x_prev,
    const float* __restrict__ x, float* __restrict__ ws, int* __restrict__ ctr,
    float* __restrict__ stats, float lr, int flags, unsigned long long* __restrict__ tr,
    unsigned long long* __restrict__ trs, const OptArgsOf<EMA>& oa = OptArgsOf<EMA>{}) {
  const int B = flags & 511, stats_on = (flags >> 9) & 1, stats_ring = flags >> 10;
  const Bufs w = ws_bufs(ws, NGT > 0 ? NGT * 16 : ((B + 15) >> 4) * 16);
  if constexpr (EMA)
    fwdapply_block<NGT, 0, TRACE, false, KS3, FWD, true, true, OPT, SCHED, WD, true>(
        blockIdx.x, p_old, p_new, lr, x_prev, x, w, ctr, stats, stats_ring, B, stats_on, MlpXg{},
        tr, trs, oa);
  else if constexpr (WD)
    fwdapply_block<NGT, 0, TRACE, false, KS3, FWD, true, true, OPT, SCHED, true>(
        blockIdx.x, p_old, p_new, lr, x_prev, x, w, ctr, stats, stats_ring, B, stats_on, MlpXg{},
        tr, trs, oa);
  else if constexpr (OPT != OPT_SGD || SCHED)
    fwdapply_block<NGT, 0, TRACE, false, KS3, FWD, true, true, OPT, SCHED>(
        blockIdx.x, p_old, p_new, lr, x_prev, x, w, ctr, stats, stats_ring, B, stats_on, MlpXg{},
        tr, trs, oa);
  else
  fwdapply_block<NGT, 0, TRACE, false, KS3, FWD, true, true>(
      blockIdx.x, p_old, p_new, lr, x_prev, x, w, ctr, stats, stats_ring, B, stats_on, MlpXg{}, tr,
      trs);
}

template <int NGT, bool FWD = true>
__global__ __launch_bounds__(256) void mlp_lean_fwdapply_kernel(
    const float* __restrict__ p_old, float* __restrict__ p_new, const float* __restrict__ x_prev,
    const float* __restrict__ x, float* __restrict__ ws, float lr, int flags,
    int* __restrict__ ctr, float* __restrict__ stats) {
  lean_fwdapply_body<NGT, false, FWD>(p_old, p_new, x_prev, x, ws, ctr, stats, lr, flags, nullptr,
                                      nullptr);
}

// The momentum / adam instantiations (OptArgs): the SGD kernel's nine arguments, then the slot
// planes, the step pair, the three hyper-parameter words (gpu_ps_optim.hyper_args) and
// oflags = apply | par << 1.
template <int NGT, bool FWD, int OPT>
__global__ __launch_bounds__(256) void mlp_lean_fwdapply_opt_kernel(
    const float* __restrict__ p_old, float* __restrict__ p_new, const float* __restrict__ x_prev,
    const float* __restrict__ x, float* __restrict__ ws, float lr, int flags,
    int* __restrict__ ctr, float* __restrict__ stats, float* __restrict__ s0,
    float* __restrict__ s1, int* __restrict__ tp, float h0, float h1, float h2, int oflags) {
  static_assert(OPT == OPT_MOMENTUM || OPT == OPT_ADAM, "stateful kinds");
  const OptArgs oa = {s0, s1, tp, h0, h1, h2, oflags & 1, (oflags >> 1) & 1};
  lean_fwdapply_body<NGT, false, FWD, OPT>(p_old, p_new, x_prev, x, ws, ctr, stats, lr, flags,
                                           nullptr, nullptr, oa);
}

// The scheduled instantiations (sched_rate): the optimizer kernel's arguments -- tp heads the
// 8-word schedule block, lr is the base rate -- and the rate ring.  OPT_SGD here is scheduled
// gradient descent: the step pair and the explicit apply bit, no slot planes.
template <int NGT, bool FWD, int OPT>
__global__ __launch_bounds__(256) void mlp_lean_fwdapply_sched_kernel(
    const float* __restrict__ p_old, float* __restrict__ p_new, const float* __restrict__ x_prev,
    const float* __restrict__ x, float* __restrict__ ws, float lr, int flags,
    int* __restrict__ ctr, float* __restrict__ stats, float* __restrict__ s0,
    float* __restrict__ s1, int* __restrict__ tp, float h0, float h1, float h2, int oflags,
    float* __restrict__ lrs) {
  const OptArgs oa = {s0, s1, tp, h0, h1, h2, oflags & 1, (oflags >> 1) & 1, lrs};
  lean_fwdapply_body<NGT, false, FWD, OPT, true>(p_old, p_new, x_prev, x, ws, ctr, stats, lr, flags,
                                                 nullptr, nullptr, oa);
}

// The weight-decay / Nesterov instantiations (OptArgs' WD coefficients): the scheduled kernel's
// arguments and the four coefficient words l2, dec, na, nb.  SCHED = false: tp is the plain step
// pair, lr the rate itself and lrs unused.  Every kind, sgd included, takes the explicit apply
// bit; sgd has no slot plane.
template <int NGT, bool FWD, int OPT, bool SCHED>
__global__ __launch_bounds__(256) void mlp_lean_fwdapply_wd_kernel(
    const float* __restrict__ p_old, float* __restrict__ p_new, const float* __restrict__ x_prev,
    const float* __restrict__ x, float* __restrict__ ws, float lr, int flags,
    int* __restrict__ ctr, float* __restrict__ stats, float* __restrict__ s0,
    float* __restrict__ s1, int* __restrict__ tp, float h0, float h1, float h2, int oflags,
    float* __restrict__ lrs, float l2, float dec, float na, float nb) {
  const OptArgs oa = {s0, s1, tp, h0, h1, h2, oflags & 1, (oflags >> 1) & 1, lrs, l2, dec, na, nb};
  lean_fwdapply_body<NGT, false, FWD, OPT, SCHED, true>(p_old, p_new, x_prev, x, ws, ctr, stats,
                                                        lr, flags, nullptr, nullptr, oa);
}

// The moving-average instantiations (EmaOptArgs): the weight-decay kernel's arguments,
// then the shadow plane and 1 - decay; oflags bit 2 is the num_updates flag.  ONE family for every
// optimizer with and without decay: the block is always the WD one, and without decay the
// coefficients are OptArgs' defaults (l2, dec, na, nb) = (0, 0, 0, 1), with which every WD term is
// exact for finite values -- fma(0, p, g) = g, 0 * g' + 1 * accum = accum, p - 0 * p = p -- so
// the parameters and slots are the non-WD kernels' bits (tests/test_fused_ema_gpu.py).  OPT_SGD
// is gradient descent with the step pair and no slot plane, as in the WD family.
template <int NGT, bool FWD, int OPT, bool SCHED>
__global__ __launch_bounds__(256) void mlp_lean_fwdapply_ema_kernel(
    const float* __restrict__ p_old, float* __restrict__ p_new, const float* __restrict__ x_prev,
    const float* __restrict__ x, float* __restrict__ ws, float lr, int flags,
    int* __restrict__ ctr, float* __restrict__ stats, float* __restrict__ s0,
    float* __restrict__ s1, int* __restrict__ tp, float h0, float h1, float h2, int oflags,
    float* __restrict__ lrs, float l2, float dec, float na, float nb, float* __restrict__ se,
    float omd) {
  const EmaOptArgs oa = {{s0, s1, tp, h0, h1, h2, oflags & 1, (oflags >> 1) & 1, lrs, l2, dec, na,
                          nb}, se, omd, (oflags >> 2) & 1};
  lean_fwdapply_body<NGT, false, FWD, OPT, SCHED, true, true>(p_old, p_new, x_prev, x, ws, ctr,
                                                              stats, lr, flags, nullptr, nullptr,
                                                              oa);
}

template <int NGT>
__global__ __launch_bounds__(256) void mlp_lean_fwdapply_trace_kernel(
    const float* __restrict__ p_old, float* __restrict__ p_new, const float* __restrict__ x_prev,
    const float* __restrict__ x, float* __restrict__ ws, float lr, int flags,
    int* __restrict__ ctr, float* __restrict__ stats, unsigned long long* __restrict__ tr,
    unsigned long long* __restrict__ trs) {
  lean_fwdapply_body<NGT, true, true>(p_old, p_new, x_prev, x, ws, ctr, stats, lr, flags, tr, trs);
}

template <int NGT, bool TRACE, int ACT = HACT_SIGMOID>
__device__ __forceinline__ void lean_head_body(const float* __restrict__ p,
                                               const int* __restrict__ labels,
                                               float* __restrict__ ws, int B,
                                               unsigned long long* __restrict__ tr) {
  const Bufs w = ws_bufs(ws, NGT > 0 ? NGT * 16 : ((B + 15) >> 4) * 16);
  head_row<false, TRACE, 0, KS3, true, NGT, true, false, ACT>(
      blockIdx.x, threadIdx.x, p, p, 0.f, nullptr, labels, w, B, tr, MlpXg{}, nullptr);
}

// (ACT: the hidden activation, common.h; relu and tanh exist for the plain and the dropout head)
template <int NGT, int ACT = HACT_SIGMOID>
__global__ __launch_bounds__(64) void mlp_lean_head_kernel(const float* __restrict__ p,
                                                           const int* __restrict__ labels,
                                                           float* __restrict__ ws, int B) {
  lean_head_body<NGT, false, ACT>(p, labels, ws, B, nullptr);
}

// The lean head with dropout (MlpDrop by its words: 14 argument dwords, all preloaded).
template <int NGT, int ACT = HACT_SIGMOID>
__global__ __launch_bounds__(64) void mlp_lean_head_drop_kernel(
    const float* __restrict__ p, const int* __restrict__ labels, float* __restrict__ ws, int B,
    const int* __restrict__ ctr, unsigned k0, unsigned k1, unsigned thr, unsigned stream,
    float scale) {
  const Bufs w = ws_bufs(ws, NGT > 0 ? NGT * 16 : ((B + 15) >> 4) * 16);
  const MlpDrop da = {ctr, k0, k1, thr, stream, scale};
  head_row<false, false, 0, KS3, true, NGT, true, true, ACT>(blockIdx.x, threadIdx.x, p, p, 0.f,
                                                             nullptr, labels, w, B, nullptr,
                                                             MlpXg{}, nullptr, da);
}

template <int NGT>
__global__ __launch_bounds__(64) void mlp_lean_head_trace_kernel(
    const float* __restrict__ p, const int* __restrict__ labels, float* __restrict__ ws, int B,
    unsigned long long* __restrict__ tr) {
  lean_head_body<NGT, true>(p, labels, ws, B, tr);
}

// Terminal step of a launched region with the flush folded in (opt-in,
// measured slower: see mlp_flush_fused): the head of
// the region's last step AND the apply of that step's update -- what mlp_head_kernel + the
// apply-only mlp_fwdapply_kernel<.., FWD = false> (mlp_apply_launch) do as two dependent
// launches -- in ONE launch, so the region ends on the step's own second launch.
//   blocks [0, NHB): head rows 4 * bid + wave (one wave per batch row, as mlp_head_kernel);
//     each row's wave publishes with ONE agent-scope release add on sync[0] (its stores to
//     hbuf / dz1T / dlT / rowstat retired and written back first).
//   blocks [NHB, NHB + HT * KSX + HT): apply blocks: thread 0 waits (agent-scope acquire)
//     until sync[0] == B, then the block runs the apply-only body on the step's parameters
//     p_cur -> p_next (the same code, operands and summation order as the flush launch: the
//     result is bit-identical).
// Every wait is bounded (`ticks` of s_memrealtime): a timed-out block sets sync[2] and skips
// its apply (the host raises: FusedMLPTrainer.check()).  The grid (25 + 203 blocks of 256
// threads at batch 100) is a fraction of one wave slot per CU, so every head block is resident
// while the apply blocks wait.  The last apply block to finish zeroes sync[0..1] for the next
// region (stream order: no launch reads them before this one has ended).
template <int NGT, int KSX>
__global__ __launch_bounds__(256) void mlp_head_flush_kernel(
    const float* __restrict__ p_cur, float* __restrict__ p_next, float lr,
    const float* __restrict__ x, const int* __restrict__ labels, Bufs w, int* __restrict__ ctr,
    float* __restrict__ stats, int stats_ring, int B, long long ticks) {
  const int nhb = (B + 3) >> 2;
  const int bid = blockIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (bid < nhb) {
    const int row = bid * 4 + wave;
    if (row >= B) return;
    // (KS3: row-major factors, what its apply blocks' fwdapply_block<.., 0, .., KS3> reads)
    head_row<false, false, 0, KSX, KSX == KS3>(row, lane, p_cur, p_cur, 0.f, nullptr, labels, w, B,
                                               nullptr, MlpXg{}, nullptr);
    // release at agent scope: the wave's stores are complete and written back past this
    // XCD's L2 before the count moves (one add per row)
    if (lane == 0) __hip_atomic_fetch_add(w.sync, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  __shared__ int ok_s;
  if (threadIdx.x == 0) {
    const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
    int ok = 1;
    while (__hip_atomic_load(w.sync, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < B) {
      if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > ticks ||
          __hip_atomic_load(w.sync + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        ok = 0;
        __hip_atomic_store(w.sync + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    ok_s = ok;
  }
  __syncthreads();
  if (ok_s)
    fwdapply_block<NGT, 0, false, false, KSX, false>(bid - nhb, p_cur, p_next, lr, x, x, w, ctr,
                                                     stats, stats_ring, B, 1, MlpXg{}, nullptr);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int napply = (int)gridDim.x - nhb;
    if (__hip_atomic_fetch_add(w.sync + 1, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == napply - 1) {
      __hip_atomic_store(w.sync, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(w.sync + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace mlp
}  // namespace dtfx
