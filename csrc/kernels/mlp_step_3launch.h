// Fused MLP step (mlp_step.hip): the three-launch step -- mlp_fwd / mlp_head / mlp_wgrad.
// head_row and wgrad_small are also the bodies of the two-launch step's head and of its
// small-parameter blocks (mlp_step_fwdapply.h, mlp_step_factor.h).
//
// Design rule (measured, profiles/): at this size the step is bound by how
// many bytes EACH CU must pull and by dependent kernel boundaries (~1.5 us),
// not by FLOPs (32 MFLOP = 0.2 us of f32 MFMA).  A first version that gave
// each of 49 workgroups a full-K 16x16 tile moved ~150 KB per CU and took
// ~10 us per kernel.  This version keeps every workgroup at 7-21 KB and
// spreads each phase over ~100-350 workgroups:
//
//   K1 mlp_fwd   grid (row tile 16) x (hidden tile 16) x (K slice of 112):
//                partial z1 = x . W1 over its K slice -> slab[ks]
//                (deferred-apply mode: W1 <- W1 - lr * G on the fly,
//                 published to the ping-pong buffer by the rt == 0 blocks)
//   K2 mlp_head  one wave per batch row: z1 = sum of 7 slabs + b1,
//                h = sigmoid, logits = h . W2 + b2, softmax, xent, accuracy,
//                dlogits = (p - y)/B, dz1 = (dlogits . W2^T) * h * (1 - h)
//                -> hbuf [b][j], dz1T [j][b], dlT [c][b], rowstat [b]
//                (head of the single-GPU two-launch step, RM: the factors go out
//                 ROW-major instead, dz1R [b][j] as one 8-B store per lane -- a
//                 coalesced 400-B run per row -- and dlR [b][16]; nothing is
//                 stored to dz1T / dlT then)
//   K3 mlp_wgrad 343 blocks: dW1^T tile = dz1^T . x   (f32 MFMA, K = batch)
//                  7 blocks: dW2^T = dl^T . h, db1, db2 (MFMA against ones),
//                            mean loss / accuracy -> stats ring
//                (the single-GPU two-launch step's first launch, mlp_fwdapply
//                 <.., XW = 0, KS3>, reads dz1R / dlR: its W1 update runs over
//                 quads of 4 batch rows, one dz1R value and one float2 of x per
//                 lane and quad)
//                direct mode: the SGD apply is fused into the epilogue
//                (each parameter element is owned by exactly one lane);
//                grad mode: writes the flat gradient for an all-reduce.
//
// global_step (worker.py:29-32,141) is a device int advanced by ONE thread of
// mlp_wgrad after it has used the value as the stats-ring index; no other
// thread of any launch touches it.
#pragma once
#include "mlp_step_api.h"
#include "mlp_step_opt.h"
#include "mlp_step_ws.h"
#include "mlp_step_xg.h"
#include "philox.h"

// Where the dropout mask's Philox rounds run in head_row (measured: profiles/dropout/README.md).
//   0: pinned behind the loads' fence, ahead of the first use of a slab value
//   1: behind the fence, not pinned: the compiler spreads the rounds over the per-plane adds,
//      between the loads' waits (the default)
//   2: after the slab sum (through a data dependence on it)
#ifndef DTFX_MLP_DROP_PLACE
#define DTFX_MLP_DROP_PLACE 1
#endif

namespace dtfx {
namespace mlp {

// ---------------------------------------------------------------------------
// K1: partial z1 over one K slice (+ deferred W1 apply)
// ---------------------------------------------------------------------------
template <bool APPLY, bool TRACE>
__global__ __launch_bounds__(64) void mlp_fwd_kernel(
    const float* __restrict__ p_old, const float* __restrict__ grad, float lr,
    float* __restrict__ p_new, const float* __restrict__ x, Bufs w, int B,
    unsigned long long* __restrict__ tr) {
  if (TRACE) trace_stamp(tr, blockIdx.x * 4 + 0);
  const int RT = (B + 15) >> 4, BP = RT * 16;
  const int rt = blockIdx.x % RT, jt = (blockIdx.x / RT) % HT, ks = blockIdx.x / (RT * HT);
  const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;

  const int row = rt * 16 + r, col = jt * 16 + r;
  const bool rv = row < B, cv = col < H;
  const int k0 = ks * KW + q * 4;
  const float* xr = x + (size_t)(rv ? row : 0) * D + k0;
  const size_t woff = OFF_W1 + (size_t)(cv ? col : 0) * D + k0;

  // Loads are unconditional (clamped rows/cols) and masked after the fact:
  // a guarded load becomes its own exec-masked branch in the ISA.
  const float rm = rv ? 1.f : 0.f, cm = cv ? 1.f : 0.f;
  float4 xa[KW / 16], wa[KW / 16];
#pragma unroll
  for (int g = 0; g < KW / 16; ++g) {
    xa[g] = f4(xr + g * 16);
    wa[g] = f4(p_old + woff + g * 16);
  }
  float4 ga[KW / 16];
  if (APPLY) {
#pragma unroll
    for (int g = 0; g < KW / 16; ++g) ga[g] = f4(grad + woff + g * 16);
  }
  // Keep every load above this point in flight together: without the fence
  // hipcc sinks them into the MFMA chain as 3-4 serial vmcnt(0) round trips.
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = 0; g < KW / 16; ++g) {
    xa[g].x *= rm; xa[g].y *= rm; xa[g].z *= rm; xa[g].w *= rm;
    wa[g].x *= cm; wa[g].y *= cm; wa[g].z *= cm; wa[g].w *= cm;
  }
  if (APPLY) {
#pragma unroll
    for (int g = 0; g < KW / 16; ++g) {
      float4 gg = ga[g];
      gg.x *= cm; gg.y *= cm; gg.z *= cm; gg.w *= cm;
      wa[g].x -= lr * gg.x;
      wa[g].y -= lr * gg.y;
      wa[g].z -= lr * gg.z;
      wa[g].w -= lr * gg.w;
      if (rt == 0 && cv) *reinterpret_cast<float4*>(p_new + woff + g * 16) = wa[g];
    }
  }
  if (TRACE) trace_stamp(tr, blockIdx.x * 4 + 1);
  f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
  for (int g = 0; g < KW / 16; ++g) {
    acc0 = mfma16x16x4(xa[g].x, wa[g].x, acc0);
    acc1 = mfma16x16x4(xa[g].y, wa[g].y, acc1);
    acc0 = mfma16x16x4(xa[g].z, wa[g].z, acc0);
    acc1 = mfma16x16x4(xa[g].w, wa[g].w, acc1);
  }
  float* out = w.slab + ((size_t)ks * BP + rt * 16 + q * 4) * HP + jt * 16 + r;
  if (TRACE) {
    asm volatile("" ::"v"(acc0[0]), "v"(acc1[0]));
    trace_stamp(tr, blockIdx.x * 4 + 2);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) out[(size_t)i * HP] = acc0[i] + acc1[i];
  if (TRACE) trace_stamp(tr, blockIdx.x * 4 + 3);
}

// ---------------------------------------------------------------------------
// K2: per-row head (one wave per batch row)
// ---------------------------------------------------------------------------
// XW > 0 (factor exchange, MlpXg in xgmi.h): the row's dz1 values are also pushed as LL
// words into slot (parity, me) of every peer and every peer's values for the same (j, row)
// are gathered from local memory into dz1A [XW][BP][HP] -- the all-gather of the backprop
// factors that mlp_wgrad_factor_kernel turns into the global weight gradient.
// (the body of one row's wave: mlp_head_kernel runs it as a one-wave block, the terminal
// head + apply kernel of a launched region as one of four waves of a block)
// RM: the factors are stored row-major (dz1R / dlR) for mlp_fwdapply_kernel<.., 0, .., KS3>
// and NOT to dz1T / dlT.
// NGT > 0: the batch is padded to NGT * 16 rows at compile time.
// Load placement (ISA read and A/B measured: profiles/head_label_load/README.md).  Everything
// behind the scheduling fence is ONE unmasked instruction stream up to the hbuf store: a lane's
// two units are summed as a pair (one v_pk_add_f32 per slab plane, started from 0, planes in
// order) and masked by select, where two exec-masked blocks used to run one 28-add chain each.
// With no branch behind the fence the compiler issues the label's load -- a plain scalar load,
// the address is wave-uniform -- at the head of the kernel, ahead of the operand loads; it used
// to sink it behind the first unit's chain and wait for it in the tail.  The label is NOT read
// with a per-lane vector load (row offset laundered through a VGPR): that form puts a cold
// 64-lane load at the head of the in-order vmcnt queue and was measured slower than the late
// scalar load.  Loads from a `const __restrict__` kernel argument are constant memory to the
// compiler and carry no ordering against the fence, so the b1 / W2 / b2 loads go through a
// laundered global pointer: ordinary loads, which stay in front of it.
// DROP (MlpDrop, mlp_step_api.h): inverted dropout on h.  The step word is one more wave-uniform
// scalar load at the head of the kernel, beside the label's; the lane's ONE Philox call (units
// 2l, 2l + 1 share the counter (100 row + 2l) >> 2 and take words 0, 1 or 2, 3 of it) runs behind
// the loads' fence, its ~60 integer VALU issues spread over the slab planes' adds between the
// loads' waits (DTFX_MLP_DROP_PLACE above: pinned ahead of the first slab use it measured no
// faster).  hbuf and the logits take the dropped, rescaled h; dz1 the mask factor
// and the undropped h.  DROP = false compiles to the code without it.
// ACT (common.h: hidden_act / hidden_act_bwd): the hidden activation.  Its derivative comes from
// the h the lane already holds, so ReLU and tanh add no load, no launch and no workspace; ReLU's
// h is a select (exactly +0 for z <= 0, padding lanes too).  HACT_SIGMOID compiles to the code
// before the parameter existed.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <bool APPLY, bool TRACE, int XW = 0, int NSLAB = KS, bool RM = false, int NGT = 0,
          bool SB = false, bool DROP = false, int ACT = HACT_SIGMOID>
__device__ __forceinline__ void head_row(
    const int row, const int lane, const float* __restrict__ p_old,
    const float* __restrict__ grad, float lr, float* __restrict__ p_new,
    const int* __restrict__ labels, const Bufs& w, int B, unsigned long long* __restrict__ tr,
    const MlpXg& xg, float* __restrict__ dz1A, const MlpDrop& da = MlpDrop{}) {
  static_assert(XW == 0 || (!APPLY && !TRACE), "the factor exchange runs the direct step");
  static_assert(!DROP || (XW == 0 && !TRACE), "dropout: the lean head and the three-launch head");
  static_assert(ACT == HACT_SIGMOID || (XW == 0 && !TRACE),
                "relu / tanh: the lean head and the three-launch head");
  static_assert(!RM || (XW == 0 && !APPLY), "row-major factors: the single-GPU two-launch step");
  static_assert(!SB || (RM && NSLAB == KS3), "slab loads through a descriptor: the lean head");
  if (TRACE) trace_stamp(tr, row * 4 + 0);
  const int BP = NGT > 0 ? NGT * 16 : ((B + 15) >> 4) * 16;
  const int y = labels[row];
  [[maybe_unused]] unsigned dstep = 0;  // DROP: global_step of this step (wave-uniform)
  if constexpr (DROP) dstep = (unsigned)*da.ctr;
  // (an IEEE division sequence of 13 instructions; the asm pins it HERE, which in the ISA is
  // ahead of every operand load, not under the memory wait.  Computed behind the loads' fence
  // instead it measured the same: profiles/lean_prologue/)
  float invB = 1.f / (float)B;
  asm volatile("" : "+v"(invB));
  const unsigned ep = XW > 0 ? xg.epochs[MLP_XG_HEAD_EPOCH + row] + 1 : 0u;
  const bool publish = APPLY && row == 0;

  // All loads first, unconditional (clamped), masked afterwards.  Lane l owns the ADJACENT
  // hidden units 2l, 2l + 1 (lanes 0..49), so every per-unit operand -- the NSLAB partial
  // z1 slabs, b1, the 10 W2 columns -- arrives as one 8-B load per pair: 49 load
  // instructions per lane instead of 88 (more than the 63 a wave can keep in flight:
  // the 28-slab step waited out a second round trip here).
  float hv[2], w2[2][C], b1v[2];
  int jj[2];
  bool jv[2];
  const int j0 = min(2 * lane, H - 2);  // (H even: j0, j0 + 1 always a valid, aligned pair)
  const bool pv = lane < H / 2;         // (so both units of a lane are live or neither is)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    jv[u] = 2 * lane + u < H;
    jj[u] = j0 + u;
  }
  f32x2 sv[NSLAB];
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  if constexpr (SB) {
    // ONE descriptor over the slab planes, built from wave-uniform values (the workspace base, a
    // kernel argument, and BP); the lane's j0 * 4 is the vector offset, plane and row the scalar
    // one: 28 buffer loads with one s_add each between them.  The pointer form keeps a 64-bit
    // address per lane and rebuilds it for every plane (the plane stride, BP * HP * 4, fits no
    // immediate offset): two VALU adds, an s_mov and an s_nop per load of the one in-order wave.
    const __amdgpu_buffer_rsrc_t sr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)w.slab, (short)0, NSLAB * BP * HP * 4, 0x00020000);
#pragma unroll
    for (int s = 0; s < NSLAB; ++s) {
      const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(sr, j0 * 4, (s * BP + row) * HP * 4, 0);
      sv[s] = f32x2{__uint_as_float(v.x), __uint_as_float(v.y)};
    }
  } else {
#pragma unroll
  for (int s = 0; s < NSLAB; ++s)
    sv[s] = *reinterpret_cast<const f32x2*>(&w.slab[((size_t)s * BP + row) * HP + j0]);
  }
  typedef const __attribute__((address_space(1))) float* gcf;
  typedef const __attribute__((address_space(1))) f32x2* gcf2;
  unsigned long long pa = (unsigned long long)p_old;
  asm("" : "+s"(pa));
  const gcf pq = (gcf)pa;
  {
    const f32x2 v = *(gcf2)(pq + OFF_B1 + j0);
    b1v[0] = v.x;
    b1v[1] = v.y;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const f32x2 v = *(gcf2)(pq + OFF_W2 + c * H + j0);
    w2[0][c] = v.x;
    w2[1][c] = v.y;
  }
  // class-per-lane part of the row: lane l works on class cl = l & 15 (live: cl < C; all four
  // 16-lane rows carry the same values)
  const int cl = lane & 15, cc = min(cl, C - 1);
  const bool clive = cl < C;
  float b2l = pq[OFF_B2 + cc];
  float gb1[2], gw2[2][C], gb2l = 0.f;
  if (APPLY) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      gb1[u] = grad[OFF_B1 + jj[u]];
#pragma unroll
      for (int c = 0; c < C; ++c) gw2[u][c] = grad[OFF_W2 + c * H + jj[u]];
    }
    gb2l = grad[OFF_B2 + cc];
  }
  __builtin_amdgcn_sched_barrier(0);  // all loads in flight together
  if (APPLY) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      b1v[u] -= lr * gb1[u];
#pragma unroll
      for (int c = 0; c < C; ++c) w2[u][c] -= lr * gw2[u][c];
    }
    b2l -= lr * gb2l;
    if (publish) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (jv[u]) {
          p_new[OFF_B1 + jj[u]] = b1v[u];
#pragma unroll
          for (int c = 0; c < C; ++c) p_new[OFF_W2 + c * H + jj[u]] = w2[u][c];
        }
      if (lane < C) p_new[OFF_B2 + lane] = b2l;
    }
  }
  if (TRACE) trace_stamp(tr, row * 4 + 1);
  // DROP: mf[u] = scale where unit 2l + u is kept, else 0 (integer decisions only)
  [[maybe_unused]] float mf[2] = {1.f, 1.f};
  [[maybe_unused]] auto drop_mask = [&](unsigned dep) {  // (dep: 0, place 2's tie to the sum)
    // (H % 4 == 0, j0 even: n & 3 is 0 or 2)
    const unsigned n = (unsigned)row * H + (unsigned)j0 + dep;
    const U4 r = philox10(U4{n >> 2, 0u, dstep, da.stream}, da.k0, da.k1);
    const bool hi = (n & 2u) != 0;
    mf[0] = ((hi ? r.z : r.x) >> 8) < da.thr ? da.scale : 0.f;
    mf[1] = ((hi ? r.w : r.y) >> 8) < da.thr ? da.scale : 0.f;
  };
  if constexpr (DROP && DTFX_MLP_DROP_PLACE == 0) {
    drop_mask(0u);
    // (pinned here, under the loads' wait: nothing below may be scheduled ahead of the rounds)
    asm volatile("" : "+v"(mf[0]), "+v"(mf[1]));
  }
  f32x2 zp = {0.f, 0.f};  // (from 0, planes in order: 0 + (-0) is +0, a sum begun at plane 0 not)
#pragma unroll
  for (int s = 0; s < NSLAB; ++s) zp += sv[s];
  const float zs[2] = {zp.x, zp.y};
  if constexpr (DROP && DTFX_MLP_DROP_PLACE == 1) {
    asm volatile("" ::"v"(zp.x), "v"(zp.y));
    drop_mask(0u);  // (no dependence on the sum: scheduled between the waits above)
  }
  if constexpr (DROP && DTFX_MLP_DROP_PLACE == 2) {
    unsigned dep = 0;
    asm volatile("" : "+v"(dep) : "v"(zp.x), "v"(zp.y));
    drop_mask(dep);
  }
  float hd[2];  // what the logits and hbuf take: h, or with DROP the dropped, rescaled h
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const float sg = hidden_act<ACT>(zs[u] + b1v[u]);
    hv[u] = pv ? sg : 0.f;
    if constexpr (DROP) hd[u] = hv[u] * mf[u];
    else hd[u] = hv[u];
#pragma unroll
    for (int c = 0; c < C; ++c) w2[u][c] = pv ? w2[u][c] : 0.f;
  }
  if (pv)
    *reinterpret_cast<float2*>(&w.hbuf[(size_t)row * HP + 2 * lane]) = make_float2(hd[0], hd[1]);
  // logits = h . W2 + b2: a reduce-scatter leaves class cl's logit on lane l, and the softmax
  // runs ONE class per lane -- one v_exp_f32 per lane, 16-lane row reductions for the max and
  // the denominator -- where all 64 lanes used to repeat the 10-class chains on the same ten
  // numbers (~400 VALU issues of the one wave, the head's compute span)
  float lgp[C];
#pragma unroll
  for (int c = 0; c < C; ++c) lgp[c] = hd[0] * w2[0][c] + hd[1] * w2[1][c];
  const float lgc = wave_reduce_scatter(lgp, lane) + b2l;
  const float m = row_max16(clive ? lgc : -INFINITY);
  // first max, like tf.argmax: the lowest class whose logit equals the max
  const unsigned long long atmax = __ballot(lane < C && lgc == m);
  const int am = atmax ? __builtin_ctzll(atmax) : 0;
  const float ec = clive ? __expf(lgc - m) : 0.f;
  const float se = row_sum16(ec);
  const float inv = fast_rcp(se);
  const int yu = __builtin_amdgcn_readfirstlane(y);  // (wave-uniform: the row's label)
  const float mydl = (ec * inv - (cl == yu ? 1.f : 0.f)) * invB;  // dlogits of class cl
  const float ly = (unsigned)yu < (unsigned)C  // the label's logit (0 for a label out of range)
                       ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lgc), yu & 15))
                       : 0.f;
  float dl[C];
#pragma unroll
  for (int c = 0; c < C; ++c)
    dl[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mydl), c));
  float dzv[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = 2 * lane + u;
    dzv[u] = 0.f;
    if (j < H) {
      float dh = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) dh += dl[c] * w2[u][c];
      if constexpr (DROP) dh *= mf[u];
      dzv[u] = hidden_act_bwd<ACT>(dh, hv[u]);
      if (!RM) w.dz1T[(size_t)j * BP + row] = dzv[u];
    }
  }
  if (RM && lane < H / 2)
    *reinterpret_cast<float2*>(&w.dz1R[(size_t)row * HP + 2 * lane]) =
        make_float2(dzv[0], dzv[1]);
  if constexpr (XW > 0) {
    bool fail = false;
    if (xg.split & 16) head_allgather<XW, true>(xg, ep, row, lane, BP, dzv, dz1A, fail);
    else head_allgather<XW, false>(xg, ep, row, lane, BP, dzv, dz1A, fail);
    if (lane == 0) xg.epochs[MLP_XG_HEAD_EPOCH + row] = ep;
    if (fail) atomicExch(xg.err, 1);
  }
  if (TRACE) trace_stamp(tr, row * 4 + 2);
  if (lane < C) {
    if (RM) w.dlR[(size_t)row * 16 + lane] = mydl;
    else w.dlT[(size_t)lane * BP + row] = mydl;
  }
  if (lane == 0) {
    w.rowstat[2 * row] = m + __logf(se) - ly;  // xent of this row
    w.rowstat[2 * row + 1] = (am == y) ? 1.f : 0.f;
  }
  if (TRACE) trace_stamp(tr, row * 4 + 3);
}

template <bool APPLY, bool TRACE, int XW = 0, int NSLAB = KS, bool RM = false,
          int ACT = HACT_SIGMOID>
__global__ __launch_bounds__(64) void mlp_head_kernel(
    const float* __restrict__ p_old, const float* __restrict__ grad, float lr,
    float* __restrict__ p_new, const int* __restrict__ labels, Bufs w, int B,
    unsigned long long* __restrict__ tr, MlpXg xg, float* __restrict__ dz1A) {
  head_row<APPLY, TRACE, XW, NSLAB, RM, 0, false, false, ACT>(
      blockIdx.x, threadIdx.x, p_old, grad, lr, p_new, labels, w, B, tr, xg, dz1A);
}

// The three-launch head with dropout (the direct step, and the all-reduce engine's step_grad with
// and without its deferred apply).  ctr apart: `const int* __restrict__`, so the step word is a
// scalar load issued with the label's.
template <bool APPLY, int ACT = HACT_SIGMOID>
__global__ __launch_bounds__(64) void mlp_head_drop_kernel(
    const float* __restrict__ p_old, const float* __restrict__ grad, float lr,
    float* __restrict__ p_new, const int* __restrict__ labels, Bufs w, int B,
    const int* __restrict__ ctr, unsigned k0, unsigned k1, unsigned thr, unsigned stream,
    float scale) {
  const MlpDrop da = {ctr, k0, k1, thr, stream, scale};
  head_row<APPLY, false, 0, KS, false, 0, false, true, ACT>(blockIdx.x, threadIdx.x, p_old, grad,
                                                            lr, p_new, labels, w, B, nullptr,
                                                            MlpXg{}, nullptr, da);
}

// ---------------------------------------------------------------------------
// K3: weight gradients (+ fused SGD apply in direct mode)
// ---------------------------------------------------------------------------
// NGT > 0: batch padded to NGT*16 rows at compile time (branch-free loads);
// NGT == 0: generic (runtime NG, guarded loops).
// XW > 0: fused xGMI gradient exchange over XW ranks before the (direct) apply.

// Small parameters of hidden tile jt (one product per wave), shared by mlp_wgrad_kernel and
// mlp_wgrad_factor_kernel; eidx = this wave's exchange-epoch slot.
// p_src: where the current parameter values are read (== p except in the pipelined step,
// which reads the old ping-pong buffer and writes the new one); stats_on = 0 skips the
// loss/accuracy record and the global_step increment.
// RM: the factors are read from the row-major regions dz1R / dlR (one value per lane and batch
// row; the same (group, element) -> row order of the K sum as the transposed form's float4).
// OPT (the lean step's optimizer variants; DIRECT, no exchange): the owning lane also reads and
// rewrites its slot values (addresses clamped like p_src's, stores behind the p store's
// predicate and oa.apply); the stats lane hands the step word on (tp[par ^ 1]).
// WD: the weight-decay / Nesterov family (opt_update<OPT, WD>); decay reaches b1 / W2 / b2 here.
// EMA: the owning lane also reads and rewrites its shadow value (ema_update of the new parameter
// value, behind the p store's predicate and oa.apply), so the shadow covers b1 / W2 / b2.
template <bool DIRECT, int NGT, int XW, bool RM = false, int OPT = OPT_SGD, bool SCHED = false,
          bool WD = false, bool EMA = false>
__device__ __forceinline__ void wgrad_small(int jt, int wave, int lane, int eidx,
                                            float* __restrict__ p, float lr,
                                            float* __restrict__ grad, const Bufs& w,
                                            int* __restrict__ ctr, float* __restrict__ stats,
                                            int stats_ring, int B, const MlpXg& xg,
                                            const float* __restrict__ p_src = nullptr,
                                            int stats_on = 1,
                                            const OptArgsOf<EMA>& oa = OptArgsOf<EMA>{}) {
  constexpr bool OX = OPT != OPT_SGD || SCHED || WD || EMA;  // the OptArgs path (sgd: no slots)
  static_assert(!OX || (DIRECT && XW == 0), "optimizer variants: the lean step only");
  if (p_src == nullptr) p_src = p;
  const int BP = NGT > 0 ? NGT * 16 : ((B + 15) >> 4) * 16;
  const int NG = NGT > 0 ? NGT : BP / 16;
  const int r = lane & 15, q = lane >> 4;
  constexpr int MAXG = NGT > 0 ? NGT : MAXB / 16;
  // ---- small parameters of hidden tile jt: one product per wave -----------
  //   wave 0: dW2^T[:, jt] = dlT . h[:, jt]   wave 1: db1[jt] = dz1T[jt] . 1
  //   wave 2: db2 = dlT . 1 (jt == 0)         wave 3: loss/accuracy (jt == 0)
  // With an exchange (XW > 0), the dW2 product is formed by waves 0 AND 2, each exchanging
  // and applying half of every lane's elements (the exchange's uncached-memory transactions
  // bound these blocks, as in mlp_fwdapply_kernel's split exchange), and db2 moves to wave 3
  // after the loss / accuracy record.
  const bool SPLIT = XW > 0 && (xg.split & 2);
  int role = wave;  // 0 / 2 (SPLIT): dW2 (halves), 1: db1, 2 (!SPLIT): db2, 3: stats (+ db2)
  if (wave == 3) {
    if (jt != 0) return;
    [[maybe_unused]] float rate = 0.f;  // SCHED: the rate of the step this launch applies
    if constexpr (OX) {  // the next launch's step word (this one reads tp[par])
      const int s = oa.tp[oa.par];
      if constexpr (SCHED) rate = sched_rate(lr, s, sched_load(oa.tp));
      if (lane == 0) oa.tp[oa.par ^ 1] = s + (stats_on ? 1 : 0);
    }
    if (stats_on) {
      float l = 0.f, a = 0.f;
      for (int b = lane; b < B; b += 64) {
        l += w.rowstat[2 * b];
        a += w.rowstat[2 * b + 1];
      }
      l = wave_sum(l);
      a = wave_sum(a);
      if (lane == 0) {
        const int step = *ctr;  // this thread is the only reader/writer of ctr
        if (stats) {
          float* st = stats + (size_t)(step % stats_ring) * 2;
          st[0] = l / (float)B;
          st[1] = a / (float)B;
        }
        if constexpr (SCHED) {
          if (oa.lrs) oa.lrs[step % stats_ring] = rate;
        }
        *ctr = step + 1;
      }
    }
    if (!SPLIT) return;
    role = 4;  // db2
  }
  if (!SPLIT && wave == 2 && jt != 0) return;
  const bool dw2 = role == 0 || (SPLIT && role == 2);
  const bool db2 = role == 4 || (!SPLIT && role == 2);
  const float* A = (role == 1) ? w.dz1T + (size_t)(jt * 16 + r) * BP + q * 4
                               : w.dlT + (size_t)r * BP + q * 4;
  const float* hb = w.hbuf + jt * 16 + r;
  const unsigned ep = XW > 0 ? xg.epochs[eidx] + 1 : 0u;
  float4 av[MAXG];
  float bv[MAXG][4];
#pragma unroll
  for (int g = 0; g < MAXG; ++g)
    if (g < NG) {
      if constexpr (RM) {
        const float* AR = (role == 1) ? w.dz1R + jt * 16 + r : w.dlR + r;
        const int pitch = (role == 1) ? HP : 16;
        const int b = g * 16 + q * 4;
        av[g] = float4{AR[(size_t)b * pitch], AR[(size_t)(b + 1) * pitch],
                       AR[(size_t)(b + 2) * pitch], AR[(size_t)(b + 3) * pitch]};
      } else {
        av[g] = f4(A + g * 16);
      }
    }
  if (dw2) {  // one uniform branch around the whole B-operand load block
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
      if (g < NG)
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[g][e] = hb[(size_t)(g * 16 + q * 4 + e) * HP];
  } else {
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[g][e] = 1.f;
  }
  __builtin_amdgcn_sched_barrier(0);  // all loads in flight together
  // Destination offsets (and, in direct mode, the current values) resolved
  // before the MFMAs so the epilogue is a pure store.
  size_t off[4];
  bool ok[4];
  float pv[4];
  float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};  // OPT: slot values
  [[maybe_unused]] EmaRegs<EMA> em;  // EMA: shadow values and 1 - d_t (else: nothing at all)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (dw2) {  // C[c = q*4+i][j = jt*16 + r] -> dW2t[c][j]; SPLIT: wave 0 i < 2, wave 2 i >= 2
      const int c = q * 4 + i, j = jt * 16 + r;
      ok[i] = c < C && j < H && (!SPLIT || (i >> 1) == (role >> 1));
      off[i] = OFF_W2 + (c < C && j < H ? c * H + j : 0);
    } else if (role == 1) {  // C[j = jt*16 + q*4+i][*] -> db1[j]
      const int j = jt * 16 + q * 4 + i;
      ok[i] = r == 0 && j < H;
      off[i] = OFF_B1 + (j < H ? j : 0);
    } else {  // db2: C[c = q*4+i][*] -> db2[c]
      const int c = q * 4 + i;
      ok[i] = r == 0 && c < C;
      off[i] = OFF_B2 + (c < C ? c : 0);
    }
    if (DIRECT) pv[i] = p_src[off[i]];
    if constexpr (OPT != OPT_SGD) sa[i] = oa.s0[off[i]];
    if constexpr (OPT == OPT_ADAM) sb[i] = oa.s1[off[i]];
    if constexpr (EMA) em.e[i] = oa.se[off[i]];
  }
  (void)db2;
  __builtin_amdgcn_sched_barrier(0);
  [[maybe_unused]] OptCoef oc = {};  // (adam's b1^t / b2^t while the loads are in flight)
  if constexpr (OX) oc = opt_coef<OPT, SCHED, WD>(lr, oa);
  if constexpr (EMA) em.om = ema_omd(oa);  // (1 - d_t of the step applied, once per wave)
  // NB: padded batch columns of dz1T/dlT are zero, so multiplying by 1 is exact.
  f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
  for (int g = 0; g < MAXG; ++g) {
    if (g < NG) {
      acc0 = mfma16x16x4(av[g].x, bv[g][0], acc0);
      acc1 = mfma16x16x4(av[g].y, bv[g][1], acc1);
      acc0 = mfma16x16x4(av[g].z, bv[g][2], acc0);
      acc1 = mfma16x16x4(av[g].w, bv[g][3], acc1);
    }
  }
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = acc0[i] + acc1[i];
  bool fail = false;
  if constexpr (XW > 0) {
    if (SPLIT && (role == 1 || role == 4)) {
      // db1 / db2: the product against ones replicates every value over the 16 lanes of its
      // row group, so lane r < 4 of group q takes element i = r alone -- ONE element per lane
      // (W-1 stores, W-1 loads) instead of four with one live lane in sixteen (the traced
      // tail of these blocks: 6.4 us at 8 ranks, profiles/r4/engine_trace/)
      const int is = r & 3;
      auto sel = [&](auto (&a)[4]) { return is == 0 ? a[0] : is == 1 ? a[1] : is == 2 ? a[2] : a[3]; };
      const bool live = r < 4 && (role == 1 ? (jt * 16 + q * 4 + is < H) : (q * 4 + is < C));
      size_t o1[1] = {sel(off)};
      bool k1[1] = {live};
      float v1[1] = {sel(v)};
      xg_exchange<XW, 1>(xg, ep, o1, k1, v1, fail);
      if (live && !fail) {
        if (DIRECT) p[o1[0]] = sel(pv) - lr * v1[0];
        else grad[o1[0]] = v1[0];
      }
      if (lane == 0) xg.epochs[eidx] = ep;
      if (fail) atomicExch(xg.err, 1);
      return;
    }
    if (SPLIT && dw2) {  // this wave's half: elements 2 (role / 2) + e of every lane
      const bool hi = role == 2;  // (selects: no dynamically indexed register arrays)
      size_t o2[2] = {hi ? off[2] : off[0], hi ? off[3] : off[1]};
      bool k2[2] = {hi ? ok[2] : ok[0], hi ? ok[3] : ok[1]};
      float v2[2] = {hi ? v[2] : v[0], hi ? v[3] : v[1]};
      xg_exchange<XW, 2>(xg, ep, o2, k2, v2, fail);
      if (hi) {
        v[2] = v2[0];
        v[3] = v2[1];
      } else {
        v[0] = v2[0];
        v[1] = v2[1];
      }
    } else {
      xg_exchange<XW>(xg, ep, off, ok, v, fail);
    }
  }
  if constexpr (OX) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // (computed by every lane and selected: oa.apply == 0 copies p and leaves the slots)
      const float pn = opt_update<OPT, WD>(pv[i], v[i], sa[i], sb[i], oc);
      if (ok[i]) {
        p[off[i]] = oa.apply ? pn : pv[i];
        if constexpr (OPT != OPT_SGD) {
          if (oa.apply) {
            oa.s0[off[i]] = sa[i];
            if constexpr (OPT == OPT_ADAM) oa.s1[off[i]] = sb[i];
          }
        }
        if constexpr (EMA) {
          if (oa.apply) oa.se[off[i]] = ema_update(em.e[i], pn, em.om);
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (ok[i] && !fail) {
      if (DIRECT) p[off[i]] = pv[i] - lr * v[i];
      else grad[off[i]] = v[i];
    }
  }
  if constexpr (XW > 0) {
    if (lane == 0) xg.epochs[eidx] = ep;
    if (fail) atomicExch(xg.err, 1);
  }
}

template <bool DIRECT, bool TRACE, int NGT, int XW = 0>
__global__ __launch_bounds__(256) void mlp_wgrad_kernel(
    float* __restrict__ p, float lr, float* __restrict__ grad, const float* __restrict__ x,
    Bufs w, int* __restrict__ ctr, float* __restrict__ stats, int stats_ring, int B,
    unsigned long long* __restrict__ tr, MlpXg xg) {
  static_assert(XW == 0 || DIRECT, "the fused exchange applies the update directly");
  const int BP = NGT > 0 ? NGT * 16 : ((B + 15) >> 4) * 16;
  const int NG = NGT > 0 ? NGT : BP / 16;
  // readfirstlane: make the wave id provably uniform (scalar branches, not exec masks)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  constexpr int MAXG = NGT > 0 ? NGT : MAXB / 16;
  constexpr int FG = (FT + 3) / 4;  // 13 feature groups of 4 waves
  const int bid = blockIdx.x;

  if (bid < HT * FG) {
    // ---- dW1^T tile (jt, kt) = dz1T[jt] . x[:, kt], one tile per wave ------
    const int jt = bid / FG, kt = (bid % FG) * 4 + wave;
    if (kt >= FT) return;
    unsigned long long* trw = tr + (size_t)(bid * 4 + wave) * 4;
    if (TRACE) trace_stamp(trw, 0);
    const float* xc = x + kt * 16 + r;
    const float* a = w.dz1T + (size_t)(jt * 16 + r) * BP + q * 4;
    float4 av[MAXG];
    float xv[MAXG][4];
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
      if (g < NG) {
        av[g] = f4(a + g * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int b = g * 16 + q * 4 + e;  // rows >= B: dz1T is zero there
          xv[g][e] = xc[(size_t)(b < B ? b : B - 1) * D];
        }
      }
    }
    const unsigned ep = XW > 0 ? xg.epochs[bid * 4 + wave] + 1 : 0u;
    float pw[4];
    if (DIRECT) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = jt * 16 + q * 4 + i;
        pw[i] = p[OFF_W1 + (size_t)(j < H ? j : H - 1) * D + kt * 16 + r];
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // all loads in flight together
    if (TRACE) trace_stamp(trw, 1);
    f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
      if (g < NG) {
        acc0 = mfma16x16x4(av[g].x, xv[g][0], acc0);
        acc1 = mfma16x16x4(av[g].y, xv[g][1], acc1);
        acc0 = mfma16x16x4(av[g].z, xv[g][2], acc0);
        acc1 = mfma16x16x4(av[g].w, xv[g][3], acc1);
      }
    }
    if (TRACE) {
      asm volatile("" ::"v"(acc0[0]), "v"(acc1[0]));
      trace_stamp(trw, 2);
    }
    size_t offw[4];
    bool okw[4];
    float gv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = jt * 16 + q * 4 + i;
      okw[i] = j < H;
      offw[i] = OFF_W1 + (size_t)(j < H ? j : 0) * D + kt * 16 + r;
      gv[i] = acc0[i] + acc1[i];
    }
    bool fail = false;
    if constexpr (XW > 0) xg_exchange<XW>(xg, ep, offw, okw, gv, fail);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (okw[i] && !fail) {
        if (DIRECT) p[offw[i]] = pw[i] - lr * gv[i];
        else grad[offw[i]] = gv[i];
      }
    }
    if constexpr (XW > 0) {
      if (lane == 0) xg.epochs[bid * 4 + wave] = ep;
      if (fail) atomicExch(xg.err, 1);
    }
    if (TRACE) trace_stamp(trw, 3);
    return;
  }

  wgrad_small<DIRECT, NGT, XW>(bid - HT * FG, wave, lane, bid * 4 + wave, p, lr, grad, w, ctr,
                               stats, stats_ring, B, xg);
}

}  // namespace mlp
}  // namespace dtfx
