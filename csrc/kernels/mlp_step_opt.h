// Fused MLP step (mlp_step.hip): stateful optimizers and learning-rate schedules inside the lean
// two-launch step's first launch.
//
// Momentum and Adam live in that first launch too (mlp_lean_fwdapply_opt_kernel, OptArgs below):
// the lane that owns a parameter element also owns its slot values, so no gradient buffer and no
// optimizer launch exist; the SGD instantiations are unchanged (profiles/fused_optim/).
// Learning-rate schedules (sched_rate, mlp_lean_fwdapply_sched_kernel): scheduled instantiations
// of that entry point -- sgd among them -- compute the rate of the step they apply from the step
// word and an 8-word schedule block, once per wave, and the stats lane publishes it to a rate
// ring; the constant-rate kernels are unchanged (profiles/lr_schedule/: +0.03 .. +0.2 us a step).
// Moving average of the parameters (ema_omd / ema_update, mlp_lean_fwdapply_ema_kernel): the lane
// that stores a new parameter value also reads and rewrites its element of a shadow plane, as it
// does its slot values; every other kernel is unchanged (profiles/ema/).
#pragma once
#include "mlp_step_ws.h"

namespace dtfx {
namespace mlp {

// ---------------------------------------------------------------------------
// Stateful optimizers inside the lean two-launch step (mlp_lean_fwdapply_opt_kernel): gpu_ps.hip's
// formulas (ops/optim.py's momentum_ / adam_; weight decay and Nesterov: the WD family below)
// applied by the lane that owns the element -- the A16 item of fwdapply_block for W1, the ok[i]
// lane of wgrad_small for b1 / W2 / b2.  The slot planes s0 (momentum: accum; adam: m) and s1
// (adam: v) are flat f32 [NPARAM] buffers in the parameter layout, updated IN PLACE (one owner
// per element, read once and written once by it); only the parameters ping-pong.
//   momentum  accum = mu * accum + g;  p -= lr * accum   (mu = 0: accum = g and the SGD bits)
//   adam      m = b1 * m + (1 - b1) * g;  v = b2 * v + (1 - b2) * g * g
//             p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// t = global_step + 1 of the step being applied.  It is NOT read from ctr: the stats lane of the
// small-parameter block jt == 0 writes ctr in this same launch.  tp is a pair of step words
// indexed by the launch's buffer parity par (the index of p_old in the trainer's ping-pong pair):
// every wave reads tp[par], the stats lane alone writes tp[par ^ 1] = tp[par] + stats_on, which
// the NEXT launch (parity par ^ 1) reads -- no word is read and written in one launch.
// apply == 0 (nothing pending): p_old is copied, no slot byte is written.
enum : int { OPT_SGD = 0, OPT_MOMENTUM = 1, OPT_ADAM = 2 };
struct OptArgs {
  float* s0;
  float* s1;
  int* tp;
  float h0, h1, h2;  // momentum: mu; adam: beta1, beta2, epsilon
  int apply, par;
  float* lrs;        // SCHED: the rate ring (f32 [stats_ring], parallel to the stats ring), or null
  // WD (mlp_lean_fwdapply_wd_kernel): wave-uniform coefficients, read by that family alone
  float l2 = 0.f, dec = 0.f, na = 0.f, nb = 1.f;
};
// EMA (mlp_lean_fwdapply_ema_kernel): OptArgs, then the shadow plane, 1 - decay and the
// num_updates flag.  A type of its own, which only the EMA instantiations name (OptArgsOf): three
// more members in OptArgs itself grew the defaulted temporary at every other call site, and
// three traced exchange kernels came out with one renamed register (profiles/ema/).
struct EmaOptArgs : OptArgs {
  float* se = nullptr;
  float omd = 0.f;
  int nu = 0;
};
template <bool EMA>
struct OptArgsSel { typedef OptArgs type; };
template <>
struct OptArgsSel<true> { typedef EmaOptArgs type; };
template <bool EMA>
using OptArgsOf = typename OptArgsSel<EMA>::type;
// Weight decay and Nesterov momentum (the WD instantiations; ops/weight_decay.py is the
// definition, which is ops/optim.py's and torch.optim's).  g' = g + l2 * p is the gradient
// every kind uses -- the parameter is already in the owning lane's registers -- and
//   sgd       p -= rate * g'
//   momentum  accum = mu * accum + g';  p -= rate * (na * g' + nb * accum)
//             (na, nb) = (0, 1) plain, (1, mu) Nesterov: one instantiation for both
//   adam      m, v take g';  p = (p - rate * dec * p) - (rate / (1 - b1^t)) * m / (...)
//             adamw: l2 = 0, dec = wd (decoupled);  not adamw: l2 = wd, dec = 0
// rate is the rate of the step applied: sched_rate's value with a schedule, never adam's
// bias-corrected c.lr.  Decay is uniform over the flat buffer, biases included.
// Moving average of the parameters (the EMA instantiations; ops/ema.py is the definition, which
// is tf.train.ExponentialMovingAverage's): se is one more flat f32 [NPARAM] plane in the
// parameter layout, read and rewritten IN PLACE by the lane that owns the element, after the
// update of step s (t = s + 1) has produced the new value v, in TF's assign_sub form
//   shadow -= (1 - d_t) * (shadow - v)
//   d_t = decay, or with num_updates min(decay, (1 + t) / (10 + t)): 1 - d_t = max(omd, 9 / (10 + t))
// 1 - d_t is wave-uniform (ema_omd: once per wave from the step word tp[par], a correctly rounded
// division; ops/ema.py's one_minus_decay_f32 is this arithmetic operation for operation).  The
// shadow never feeds back into the update, and apply == 0 writes no shadow byte.
// Learning-rate schedules evaluated on the device (the SCHED instantiations; ops/lr_schedule.py
// is the definition, its value_f32 this arithmetic operation for operation).  The step pair is
// then the head of an 8-word block [tp0, tp1, kind | staircase << 2, decay_steps, a, inv_decay,
// inv_warmup, 0], 32-byte aligned.  a = f32(log2 decay_rate) (exponential) or decay_rate (inverse
// time); inv_warmup = 0 skips the warm-up.  s: the 0-based global_step of the step applied.
// Wave-uniform: the whole block is fetched at once (sched_load: every word unconditionally, so
// the wave makes ONE round trip instead of one per word a branch happens to need) and a handful
// of scalar-side operations follow, every alternative computed and selected.
//   staircase q: integer division of the step word (float(s) * f32(1 / 3) misses exact multiples)
//   exponential: exp2(q * log2 rate) on the transcendental unit, as opt_coef's b^t
enum : int { SCHED_CONSTANT = 0, SCHED_EXPONENTIAL = 1, SCHED_INVERSE_TIME = 2 };
typedef int i32x4 __attribute__((ext_vector_type(4)));
struct SchedBlock {
  i32x4 lo, hi;  // lo = {tp0, tp1, flags, decay_steps}, hi = {a, inv_decay, inv_warmup, 0}
};
__device__ __forceinline__ SchedBlock sched_load(const int* __restrict__ blk) {
  return {*reinterpret_cast<const i32x4*>(blk), *reinterpret_cast<const i32x4*>(blk + 4)};
}
__device__ __forceinline__ float sched_rate(float lr0, int s, const SchedBlock& w) {
  const int kind = w.lo.z & 3, stair = (w.lo.z >> 2) & 1;
  const unsigned ds = (unsigned)w.lo.w;
  const float a = __int_as_float(w.hi.x), inv_ds = __int_as_float(w.hi.y);
  const float inv_warm = __int_as_float(w.hi.z);
  const float qi = (float)((unsigned)s / ds), qf = (float)s * inv_ds;
  const float q = stair ? qi : qf;
  const float e = __builtin_amdgcn_exp2f(q * a);
  const float r = __builtin_amdgcn_rcpf(__builtin_fmaf(a, q, 1.f));
  const float decay = kind == SCHED_EXPONENTIAL ? e : kind == SCHED_INVERSE_TIME ? r : 1.f;
  const float lr = lr0 * decay;
  const float warm = fminf(1.f, (float)(s + 1) * inv_warm);
  return inv_warm > 0.f ? lr * warm : lr;
}
// momentum: lr, h0 = mu.  adam: lr = lr / (1 - b1^t), rbc2 = 1 / sqrt(1 - b2^t)
// WD: l2, rd = rate * dec, na, nb (lr stays the rate for sgd and momentum)
struct OptCoef {
  float lr, h0, h1, h2, rbc2;
  float l2, rd, na, nb;
};
template <int OPT, bool SCHED = false, bool WD = false>
__device__ __forceinline__ OptCoef opt_coef(float lr, const OptArgs& oa) {
  if constexpr (SCHED) {  // the applied step's rate
    const SchedBlock w = sched_load(oa.tp);
    lr = sched_rate(lr, oa.par ? w.lo.y : w.lo.x, w);
  }
  OptCoef c = {lr, oa.h0, oa.h1, oa.h2, 1.f};
  if constexpr (WD) c.l2 = oa.l2, c.rd = lr * oa.dec, c.na = oa.na, c.nb = oa.nb;
  if constexpr (OPT == OPT_ADAM) {  // (wave-uniform: once per wave, not per element)
    // b^t = exp2(t log2 b) on the transcendental unit: 0 <= b < 1, so the product is <= 0, and
    // wherever b^t is not negligible against 1 (t |log2 b| < 24) its relative error stays below
    // 24 ulp of the exponent ~ 3e-6 -- 1e-6 of an update of ~lr.  powf would add ~6 KB of code
    // per instantiation in front of the apply.
    const float tf = (float)(oa.tp[oa.par] + 1);
    c.lr = lr / (1.f - __builtin_amdgcn_exp2f(tf * __builtin_amdgcn_logf(oa.h0)));
    c.rbc2 = rsqrtf(1.f - __builtin_amdgcn_exp2f(tf * __builtin_amdgcn_logf(oa.h1)));
  }
  return c;
}
// -> the new parameter value; s0 / s1 become the new slot values
template <int OPT, bool WD = false>
__device__ __forceinline__ float opt_update(float p, float g, float& s0, float& s1,
                                            const OptCoef& c) {
  if constexpr (WD) {  // (optim.hip's expressions; one or two fmas per element on top)
    const float gg = g + c.l2 * p;
    if constexpr (OPT == OPT_SGD) {
      return p - c.lr * gg;
    } else if constexpr (OPT == OPT_MOMENTUM) {
      s0 = c.h0 * s0 + gg;
      return p - c.lr * (c.na * gg + c.nb * s0);
    } else {
      s0 = c.h0 * s0 + (1.f - c.h0) * gg;
      s1 = c.h1 * s1 + (1.f - c.h1) * gg * gg;
      const float pd = p - c.rd * p;
      return pd - c.lr * s0 * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(s1) * c.rbc2 + c.h2);
    }
  } else if constexpr (OPT == OPT_SGD) {  // (scheduled gradient descent: the SGD step's own)
    return p - c.lr * g;
  } else if constexpr (OPT == OPT_MOMENTUM) {
    s0 = c.h0 * s0 + g;
    return p - c.lr * s0;
  } else {
    s0 = c.h0 * s0 + (1.f - c.h0) * g;
    s1 = c.h1 * s1 + (1.f - c.h1) * g * g;
    // v_sqrt_f32 / v_rcp_f32 (1 ulp each) instead of the correctly rounded sqrtf and division
    // (~25 instructions per element between the LDS sum and the Wt / p_new stores): 2 ulp of an
    // update of ~lr, far below half an ulp of p
    return p - c.lr * s0 * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(s1) * c.rbc2 + c.h2);
  }
}

// EMA: 1 - d_t of the step applied, and the new shadow value of one element.  The branch on the
// num_updates flag is wave-uniform (a kernel argument): without it no step word is read and the
// division's div_scale / fma / fixup sequence does not run.
__device__ __forceinline__ float ema_omd(const EmaOptArgs& oa) {
  if (!oa.nu) return oa.omd;
  const float t = (float)(oa.tp[oa.par] + 1);
  return fmaxf(oa.omd, 9.f / (10.f + t));
}
__device__ __forceinline__ float ema_update(float e, float v, float om) {
  return e - om * (e - v);
}
// the owning lane's shadow values (float4: the W1 item; float[4]: the small parameters) and the
// wave's 1 - d_t -- an empty type without EMA, so the other instantiations declare nothing
template <bool EMA, class V = float[4]>
struct EmaRegs {};
template <class V>
struct EmaRegs<true, V> {
  V e;
  float om;
};

// The all-reduce engine's rate (FusedMLPTrainer._apply_reduced): one wave writes lr(s) of the
// pending step -- s = ctr - 1: the step that produced the gradient has advanced the counter --
// into a device float that ops.optim's lr_tensor reads, and into the rate ring (lrs may be null).
__global__ __launch_bounds__(64) void mlp_lr_sched_kernel(const int* __restrict__ ctr,
                                                          const int* __restrict__ blk, float lr0,
                                                          float* __restrict__ out,
                                                          float* __restrict__ lrs, int ring) {
  const int s = *ctr - 1;
  const float rate = sched_rate(lr0, s, sched_load(blk));
  if (threadIdx.x == 0) {
    *out = rate;
    if (lrs && s >= 0) lrs[s % ring] = rate;
  }
}

}  // namespace mlp
}  // namespace dtfx
