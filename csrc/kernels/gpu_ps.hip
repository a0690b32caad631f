// Kernels of the GPU-resident parameter store (async-PS mode with the variables in GPU memory;
// SURVEY.md §2.4 (2), the "GPU-PS variant" of the reference's ps task, main.py:66-70, whose
// variables TF's replica_device_setter places on /job:ps, worker.py:24-32).
//
// The store is ONE uncached (MTYPE UC) allocation on the owning GPU: the flat f32 parameters
// followed by a control block of 64-bit words (global_step, initialised flag).  Workers on
// other GPUs map it over IPC, so every access below is a direct xGMI read / write of the
// owner's HBM; workers on the owner's GPU access it locally.  UC accesses bypass every GPU
// cache: a pull always sees the latest applied values, an apply lands in memory without any
// cache write-back, and no fence is needed between processes.
//
//   gps_pull_kernel   local replica <- store              (worker.py:81-85 sync_op)
//   gps_apply_kernel  store -= lr * local gradient        (worker.py:79 ApplyGradientDescent:
//                     use_locking=False -> plain read-modify-write, lock-free / Hogwild like
//                     TF's default; use_locking=True -> one f32 atomic add per element)
//   gps_apply_opt_kernel  --optimizer momentum | adam: the same lock-free read-modify-write
//                     over the parameters AND the optimizer's slot planes (accum, or m and v),
//                     which live in the store's allocation behind everything else
//   gps_fetch_add     store.global_step += delta, old value returned (worker.py:32,141)
//   gps_sync_join / gps_sync_push   --sync_replicas: ticket of the open round, gradient into the
//                     ticket's slot; the R-th arrival of a chunk applies the mean (below)
#include "common.h"
#include "gpu_ps.h"

#include <stdexcept>

namespace dtfx {
namespace gps {

__global__ __launch_bounds__(256) void gps_pull_kernel(float* __restrict__ dst,
                                                       const float* __restrict__ src,
                                                       long long n) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 3 < n) {
    *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
  } else {
    for (long long k = i; k < n; ++k) dst[k] = src[k];
  }
}

template <bool LOCKING>
__global__ __launch_bounds__(256) void gps_apply_kernel(float* __restrict__ p,
                                                        const float* __restrict__ g, float lr,
                                                        long long n) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (LOCKING) {
    for (long long k = i; k < i + 4 && k < n; ++k)
      __hip_atomic_fetch_add(p + k, -lr * g[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  } else if (i + 3 < n) {
    const float4 gv = *reinterpret_cast<const float4*>(g + i);
    float4 pv = *reinterpret_cast<const float4*>(p + i);
    pv.x -= lr * gv.x;
    pv.y -= lr * gv.y;
    pv.z -= lr * gv.z;
    pv.w -= lr * gv.w;
    *reinterpret_cast<float4*>(p + i) = pv;
  } else {
    for (long long k = i; k < n; ++k) p[k] -= lr * g[k];
  }
}

// ---------------------------------------------------------------------------------------------
// Stateful optimizers (--optimizer momentum | adam): ops/optim.py's formulas (optim.hip's
// momentum_kernel / adam_kernel) on the store's planes.  The store applies them with weight_decay
// = 0 and without Nesterov: those terms exist in the fused MLP trainer's first launch
// (mlp_step_opt.h, the WD family) and ps_async refuses --weight_decay / --nesterov.
//   momentum  accum = mu * accum + g;  p -= lr * accum                        slot0 = accum
//   adam      m = b1 * m + (1 - b1) * g;  v = b2 * v + (1 - b2) * g * g       slot0 = m, slot1 = v
//             p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// t is not stored: it is global_step + 1 at apply time (a sync round's closer has the round in
// its decision word; an async block reads the step word once at entry), so a restored
// global_step restores t.  Under concurrent async workers t is whatever the block read, like
// every other value in a Hogwild apply.
enum : int { GPS_SGD = 0, GPS_MOMENTUM = 1, GPS_ADAM = 2 };

// momentum: lr, h0 = mu.  adam: lr = lr / (1 - b1^t), h0 = b1, h1 = b2, h2 = eps,
// rbc2 = 1 / sqrt(1 - b2^t)
struct GpsCoef {
  float lr, h0, h1, h2, rbc2;
};

template <int OPT>
__device__ __forceinline__ GpsCoef gps_coef(float lr, float h0, float h1, float h2,
                                            unsigned long long t) {
  GpsCoef c = {lr, h0, h1, h2, 1.f};
  if (OPT == GPS_ADAM) {
    const float tf = (float)t;
    c.lr = lr / (1.f - powf(h0, tf));
    c.rbc2 = rsqrtf(1.f - powf(h1, tf));
  }
  return c;
}

template <int OPT>
__device__ __forceinline__ void gps_update(float& p, float g, float& s0, float& s1,
                                           const GpsCoef& c) {
  if (OPT == GPS_MOMENTUM) {
    s0 = c.h0 * s0 + g;
    p -= c.lr * s0;
  } else {
    s0 = c.h0 * s0 + (1.f - c.h0) * g;
    s1 = c.h1 * s1 + (1.f - c.h1) * g * g;
    p -= c.lr * s0 / (sqrtf(s1) * c.rbc2 + c.h2);
  }
}

// One optimizer step over elements [i, i + 4) (float4) or the scalar tail [i, n) of a chunk:
// parameters and slot planes read, updated and stored.  `grad(k)` is element k's gradient.
template <int OPT, class Grad4, class Grad1>
__device__ __forceinline__ void gps_step_chunk(float* __restrict__ p, float* __restrict__ s0,
                                               float* __restrict__ s1, long long i, long long n,
                                               const GpsCoef& c, Grad4 grad4, Grad1 grad1) {
  if (i + 3 < n) {
    const float4 gv = grad4(i);
    float4 pv = *reinterpret_cast<const float4*>(p + i);
    float4 av = *reinterpret_cast<const float4*>(s0 + i);
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (OPT == GPS_ADAM) bv = *reinterpret_cast<const float4*>(s1 + i);
    gps_update<OPT>(pv.x, gv.x, av.x, bv.x, c);
    gps_update<OPT>(pv.y, gv.y, av.y, bv.y, c);
    gps_update<OPT>(pv.z, gv.z, av.z, bv.z, c);
    gps_update<OPT>(pv.w, gv.w, av.w, bv.w, c);
    *reinterpret_cast<float4*>(s0 + i) = av;
    if (OPT == GPS_ADAM) *reinterpret_cast<float4*>(s1 + i) = bv;
    *reinterpret_cast<float4*>(p + i) = pv;
  } else {
    for (long long k = i; k < n; ++k) {
      float pp = p[k], a = s0[k], b = 0.f;
      if (OPT == GPS_ADAM) b = s1[k];
      gps_update<OPT>(pp, grad1(k), a, b, c);
      s0[k] = a;
      if (OPT == GPS_ADAM) s1[k] = b;
      p[k] = pp;
    }
  }
}

// Async (Hogwild) apply of a stateful optimizer: gps_apply_kernel<false>'s shape with the slot
// planes next to the parameters.  The store is uncached memory, so p, s0 and s1 are read and
// written in HBM directly; g is the worker's own gradient.
template <int OPT>
__global__ __launch_bounds__(256) void gps_apply_opt_kernel(
    float* __restrict__ p, float* __restrict__ s0, float* __restrict__ s1,
    const float* __restrict__ g, const unsigned long long* step_word, float lr, float h0,
    float h1, float h2, long long n) {
  unsigned long long t = 1;
  if (OPT == GPS_ADAM)  // read once per block, at entry
    t = __hip_atomic_load(step_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + 1;
  const GpsCoef c = gps_coef<OPT>(lr, h0, h1, h2, t);
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  gps_step_chunk<OPT>(
      p, s0, s1, i, n, c, [&](long long k) { return *reinterpret_cast<const float4*>(g + k); },
      [&](long long k) { return g[k]; });
}

// out[0] = old counter value; out[1 ..] = `nextra` f32 words copied from `extra` (the
// worker's loss / accuracy record of the step), so one read-back serves both
__global__ void gps_fetch_add_kernel(unsigned long long* ctr, long long delta,
                                     unsigned long long* out, const float* extra, int nextra) {
  if (threadIdx.x == 0)
    *out = __hip_atomic_fetch_add(ctr, (unsigned long long)delta, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_SYSTEM);
  if ((int)threadIdx.x < nextra)
    reinterpret_cast<float*>(out + 1)[threadIdx.x] = extra[threadIdx.x];
}

// ---------------------------------------------------------------------------------------------
// Synchronous replicas (tf.train.SyncReplicasOptimizer on the store): a push is the two launches
// below, back to back on the worker's stream.  No kernel waits on another process: both run to
// completion, and the wait for the round to close is a host poll of the round word
// (parallel/gpu_ps_sync.py).  Sums are slab sums in ticket order (no float atomics), so a round
// is bitwise reproducible for a given arrival order.
//
// Sync control region (after the control block; layout in gpu_ps.cpp):
//   u64 round word  (round << 32) | tickets_taken      u32 chunks_done      u32 R
//   u32 arrivals[ceil(n / 1024)]
// followed by R gradient slots of n f32 each, then the optimizer's slot planes (0, 1 or 2).

enum : unsigned { GPS_JOINED = 0, GPS_STALE = 1, GPS_AHEAD = 2, GPS_LATE = 3, GPS_CONTENDED = 4 };
constexpr int kJoinRetries = 1 << 16;

// One thread.  dec[0] = status, dec[1] = ticket, dec[2] = round seen, dec[3] = tickets seen;
// dec[4 ..] = `nextra` f32 words copied from `extra` (the step's loss / accuracy record), so
// one read-back serves both.  The loop retries only when another worker's CAS won the word in
// between (at most R - 1 times per round in a correct run); the bound ends it regardless.
__global__ void gps_sync_join_kernel(unsigned long long* round_word, unsigned local_step,
                                     unsigned R, unsigned* dec, const float* extra, int nextra) {
  if (threadIdx.x == 0) {
    unsigned long long w =
        __hip_atomic_load(round_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    unsigned status = GPS_CONTENDED;
    for (int it = 0; it < kJoinRetries; ++it) {
      const unsigned round = (unsigned)(w >> 32), taken = (unsigned)w;
      if (local_step < round) {
        status = GPS_STALE;
        break;
      }
      if (local_step > round) {
        status = GPS_AHEAD;
        break;
      }
      if (taken >= R) {
        status = GPS_LATE;
        break;
      }
      // on failure `w` is reloaded with the word's current value
      if (__hip_atomic_compare_exchange_strong(round_word, &w, w + 1, __ATOMIC_RELAXED,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) {
        status = GPS_JOINED;
        break;
      }
    }
    dec[0] = status;
    dec[1] = (unsigned)w;  // JOINED: the ticket (the count before this worker's increment)
    dec[2] = (unsigned)(w >> 32);
    dec[3] = (unsigned)w;
  }
  if ((int)threadIdx.x < nextra) reinterpret_cast<float*>(dec + 4)[threadIdx.x] = extra[threadIdx.x];
}

// Why a worker of round r+1 never meets state of round r.  It can only JOIN after the round
// word reads r+1, and that word is published last, by the one block that completed the last
// chunk of round r, behind a system-scope release.  Before it, in program order of that block:
// its own chunk's slot reads (their values fed the parameter stores it drained with vmcnt(0)),
// its counter reset and its chunks_done add.  Every other chunk's closer drained its parameter
// stores, reset its arrival counter and released BEFORE its chunks_done add, and the finishing
// block acquires after drawing the last chunks_done ticket.  So every slot read, every
// parameter store, every counter reset and the global_step store of round r happen-before the
// round word r+1, hence before any ticket, slot store or counter add of round r+1 -- and
// before any pull a worker issues after its host poll saw r+1.  Within a round, a slot is
// written by exactly one ticket holder, and the closer of a chunk reads the R slots only after
// drawing arrival R-1 (each arrival is behind its writer's drain + release) and acquiring.
// There is no loop on memory another kernel writes anywhere in this kernel.
//
// The optimizer's slot planes (OPT = momentum: accum; adam: m, v) are read and written ONLY by a
// chunk's closer, over that chunk's elements, and every such store is issued before the same
// vmcnt(0) drain, counter reset and release that cover the parameter stores.  So the argument
// above holds for them word for word: the slot-plane stores of round r happen-before the round
// word r+1, hence before the closer of the same chunk in round r+1 reads them.  OPT = sgd is
// the arithmetic p -= (lr / R) * s it always was; the others form gbar = s * (1 / R) (1 / R
// rounded to f32 on the host) and run the optimizer on gbar with t = round + 1.
template <int OPT>
__global__ __launch_bounds__(256) void gps_sync_push_kernel(
    float* p, float* slots, long long slot_stride, const float* __restrict__ g,
    const unsigned* __restrict__ dec, unsigned* arrivals,
    unsigned* chunks_done, unsigned long long* round_word, unsigned long long* step_word,
    float scale, unsigned R, long long n, unsigned nchunks, float* opt0, float* opt1, float lr,
    float h0, float h1, float h2) {
  __shared__ unsigned last_s;  // the one LDS word: "this block closes its chunk"
  if (dec[0] != GPS_JOINED) return;  // STALE / AHEAD / LATE / CONTENDED: touch nothing
  const unsigned t = dec[1], round = dec[2];
  if (t >= R) return;
  // the optimizer's per-step scalars depend on the decision word alone: formed here, ahead of
  // the chain of memory round trips below, by every block (only a closer uses them)
  const GpsCoef c = gps_coef<OPT>(lr, h0, h1, h2, (unsigned long long)round + 1);
  const unsigned chunk = blockIdx.x;
  const long long i = ((long long)chunk * 256 + threadIdx.x) * 4;
  float* slot = slots + (long long)t * slot_stride;
  if (i + 3 < n) {
    *reinterpret_cast<float4*>(slot + i) = *reinterpret_cast<const float4*>(g + i);
  } else {
    for (long long k = i; k < n; ++k) slot[k] = g[k];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope; fence BEFORE the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned a = __hip_atomic_fetch_add(arrivals + chunk, 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_SYSTEM);
    last_s = (a == R - 1);
    if (a == R - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last_s) return;

  // the R-th arrival of this chunk: s = ((slot0 + slot1) + ...) in ticket order, one apply
  if (OPT != GPS_SGD) {  // `scale` is 1 / R here: the optimizer runs on the mean gradient
    gps_step_chunk<OPT>(
        p, opt0, opt1, i, n, c,
        [&](long long e) {
          float4 s = *reinterpret_cast<const float4*>(slots + e);
          for (unsigned k = 1; k < R; ++k) {
            const float4 v =
                *reinterpret_cast<const float4*>(slots + (long long)k * slot_stride + e);
            s.x += v.x;
            s.y += v.y;
            s.z += v.z;
            s.w += v.w;
          }
          return make_float4(s.x * scale, s.y * scale, s.z * scale, s.w * scale);
        },
        [&](long long e) {
          float s = slots[e];
          for (unsigned r = 1; r < R; ++r) s += slots[(long long)r * slot_stride + e];
          return s * scale;
        });
  } else if (i + 3 < n) {
    float4 s = *reinterpret_cast<const float4*>(slots + i);
    for (unsigned k = 1; k < R; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(slots + (long long)k * slot_stride + i);
      s.x += v.x;
      s.y += v.y;
      s.z += v.z;
      s.w += v.w;
    }
    float4 pv = *reinterpret_cast<const float4*>(p + i);
    pv.x -= scale * s.x;
    pv.y -= scale * s.y;
    pv.z -= scale * s.z;
    pv.w -= scale * s.w;
    *reinterpret_cast<float4*>(p + i) = pv;
  } else {
    for (long long k = i; k < n; ++k) {
      float s = slots[k];
      for (unsigned r = 1; r < R; ++r) s += slots[(long long)r * slot_stride + k];
      p[k] -= scale * s;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store(arrivals + chunk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned d = __hip_atomic_fetch_add(chunks_done, 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_SYSTEM);
    if (d == nchunks - 1) {  // the last chunk of the round: finish it
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
      __hip_atomic_store(chunks_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(step_word, (unsigned long long)round + 1, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(round_word, ((unsigned long long)round + 1) << 32, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace gps

void gps_sync_join_launch(unsigned long long* round_word, unsigned local_step, unsigned R,
                          unsigned* dec, const float* extra, int nextra, hipStream_t s) {
  if (nextra < 0 || nextra > 14) throw std::runtime_error("gpu_ps: at most 14 extra words");
  hipLaunchKernelGGL(gps::gps_sync_join_kernel, dim3(1), dim3(64), 0, s, round_word, local_step,
                     R, dec, extra, nextra);
  DTFX_HIP_CHECK(hipGetLastError());
}

void gps_sync_push_launch(float* p, float* slots, long long slot_stride, const float* g,
                          const unsigned* dec, unsigned* arrivals, unsigned* chunks_done,
                          unsigned long long* round_word, unsigned long long* step_word, float lr,
                          unsigned R, long long n, int opt, float* opt0, float* opt1, float h0,
                          float h1, float h2, hipStream_t s) {
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) |
       reinterpret_cast<uintptr_t>(slots) | reinterpret_cast<uintptr_t>(opt0) |
       reinterpret_cast<uintptr_t>(opt1)) & 15 || (slot_stride & 3))
    throw std::runtime_error("gpu_ps: buffers must be 16-byte aligned");
  if (R < 1 || slot_stride < n) throw std::runtime_error("gpu_ps: bad sync slot layout");
  if (opt < gps::GPS_SGD || opt > gps::GPS_ADAM || (opt >= gps::GPS_MOMENTUM && !opt0) ||
      (opt == gps::GPS_ADAM && !opt1))
    throw std::runtime_error("gpu_ps: bad optimizer kind / slot planes");
  const long long blocks = (n + 1023) / 1024;
  const dim3 grid((unsigned)blocks), block(256);
  // sgd: p -= (lr / R) * s.  Otherwise the closer scales s by 1 / R, rounded to f32 here, once
  const float scale = opt == gps::GPS_SGD ? lr / (float)R : 1.f / (float)R;
#define GPS_SYNC_PUSH(OPT)                                                                      \
  hipLaunchKernelGGL(gps::gps_sync_push_kernel<OPT>, grid, block, 0, s, p, slots, slot_stride,  \
                     g, dec, arrivals, chunks_done, round_word, step_word, scale, R, n,         \
                     (unsigned)blocks, opt0, opt1, lr, h0, h1, h2)
  if (opt == gps::GPS_SGD) GPS_SYNC_PUSH(gps::GPS_SGD);
  else if (opt == gps::GPS_MOMENTUM) GPS_SYNC_PUSH(gps::GPS_MOMENTUM);
  else GPS_SYNC_PUSH(gps::GPS_ADAM);
#undef GPS_SYNC_PUSH
  DTFX_HIP_CHECK(hipGetLastError());
}

// async apply of a stateful optimizer: opt = 1 momentum (h0 = mu), 2 adam (h0 = b1, h1 = b2,
// h2 = eps); s0 / s1 the slot planes
void gps_apply_opt_launch(float* p, float* s0, float* s1, const float* g,
                          const unsigned long long* step_word, float lr, int opt, float h0,
                          float h1, float h2, long long n, hipStream_t s) {
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) |
       reinterpret_cast<uintptr_t>(s0) | reinterpret_cast<uintptr_t>(s1)) & 15)
    throw std::runtime_error("gpu_ps: buffers must be 16-byte aligned");
  if ((opt != gps::GPS_MOMENTUM && opt != gps::GPS_ADAM) || !s0 || (opt == gps::GPS_ADAM && !s1))
    throw std::runtime_error("gpu_ps: bad optimizer kind / slot planes");
  const long long blocks = (n + 1023) / 1024;
  if (opt == gps::GPS_MOMENTUM)
    hipLaunchKernelGGL(gps::gps_apply_opt_kernel<gps::GPS_MOMENTUM>, dim3((unsigned)blocks),
                       dim3(256), 0, s, p, s0, s1, g, step_word, lr, h0, h1, h2, n);
  else
    hipLaunchKernelGGL(gps::gps_apply_opt_kernel<gps::GPS_ADAM>, dim3((unsigned)blocks),
                       dim3(256), 0, s, p, s0, s1, g, step_word, lr, h0, h1, h2, n);
  DTFX_HIP_CHECK(hipGetLastError());
}

void gps_pull_launch(float* dst, const float* src, long long n, hipStream_t s) {
  if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15)
    throw std::runtime_error("gpu_ps: buffers must be 16-byte aligned");
  const long long blocks = (n + 1023) / 1024;
  hipLaunchKernelGGL(gps::gps_pull_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dst, src, n);
  DTFX_HIP_CHECK(hipGetLastError());
}

void gps_apply_launch(float* p, const float* g, float lr, long long n, bool locking,
                      hipStream_t s) {
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g)) & 15)
    throw std::runtime_error("gpu_ps: buffers must be 16-byte aligned");
  const long long blocks = (n + 1023) / 1024;
  if (locking)
    hipLaunchKernelGGL(gps::gps_apply_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, p, g,
                       lr, n);
  else
    hipLaunchKernelGGL(gps::gps_apply_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, p,
                       g, lr, n);
  DTFX_HIP_CHECK(hipGetLastError());
}

void gps_fetch_add_launch(unsigned long long* ctr, long long delta, unsigned long long* out,
                          const float* extra, int nextra, hipStream_t s) {
  if (nextra < 0 || nextra > 14) throw std::runtime_error("gpu_ps: at most 14 extra words");
  hipLaunchKernelGGL(gps::gps_fetch_add_kernel, dim3(1), dim3(64), 0, s, ctr, delta, out, extra,
                     nextra);
  DTFX_HIP_CHECK(hipGetLastError());
}

}  // namespace dtfx
