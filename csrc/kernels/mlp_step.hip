// Fused training step for the reference's MNIST MLP (784 -> 100 sigmoid -> 10,
// softmax cross-entropy, plain SGD).  Reference graph: worker.py:46-79.
//
// One translation unit, split by engine (every kernel of the step is compiled from this file and
// with this file's flags; each header opens with what was measured for its engine, kept or not):
//   mlp_model.h          sizes, flat parameter layout (shared with mlp_persistent / mlp_eval)
//   mlp_step_ws.h        K slicing, workspace layout (Bufs / ws_layout), the MFMA operand layout
//   mlp_step_xg.h        xGMI exchange engines: xg_exchange*, head_allgather
//   mlp_step_opt.h       momentum / Adam / learning-rate schedules / weight decay and Nesterov:
//                        OptArgs, sched_rate, opt_update
//   mlp_step_3launch.h   the three-launch step: mlp_fwd, head_row / mlp_head, wgrad_small / mlp_wgrad
//   mlp_step_fwdapply.h  the two-launch step: fwdapply_block, lean entry points, the fused flush
//   mlp_step_factor.h    the factor engines: mlp_fwdapply_factor / mlp_wgrad_factor
//   mlp_step_api.h       every host function this file exports (bindings.cpp, xgmi_comm.cpp)
// Below: the TF-layout and test kernels, the host launchers, the parameter-server worker step.
//
// Batch selection: every launch takes the batch's own x / label pointer.  A
// captured hipGraph therefore freezes one batch per captured step; the
// trainer captures a whole epoch (one graph = nbatches steps), so replaying
// it walks the device-resident dataset exactly like next_batch does.  No
// kernel starts with a dependent "which batch?" load (measured: ~0.5 us per
// dependent round trip on this chip).
#include "mlp_step_api.h"
#include "mlp_step_factor.h"
#include "mlp_step_fwdapply.h"

#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace dtfx {

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
static mlp::Bufs make_bufs(float* ws, int B) {
  return mlp::ws_bufs(ws, ((B + 15) / 16) * 16);
}

// Compile-time dispatch of the launchers: f is a generic lambda that takes the chosen value as a
// std::integral_constant (`auto NGT` -> `kernel<.., NGT()>`), so every launch line is written
// once.  Inlined: no std::function, no allocation, and no string before a throw.
//   with_ngt: NGT = 7 for the batches of 7 row tiles (97..112 rows: loads without guards), else
//     0, the generic instantiation.
template <class F>
static inline void with_ngt(int B, F&& f) {
  if ((B + 15) / 16 == 7) f(std::integral_constant<int, 7>{});
  else f(std::integral_constant<int, 0>{});
}
//   with_flag: a run-time flag as std::true_type / std::false_type.
template <class F>
static inline void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}
//   with_const<Vs...>: v as the one of Vs it equals; anything else throws `msg`.
template <int... Vs, class F>
static inline void with_const(int v, const char* msg, F&& f) {
  const bool hit = ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  if (!hit) throw std::runtime_error(msg);
}
//   with_world: the data-parallel engines' world size, 2..8.
template <class F>
static inline void with_world(int world, const char* msg, F&& f) {
  with_const<2, 3, 4, 5, 6, 7, 8>(world, msg, f);
}

// TF checkpoint layout <-> the kernels' flat layout of the MLP parameters / gradients (the
// async-PS wire format is TF's: worker.py:27-31 kernels [in, out]).  The four segments sit at
// the same offsets in both (78400 | 100 | 1000 | 10); only the kernels are transposed.
// to_tf = 1: flat -> TF (+ `extra` floats copied from `xsrc` after NPARAM: the step's loss /
// accuracy record rides along in the same D2H copy); 0: TF -> flat.
__global__ __launch_bounds__(256) void mlp_tf_layout_kernel(const float* __restrict__ src,
                                                            float* __restrict__ dst, int to_tf,
                                                            const float* __restrict__ xsrc,
                                                            int extra) {
  using namespace mlp;
  const int i = blockIdx.x * 256 + threadIdx.x;  // destination index
  if (i < NPARAM) {
    int j = i;  // source index
    if (i < OFF_B1) {  // W1: TF [784][100] <-> flat [100][784]
      j = to_tf ? (i % H) * D + i / H : (i % D) * H + i / D;
    } else if (i >= OFF_W2 && i < OFF_B2) {  // W2: TF [100][10] <-> flat [10][100]
      const int k = i - OFF_W2;
      j = OFF_W2 + (to_tf ? (k % C) * H + k / C : (k % H) * C + k / H);
    }
    dst[i] = src[j];
  } else if (to_tf && i < NPARAM + extra) {
    dst[i] = xsrc[i - NPARAM];
  }
}

// TF layout -> flat layout iterating over the SOURCE (TF) index: consecutive threads read
// consecutive words (the source may be host memory read over the host link, where the
// destination-major walk of mlp_tf_layout_kernel would issue 4-byte reads 400 bytes apart)
// and scatter into device memory.
__global__ __launch_bounds__(256) void mlp_from_tf_src_major_kernel(const float* __restrict__ src,
                                                                    float* __restrict__ dst) {
  using namespace mlp;
  const int k = blockIdx.x * 256 + threadIdx.x;  // source (TF) index
  if (k >= NPARAM) return;
  int i = k;  // destination (flat) index
  if (k < OFF_B1) {  // TF W1 [784][100] -> flat W1t [100][784]
    i = (k % H) * D + k / H;
  } else if (k >= OFF_W2 && k < OFF_B2) {  // TF W2 [100][10] -> flat W2t [10][100]
    const int m = k - OFF_W2;
    i = OFF_W2 + (m % C) * H + m / C;
  }
  dst[i] = src[k];
}

void mlp_tf_layout_launch(const float* src, float* dst, int to_tf, const float* xsrc, int extra,
                          hipStream_t stream) {
  using namespace mlp;
  if (extra < 0 || extra > 64 || (extra && !xsrc))
    throw std::runtime_error("mlp_tf_layout: 0..64 extra floats with a source");
  const int n = NPARAM + (to_tf ? extra : 0);
  hipLaunchKernelGGL(mlp_tf_layout_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, src, dst,
                     to_tf, xsrc, to_tf ? extra : 0);
  DTFX_HIP_CHECK(hipGetLastError());
}

long long mlp_workspace_floats(int B) {
  using namespace mlp;
  return ws_layout(((B + 15) / 16) * 16).total;
}

static void check_b(int B) {
  if (B < 1 || B > mlp::MAXB) throw std::runtime_error("fused MLP step: batch must be in [1, 256]");
}

// Test kernel of wave_reduce_scatter (common.h): one wave, in [64][N] -> out [64]
// (out[l] = the value lane l holds: the sum over all lanes of value l & 15).
template <int N>
__global__ __launch_bounds__(64) void wave_reduce_scatter_test_kernel(
    const float* __restrict__ in, float* __restrict__ out) {
  const int lane = threadIdx.x;
  float v[N];
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = in[lane * N + i];
  out[lane] = wave_reduce_scatter(v, lane);
}

void wave_reduce_scatter_test_launch(const float* in, float* out, int n, hipStream_t stream) {
  with_const<10, 16>(n, "wave_reduce_scatter_test: n must be 10 or 16", [&](auto N) {
    hipLaunchKernelGGL((wave_reduce_scatter_test_kernel<N()>), dim3(1), dim3(64), 0, stream, in,
                       out);
  });
  DTFX_HIP_CHECK(hipGetLastError());
}

// Float offsets of the row-major factor regions in a workspace of batch B: out = {dz1R, dlR,
// BP}.  The sync words are the 4 floats before dz1R (where StepWorkspace.buf ends).
void mlp_rowmajor_layout(int B, long long* out) {
  check_b(B);
  float* const base = reinterpret_cast<float*>(uintptr_t(1) << 32);  // (never dereferenced)
  const mlp::Bufs b = make_bufs(base, B);
  out[0] = b.dz1R - base;
  out[1] = b.dlR - base;
  out[2] = ((B + 15) / 16) * 16;
  if (reinterpret_cast<float*>(b.sync) + 4 != b.dz1R ||
      b.dlR + 16 * out[2] - base != mlp_workspace_floats(B))
    throw std::runtime_error("mlp_rowmajor_layout: workspace size out of step with its layout");
}

// K1: grad != nullptr => deferred apply (p_new must differ from p_old)
void mlp_fwd_launch(const float* p_old, const float* grad, float lr, float* p_new, const float* x,
                    float* ws, int B, hipStream_t stream, unsigned long long* tr) {
  using namespace mlp;
  check_b(B);
  const Bufs w = make_bufs(ws, B);
  const int RT = (B + 15) / 16;
  dim3 grid(RT * HT * KS), block(64);
  if (grad && (!p_new || p_new == p_old))
    throw std::runtime_error("mlp_fwd: apply needs ping-pong p_new");
  auto launch = [&](auto APPLY, auto TRACE) {  // (no apply: grad = p_old, lr = 0, no p_new)
    hipLaunchKernelGGL((mlp_fwd_kernel<APPLY(), TRACE()>), grid, block, 0, stream, p_old,
                       APPLY() ? grad : p_old, APPLY() ? lr : 0.f, APPLY() ? p_new : nullptr, x, w,
                       B, tr);
  };
  if (grad) launch(std::true_type{}, std::false_type{});
  else with_flag(tr != nullptr, [&](auto TRACE) { launch(std::false_type{}, TRACE); });
  DTFX_HIP_CHECK(hipGetLastError());
}

// Dropout (MlpDrop, mlp_step_api.h): the head's DROP instantiations.  thr in [1, 2^24] (ops/
// dropout.py: threshold()); the step word is read from drop->ctr by the kernel.
static void check_drop(const MlpDrop& d, const char* who) {
  const char* bad = nullptr;
  if (!d.ctr) bad = ": dropout needs the global_step counter";
  else if (d.thr < 1u || d.thr > (1u << 24)) bad = ": dropout threshold must be in [1, 2^24]";
  if (bad) throw std::runtime_error(std::string(who) + bad);
}

// The hidden activation (common.h: HACT_*; ops/hidden_act.py) as a compile-time constant; an id
// outside the set throws.  The heads' relu / tanh instantiations are the plain and the dropout
// form of the lean head and of the three-launch head: nothing else has a variant.
template <class F>
static inline void with_act(int act, const char* who, F&& f) {
  if (act == HACT_SIGMOID) f(std::integral_constant<int, HACT_SIGMOID>{});
  else if (act == HACT_RELU) f(std::integral_constant<int, HACT_RELU>{});
  else if (act == HACT_TANH) f(std::integral_constant<int, HACT_TANH>{});
  else
    throw std::runtime_error(std::string(who) + ": unknown hidden activation id " +
                             std::to_string(act) + " (0 sigmoid, 1 relu, 2 tanh)");
}
static void check_act(int act, const char* who) { with_act(act, who, [](auto) {}); }

void mlp_head_launch(const float* p_old, const float* grad, float lr, float* p_new,
                     const int* labels, float* ws, int B, hipStream_t stream,
                     unsigned long long* tr, const MlpDrop* drop, int act) {
  using namespace mlp;
  check_b(B);
  const Bufs w = make_bufs(ws, B);
  if (grad && (!p_new || p_new == p_old))
    throw std::runtime_error("mlp_head: apply needs ping-pong p_new");
  if (drop) {
    check_drop(*drop, "mlp_head");
    if (tr) throw std::runtime_error("mlp_head: the trace launch has no dropout variant");
    with_act(act, "mlp_head", [&](auto ACT) {
      with_flag(grad != nullptr, [&](auto APPLY) {
        hipLaunchKernelGGL((mlp_head_drop_kernel<APPLY(), ACT()>), dim3(B), dim3(64), 0, stream,
                           p_old, APPLY() ? grad : p_old, APPLY() ? lr : 0.f,
                           APPLY() ? p_new : nullptr, labels, w, B, drop->ctr, drop->k0, drop->k1,
                           drop->thr, drop->stream, drop->scale);
      });
    });
    DTFX_HIP_CHECK(hipGetLastError());
    return;
  }
  if (act != HACT_SIGMOID) {
    if (tr) throw std::runtime_error("mlp_head: the trace launch has no relu / tanh variant");
    with_act(act, "mlp_head", [&](auto ACT) {
      with_flag(grad != nullptr, [&](auto APPLY) {
        hipLaunchKernelGGL((mlp_head_kernel<APPLY(), false, 0, KS, false, ACT()>), dim3(B),
                           dim3(64), 0, stream, p_old, APPLY() ? grad : p_old,
                           APPLY() ? lr : 0.f, APPLY() ? p_new : nullptr, labels, w, B, nullptr,
                           MlpXg{}, nullptr);
      });
    });
    DTFX_HIP_CHECK(hipGetLastError());
    return;
  }
  auto launch = [&](auto APPLY, auto TRACE) {  // (no apply: grad = p_old, lr = 0, no p_new)
    hipLaunchKernelGGL((mlp_head_kernel<APPLY(), TRACE()>), dim3(B), dim3(64), 0, stream, p_old,
                       APPLY() ? grad : p_old, APPLY() ? lr : 0.f, APPLY() ? p_new : nullptr,
                       labels, w, B, tr, MlpXg{}, nullptr);
  };
  if (grad) launch(std::true_type{}, std::false_type{});
  else with_flag(tr != nullptr, [&](auto TRACE) { launch(std::false_type{}, TRACE); });
  DTFX_HIP_CHECK(hipGetLastError());
}

// K3: grad == nullptr => direct mode (p -= lr * g fused); else writes grad
void mlp_wgrad_launch(float* p, float lr, float* grad, const float* x, float* ws, int* ctr,
                      float* stats, int stats_ring, int B, hipStream_t stream,
                      unsigned long long* tr) {
  using namespace mlp;
  check_b(B);
  if (stats && stats_ring < 1) throw std::runtime_error("mlp_wgrad: stats_ring < 1");
  if (!ctr) throw std::runtime_error("mlp_wgrad: needs the global_step counter");
  const Bufs w = make_bufs(ws, B);
  dim3 grid(HT * ((FT + 3) / 4) + HT), block(256);
  if (!grad && !p) throw std::runtime_error("mlp_wgrad: direct mode needs parameters");
  const MlpXg noxg{};
  with_ngt(B, [&](auto NGT) {
    auto launch = [&](auto DIR, auto TR) {
      hipLaunchKernelGGL((mlp_wgrad_kernel<DIR(), TR(), NGT()>), grid, block, 0, stream, p,
                         DIR() ? lr : 0.f, DIR() ? nullptr : grad, x, w, ctr, stats, stats_ring, B,
                         tr, noxg);
    };
    if (grad) launch(std::false_type{}, std::false_type{});
    else with_flag(tr != nullptr, [&](auto TR) { launch(std::true_type{}, TR); });
  });
  DTFX_HIP_CHECK(hipGetLastError());
}

// K3 with the fused xGMI gradient exchange (direct apply with lr = lr / world).
void mlp_wgrad_xg_launch(float* p, float lr, const float* x, float* ws, int* ctr, float* stats,
                         int stats_ring, int B, hipStream_t stream, const MlpXg& xg, int world) {
  using namespace mlp;
  check_b(B);
  if (stats && stats_ring < 1) throw std::runtime_error("mlp_wgrad: stats_ring < 1");
  if (!ctr || !p) throw std::runtime_error("mlp_wgrad_xg: needs parameters and the step counter");
  if (xg.S < NPARAM) throw std::runtime_error("mlp_wgrad_xg: exchange slots smaller than the model");
  const Bufs w = make_bufs(ws, B);
  const int nblk = HT * ((FT + 3) / 4) + HT;
  if (nblk * 4 > MLP_XG_EPOCHS) throw std::runtime_error("mlp_wgrad_xg: epoch array too small");
  dim3 grid(nblk), block(256);
  with_world(world, "mlp_wgrad_xg: world must be 2..8", [&](auto WW) {
    with_ngt(B, [&](auto NGT) {
      hipLaunchKernelGGL((mlp_wgrad_kernel<true, false, NGT(), WW()>), grid, block, 0, stream, p,
                         lr, nullptr, x, w, ctr, stats, stats_ring, B, nullptr, xg);
    });
  });
  DTFX_HIP_CHECK(hipGetLastError());
}

// Factor engine launches (see mlp_wgrad_factor_kernel).
void mlp_head_xg_launch(const float* p, const int* labels, float* ws, float* dz1A, int B,
                        hipStream_t stream, const MlpXg& xg, int world, int nslab) {
  using namespace mlp;
  check_b(B);
  const char* bad_nslab = "mlp_head_xg: nslab must be 7 or 28";
  if (nslab != KS && nslab != KS3) throw std::runtime_error(bad_nslab);
  if (xg.S < (long long)HP * (((B + 15) / 16) * 16))
    throw std::runtime_error("mlp_head_xg: exchange slots smaller than the factor plane");
  const Bufs w = make_bufs(ws, B);
  with_world(world, "mlp_head_xg: world must be 2..8", [&](auto WW) {  // (no NGT split here)
    with_const<KS, KS3>(nslab, bad_nslab, [&](auto NSLAB) {
      hipLaunchKernelGGL((mlp_head_kernel<false, false, WW(), NSLAB()>), dim3(B), dim3(64), 0,
                         stream, p, p, 0.f, nullptr, labels, w, B, nullptr, xg, dz1A);
    });
  });
  DTFX_HIP_CHECK(hipGetLastError());
}

void mlp_wgrad_factor_launch(float* p, float lr, const float* x, long long xstride,
                             const float* dz1A, float* ws, int* ctr, float* stats, int stats_ring,
                             int B, hipStream_t stream, const MlpXg& xg, int world) {
  using namespace mlp;
  check_b(B);
  if (stats && stats_ring < 1) throw std::runtime_error("mlp_wgrad: stats_ring < 1");
  if (!ctr || !p || !dz1A) throw std::runtime_error("mlp_wgrad_factor: null buffer");
  if (xg.S < NPARAM) throw std::runtime_error("mlp_wgrad_factor: exchange slots smaller than the model");
  const Bufs w = make_bufs(ws, B);
  dim3 grid(8 * HT * ((FT + 7) / 8) + HT), block(256);
  with_world(world, "mlp_wgrad_factor: world must be 2..8", [&](auto WW) {
    with_ngt(B, [&](auto NGT) {
      hipLaunchKernelGGL((mlp_wgrad_factor_kernel<WW(), NGT()>), grid, block, 0, stream, p, lr, x,
                         xstride, dz1A, w, ctr, stats, stats_ring, B, xg);
    });
  });
  DTFX_HIP_CHECK(hipGetLastError());
}

// K slices of the single-GPU pipelined step (fwdapply + head agree on it): KS3 = 28, or
// DTFX_MLP_KS=14 for the layout of the data-parallel engines (A/B runs).
static int mlp_single_ks() {
  static const int ks = [] {
    const char* e = std::getenv("DTFX_MLP_KS");
    return e && std::atoi(e) == 14 ? 14 : 28;
  }();
  return ks;
}

// The lean pair (mlp_lean_fwdapply_kernel / mlp_lean_head_kernel): what step_pipelined, the
// graph capture, mlp_run_pipelined_launch and the flush run at the default K slicing.
static int lean_flags(int B, int stats_on, const float* stats, int stats_ring) {
  if (!stats) stats_ring = 1;
  if (stats_ring < 1 || stats_ring >= (1 << 21))
    throw std::runtime_error("fused MLP step: stats_ring must be in [1, 2^21)");
  return B | (stats_on ? 1 << 9 : 0) | stats_ring << 10;
}

template <bool FWD>
static void lean_first_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                              const float* x, float* ws, int* ctr, float* stats, int stats_ring,
                              int B, int stats_on, hipStream_t stream) {
  using namespace mlp;
  const int flags = lean_flags(B, stats_on, stats, stats_ring);
  // (fwdapply_block<.., A16>: W1 moves as float4s)
  if ((reinterpret_cast<uintptr_t>(p_old) | reinterpret_cast<uintptr_t>(p_new)) & 15)
    throw std::runtime_error("fused MLP step: parameter buffers must be 16-byte aligned");
  dim3 grid(HT * KS3 + HT), block(256);
  with_ngt(B, [&](auto NGT) {
    hipLaunchKernelGGL((mlp_lean_fwdapply_kernel<NGT(), FWD>), grid, block, 0, stream, p_old, p_new,
                       x_prev, x, ws, lr, flags, ctr, stats);
  });
}

static void lean_head_launch(const float* p, const int* labels, float* ws, int B,
                             hipStream_t stream, const MlpDrop* drop = nullptr,
                             int act = HACT_SIGMOID) {
  using namespace mlp;
  with_act(act, "mlp_lean_head", [&](auto ACT) {
    with_ngt(B, [&](auto NGT) {
      if (drop)
        hipLaunchKernelGGL((mlp_lean_head_drop_kernel<NGT(), ACT()>), dim3(B), dim3(64), 0, stream,
                           p, labels, ws, B, drop->ctr, drop->k0, drop->k1, drop->thr,
                           drop->stream, drop->scale);
      else
        hipLaunchKernelGGL((mlp_lean_head_kernel<NGT(), ACT()>), dim3(B), dim3(64), 0, stream, p,
                           labels, ws, B);
    });
  });
}

// The same two launches on the general kernels (no checks, as the lean pair above):
// mlp_fwdapply_kernel<NGT, 0, false, false, KSX, FWD> -- what mlp_fwdapply_launch, the
// DTFX_MLP_KS=14 step and the fused flush's last step run -- and mlp_head_kernel over NSLAB slabs
// (RM: row-major factors out).
template <int KSX, bool FWD = true>
static void fwdapply_single_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                                   const float* x, const mlp::Bufs& w, int* ctr, float* stats,
                                   int stats_ring, int B, int stats_on, hipStream_t stream) {
  using namespace mlp;
  with_ngt(B, [&](auto NGT) {
    hipLaunchKernelGGL((mlp_fwdapply_kernel<NGT(), 0, false, false, KSX, FWD>), dim3(HT * KSX + HT),
                       dim3(256), 0, stream, p_old, p_new, lr, x_prev, x, w, ctr, stats, stats_ring,
                       B, stats_on, MlpXg{}, nullptr);
  });
}

template <int NSLAB, bool RM = false>
static void head_plain_launch(const float* p, const int* labels, const mlp::Bufs& w, int B,
                              hipStream_t stream) {
  hipLaunchKernelGGL((mlp::mlp_head_kernel<false, false, 0, NSLAB, RM>), dim3(B), dim3(64), 0,
                     stream, p, p, 0.f, nullptr, labels, w, B, nullptr, MlpXg{}, nullptr);
}

// First launch of the single-GPU two-launch step: the lean kernel, or with DTFX_MLP_KS=14 the
// 14-slice mlp_fwdapply_kernel.
void mlp_lean_fwdapply_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                              const float* x, float* ws, int* ctr, float* stats, int stats_ring,
                              int B, int stats_on, hipStream_t stream) {
  if (mlp_single_ks() != mlp::KS3)
    return mlp_fwdapply_launch(p_old, p_new, lr, x_prev, x, ws, ctr, stats, stats_ring, B, stats_on,
                               stream, mlp::KS2);
  check_b(B);
  if (!p_old || !p_new || p_old == p_new || !x_prev || !x || !ctr || !ws)
    throw std::runtime_error(
        "mlp_lean_fwdapply: needs distinct ping-pong buffers, both batches, ctr");
  lean_first_launch<true>(p_old, p_new, lr, x_prev, x, ws, ctr, stats, stats_ring, B, stats_on,
                          stream);
  DTFX_HIP_CHECK(hipGetLastError());
}

// Its head (row-major factors out); DTFX_MLP_KS=14: mlp_head2_launch.
void mlp_lean_head_launch(const float* p, const int* labels, float* ws, int B,
                          hipStream_t stream, const MlpDrop* drop, int act) {
  if (drop) {
    check_drop(*drop, "mlp_lean_head");
    if (mlp_single_ks() != mlp::KS3)
      throw std::runtime_error("mlp_lean_head: DTFX_MLP_KS=14 has no dropout variant");
  }
  check_act(act, "mlp_lean_head");
  if (act != HACT_SIGMOID && mlp_single_ks() != mlp::KS3)
    throw std::runtime_error("mlp_lean_head: DTFX_MLP_KS=14 has no relu / tanh variant");
  if (mlp_single_ks() != mlp::KS3) return mlp_head2_launch(p, labels, ws, B, stream, mlp::KS2);
  check_b(B);
  if (!p || !labels || !ws) throw std::runtime_error("mlp_lean_head: null buffer");
  lean_head_launch(p, labels, ws, B, stream, drop, act);
  DTFX_HIP_CHECK(hipGetLastError());
}

// Pipelined single-GPU step (see mlp_fwdapply_kernel): K1' then the head over the K slabs.
void mlp_fwdapply_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                         const float* x, float* ws, int* ctr, float* stats, int stats_ring, int B,
                         int stats_on, hipStream_t stream, int ks) {
  using namespace mlp;
  check_b(B);
  if (!p_old || !p_new || p_old == p_new || !x_prev || !x || !ctr)
    throw std::runtime_error("mlp_fwdapply: needs distinct ping-pong buffers, both batches, ctr");
  if (stats && stats_ring < 1) throw std::runtime_error("mlp_fwdapply: stats_ring < 1");
  const Bufs w = make_bufs(ws, B);
  if (ks == 0) ks = mlp_single_ks();
  with_const<KS2, KS3>(ks, "mlp_fwdapply: ks must be 0, 14 or 28", [&](auto KSX) {
    fwdapply_single_launch<KSX()>(p_old, p_new, lr, x_prev, x, w, ctr, stats, stats_ring, B,
                                  stats_on, stream);
  });
  DTFX_HIP_CHECK(hipGetLastError());
}

// The pending update of the last single-GPU pipelined step (the flush): W1 from step t's
// factors and its small parameters, p_old -> p_new, with step t's loss / accuracy record and
// global_step += 1 -- the first launch's apply half alone (mlp_lean_fwdapply_kernel<.., FWD =
// false>; DTFX_MLP_KS=14: mlp_fwdapply_kernel<.., KS2, false>), ~half the MFMAs per wave of the
// 3-launch step's mlp_wgrad_kernel.
void mlp_apply_launch(const float* p_old, float* p_new, float lr, const float* x_prev, float* ws,
                      int* ctr, float* stats, int stats_ring, int B, hipStream_t stream) {
  using namespace mlp;
  check_b(B);
  if (!p_old || !p_new || p_old == p_new || !x_prev || !ctr)
    throw std::runtime_error("mlp_apply: needs distinct ping-pong buffers, the batch, ctr");
  if (stats && stats_ring < 1) throw std::runtime_error("mlp_apply: stats_ring < 1");
  // DTFX_MLP_FLUSH_FWD=1: the flush runs the steps' own instantiation (FWD = true, its forward
  // over x_prev into the workspace slab, which the next step overwrites) instead of the
  // apply-only one: A/B of whether the flush pays for a code object no step keeps hot
  static const bool ffwd = [] {
    const char* e = std::getenv("DTFX_MLP_FLUSH_FWD");
    return e && std::atoi(e) == 1;
  }();
  if (mlp_single_ks() == KS3) {  // the lean first launch, apply-only (or whole: ffwd)
    with_flag(ffwd, [&](auto FWD) {
      lean_first_launch<FWD()>(p_old, p_new, lr, x_prev, x_prev, ws, ctr, stats, stats_ring, B, 1,
                               stream);
    });
  } else {
    fwdapply_single_launch<KS2, false>(p_old, p_new, lr, x_prev, x_prev, make_bufs(ws, B), ctr,
                                       stats, stats_ring, B, 1, stream);
  }
  DTFX_HIP_CHECK(hipGetLastError());
}

// Pipelined fused data-parallel step, first launch (mlp_fwdapply_kernel<.., XW>); the head is
// mlp_head2_launch.  lr already divided by the world size.
void mlp_fwdapply_xg_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                            const float* x, float* ws, int* ctr, float* stats, int stats_ring,
                            int B, int stats_on, hipStream_t stream, const MlpXg& xg, int world,
                            int two_shot, unsigned long long* trace) {
  using namespace mlp;
  check_b(B);
  if (!p_old || !p_new || p_old == p_new || !x_prev || !x || !ctr)
    throw std::runtime_error("mlp_fwdapply_xg: needs distinct ping-pong buffers, both batches, ctr");
  if (stats && stats_ring < 1) throw std::runtime_error("mlp_fwdapply_xg: stats_ring < 1");
  if (xg.S < NPARAM) throw std::runtime_error("mlp_fwdapply_xg: exchange slots smaller than the model");
  if ((xg.split & 1) && !(two_shot && (xg.split & 4)) && xg.S < XG_SLOT_WORDS)
    throw std::runtime_error("mlp_fwdapply_xg: the split exchange's 16-byte pair layout needs "
                             "slots of mlp_step.XG_SLOT_WORDS words (create the communicator "
                             "with that max_numel)");
  // 28 K slices (as the single-GPU step): 196 W1 blocks x 2 column groups of epoch slots
  static_assert(HT * KS3 * 2 <= MLP_XG_SMALL_EPOCH, "W1 epoch slots overlap the small ones");
  const Bufs w = make_bufs(ws, B);
  dim3 grid(HT * KS3 + HT), block(256);
  if (trace) {  // probe builds (tools/probes/engine_trace.py): [blocks * 4 waves][8] stamps
    if ((B + 15) / 16 != 7) throw std::runtime_error("mlp_fwdapply_xg trace: batch 97..112 only");
    // (the trace instantiations exist for NGT = 7 and world 2, 4, 8 only)
    with_const<2, 4, 8>(world, "mlp_fwdapply_xg trace: world 2, 4 or 8", [&](auto WW) {
      with_flag(two_shot != 0, [&](auto TWO) {
        hipLaunchKernelGGL((mlp_fwdapply_kernel<7, WW(), true, TWO(), KS3>), grid, block, 0,
                           stream, p_old, p_new, lr, x_prev, x, w, ctr, stats, stats_ring, B,
                           stats_on, xg, trace);
      });
    });
    DTFX_HIP_CHECK(hipGetLastError());
    return;
  }
  with_world(world, "mlp_fwdapply_xg: world must be 2..8", [&](auto WW) {
    with_ngt(B, [&](auto NGT) {
      with_flag(two_shot != 0, [&](auto TWO) {
        hipLaunchKernelGGL((mlp_fwdapply_kernel<NGT(), WW(), false, TWO(), KS3>), grid, block,
                           0, stream, p_old, p_new, lr, x_prev, x, w, ctr, stats, stats_ring, B,
                           stats_on, xg, nullptr);
      });
    });
  });
  DTFX_HIP_CHECK(hipGetLastError());
}

// Probe: one pipelined step with in-kernel stamps in both launches (trf: (7 * ks + 7) * 4 * 4
// with ks = mlp_single_ks_query(), trh: B * 4 entries; trs, optional: the 28-slice first launch's
// split stamps, (7 * 28 + 7) * 4 * 2); batch 100 only.
int mlp_single_ks_query() { return mlp_single_ks(); }
void mlp_pipelined_trace_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                                const float* x, const int* labels, float* ws, int* ctr,
                                float* stats, int stats_ring, int B, hipStream_t stream,
                                unsigned long long* trf, unsigned long long* trh,
                                unsigned long long* trs) {
  using namespace mlp;
  check_b(B);
  if ((B + 15) / 16 != 7) throw std::runtime_error("mlp_pipelined_trace: batch 97..112 only");
  const Bufs w = make_bufs(ws, B);
  if (mlp_single_ks() == KS3) {
    // the lean pair's TRACE instantiations; trs (optional): [(7 * 28 + 7) * 4 waves][2] split
    // stamps of the first launch (fwdapply_block)
    hipLaunchKernelGGL((mlp_lean_fwdapply_trace_kernel<7>), dim3(HT * KS3 + HT), dim3(256), 0,
                       stream, p_old, p_new, x_prev, x, ws, lr,
                       lean_flags(B, 1, stats, stats_ring), ctr, stats, trf, trs);
    hipLaunchKernelGGL((mlp_lean_head_trace_kernel<7>), dim3(B), dim3(64), 0, stream,
                       (const float*)p_new, labels, ws, B, trh);
  } else {
    hipLaunchKernelGGL((mlp_fwdapply_kernel<7, 0, true>), dim3(HT * KS2 + HT), dim3(256), 0, stream,
                       p_old, p_new, lr, x_prev, x, w, ctr, stats, stats_ring, B, 1, MlpXg{}, trf);
    hipLaunchKernelGGL((mlp_head_kernel<false, true, 0, KS2>), dim3(B), dim3(64), 0, stream, p_new,
                       p_new, 0.f, nullptr, labels, w, B, trh, MlpXg{}, nullptr);
  }
  DTFX_HIP_CHECK(hipGetLastError());
}

// nslab: the K slabs the first launch wrote -- 0: the single-GPU step's (mlp_single_ks());
// the fused2 / fused2x first launch writes KS3 = 28, the factor engine's KS2 = 14.
void mlp_head2_launch(const float* p, const int* labels, float* ws, int B, hipStream_t stream,
                      int nslab) {
  using namespace mlp;
  check_b(B);
  if (nslab == 0) nslab = mlp_single_ks();
  with_const<KS2, KS3>(nslab, "mlp_head2: nslab must be 0, 14 or 28", [&](auto NSLAB) {
    head_plain_launch<NSLAB()>(p, labels, make_bufs(ws, B), B, stream);
  });
  DTFX_HIP_CHECK(hipGetLastError());
}

// Head of the single-GPU two-launch step: after mlp_fwdapply_launch's 28-slice form it leaves
// the factors ROW-major (dz1R / dlR), which the next step's first launch and the flush
// (mlp_apply_launch) read; with DTFX_MLP_KS=14 the step keeps the transposed layout.  (The
// data-parallel engines' heads -- mlp_head2_launch with their nslab -- stay transposed.)
void mlp_head2_single_launch(const float* p, const int* labels, float* ws, int B,
                             hipStream_t stream) {
  using namespace mlp;
  if (mlp_single_ks() != KS3) return mlp_head2_launch(p, labels, ws, B, stream, KS2);
  check_b(B);
  head_plain_launch<KS3, true>(p, labels, make_bufs(ws, B), B, stream);
  DTFX_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Momentum / Adam inside the two-launch step (mlp_lean_fwdapply_opt_kernel; the head launch is
// the SGD step's).  kind: 1 momentum, 2 adam; s0 / s1: the slot planes (flat f32 [79510],
// 16-byte aligned; s1 adam only); tp: the int32[2] step pair; h0..h2: gpu_ps_optim.hyper_args.
// par is the index of p_old in the caller's ping-pong pair: the launch reads tp[par] and writes
// tp[par ^ 1], so consecutive launches must alternate it (as they alternate the buffers).
// Only the lean 28-slice step has these variants: DTFX_MLP_KS=14 and the fused flush
// (DTFX_MLP_FLUSH_FUSED) are refused.
// sched != 0: the scheduled instantiations (mlp_lean_fwdapply_sched_kernel) -- tp then heads the
// 8-word schedule block, lr is the base rate, lrs the rate ring (f32 [stats_ring], or null), and
// kind 0 is scheduled gradient descent (no slot planes).  (struct MlpOpt: mlp_step_api.h)
// wd != 0: the weight-decay / Nesterov instantiations (mlp_lean_fwdapply_wd_kernel) with the
// coefficients l2, dec, na, nb (ops/weight_decay.py: words()); kind 0 is then allowed at a
// constant rate too (tp: the plain step pair, no slot plane).
// ema != 0: the moving-average instantiations (mlp_lean_fwdapply_ema_kernel) with the shadow plane
// se, omd = 1 - decay and the num_updates flag (ops/ema.py: words()); every kind 0..2, with or
// without a schedule and the weight-decay words.
static void check_opt(const MlpOpt& o, const char* who) {
  const char* bad = nullptr;  // (the message is put together only when there is one)
  if (o.ema) {
    if (o.kind != mlp::OPT_SGD && o.kind != mlp::OPT_MOMENTUM && o.kind != mlp::OPT_ADAM)
      bad = ": moving-average optimizer kind must be 0 (sgd), 1 or 2";
    else if (mlp_single_ks() != mlp::KS3)
      bad = ": DTFX_MLP_KS=14 has no moving-average variant";
    else if (!o.tp || (o.kind != mlp::OPT_SGD && !o.s0) || (o.kind == mlp::OPT_ADAM && !o.s1))
      bad = ": null slot plane / step pair";
    else if (o.sched && (reinterpret_cast<uintptr_t>(o.tp) & 31))
      bad = ": the schedule block must be 32-byte aligned";
    else if (!o.se)
      bad = ": null shadow plane";
    else if (reinterpret_cast<uintptr_t>(o.se) & 15)
      bad = ": the shadow plane must be 16-byte aligned";
    else if (!(o.omd > 0.f && o.omd < 1.f))
      bad = ": the moving-average decay must lie in (0, 1)";
  } else if (o.wd && !o.sched) {
    if (o.kind != mlp::OPT_SGD && o.kind != mlp::OPT_MOMENTUM && o.kind != mlp::OPT_ADAM)
      bad = ": weight-decay optimizer kind must be 0 (sgd), 1 or 2";
    else if (mlp_single_ks() != mlp::KS3)
      bad = ": DTFX_MLP_KS=14 has no weight-decay variant";
    else if (!o.tp || (o.kind != mlp::OPT_SGD && !o.s0) || (o.kind == mlp::OPT_ADAM && !o.s1))
      bad = ": null slot plane / step pair";
  } else if (o.sched) {  // (scheduled gradient descent is kind 0 and has no slot plane)
    if (o.kind != mlp::OPT_SGD && o.kind != mlp::OPT_MOMENTUM && o.kind != mlp::OPT_ADAM)
      bad = ": scheduled optimizer kind must be 0 (sgd), 1 or 2";
    else if (mlp_single_ks() != mlp::KS3)
      bad = ": DTFX_MLP_KS=14 has no learning-rate schedule variant";
    else if (!o.tp || (o.kind != mlp::OPT_SGD && !o.s0) || (o.kind == mlp::OPT_ADAM && !o.s1))
      bad = ": null slot plane / schedule block";
    else if (reinterpret_cast<uintptr_t>(o.tp) & 31)
      bad = ": the schedule block must be 32-byte aligned";
  } else {
    if (o.kind != mlp::OPT_MOMENTUM && o.kind != mlp::OPT_ADAM)
      bad = ": optimizer kind must be 1 (momentum) or 2 (adam)";
    else if (mlp_single_ks() != mlp::KS3)
      bad = ": DTFX_MLP_KS=14 has no optimizer variant (sgd only)";
    else if (!o.s0 || !o.tp || (o.kind == mlp::OPT_ADAM && !o.s1))
      bad = ": null slot plane / step pair";
  }
  if (!bad && ((reinterpret_cast<uintptr_t>(o.s0) | reinterpret_cast<uintptr_t>(o.s1)) & 15))
    bad = ": slot planes must be 16-byte aligned";
  if (!bad && o.wd && !(o.l2 >= 0.f && o.dec >= 0.f && o.l2 < INFINITY && o.dec < INFINITY))
    bad = ": weight decay must be finite and >= 0";
  if (bad) throw std::runtime_error(std::string(who) + bad);
}

template <bool FWD>
static void lean_first_opt_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                                  const float* x, float* ws, int* ctr, float* stats,
                                  int stats_ring, int B, int apply, int par, const MlpOpt& o,
                                  hipStream_t stream) {
  using namespace mlp;
  const int flags = lean_flags(B, apply, stats, stats_ring);
  if ((reinterpret_cast<uintptr_t>(p_old) | reinterpret_cast<uintptr_t>(p_new)) & 15)
    throw std::runtime_error("fused MLP step: parameter buffers must be 16-byte aligned");
  const int oflags = (apply ? 1 : 0) | (par & 1) << 1;
  dim3 grid(HT * KS3 + HT), block(256);
  // (check_opt has admitted the kind: 0..2 scheduled, 1..2 not)
  const char* bad_kind = "fused MLP step: optimizer kind out of range";
  with_ngt(B, [&](auto NGT) {
    if (o.ema)  // (without decay the coefficient words are MlpOpt's defaults 0, 0, 0, 1)
      with_const<OPT_SGD, OPT_MOMENTUM, OPT_ADAM>(o.kind, bad_kind, [&](auto OPTK) {
        with_flag(o.sched != 0, [&](auto SCHED) {
          hipLaunchKernelGGL((mlp_lean_fwdapply_ema_kernel<NGT(), FWD, OPTK(), SCHED()>), grid,
                             block, 0, stream, p_old, p_new, x_prev, x, ws, lr, flags, ctr, stats,
                             o.s0, o.s1, o.tp, o.h0, o.h1, o.h2, oflags | (o.nu ? 4 : 0),
                             SCHED() ? o.lrs : nullptr, o.l2, o.dec, o.na, o.nb, o.se, o.omd);
        });
      });
    else if (o.wd)
      with_const<OPT_SGD, OPT_MOMENTUM, OPT_ADAM>(o.kind, bad_kind, [&](auto OPTK) {
        with_flag(o.sched != 0, [&](auto SCHED) {
          hipLaunchKernelGGL((mlp_lean_fwdapply_wd_kernel<NGT(), FWD, OPTK(), SCHED()>), grid,
                             block, 0, stream, p_old, p_new, x_prev, x, ws, lr, flags, ctr, stats,
                             o.s0, o.s1, o.tp, o.h0, o.h1, o.h2, oflags, SCHED() ? o.lrs : nullptr,
                             o.l2, o.dec, o.na, o.nb);
        });
      });
    else if (o.sched)
      with_const<OPT_SGD, OPT_MOMENTUM, OPT_ADAM>(o.kind, bad_kind, [&](auto OPTK) {
        hipLaunchKernelGGL((mlp_lean_fwdapply_sched_kernel<NGT(), FWD, OPTK()>), grid, block, 0,
                           stream, p_old, p_new, x_prev, x, ws, lr, flags, ctr, stats, o.s0, o.s1,
                           o.tp, o.h0, o.h1, o.h2, oflags, o.lrs);
      });
    else
      with_const<OPT_MOMENTUM, OPT_ADAM>(o.kind, bad_kind, [&](auto OPTK) {
        hipLaunchKernelGGL((mlp_lean_fwdapply_opt_kernel<NGT(), FWD, OPTK()>), grid, block, 0,
                           stream, p_old, p_new, x_prev, x, ws, lr, flags, ctr, stats, o.s0, o.s1,
                           o.tp, o.h0, o.h1, o.h2, oflags);
      });
  });
}

// First launch of a step: apply != 0 applies the pending update (and records its stats, global
// step += 1); apply == 0 copies p_old -> p_new, touches no slot byte and runs the forward.
void mlp_lean_fwdapply_opt_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                                  const float* x, float* ws, int* ctr, float* stats,
                                  int stats_ring, int B, int apply, int par, const MlpOpt& o,
                                  hipStream_t stream) {
  check_b(B);
  check_opt(o, "mlp_lean_fwdapply_opt");
  if (!p_old || !p_new || p_old == p_new || !x_prev || !x || !ctr || !ws)
    throw std::runtime_error(
        "mlp_lean_fwdapply_opt: needs distinct ping-pong buffers, both batches, ctr");
  lean_first_opt_launch<true>(p_old, p_new, lr, x_prev, x, ws, ctr, stats, stats_ring, B, apply,
                              par, o, stream);
  DTFX_HIP_CHECK(hipGetLastError());
}

// The flush: the pending update alone (apply-only instantiation), p_old -> p_new.
void mlp_apply_opt_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                          float* ws, int* ctr, float* stats, int stats_ring, int B, int par,
                          const MlpOpt& o, hipStream_t stream) {
  check_b(B);
  check_opt(o, "mlp_apply_opt");
  if (!p_old || !p_new || p_old == p_new || !x_prev || !ctr || !ws)
    throw std::runtime_error("mlp_apply_opt: needs distinct ping-pong buffers, the batch, ctr");
  lean_first_opt_launch<false>(p_old, p_new, lr, x_prev, x_prev, ws, ctr, stats, stats_ring, B, 1,
                               par, o, stream);
  DTFX_HIP_CHECK(hipGetLastError());
}

// n pipelined single-GPU steps issued from ONE host call (no Python, no hipGraph): step i
// trains on batch (pos + i) % nbatches of the device-resident dataset and ping-pongs the
// parameter buffers exactly like n calls of mlp_lean_fwdapply_launch + mlp_lean_head_launch.
// A graph replay pays ~15 us of submission before its first kernel runs; these launches reach the GPU
// one by one while the host keeps queueing ahead (host ~2 us per launch < ~4 us of GPU time
// per launch), so a short run starts at once.  Returns nothing: the caller advances its host
// mirrors (batch position, parity, pending) by n.
// flush != 0: the pending update of the last step is applied by one more launch
// (mlp_apply_launch, into the other buffer: the parity then moves by n + 1).
// DTFX_MLP_FLUSH_FUSED=1: the last step's head and the flush in ONE launch
// (mlp_head_flush_kernel).  Opt-in: correct (bit-identical to the separate flush, tests/
// test_kernels_gpu.py) but measured SLOWER in the driver-sized region -- 10.97-11.05 M vs
// 11.37-11.46 M samples/s, six interleaved pairs on one box (profiles/r6/k20/flush_fused_ab/):
// the in-kernel hand-off (release adds of 100 row waves, the apply blocks' acquire poll, their
// cold operand loads after it) costs ~7 us more than the kernel boundary it replaces, as the
// persistent engine's hand-offs did (mlp_persistent.hip).
static int g_flush_fused = -1;  // -1: read DTFX_MLP_FLUSH_FUSED on first use
static bool mlp_flush_fused() {
  if (g_flush_fused < 0) {
    const char* e = std::getenv("DTFX_MLP_FLUSH_FUSED");
    g_flush_fused = e && std::atoi(e) == 1 ? 1 : 0;
  }
  return g_flush_fused == 1;
}
// tests: select the terminal form in-process (returns the previous setting)
int mlp_set_flush_fused(int on) {
  const int old = mlp_flush_fused() ? 1 : 0;
  g_flush_fused = on ? 1 : 0;
  return old;
}

// The ONE walk over the resident dataset: batch position, buffer parity, pending flag and the
// terminal flush.  The launches come from the caller's policy:
//   step(po, pn, xprev, xcur, lab, pending, par)  both launches of a step, po -> pn (pending: an
//     update waits to be applied; par: po's index in the ping-pong pair);
//   last(po, pn, xprev, xcur, lab, pending)  fused_last only: the region's last step with the
//     flush folded into its second launch (the update lands back in po: net parity n + 1);
//   flush(po, pn, xprev, par)  the pending update alone, po -> pn.
template <class Step, class Last, class Flush>
static void run_pipelined(float* p0, float* p1, int cur, int pending, const float* x,
                          const int* labels, int nbatches, int pos, int n, int B, bool do_flush,
                          bool fused_last, Step&& step, Last&& last, Flush&& flush) {
  float* bufs[2] = {p0, p1};
  const size_t xb = (size_t)B * mlp::D;
  auto prev = [&] { return x + (size_t)((pos + nbatches - 1) % nbatches) * xb; };
  for (int i = 0; i < n; ++i) {
    const float* xcur = x + (size_t)pos * xb;
    const float* xprev = pending ? prev() : xcur;
    const int* lab = labels + (size_t)pos * B;
    const bool fused = fused_last && i == n - 1;
    if (fused) last(bufs[cur], bufs[cur ^ 1], xprev, xcur, lab, pending);
    else step(bufs[cur], bufs[cur ^ 1], xprev, xcur, lab, pending, cur);
    cur ^= 1;
    pending = fused ? 0 : 1;
    pos = (pos + 1) % nbatches;
  }
  if (do_flush && pending) flush(bufs[cur], bufs[cur ^ 1], prev(), cur);
  DTFX_HIP_CHECK(hipGetLastError());
}

// Plain SGD: the lean pair, or with DTFX_MLP_KS=14 the general kernels over 14 slices.  pending
// doubles as the kernel's "apply / record the previous step" flag, as in step_pipelined: nothing
// pending runs with lr = 0.
void mlp_run_pipelined_launch(float* p0, float* p1, int cur, int pending, float lr,
                              const float* x, const int* labels, int nbatches, int pos, int n,
                              float* ws, int* ctr, float* stats, int stats_ring, int B,
                              hipStream_t stream, int flush, const MlpDrop* drop, int act) {
  using namespace mlp;
  check_b(B);
  check_act(act, "mlp_run_pipelined");
  if (act != HACT_SIGMOID) {
    if (mlp_single_ks() != KS3)
      throw std::runtime_error("mlp_run_pipelined: DTFX_MLP_KS=14 has no relu / tanh variant");
    if (flush && mlp_flush_fused())
      throw std::runtime_error(
          "mlp_run_pipelined: the fused flush (DTFX_MLP_FLUSH_FUSED) has no relu / tanh variant");
  }
  if (drop) {
    check_drop(*drop, "mlp_run_pipelined");
    if (mlp_single_ks() != KS3)
      throw std::runtime_error("mlp_run_pipelined: DTFX_MLP_KS=14 has no dropout variant");
    if (flush && mlp_flush_fused())
      throw std::runtime_error(
          "mlp_run_pipelined: the fused flush (DTFX_MLP_FLUSH_FUSED) has no dropout variant");
  }
  if (!p0 || !p1 || p0 == p1 || !x || !labels || !ctr || nbatches < 1 || pos < 0 ||
      pos >= nbatches || n < 0)
    throw std::runtime_error("mlp_run_pipelined: bad buffers / position / count");
  if (stats && stats_ring < 1) throw std::runtime_error("mlp_run_pipelined: stats_ring < 1");
  const Bufs w = make_bufs(ws, B);
  with_const<KS2, KS3>(mlp_single_ks(), "mlp_run_pipelined: K slicing", [&](auto KSV) {
    auto first = [&](const float* po, float* pn, const float* xprev, const float* xcur, int pend) {
      fwdapply_single_launch<KSV()>(po, pn, pend ? lr : 0.f, xprev, xcur, w, ctr, stats, stats_ring,
                                    B, pend, stream);
    };
    auto step = [&](const float* po, float* pn, const float* xprev, const float* xcur,
                    const int* lab, int pend, int) {
      if constexpr (KSV() == KS3) {
        lean_first_launch<true>(po, pn, pend ? lr : 0.f, xprev, xcur, ws, ctr, stats, stats_ring, B,
                                pend, stream);
        lean_head_launch(pn, lab, ws, B, stream, drop, act);
      } else {
        first(po, pn, xprev, xcur, pend);
        head_plain_launch<KSV()>(pn, lab, w, B, stream);
      }
    };
    // the first launch on the general kernel, then ONE launch for the head and the apply of
    // the step's update (pn -> po: the flush's destination, the other buffer)
    auto last = [&](float* po, float* pn, const float* xprev, const float* xcur, const int* lab,
                    int pend) {
      first(po, pn, xprev, xcur, pend);
      const long long ticks = 200000000LL;  // 2 s of s_memrealtime (100 MHz)
      with_ngt(B, [&](auto NGT) {
        hipLaunchKernelGGL((mlp_head_flush_kernel<NGT(), KSV()>),
                           dim3((B + 3) / 4 + HT * KSV() + HT), dim3(256), 0, stream, pn, po, lr,
                           xcur, lab, w, ctr, stats, stats_ring, B, ticks);
      });
    };
    auto apply = [&](const float* po, float* pn, const float* xprev, int) {
      mlp_apply_launch(po, pn, lr, xprev, ws, ctr, stats, stats_ring, B, stream);
    };
    run_pipelined(p0, p1, cur, pending, x, labels, nbatches, pos, n, B, flush != 0,
                  flush && n > 0 && mlp_flush_fused(), step, last, apply);
  });
}

// mlp_run_pipelined_launch with an optimizer: the same walk; every first launch takes par = the
// parity it reads, and lr with the explicit apply bit.
void mlp_run_pipelined_opt_launch(float* p0, float* p1, int cur, int pending, float lr,
                                  const float* x, const int* labels, int nbatches, int pos, int n,
                                  float* ws, int* ctr, float* stats, int stats_ring, int B,
                                  hipStream_t stream, int flush, const MlpOpt& o,
                                  const MlpDrop* drop, int act) {
  check_b(B);
  check_opt(o, "mlp_run_pipelined_opt");
  check_act(act, "mlp_run_pipelined_opt");
  if (drop) check_drop(*drop, "mlp_run_pipelined_opt");
  if (!p0 || !p1 || p0 == p1 || !x || !labels || !ctr || !ws || nbatches < 1 || pos < 0 ||
      pos >= nbatches || n < 0 || (cur != 0 && cur != 1))
    throw std::runtime_error("mlp_run_pipelined_opt: bad buffers / position / count");
  if (flush && mlp_flush_fused())
    throw std::runtime_error(
        std::string("mlp_run_pipelined_opt: the fused flush (DTFX_MLP_FLUSH_FUSED) has ") +
        (o.ema     ? "no moving-average variant"
         : o.wd    ? "no weight-decay variant"
         : o.sched ? "no learning-rate schedule variant"
                   : "no optimizer variant (sgd only)"));
  auto step = [&](const float* po, float* pn, const float* xprev, const float* xcur,
                  const int* lab, int pend, int par) {
    lean_first_opt_launch<true>(po, pn, lr, xprev, xcur, ws, ctr, stats, stats_ring, B, pend, par,
                                o, stream);
    lean_head_launch(pn, lab, ws, B, stream, drop, act);
  };
  auto apply = [&](const float* po, float* pn, const float* xprev, int par) {
    lean_first_opt_launch<false>(po, pn, lr, xprev, xprev, ws, ctr, stats, stats_ring, B, 1, par, o,
                                 stream);
  };
  run_pipelined(p0, p1, cur, pending, x, labels, nbatches, pos, n, B, flush != 0, false, step,
                [](auto...) {}, apply);
}

// The all-reduce engine's scheduled rate (mlp_lr_sched_kernel): lr(ctr - 1) -> out[0] and, with
// lrs, the rate ring.  blk: the 8-word schedule block (32-byte aligned).
void mlp_lr_sched_launch(const int* ctr, const int* blk, float lr0, float* out, float* lrs,
                         int ring, hipStream_t stream) {
  if (!ctr || !blk || !out || (reinterpret_cast<uintptr_t>(blk) & 31) || (lrs && ring < 1))
    throw std::runtime_error("mlp_lr_sched: needs ctr, a 32-byte aligned schedule block, out");
  hipLaunchKernelGGL(mlp::mlp_lr_sched_kernel, dim3(1), dim3(64), 0, stream, ctr, blk, lr0, out,
                     lrs, lrs ? ring : 1);
  DTFX_HIP_CHECK(hipGetLastError());
}

// Pipelined factor engine, first launch (see mlp_fwdapply_factor_kernel).
void mlp_fwdapply_factor_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                                const float* x, long long xstride, const float* dz1A, float* ws,
                                int* ctr, float* stats, int stats_ring, int B, int stats_on,
                                hipStream_t stream, const MlpXg& xg, int world) {
  using namespace mlp;
  check_b(B);
  if ((B + 15) / 16 > 8) throw std::runtime_error("mlp_fwdapply_factor: batch must be <= 128");
  if (!p_old || !p_new || p_old == p_new || !x_prev || !x || !ctr || !dz1A)
    throw std::runtime_error("mlp_fwdapply_factor: needs ping-pong buffers, batches, ctr, dz1A");
  if (xg.S < NPARAM) throw std::runtime_error("mlp_fwdapply_factor: exchange slots too small");
  const Bufs w = make_bufs(ws, B);
  dim3 grid(8 * FX_SLOTS + HT);
  with_world(world, "mlp_fwdapply_factor: world must be 2..8", [&](auto WW) {
    with_ngt(B, [&](auto NGT) {
      hipLaunchKernelGGL((mlp_fwdapply_factor_kernel<WW(), NGT()>), grid,
                         dim3(128 * fx_kspl<NGT()>()), 0, stream, p_old, p_new, lr, x_prev, x,
                         xstride, dz1A, w, ctr, stats, stats_ring, B, stats_on, xg);
    });
  });
  DTFX_HIP_CHECK(hipGetLastError());
}


// Async-PS worker step (train/worker.py, the reference's hot loop worker.py:131-137) in ONE
// host call: the staged batch (pinned host -> device), the parameters pulled by the last
// push/step/pull exchange (pinned host, TF layout -> device flat layout; skipped when
// pulled_host is null), forward + backward writing the flat gradient, the gradient in TF
// layout with the step's loss / accuracy record appended (-> pinned host), and a wait for the
// stream.  Replaces ~10 Python-issued copies / launches / syncs per step; the caller releases
// the GIL for the call.  Host buffers must be pinned (hipHostMalloc'd); *_dev are device staging
// buffers of NPARAM + 2 floats.
// Device address of a pinned host buffer when the runtime maps it into the GPU's address
// space (hipHostMalloc'd memory: the kernels then read / write it over the host link
// directly), else null and the caller moves it with a DMA copy.  Looked up per buffer once.
static const void* mapped_device_ptr(const void* host) {
  static std::mutex mu;
  static std::map<const void*, const void*> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(host);
  if (it != cache.end()) return it->second;
  hipPointerAttribute_t a{};
  const void* d = nullptr;
  if (hipPointerGetAttributes(&a, host) == hipSuccess) {
    if (a.type == hipMemoryTypeHost && a.devicePointer) d = a.devicePointer;
  } else {
    (void)hipGetLastError();  // not a HIP allocation: clear the sticky error
  }
  if (getenv("DTFX_PS_NO_ZERO_COPY")) d = nullptr;
  cache[host] = d;
  return d;
}

void mlp_ps_worker_step(float* p, const float* pulled_host, float* pull_dev, const float* x_host,
                        const int* y_host, float* x_dev, int* y_dev, float* grad, float* ws,
                        int* ctr, float* stats, int stats_ring, const float* record, int B,
                        float* grad_dev, float* grad_host, hipStream_t s) {
  using namespace mlp;
  check_b(B);
  if (!p || (x_host && !y_host) || !x_dev || !y_dev || !grad || !ws || !ctr || !grad_dev ||
      !grad_host || (pulled_host && !pull_dev) || (record && !stats))
    throw std::runtime_error("mlp_ps_worker_step: missing buffer");
  if (x_host) {  // (null: already staged by mlp_ps_stage while the last exchange was in flight)
    DTFX_HIP_CHECK(hipMemcpyAsync(x_dev, x_host, sizeof(float) * (size_t)B * D,
                                  hipMemcpyHostToDevice, s));
    DTFX_HIP_CHECK(hipMemcpyAsync(y_dev, y_host, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, s));
  }
  // zero copy where the pinned buffers are device-mapped: the layout kernels read the pulled
  // parameters from / write the gradient to host memory themselves -- no DMA copy (each has
  // a setup latency of several us on top of the transfer) and two fewer queue entries
  const float* pulled_map = pulled_host ? (const float*)mapped_device_ptr(pulled_host) : nullptr;
  float* grad_map = (float*)mapped_device_ptr(grad_host);
  if (pulled_host) {
    if (pulled_map) {
      hipLaunchKernelGGL(mlp_from_tf_src_major_kernel, dim3((NPARAM + 255) / 256), dim3(256), 0,
                         s, pulled_map, p);
      DTFX_HIP_CHECK(hipGetLastError());
    } else {
      DTFX_HIP_CHECK(hipMemcpyAsync(pull_dev, pulled_host, sizeof(float) * NPARAM,
                                    hipMemcpyHostToDevice, s));
      mlp_tf_layout_launch(pull_dev, p, 0, nullptr, 0, s);
    }
  }
  mlp_fwd_launch(p, nullptr, 0.f, nullptr, x_dev, ws, B, s, nullptr);
  mlp_head_launch(p, nullptr, 0.f, nullptr, y_dev, ws, B, s, nullptr);
  mlp_wgrad_launch(nullptr, 0.f, grad, x_dev, ws, ctr, stats, stats_ring, B, s, nullptr);
  if (grad_map) {
    mlp_tf_layout_launch(grad, grad_map, 1, record, record ? 2 : 0, s);
  } else {
    mlp_tf_layout_launch(grad, grad_dev, 1, record, record ? 2 : 0, s);
    DTFX_HIP_CHECK(hipMemcpyAsync(grad_host, grad_dev, sizeof(float) * (NPARAM + (record ? 2 : 0)),
                                  hipMemcpyDeviceToHost, s));
  }
  DTFX_HIP_CHECK(hipStreamSynchronize(s));
}

// The next batch's H2D copies (pinned host -> device), issued while the previous step's
// push/step/pull exchange is on the wire; mlp_ps_worker_step then runs with x_host = null.
void mlp_ps_stage(const float* x_host, const int* y_host, float* x_dev, int* y_dev, int B,
                  hipStream_t s) {
  check_b(B);
  DTFX_HIP_CHECK(hipMemcpyAsync(x_dev, x_host, sizeof(float) * (size_t)B * mlp::D,
                                hipMemcpyHostToDevice, s));
  DTFX_HIP_CHECK(hipMemcpyAsync(y_dev, y_host, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, s));
}
}  // namespace dtfx
