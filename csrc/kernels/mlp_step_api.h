// Host API of the fused MLP step (mlp_step.hip): every function the file exports (and, at the
// end, its two sibling files'), declared ONCE for the defining files, the Python bindings
// (bindings.cpp) and the xGMI communicator (xgmi_comm.cpp).  Plain C++: no kernel, no device
// code.  Pointers are device addresses unless named *_host; the comments at the definitions say
// what each launch computes.
#pragma once
#include <hip/hip_runtime.h>

#include "xgmi.h"

namespace dtfx {

// ---- hidden-layer dropout of the step's head (ops/dropout.py has the definition).  Element
// (batch row r, hidden unit j) is kept iff (w >> 8) < thr, w = word (n & 3), n = 100 r + j, of
// philox4x32_10(counter {n >> 2, 0, *ctr, stream}, key {k0, k1}); kept values are scaled by
// `scale` = 2^24 / thr.  ctr: the device global_step counter (equal to the step's own index at
// every head launch: the only writer is the stats lane of the launch that records the step
// before).  A null `const MlpDrop*` is no dropout and launches the plain kernels.
struct MlpDrop {
  const int* ctr;
  unsigned k0, k1, thr, stream;
  float scale;
};

// ---- the hidden activation of the step's head and of the evaluation kernel (ops/hidden_act.py
// has the definition; the ids are common.h's HACT_*): 0 sigmoid, the reference's and every
// launcher's default, 1 relu, 2 tanh.  Launchers throw on any other id, and where no relu / tanh
// variant exists (DTFX_MLP_KS=14, the fused flush, the trace launches).
constexpr int kMlpActSigmoid = 0;

// ---- workspace / layout queries and knobs
long long mlp_workspace_floats(int B);
void mlp_rowmajor_layout(int B, long long* out);
int mlp_single_ks_query();
int mlp_set_flush_fused(int on);

// ---- TF checkpoint layout <-> flat layout, and the wave_reduce_scatter test kernel
void mlp_tf_layout_launch(const float* src, float* dst, int to_tf, const float* xsrc, int extra,
                          hipStream_t stream);
void wave_reduce_scatter_test_launch(const float* in, float* out, int n, hipStream_t stream);

// ---- the three-launch step
void mlp_fwd_launch(const float* p_old, const float* grad, float lr, float* p_new, const float* x,
                    float* ws, int B, hipStream_t stream, unsigned long long* tr);
void mlp_head_launch(const float* p_old, const float* grad, float lr, float* p_new,
                     const int* labels, float* ws, int B, hipStream_t stream,
                     unsigned long long* tr, const MlpDrop* drop = nullptr,
                     int act = kMlpActSigmoid);
void mlp_wgrad_launch(float* p, float lr, float* grad, const float* x, float* ws, int* ctr,
                      float* stats, int stats_ring, int B, hipStream_t stream,
                      unsigned long long* tr);

// ---- the two-launch step (ks / nslab = 0: the single-GPU step's K slicing)
void mlp_fwdapply_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                         const float* x, float* ws, int* ctr, float* stats, int stats_ring, int B,
                         int stats_on, hipStream_t stream, int ks);
void mlp_head2_launch(const float* p, const int* labels, float* ws, int B, hipStream_t stream,
                      int nslab);
void mlp_head2_single_launch(const float* p, const int* labels, float* ws, int B,
                             hipStream_t stream);
void mlp_apply_launch(const float* p_old, float* p_new, float lr, const float* x_prev, float* ws,
                      int* ctr, float* stats, int stats_ring, int B, hipStream_t stream);
void mlp_lean_fwdapply_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                              const float* x, float* ws, int* ctr, float* stats, int stats_ring,
                              int B, int stats_on, hipStream_t stream);
void mlp_lean_head_launch(const float* p, const int* labels, float* ws, int B, hipStream_t stream,
                          const MlpDrop* drop = nullptr, int act = kMlpActSigmoid);
void mlp_pipelined_trace_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                                const float* x, const int* labels, float* ws, int* ctr,
                                float* stats, int stats_ring, int B, hipStream_t stream,
                                unsigned long long* trf, unsigned long long* trh,
                                unsigned long long* trs);
void mlp_run_pipelined_launch(float* p0, float* p1, int cur, int pending, float lr, const float* x,
                              const int* labels, int nbatches, int pos, int n, float* ws, int* ctr,
                              float* stats, int stats_ring, int B, hipStream_t stream, int flush,
                              const MlpDrop* drop = nullptr, int act = kMlpActSigmoid);

// ---- momentum / Adam / learning-rate schedules inside the lean two-launch step.  kind: 1
// momentum, 2 adam; s0 / s1: the slot planes; tp: the int32[2] step pair; h0..h2:
// gpu_ps_optim.hyper_args.
struct MlpOpt {
  int kind;
  float *s0, *s1;
  int* tp;
  float h0, h1, h2;
  int sched = 0;         // != 0: the scheduled instantiations (tp heads the 8-word schedule block;
                         // kind 0 is then scheduled gradient descent)
  float* lrs = nullptr;  // their rate ring
  // wd != 0: the weight-decay / Nesterov instantiations (ops/weight_decay.py: words()).  g' =
  // g + l2 * p feeds every kind; adam's parameter also loses rate * dec * p (AdamW); momentum
  // applies rate * (na * g' + nb * accum) -- (0, 1) plain, (1, mu) Nesterov.  kind 0 is then
  // gradient descent with the step pair and no slot plane, scheduled or not.
  int wd = 0;
  float l2 = 0.f, dec = 0.f, na = 0.f, nb = 1.f;
  // ema != 0: the moving-average instantiations (ops/ema.py: words()).  se: the shadow plane (flat
  // f32 [79510], 16-byte aligned), updated in place by shadow -= (1 - d_t) * (shadow - p_new);
  // omd = 1 - decay, 0 < omd < 1; nu != 0: d_t = min(decay, (1 + t) / (10 + t)).  Every kind
  // 0..2, scheduled or not, with or without the weight-decay words (kind 0: the step pair and no
  // slot plane).
  int ema = 0;
  float* se = nullptr;
  float omd = 0.f;
  int nu = 0;
};
void mlp_lean_fwdapply_opt_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                                  const float* x, float* ws, int* ctr, float* stats,
                                  int stats_ring, int B, int apply, int par, const MlpOpt& o,
                                  hipStream_t stream);
void mlp_apply_opt_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                          float* ws, int* ctr, float* stats, int stats_ring, int B, int par,
                          const MlpOpt& o, hipStream_t stream);
void mlp_run_pipelined_opt_launch(float* p0, float* p1, int cur, int pending, float lr,
                                  const float* x, const int* labels, int nbatches, int pos, int n,
                                  float* ws, int* ctr, float* stats, int stats_ring, int B,
                                  hipStream_t stream, int flush, const MlpOpt& o,
                                  const MlpDrop* drop = nullptr, int act = kMlpActSigmoid);
void mlp_lr_sched_launch(const int* ctr, const int* blk, float lr0, float* out, float* lrs,
                         int ring, hipStream_t stream);

// ---- data-parallel engines (MlpXg: xgmi.h).  lr already divided by the world size.
// Three-launch fused engine: mlp_wgrad with the gradient exchange in its epilogue.
void mlp_wgrad_xg_launch(float* p, float lr, const float* x, float* ws, int* ctr, float* stats,
                         int stats_ring, int B, hipStream_t stream, const MlpXg& xg, int world);
// Factor engine (sufficient-factor exchange): head launch that all-gathers the backprop
// factors dz1 of every rank into dz1A [world][112][BP], then the weight-gradient launch that
// forms the global dW1 from them and every rank's (resident) batch x, applying directly.
void mlp_head_xg_launch(const float* p, const int* labels, float* ws, float* dz1A, int B,
                        hipStream_t stream, const MlpXg& xg, int world, int nslab = 7);
void mlp_wgrad_factor_launch(float* p, float lr, const float* x, long long xstride,
                             const float* dz1A, float* ws, int* ctr, float* stats, int stats_ring,
                             int B, hipStream_t stream, const MlpXg& xg, int world);
// Pipelined factor engine: step t-1's global W1 update (from dz1A and every rank's x_prev)
// fused with step t's forward (head of step t: mlp_head_xg_launch with nslab = 14).
void mlp_fwdapply_factor_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                                const float* x, long long xstride, const float* dz1A, float* ws,
                                int* ctr, float* stats, int stats_ring, int B, int stats_on,
                                hipStream_t stream, const MlpXg& xg, int world);
// Pipelined fused engine: step t-1's local W1/W2/b gradient tiles exchanged and applied
// (p_old -> p_new) in the launch that runs step t's forward; the head is mlp_head2_launch with
// nslab = 28.  two_shot: the W1 tiles' exchange as reduce-scatter + all-gather (xg_exchange2):
// 2 (W-1)/W words per element per rank instead of W-1 (needs the push layout's result region)
void mlp_fwdapply_xg_launch(const float* p_old, float* p_new, float lr, const float* x_prev,
                            const float* x, float* ws, int* ctr, float* stats, int stats_ring,
                            int B, int stats_on, hipStream_t stream, const MlpXg& xg, int world,
                            int two_shot = 0, unsigned long long* trace = nullptr);

// ---- async parameter-server worker step (pinned host buffers: *_host)
void mlp_ps_worker_step(float* p, const float* pulled_host, float* pull_dev, const float* x_host,
                        const int* y_host, float* x_dev, int* y_dev, float* grad, float* ws,
                        int* ctr, float* stats, int stats_ring, const float* record, int B,
                        float* grad_dev, float* grad_host, hipStream_t s);
void mlp_ps_stage(const float* x_host, const int* y_host, float* x_dev, int* y_dev, int B,
                  hipStream_t s);

// ---- the step's siblings on the same model: the persistent engine (mlp_persistent.hip) and the
// fused evaluation kernel (mlp_eval.hip)
long long mlp_persistent_ll_words();
int mlp_persistent_blocks();
int mlp_persistent_trace_steps();
void mlp_persistent_launch(float* p, const float* x, const int* labels, int nbatches, int pos,
                           int steps, float lr, unsigned ebase, unsigned long long* ll, int* ctr,
                           float* stats, int ring, int B, long long ticks,
                           unsigned long long* trace, hipStream_t stream);
int mlp_eval_acc_bytes();
int mlp_eval_row_tile();
int mlp_eval_max_rows();
void mlp_eval_launch(const float* p, const float* x, const int* labels, int n, void* acc, int* pred,
                     float* probs, hipStream_t stream, int act = kMlpActSigmoid);

}  // namespace dtfx
