// Python bindings of the gfx950 kernel launchers (module `_hip`).
//
// The binding deliberately takes raw device addresses and a hipStream_t handle
// (Python passes tensor.data_ptr() and torch.cuda.current_stream().cuda_stream)
// instead of including torch headers: the module then builds in seconds, has
// no C++ ABI coupling to the torch build, and every launch lands on whatever
// stream the caller is on, including a stream under hipGraph capture.
// Shape/dtype/device validation lives in the Python wrappers
// (distributedtensorflowexample_amd/ops/).
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "f32_api.h"
#include "mlp_step_api.h"

namespace py = pybind11;

void register_rccl(py::module_& m);
void register_nn(py::module_& m);
void register_xgmi(py::module_& m);
void register_gpu_ps(py::module_& m);

template <typename T>
static inline T* P(uintptr_t a) { return reinterpret_cast<T*>(a); }
static inline hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

PYBIND11_MODULE(_hip, m) {
  m.doc() = "gfx950 HIP kernels of distributedtensorflowexample_amd";
  m.attr("ARCH") = "gfx950";

  m.def("mlp_workspace_floats", &dtfx::mlp_workspace_floats);
  m.def("mlp_tf_layout", [](uintptr_t src, uintptr_t dst, int to_tf, uintptr_t xsrc, int extra,
                            uintptr_t s) {
    dtfx::mlp_tf_layout_launch(P<const float>(src), P<float>(dst), to_tf, P<const float>(xsrc),
                               extra, S(s));
  });
  m.def("mlp_ps_worker_step", [](uintptr_t p, uintptr_t pulled_host, uintptr_t pull_dev,
                                 uintptr_t x_host, uintptr_t y_host, uintptr_t x_dev,
                                 uintptr_t y_dev, uintptr_t grad, uintptr_t ws, uintptr_t ctr,
                                 uintptr_t stats, int ring, uintptr_t record, int B,
                                 uintptr_t grad_dev, uintptr_t grad_host, uintptr_t s) {
    dtfx::mlp_ps_worker_step(P<float>(p), P<const float>(pulled_host), P<float>(pull_dev),
                             P<const float>(x_host), P<const int>(y_host), P<float>(x_dev),
                             P<int>(y_dev), P<float>(grad), P<float>(ws), P<int>(ctr),
                             P<float>(stats), ring, P<const float>(record), B, P<float>(grad_dev),
                             P<float>(grad_host), S(s));
  }, py::call_guard<py::gil_scoped_release>(),
     "async-PS worker step: staged batch + pulled params (TF layout) in, TF-layout gradient "
     "+ loss/accuracy record out, one call (train/worker.py)");
  m.def("mlp_ps_stage", [](uintptr_t x_host, uintptr_t y_host, uintptr_t x_dev, uintptr_t y_dev,
                           int B, uintptr_t s) {
    dtfx::mlp_ps_stage(P<const float>(x_host), P<const int>(y_host), P<float>(x_dev),
                       P<int>(y_dev), B, S(s));
  });
  m.def("mlp_fwd", [](uintptr_t p_old, uintptr_t grad, float lr, uintptr_t p_new, uintptr_t x,
                      uintptr_t ws, int B, uintptr_t s, uintptr_t tr) {
    dtfx::mlp_fwd_launch(P<const float>(p_old), P<const float>(grad), lr, P<float>(p_new),
                         P<const float>(x), P<float>(ws), B, S(s), P<unsigned long long>(tr));
  }, py::arg("p_old"), py::arg("grad"), py::arg("lr"), py::arg("p_new"), py::arg("x"),
     py::arg("ws"), py::arg("B"), py::arg("stream"), py::arg("trace") = 0);
  m.def("mlp_head", [](uintptr_t p_old, uintptr_t grad, float lr, uintptr_t p_new, uintptr_t lab,
                       uintptr_t ws, int B, uintptr_t s, uintptr_t tr, int act) {
    dtfx::mlp_head_launch(P<const float>(p_old), P<const float>(grad), lr, P<float>(p_new),
                          P<const int>(lab), P<float>(ws), B, S(s), P<unsigned long long>(tr),
                          nullptr, act);
  }, py::arg("p_old"), py::arg("grad"), py::arg("lr"), py::arg("p_new"), py::arg("labels"),
     py::arg("ws"), py::arg("B"), py::arg("stream"), py::arg("trace") = 0, py::arg("act") = 0);
  // Hidden-layer dropout (ops/dropout.py): the heads' DROP forms.  ctr: the device global_step
  // counter; k0 / k1: the seed's words; thr, scale: dropout.threshold(rate); rank: the stream.
  // act (here and in mlp_head / mlp_lean_head / mlp_eval / the plans' set_act): the hidden
  // activation's id, ops/hidden_act.py (0 sigmoid, 1 relu, 2 tanh).
  m.def("mlp_head_drop", [](uintptr_t p_old, uintptr_t grad, float lr, uintptr_t p_new,
                            uintptr_t lab, uintptr_t ws, int B, uintptr_t s, uintptr_t ctr,
                            unsigned k0, unsigned k1, unsigned thr, unsigned rank, float scale,
                            int act) {
    const dtfx::MlpDrop d{P<const int>(ctr), k0, k1, thr, rank, scale};
    dtfx::mlp_head_launch(P<const float>(p_old), P<const float>(grad), lr, P<float>(p_new),
                          P<const int>(lab), P<float>(ws), B, S(s), nullptr, &d, act);
  }, py::arg("p_old"), py::arg("grad"), py::arg("lr"), py::arg("p_new"), py::arg("labels"),
     py::arg("ws"), py::arg("B"), py::arg("stream"), py::arg("ctr"), py::arg("k0"), py::arg("k1"),
     py::arg("thr"), py::arg("rank"), py::arg("scale"), py::arg("act") = 0,
     "mlp_head with inverted dropout on the hidden activation (mask: Philox of seed, *ctr, "
     "rank, row, unit)");
  m.def("mlp_lean_head_drop", [](uintptr_t p, uintptr_t lab, uintptr_t ws, int B, uintptr_t s,
                                 uintptr_t ctr, unsigned k0, unsigned k1, unsigned thr,
                                 unsigned rank, float scale, int act) {
    const dtfx::MlpDrop d{P<const int>(ctr), k0, k1, thr, rank, scale};
    dtfx::mlp_lean_head_launch(P<const float>(p), P<const int>(lab), P<float>(ws), B, S(s), &d,
                               act);
  }, py::arg("p"), py::arg("labels"), py::arg("ws"), py::arg("B"), py::arg("stream"),
     py::arg("ctr"), py::arg("k0"), py::arg("k1"), py::arg("thr"), py::arg("rank"),
     py::arg("scale"), py::arg("act") = 0, "mlp_lean_head with inverted dropout on the hidden activation");
  m.def("mlp_wgrad", [](uintptr_t p, float lr, uintptr_t grad, uintptr_t x, uintptr_t ws,
                        uintptr_t ctr, uintptr_t stats, int ring, int B, uintptr_t s,
                        uintptr_t tr) {
    dtfx::mlp_wgrad_launch(P<float>(p), lr, P<float>(grad), P<const float>(x), P<float>(ws),
                           P<int>(ctr), P<float>(stats), ring, B, S(s), P<unsigned long long>(tr));
  }, py::arg("p"), py::arg("lr"), py::arg("grad"), py::arg("x"), py::arg("ws"), py::arg("ctr"),
     py::arg("stats"), py::arg("ring"), py::arg("B"), py::arg("stream"), py::arg("trace") = 0);
  m.def("mlp_fwdapply", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                           uintptr_t x, uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring,
                           int B, int stats_on, uintptr_t s, int ks) {
    dtfx::mlp_fwdapply_launch(P<const float>(p_old), P<float>(p_new), lr, P<const float>(x_prev),
                              P<const float>(x), P<float>(ws), P<int>(ctr), P<float>(stats), ring,
                              B, stats_on, S(s), ks);
  }, py::arg("p_old"), py::arg("p_new"), py::arg("lr"), py::arg("x_prev"), py::arg("x"),
     py::arg("ws"), py::arg("ctr"), py::arg("stats"), py::arg("ring"), py::arg("B"),
     py::arg("stats_on"), py::arg("stream"), py::arg("ks") = 0,
     "first launch of the 2-launch step; ks: K slices (0: the single-GPU setting, 14, 28)");
  m.def("mlp_single_ks", &dtfx::mlp_single_ks_query,
        "K slices of the single-GPU pipelined MLP step (28, or 14 with DTFX_MLP_KS=14)");
  m.def("mlp_pipelined_trace", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                                   uintptr_t x, uintptr_t lab, uintptr_t ws, uintptr_t ctr,
                                   uintptr_t stats, int ring, int B, uintptr_t s, uintptr_t trf,
                                   uintptr_t trh, uintptr_t trs) {
    dtfx::mlp_pipelined_trace_launch(P<const float>(p_old), P<float>(p_new), lr,
                                     P<const float>(x_prev), P<const float>(x), P<const int>(lab),
                                     P<float>(ws), P<int>(ctr), P<float>(stats), ring, B, S(s),
                                     reinterpret_cast<unsigned long long*>(trf),
                                     reinterpret_cast<unsigned long long*>(trh),
                                     reinterpret_cast<unsigned long long*>(trs));
  }, py::arg("p_old"), py::arg("p_new"), py::arg("lr"), py::arg("x_prev"), py::arg("x"),
     py::arg("labels"), py::arg("ws"), py::arg("ctr"), py::arg("stats"), py::arg("ring"),
     py::arg("B"), py::arg("stream"), py::arg("trf"), py::arg("trh"), py::arg("trs") = 0,
     "one traced two-launch step; trs (optional, 28 slices): [(7 * 28 + 7) * 4][2] split stamps "
     "of the first launch (slot 0: its first-issued operand class has landed)");
  m.def("mlp_lean_fwdapply", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                                uintptr_t x, uintptr_t ws, uintptr_t ctr, uintptr_t stats,
                                int ring, int B, int stats_on, uintptr_t s) {
    dtfx::mlp_lean_fwdapply_launch(P<const float>(p_old), P<float>(p_new), lr,
                                   P<const float>(x_prev), P<const float>(x), P<float>(ws),
                                   P<int>(ctr), P<float>(stats), ring, B, stats_on, S(s));
  }, py::arg("p_old"), py::arg("p_new"), py::arg("lr"), py::arg("x_prev"), py::arg("x"),
     py::arg("ws"), py::arg("ctr"), py::arg("stats"), py::arg("ring"), py::arg("B"),
     py::arg("stats_on"), py::arg("stream"),
     "first launch of the single-GPU two-launch step: the lean kernel (packed, preloaded kernel "
     "arguments; the same results as mlp_fwdapply(ks=28)); with DTFX_MLP_KS=14 the 14-slice "
     "mlp_fwdapply");
  m.def("mlp_lean_head", [](uintptr_t p, uintptr_t lab, uintptr_t ws, int B, uintptr_t s,
                            int act) {
    dtfx::mlp_lean_head_launch(P<const float>(p), P<const int>(lab), P<float>(ws), B, S(s),
                               nullptr, act);
  }, py::arg("p"), py::arg("labels"), py::arg("ws"), py::arg("B"), py::arg("stream"),
     py::arg("act") = 0,
     "head of the single-GPU two-launch step after mlp_lean_fwdapply: row-major factors out, as "
     "mlp_head2(single=1)");
  m.def("mlp_head2", [](uintptr_t p, uintptr_t lab, uintptr_t ws, int B, uintptr_t s, int nslab,
                        int single) {
    if (single) {
      if (nslab != 0) throw std::runtime_error("mlp_head2: single=1 takes nslab=0");
      dtfx::mlp_head2_single_launch(P<const float>(p), P<const int>(lab), P<float>(ws), B, S(s));
    } else {
      dtfx::mlp_head2_launch(P<const float>(p), P<const int>(lab), P<float>(ws), B, S(s), nslab);
    }
  }, py::arg("p"), py::arg("labels"), py::arg("ws"), py::arg("B"), py::arg("stream"),
     py::arg("nslab") = 0, py::arg("single") = 0,
     "head of the 2-launch step; nslab: slabs the first launch wrote (0: the single-GPU "
     "step's, 14: every data-parallel engine's); single=1: the single-GPU step's own head, "
     "which leaves the factors row-major for the next mlp_fwdapply / mlp_apply (the default "
     "leaves them transposed, as the data-parallel engines read them)");
  m.def("wave_reduce_scatter_test", [](uintptr_t in, uintptr_t out, int n, uintptr_t s) {
    dtfx::wave_reduce_scatter_test_launch(P<const float>(in), P<float>(out), n, S(s));
  }, "one wave: in [64][n] (n = 10 or 16) -> out [64], out[l] = sum over lanes of value l & 15");
  m.def("mlp_rowmajor_layout", [](int B) {
    long long o[3];
    dtfx::mlp_rowmajor_layout(B, o);
    return py::make_tuple(o[0], o[1], o[2]);
  }, "(dz1R offset, dlR offset, BP): float offsets of the row-major factor regions dz1R "
     "[BP][112] and dlR [BP][16] in a workspace of batch B");
  m.def("mlp_run_pipelined", [](uintptr_t p0, uintptr_t p1, int cur, int pending, float lr,
                                uintptr_t x, uintptr_t lab, int nbatches, int pos, int n,
                                uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring, int B,
                                uintptr_t s, int flush, int act) {
    py::gil_scoped_release nogil;
    dtfx::mlp_run_pipelined_launch(P<float>(p0), P<float>(p1), cur, pending, lr, P<const float>(x),
                                   P<const int>(lab), nbatches, pos, n, P<float>(ws), P<int>(ctr),
                                   P<float>(stats), ring, B, S(s), flush, nullptr, act);
  }, py::arg("p0"), py::arg("p1"), py::arg("cur"), py::arg("pending"), py::arg("lr"), py::arg("x"),
     py::arg("labels"), py::arg("nbatches"), py::arg("pos"), py::arg("n"), py::arg("ws"),
     py::arg("ctr"), py::arg("stats"), py::arg("ring"), py::arg("B"), py::arg("stream"),
     py::arg("flush") = 0, py::arg("act") = 0);
  m.def("mlp_set_flush_fused", &dtfx::mlp_set_flush_fused,
        "run_launched(.., flush=True): 1 = the last step's head and the flush in one launch "
        "(mlp_head_flush_kernel; opt-in, measured slower), 0 = the flush as its own launch; "
        "returns the previous setting");
  // The C++ host loop with its fixed arguments bound once (FusedMLPTrainer.run_launched): a
  // driver-sized timed region starts on the host, so the per-call Python -> C++ argument
  // conversion of the 17-argument form sits in front of the region's first kernel.
  struct MlpRunPlan {
    float *p0, *p1;
    const float* x;
    const int* labels;
    int nbatches;
    float* ws;
    int* ctr;
    float* stats;
    int ring, B;
    dtfx::MlpDrop drop{};  // set_drop: every head of the loop drops (ctr: the plan's)
    bool has_drop = false;
    const dtfx::MlpDrop* dropp() const { return has_drop ? &drop : nullptr; }
    void set_drop(unsigned k0, unsigned k1, unsigned thr, unsigned rank, float scale) {
      drop = dtfx::MlpDrop{ctr, k0, k1, thr, rank, scale};
      has_drop = true;
    }
    int act = 0;  // set_act: the hidden activation of every head of the loop
    void set_act(int a) { act = a; }
  };
  static const auto bound = [](uintptr_t p0, uintptr_t p1, uintptr_t x, uintptr_t lab, int nbatches,
                               uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring, int B) {
    return MlpRunPlan{P<float>(p0), P<float>(p1), P<const float>(x), P<const int>(lab),
                      nbatches, P<float>(ws), P<int>(ctr), P<float>(stats), ring, B};
  };
  py::class_<MlpRunPlan>(m, "MlpRunPlan")
      .def(py::init(bound))
      .def("run", [](const MlpRunPlan& p, int cur, int pending, float lr, int pos, int n,
                     int flush, uintptr_t s) {
        py::gil_scoped_release nogil;
        dtfx::mlp_run_pipelined_launch(p.p0, p.p1, cur, pending, lr, p.x, p.labels, p.nbatches,
                                       pos, n, p.ws, p.ctr, p.stats, p.ring, p.B, S(s), flush,
                                       p.dropp(), p.act);
      }, "(cur, pending, lr, pos, n, flush, stream): mlp_run_pipelined with the bound buffers")
      .def("set_drop", &MlpRunPlan::set_drop,
           "(k0, k1, thr, rank, scale): hidden-layer dropout in every head of the loop")
      .def("set_act", &MlpRunPlan::set_act,
           "(act): the hidden activation of every head of the loop (0 sigmoid, 1 relu, 2 tanh)");
  m.def("mlp_apply", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev, uintptr_t ws,
                        uintptr_t ctr, uintptr_t stats, int ring, int B, uintptr_t s) {
    dtfx::mlp_apply_launch(P<const float>(p_old), P<float>(p_new), lr, P<const float>(x_prev),
                           P<float>(ws), P<int>(ctr), P<float>(stats), ring, B, S(s));
  });
  // Momentum / Adam inside the two-launch step.  kind: 1 momentum, 2 adam; s0 / s1: slot planes
  // (s1: adam only, else 0); tp: the int32[2] step pair; h0..h2: gpu_ps_optim.hyper_args; par:
  // the index of p_old in the ping-pong pair.
  m.def("mlp_lean_fwdapply_opt", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                                    uintptr_t x, uintptr_t ws, uintptr_t ctr, uintptr_t stats,
                                    int ring, int B, int apply, int par, int kind, uintptr_t s0,
                                    uintptr_t s1, uintptr_t tp, float h0, float h1, float h2,
                                    uintptr_t s) {
    dtfx::mlp_lean_fwdapply_opt_launch(
        P<const float>(p_old), P<float>(p_new), lr, P<const float>(x_prev), P<const float>(x),
        P<float>(ws), P<int>(ctr), P<float>(stats), ring, B, apply, par,
        dtfx::MlpOpt{kind, P<float>(s0), P<float>(s1), P<int>(tp), h0, h1, h2}, S(s));
  }, py::arg("p_old"), py::arg("p_new"), py::arg("lr"), py::arg("x_prev"), py::arg("x"),
     py::arg("ws"), py::arg("ctr"), py::arg("stats"), py::arg("ring"), py::arg("B"),
     py::arg("apply"), py::arg("par"), py::arg("kind"), py::arg("s0"), py::arg("s1"),
     py::arg("tp"), py::arg("h0"), py::arg("h1"), py::arg("h2"), py::arg("stream"),
     "first launch of the two-launch step with momentum (kind 1) or adam (kind 2): applies the "
     "pending update to the parameters and the slot planes (apply=0: copy, slots untouched) and "
     "runs the forward; mlp_lean_head finishes the step");
  m.def("mlp_apply_opt", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                            uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring, int B, int par,
                            int kind, uintptr_t s0, uintptr_t s1, uintptr_t tp, float h0, float h1,
                            float h2, uintptr_t s) {
    dtfx::mlp_apply_opt_launch(
        P<const float>(p_old), P<float>(p_new), lr, P<const float>(x_prev), P<float>(ws),
        P<int>(ctr), P<float>(stats), ring, B, par,
        dtfx::MlpOpt{kind, P<float>(s0), P<float>(s1), P<int>(tp), h0, h1, h2}, S(s));
  }, "the flush of mlp_lean_fwdapply_opt: the pending update alone, p_old -> p_new");
  // The same two launches with a learning-rate schedule evaluated on the device
  // (ops/lr_schedule.py): kind 0 (sgd), 1, 2; blk: the int32[8] schedule block whose first two
  // words are the step pair; lr: the base rate; lrs: the f32 rate ring (length `ring`), or 0.
  m.def("mlp_lean_fwdapply_sched", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                                      uintptr_t x, uintptr_t ws, uintptr_t ctr, uintptr_t stats,
                                      int ring, int B, int apply, int par, int kind, uintptr_t s0,
                                      uintptr_t s1, uintptr_t blk, float h0, float h1, float h2,
                                      uintptr_t lrs, uintptr_t s) {
    dtfx::mlp_lean_fwdapply_opt_launch(
        P<const float>(p_old), P<float>(p_new), lr, P<const float>(x_prev), P<const float>(x),
        P<float>(ws), P<int>(ctr), P<float>(stats), ring, B, apply, par,
        dtfx::MlpOpt{kind, P<float>(s0), P<float>(s1), P<int>(blk), h0, h1, h2, 1, P<float>(lrs)},
        S(s));
  }, "mlp_lean_fwdapply_opt with the rate of the applied step computed in the kernel from the "
     "schedule block (and published to the rate ring)");
  m.def("mlp_apply_sched", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                              uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring, int B,
                              int par, int kind, uintptr_t s0, uintptr_t s1, uintptr_t blk,
                              float h0, float h1, float h2, uintptr_t lrs, uintptr_t s) {
    dtfx::mlp_apply_opt_launch(
        P<const float>(p_old), P<float>(p_new), lr, P<const float>(x_prev), P<float>(ws),
        P<int>(ctr), P<float>(stats), ring, B, par,
        dtfx::MlpOpt{kind, P<float>(s0), P<float>(s1), P<int>(blk), h0, h1, h2, 1, P<float>(lrs)},
        S(s));
  }, "the flush of mlp_lean_fwdapply_sched");
  // The same two launches with weight decay / Nesterov momentum (ops/weight_decay.py): kind 0
  // (sgd), 1, 2; sched != 0: tp is the schedule block and lrs the rate ring, else the plain step
  // pair and lrs = 0; l2, dec, na, nb: WeightDecay.words().
  static const auto wd_opt = [](int kind, uintptr_t s0, uintptr_t s1, uintptr_t tp, float h0,
                                float h1, float h2, int sched, uintptr_t lrs, float l2, float dec,
                                float na, float nb) {
    return dtfx::MlpOpt{kind, P<float>(s0), P<float>(s1), P<int>(tp), h0, h1, h2, sched ? 1 : 0,
                        P<float>(lrs), 1, l2, dec, na, nb};
  };
  m.def("mlp_lean_fwdapply_wd", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                                   uintptr_t x, uintptr_t ws, uintptr_t ctr, uintptr_t stats,
                                   int ring, int B, int apply, int par, int kind, uintptr_t s0,
                                   uintptr_t s1, uintptr_t tp, float h0, float h1, float h2,
                                   int sched, uintptr_t lrs, float l2, float dec, float na,
                                   float nb, uintptr_t s) {
    dtfx::mlp_lean_fwdapply_opt_launch(
        P<const float>(p_old), P<float>(p_new), lr, P<const float>(x_prev), P<const float>(x),
        P<float>(ws), P<int>(ctr), P<float>(stats), ring, B, apply, par,
        wd_opt(kind, s0, s1, tp, h0, h1, h2, sched, lrs, l2, dec, na, nb), S(s));
  }, "mlp_lean_fwdapply_opt / _sched with weight decay (L2 or decoupled) and Nesterov momentum "
     "in the owning lane's update; apply=0 is still a pure copy");
  m.def("mlp_apply_wd", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                           uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring, int B, int par,
                           int kind, uintptr_t s0, uintptr_t s1, uintptr_t tp, float h0, float h1,
                           float h2, int sched, uintptr_t lrs, float l2, float dec, float na,
                           float nb, uintptr_t s) {
    dtfx::mlp_apply_opt_launch(
        P<const float>(p_old), P<float>(p_new), lr, P<const float>(x_prev), P<float>(ws),
        P<int>(ctr), P<float>(stats), ring, B, par,
        wd_opt(kind, s0, s1, tp, h0, h1, h2, sched, lrs, l2, dec, na, nb), S(s));
  }, "the flush of mlp_lean_fwdapply_wd");
  // The same two launches with a moving average of the parameters (ops/ema.py): the weight-decay
  // form's arguments (without decay: l2, dec, na, nb = 0, 0, 0, 1), then the shadow plane se, omd =
  // 1 - decay and the num_updates flag.
  static const auto ema_opt = [](int kind, uintptr_t s0, uintptr_t s1, uintptr_t tp, float h0,
                                 float h1, float h2, int sched, uintptr_t lrs, float l2, float dec,
                                 float na, float nb, uintptr_t se, float omd, int nu) {
    dtfx::MlpOpt o = wd_opt(kind, s0, s1, tp, h0, h1, h2, sched, lrs, l2, dec, na, nb);
    o.ema = 1, o.se = P<float>(se), o.omd = omd, o.nu = nu ? 1 : 0;
    return o;
  };
  m.def("mlp_lean_fwdapply_ema", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                                    uintptr_t x, uintptr_t ws, uintptr_t ctr, uintptr_t stats,
                                    int ring, int B, int apply, int par, int kind, uintptr_t s0,
                                    uintptr_t s1, uintptr_t tp, float h0, float h1, float h2,
                                    int sched, uintptr_t lrs, float l2, float dec, float na,
                                    float nb, uintptr_t se, float omd, int nu, uintptr_t s) {
    dtfx::mlp_lean_fwdapply_opt_launch(
        P<const float>(p_old), P<float>(p_new), lr, P<const float>(x_prev), P<const float>(x),
        P<float>(ws), P<int>(ctr), P<float>(stats), ring, B, apply, par,
        ema_opt(kind, s0, s1, tp, h0, h1, h2, sched, lrs, l2, dec, na, nb, se, omd, nu), S(s));
  }, "mlp_lean_fwdapply_wd that also updates the shadow plane se in place: shadow -= (1 - d_t) * "
     "(shadow - p_new) by the lane that stores p_new; apply=0 touches no shadow byte");
  m.def("mlp_apply_ema", [](uintptr_t p_old, uintptr_t p_new, float lr, uintptr_t x_prev,
                            uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring, int B, int par,
                            int kind, uintptr_t s0, uintptr_t s1, uintptr_t tp, float h0, float h1,
                            float h2, int sched, uintptr_t lrs, float l2, float dec, float na,
                            float nb, uintptr_t se, float omd, int nu, uintptr_t s) {
    dtfx::mlp_apply_opt_launch(
        P<const float>(p_old), P<float>(p_new), lr, P<const float>(x_prev), P<float>(ws),
        P<int>(ctr), P<float>(stats), ring, B, par,
        ema_opt(kind, s0, s1, tp, h0, h1, h2, sched, lrs, l2, dec, na, nb, se, omd, nu), S(s));
  }, "the flush of mlp_lean_fwdapply_ema");
  m.def("mlp_lr_sched", [](uintptr_t ctr, uintptr_t blk, float lr0, uintptr_t out, uintptr_t lrs,
                           int ring, uintptr_t s) {
    dtfx::mlp_lr_sched_launch(P<const int>(ctr), P<const int>(blk), lr0, P<float>(out),
                              P<float>(lrs), ring, S(s));
  }, "one wave: the scheduled rate of step ctr - 1 into out[0] (ops.optim's lr_tensor) and, with "
     "lrs != 0, into the rate ring");
  struct MlpRunOptPlan : MlpRunPlan {  // the same bound buffers, and the optimizer's
    dtfx::MlpOpt opt;
  };
  py::class_<MlpRunOptPlan>(m, "MlpRunOptPlan")
      .def(py::init([](uintptr_t p0, uintptr_t p1, uintptr_t x, uintptr_t lab, int nbatches,
                       uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring, int B, int kind,
                       uintptr_t s0, uintptr_t s1, uintptr_t tp, float h0, float h1, float h2) {
        return MlpRunOptPlan{bound(p0, p1, x, lab, nbatches, ws, ctr, stats, ring, B),
                             dtfx::MlpOpt{kind, P<float>(s0), P<float>(s1), P<int>(tp), h0, h1,
                                          h2}};
      }))
      .def(py::init([](uintptr_t p0, uintptr_t p1, uintptr_t x, uintptr_t lab, int nbatches,
                       uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring, int B, int kind,
                       uintptr_t s0, uintptr_t s1, uintptr_t blk, float h0, float h1, float h2,
                       uintptr_t lrs) {  // the scheduled form (mlp_lean_fwdapply_sched)
        return MlpRunOptPlan{bound(p0, p1, x, lab, nbatches, ws, ctr, stats, ring, B),
                             dtfx::MlpOpt{kind, P<float>(s0), P<float>(s1), P<int>(blk), h0, h1,
                                          h2, 1, P<float>(lrs)}};
      }))
      .def(py::init([](uintptr_t p0, uintptr_t p1, uintptr_t x, uintptr_t lab, int nbatches,
                       uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring, int B, int kind,
                       uintptr_t s0, uintptr_t s1, uintptr_t tp, float h0, float h1, float h2,
                       int sched, uintptr_t lrs, float l2, float dec, float na, float nb) {
        // the weight-decay / Nesterov form (mlp_lean_fwdapply_wd)
        return MlpRunOptPlan{bound(p0, p1, x, lab, nbatches, ws, ctr, stats, ring, B),
                             wd_opt(kind, s0, s1, tp, h0, h1, h2, sched, lrs, l2, dec, na, nb)};
      }))
      .def(py::init([](uintptr_t p0, uintptr_t p1, uintptr_t x, uintptr_t lab, int nbatches,
                       uintptr_t ws, uintptr_t ctr, uintptr_t stats, int ring, int B, int kind,
                       uintptr_t s0, uintptr_t s1, uintptr_t tp, float h0, float h1, float h2,
                       int sched, uintptr_t lrs, float l2, float dec, float na, float nb,
                       uintptr_t se, float omd, int nu) {
        // the moving-average form (mlp_lean_fwdapply_ema)
        return MlpRunOptPlan{bound(p0, p1, x, lab, nbatches, ws, ctr, stats, ring, B),
                             ema_opt(kind, s0, s1, tp, h0, h1, h2, sched, lrs, l2, dec, na, nb, se,
                                     omd, nu)};
      }))
      .def("run", [](const MlpRunOptPlan& p, int cur, int pending, float lr, int pos, int n,
                     int flush, uintptr_t s) {
        py::gil_scoped_release nogil;
        dtfx::mlp_run_pipelined_opt_launch(p.p0, p.p1, cur, pending, lr, p.x, p.labels,
                                           p.nbatches, pos, n, p.ws, p.ctr, p.stats, p.ring, p.B,
                                           S(s), flush, p.opt, p.dropp(), p.act);
      }, "(cur, pending, lr, pos, n, flush, stream): the C++ host loop of the two-launch step "
         "with momentum / adam over the bound buffers (MlpRunPlan's call)")
      .def("set_drop", [](MlpRunOptPlan& p, unsigned k0, unsigned k1, unsigned thr, unsigned rank,
                          float scale) { p.set_drop(k0, k1, thr, rank, scale); },
           "(k0, k1, thr, rank, scale): hidden-layer dropout in every head of the loop")
      .def("set_act", [](MlpRunOptPlan& p, int a) { p.set_act(a); },
           "(act): the hidden activation of every head of the loop (0 sigmoid, 1 relu, 2 tanh)");
  m.def("mlp_persistent_ll_words", &dtfx::mlp_persistent_ll_words);
  m.def("mlp_persistent_blocks", &dtfx::mlp_persistent_blocks);
  m.def("mlp_persistent_trace_steps", &dtfx::mlp_persistent_trace_steps);
  m.def("mlp_persistent", [](uintptr_t p, uintptr_t x, uintptr_t lab, int nbatches, int pos,
                             int steps, float lr, unsigned ebase, uintptr_t ll, uintptr_t ctr,
                             uintptr_t stats, int ring, int B, long long ticks, uintptr_t s,
                             uintptr_t trace) {
    py::gil_scoped_release nogil;
    dtfx::mlp_persistent_launch(P<float>(p), P<const float>(x), P<const int>(lab), nbatches, pos,
                                steps, lr, ebase, P<unsigned long long>(ll), P<int>(ctr),
                                P<float>(stats), ring, B, ticks, P<unsigned long long>(trace),
                                S(s));
  }, py::arg("p"), py::arg("x"), py::arg("labels"), py::arg("nbatches"), py::arg("pos"),
     py::arg("steps"), py::arg("lr"), py::arg("ebase"), py::arg("ll"), py::arg("ctr"),
     py::arg("stats"), py::arg("ring"), py::arg("B"), py::arg("ticks"), py::arg("stream"),
     py::arg("trace") = 0);
  m.def("gemm_f32", [](bool ta, bool tb, int M, int N, int K, float alpha, uintptr_t A, int lda,
                       uintptr_t B, int ldb, float beta, uintptr_t C, int ldc, uintptr_t bias,
                       int act, uintptr_t aux, int ldaux, bool act_grad, uintptr_t s) {
    dtfx::gemm_f32_launch(ta, tb, M, N, K, alpha, P<const float>(A), lda, P<const float>(B), ldb,
                          beta, P<float>(C), ldc, P<const float>(bias), act, P<const float>(aux),
                          ldaux, act_grad, S(s));
  });
  m.def("colsum", [](int M, int N, uintptr_t G, int ldg, float beta, uintptr_t out, uintptr_t s) {
    dtfx::colsum_launch(M, N, P<const float>(G), ldg, beta, P<float>(out), S(s));
  });
  m.def("softmax_xent", [](int N, int C, uintptr_t logits, int ldl, uintptr_t lab_idx,
                           uintptr_t lab_dense, int ldy, int ignore, float scale, uintptr_t loss,
                           uintptr_t dlogits, int ldd, uintptr_t correct, uintptr_t probs,
                           uintptr_t s) {
    dtfx::softmax_xent_launch(N, C, P<const float>(logits), ldl, P<const int>(lab_idx),
                              P<const float>(lab_dense), ldy, ignore, scale, P<float>(loss),
                              P<float>(dlogits), ldd, P<float>(correct), P<float>(probs), S(s));
  });
  m.def("sgd", [](long long n, uintptr_t p, uintptr_t g, float lr, uintptr_t lr_ptr, float wd,
                  uintptr_t s) {
    dtfx::sgd_launch(n, P<float>(p), P<const float>(g), lr, P<const float>(lr_ptr), wd, S(s));
  });
  m.def("momentum", [](long long n, uintptr_t p, uintptr_t g, uintptr_t v, float lr,
                       uintptr_t lr_ptr, float mu, float wd, bool nesterov, uintptr_t s) {
    dtfx::momentum_launch(n, P<float>(p), P<const float>(g), P<float>(v), lr,
                          P<const float>(lr_ptr), mu, wd, nesterov, S(s));
  });
  m.def("adam", [](long long n, uintptr_t p, uintptr_t g, uintptr_t mm, uintptr_t v, float lr,
                   uintptr_t lr_ptr, float b1, float b2, float eps, float wd, bool adamw, int step,
                   uintptr_t step_ptr, uintptr_t s) {
    dtfx::adam_launch(n, P<float>(p), P<const float>(g), P<float>(mm), P<float>(v), lr,
                      P<const float>(lr_ptr), b1, b2, eps, wd, adamw, step, P<const int>(step_ptr),
                      S(s));
  });
  m.def("ema", [](long long n, uintptr_t shadow, uintptr_t p, float omd, bool num_updates, int step,
                  uintptr_t step_ptr, uintptr_t s) {
    dtfx::ema_launch(n, P<float>(shadow), P<const float>(p), omd, num_updates, step,
                     P<const int>(step_ptr), S(s));
  }, "shadow -= (1 - d_t) * (shadow - p) in place (omd = 1 - decay; num_updates: d_t = "
     "min(decay, (1 + t) / (10 + t)), t = *step_ptr or step)");
  m.def("scale", [](long long n, uintptr_t x, float a, uintptr_t s) {
    dtfx::scale_launch(n, P<float>(x), a, S(s));
  });
  m.def("counter_add", [](uintptr_t c, int d, uintptr_t s) {
    dtfx::counter_add_launch(P<int>(c), d, S(s));
  });
  m.def("philox_init", [](long long n, uintptr_t out, unsigned long long seed,
                          unsigned long long offset, int mode, float a, float b, uintptr_t s) {
    dtfx::philox_init_launch(n, P<float>(out), seed, offset, mode, a, b, S(s));
  });
  m.def("act_bwd", [](long long n, int act, uintptr_t dy, uintptr_t sv, uintptr_t dz,
                      uintptr_t s) {
    dtfx::act_bwd_launch(n, act, P<const float>(dy), P<const float>(sv), P<float>(dz), S(s));
  });
  m.def("act_fwd", [](long long n, int act, uintptr_t x, uintptr_t y, uintptr_t s) {
    dtfx::act_fwd_launch(n, act, P<const float>(x), P<float>(y), S(s));
  });
  m.def("shuffle_rows", [](uintptr_t dst, uintptr_t src, uintptr_t dst_lab, uintptr_t src_lab,
                           long long n, int planes, long long dst_stride, long long src_stride,
                           unsigned seed, unsigned epoch, uintptr_t s) {
    dtfx::shuffle_rows_launch(P<float>(dst), P<const float>(src), P<int>(dst_lab),
                              P<const int>(src_lab), n, planes, dst_stride, src_stride, seed, epoch,
                              S(s));
  }, py::arg("dst"), py::arg("src"), py::arg("dst_labels"), py::arg("src_labels"), py::arg("n"),
     py::arg("planes"), py::arg("dst_stride"), py::arg("src_stride"), py::arg("seed"),
     py::arg("epoch"), py::arg("stream"),
     "per-epoch reshuffle gather: dst[w][j] = src[w][perm(seed, epoch, n)[j]] over `planes` "
     "planes of [n, 784] f32 (strides in floats) and the int32 labels (csrc/kernels/shuffle.hip)");
  m.def("mlp_eval", [](uintptr_t p, uintptr_t x, uintptr_t lab, int n, uintptr_t acc,
                        uintptr_t pred, uintptr_t probs, uintptr_t s, int act) {
    dtfx::mlp_eval_launch(P<const float>(p), P<const float>(x), P<const int>(lab), n, P<void>(acc),
                          P<int>(pred), P<float>(probs), S(s), act);
  }, py::arg("p"), py::arg("x"), py::arg("labels"), py::arg("n"), py::arg("acc"), py::arg("pred"),
     py::arg("probs"), py::arg("stream"), py::arg("act") = 0,
     "fused evaluation of the 784-100-10 MLP on n rows (csrc/kernels/mlp_eval.hip): pred int32 "
     "[n] / probs f32 [n, 10] optional (0); labels 0: predict only, acc untouched; otherwise acc "
     "(mlp_eval_acc_bytes bytes) is zeroed on the stream and then accumulated");
  m.def("mlp_eval_acc_bytes", &dtfx::mlp_eval_acc_bytes,
        "bytes of the accumulator block: int64 loss sum (2^-32 units), int32 correct, int32 "
        "count, int32 confusion [10][10] indexed [label][predicted]");
  m.def("mlp_eval_row_tile", &dtfx::mlp_eval_row_tile, "rows per workgroup of mlp_eval");
  m.def("mlp_eval_max_rows", &dtfx::mlp_eval_max_rows,
        "largest n of mlp_eval (the fixed-point loss sum cannot overflow up to it)");
  m.def("calib", [](int mode, int grid, int block, uintptr_t ctr, uintptr_t data, uintptr_t out,
                    uintptr_t s) {
    dtfx::calib_launch(mode, grid, block, P<const int>(ctr), P<const float>(data), P<float>(out),
                       S(s));
  });
  m.def("clock_probe", [](int iters, int grid, uintptr_t out2, uintptr_t sink, uintptr_t s) {
    dtfx::clock_probe_launch(iters, grid, P<unsigned long long>(out2), P<float>(sink), S(s));
  });
  register_rccl(m);
  register_nn(m);
  register_xgmi(m);
  register_gpu_ps(m);
  m.def("device_count", []() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
  });
}
