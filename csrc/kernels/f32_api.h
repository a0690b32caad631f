// Host API of the f32 tier's small kernel files (calibration probes, the f32 GEMM, the softmax
// cross-entropy, optimizers, activations, the row shuffle): declared ONCE for the defining files
// and the Python bindings (bindings.cpp).  Plain C++: no kernel, no device code.  Pointers are
// device addresses; *_ptr arguments, when non-null, override the scalar beside them.
#pragma once
#include <hip/hip_runtime.h>

namespace dtfx {

// ---- calib.hip
void calib_launch(int mode, int grid, int block, const int* ctr, const float* data, float* out,
                  hipStream_t s);
void clock_probe_launch(int iters, int grid, unsigned long long* out2, float* sink, hipStream_t s);

// ---- gemm_f32.hip
void gemm_f32_launch(bool ta, bool tb, int M, int N, int K, float alpha, const float* A, int lda,
                     const float* B, int ldb, float beta, float* C, int ldc, const float* bias,
                     int act, const float* aux, int ldaux, bool act_grad, hipStream_t stream);
void colsum_launch(int M, int N, const float* G, int ldg, float beta, float* out,
                   hipStream_t stream);

// ---- softmax_xent.hip
void softmax_xent_launch(int N, int C, const float* logits, int ldl, const int* lab_idx,
                         const float* lab_dense, int ldy, int ignore_index, float scale,
                         float* loss, float* dlogits, int ldd, float* correct, float* probs,
                         hipStream_t stream);

// ---- optim.hip
void sgd_launch(long long n, float* p, const float* g, float lr, const float* lr_ptr, float wd,
                hipStream_t s);
void momentum_launch(long long n, float* p, const float* g, float* v, float lr, const float* lr_ptr,
                     float mu, float wd, bool nesterov, hipStream_t s);
void adam_launch(long long n, float* p, const float* g, float* m, float* v, float lr,
                 const float* lr_ptr, float b1, float b2, float eps, float wd, bool adamw, int step,
                 const int* step_ptr, hipStream_t s);
void ema_launch(long long n, float* shadow, const float* p, float omd, bool num_updates, int step,
                const int* step_ptr, hipStream_t s);
void scale_launch(long long n, float* x, float a, hipStream_t s);
void counter_add_launch(int* c, int d, hipStream_t s);
void philox_init_launch(long long n, float* out, unsigned long long seed, unsigned long long offset,
                        int mode, float a, float b, hipStream_t s);

// ---- elementwise.hip
void act_fwd_launch(long long n, int act, const float* x, float* y, hipStream_t st);
void act_bwd_launch(long long n, int act, const float* dy, const float* s, float* dz,
                    hipStream_t st);

// ---- shuffle.hip
void shuffle_rows_launch(float* dst, const float* src, int* dst_labels, const int* src_labels,
                         long long n, int planes, long long dst_stride, long long src_stride,
                         unsigned seed, unsigned epoch, hipStream_t stream);

}  // namespace dtfx
