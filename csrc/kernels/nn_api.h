// Host API of the bf16 tier (BERT-base / ResNet-50 path): every function its kernel files export,
// declared ONCE for the defining files and the Python bindings (bindings_nn.cpp).  Plain C++: no
// kernel, no device code.  Pointers are device addresses; `const void*` / `void*` are bf16 arrays,
// `float*` f32.  The comments at the definitions say what each launch computes.
#pragma once
#include <hip/hip_runtime.h>

namespace dtfx {

// ---- transformer.hip: LayerNorm
void ln_bwd_set_slots(int v);
void ln_bwd_set_h768(int v);
void layernorm_fwd_launch(int T, int H, const void* x, const float* gamma, const float* beta,
                          float eps, void* y, float* mean, float* rstd, hipStream_t s);
void layernorm_bwd_launch(int T, int H, const void* dy, const void* x, const float* mean,
                          const float* rstd, const float* gamma, const void* dres, void* dx,
                          float* dgamma, float* dbeta, float* dxsum, hipStream_t s);

// ---- transformer.hip: embeddings
void embed_ln_fwd_launch(int T, int S, int H, const int* ids, const int* tt, const void* word,
                         const void* pos, const void* type, const float* gamma, const float* beta,
                         float eps, void* xsum, void* y, float* mean, float* rstd, hipStream_t s);
void embed_bwd_launch(int Bn, int S, int H, const int* ids, const int* tt, const void* dx,
                      float* dword, float* dpos, float* dtype_, hipStream_t s);

// ---- transformer.hip: dense attention
void attn_set_swizzle(int v);
void attn_fwd_set_variant(int v);
void attn_bwd_set_pf(int v);
void attn_bwd_set_variant(int v);
void attn_fwd_launch(int Bn, int S, int nh, const void* qkv, void* out, float* lse,
                     const float* kmask, float scale, hipStream_t s);
void attn_bwd_launch(int Bn, int S, int nh, const void* qkv, const void* o, const void* dout,
                     const float* lse, const float* kmask, float scale, void* dqkv, float* dbias,
                     hipStream_t s);

// ---- flash_attn.hip
void flash_fwd_launch(int Bn, int S, int nh, const void* qkv, void* out, float* lse, int ld_lse,
                      const float* kmask, float scale, hipStream_t st);
void flash_bwd_launch(int Bn, int S, int nh, const void* qkv, const void* o, const void* dout,
                      const float* lse, int ld_lse, const float* kmask, float scale, void* dqkv,
                      float* dbias, float* scratch_D, hipStream_t st);

// ---- transformer.hip: MLM cross-entropy
void xent_set_regs(int v);
void mlm_xent_launch(int N, int C, const void* logits, bool logits_bf16, int ldl, const int* labels,
                     float scale, float* loss, float* correct, void* dl, int ldd, hipStream_t s);

// ---- transformer.hip: mixed Adam, range zeroing, cast, activation gradient
void adam_mixed_launch(long long n, float* p, const float* g, float* m, float* v, void* pb,
                       float lr, float b1, float b2, float eps, float wd, float gscale,
                       const int* step_ptr, int step, hipStream_t s, const long long* segs,
                       int nseg, long long base4);
void zero_ranges_launch(const long long* tab, int n, long long total, hipStream_t s);
void cast_f32_bf16_launch(long long n, const float* x, void* y, hipStream_t s);
void act_grad_bf16_launch(long long n, int act, const void* dy, const void* u, void* dx,
                          hipStream_t s);

// ---- gemm_bf16.hip
void gemm_bf16_set_cfg(int cfg);
int gemm_bf16_set_pers(int on);
void colsum_set_rows_in_flight(int u);
void gemm_bf16_launch(bool ta, bool tb, bool out_f32, int M, int N, int K, const void* A, int lda,
                      const void* B, int ldb, void* C, int ldc, float alpha, float beta,
                      const float* bias, int act, const void* aux_in, void* aux_out, int ld_aux,
                      const void* residual, int ld_res, int act_grad, int splitk, int batch,
                      long long sA, long long sB, long long sC, float* colsum, hipStream_t stream,
                      float* ws, long long ws_floats, bool defer_reduce);
void colsum_bf16_launch(const void* G, int M, int N, int ldg, float* out, float beta,
                        hipStream_t stream);
long long gemm_bf16_ws_floats(bool ta, bool out_f32, int M, int N, int K, int splitk, float beta);
long long conv_wgrad_ws_floats(int N, int H, int W, int C, int Cout, int KH, int KW, int stride,
                               int pad);
long long conv_splitk_ws_floats(int mode, int N, int H, int W, int C, int Cout, int KH, int KW,
                                int stride, int pad);
void conv_bf16_launch(int mode, int N, int H, int W, int C, int Cout, int KH, int KW, int stride,
                      int pad, const void* a, const void* b, int ldw, void* out, float beta,
                      const void* residual, float* colsum, float* colsq, int splitk,
                      hipStream_t stream, const void* relu_y, const void* bn_x,
                      const float* bn_mean, const float* bn_rstd, float* ws, long long ws_floats,
                      int defer_reduce);

// ---- cnn.hip
void bn_finalize_launch(int C, long long M, const float* s, const float* q, float eps, float* mean,
                        float* rstd, float* run_mean, float* run_var, float momentum,
                        hipStream_t st);
void bn_apply_launch(long long M, int C, const void* x, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, const void* res, int relu, void* y,
                     hipStream_t st);
void bn_apply_stats_launch(long long M, int C, const void* x, const float* s, const float* q,
                           float eps, float* mean, float* rstd, float* run_mean, float* run_var,
                           float momentum, const float* gamma, const float* beta, const void* res,
                           int relu, void* y, const float* s2, const float* q2, const float* g2,
                           const float* b2, float* mean2, float* rstd2, float* run_mean2,
                           float* run_var2, hipStream_t stream);
long long bn_bwd_scratch_rows(long long M, int C);
void bn_bwd_launch(long long M, int C, const void* dy, const void* yout, const void* x,
                   const float* mean, const float* rstd, const float* gamma, int relu,
                   float* sum_dy, float* sum_dyxh, float* scratch, void* dx, void* dres,
                   hipStream_t st);
void bn_bwd_apply_launch(long long M, int C, const void* de, const void* x, const float* mean,
                         const float* rstd, const float* gamma, const float* sum_dy,
                         const float* sum_dyxh, void* dx, hipStream_t st);
void bn_fwd_coef_launch(long long M, int C, const float* s, const float* q, float eps, float* mean,
                        float* rstd, float* run_mean, float* run_var, float momentum,
                        const float* gamma, const float* beta, const float* s2, const float* q2,
                        const float* g2, const float* b2, float* mean2, float* rstd2,
                        float* run_mean2, float* run_var2, float* coef, hipStream_t stream);
void bn_bwd_coef_launch(long long M, int C, const float* mean, const float* rstd,
                        const float* gamma, const float* sum_dy, const float* sum_dyxh, float* coef,
                        hipStream_t stream);
void colpart_reduce_launch(int R, int C, const float* ps, const float* pq, float* os, float* oq,
                           hipStream_t st);
void maxpool_fwd_launch(int N, int H, int W, int C, const void* x, void* y, void* idx,
                        hipStream_t st);
void maxpool_bwd_launch(int N, int H, int W, int C, const void* dy, const void* idx, void* dx,
                        hipStream_t st);
void maxpool_bn_fwd_launch(int N, int H, int W, int C, const void* x, const float* fcoef, void* y,
                           void* idx, hipStream_t st);
int maxpool_bn_bwd_rows(int N, int H, int W, int C);
void maxpool_bn_bwd_launch(int N, int H, int W, int C, const void* dy, const void* idx,
                           const void* x, const float* fcoef, const float* mean, const float* rstd,
                           const float* gamma, float* sum_dy, float* sum_dyxh, float* scratch,
                           void* de, void* dx, float* bcoef, hipStream_t st);
void avgpool_fwd_launch(int N, int HW, int C, const void* x, void* y, hipStream_t st);
void avgpool_bwd_launch(int N, int HW, int C, const void* dy, void* dx, hipStream_t st);
void sgd_momentum_mixed_launch(long long n, float* p, const float* g, float* v, void* pb, float lr,
                               float mu, float wd, float gscale, hipStream_t st,
                               const long long* segs, int nseg);

// ---- stem_conv.hip
bool stem_conv_applies(int H, int W, int C, int Cout, int KH, int KW, int stride, int pad);
int stem_conv_fwd_rows(int N, int OH, int OW);
void stem_conv_fwd_launch(int N, int H, int W, const void* x, const void* w, int ldw, void* y,
                          float* psum, float* psq, hipStream_t s);
void stem_conv_wgrad_launch(int N, int H, int W, const void* x, const void* dy, float* dw, int ldw,
                            float beta, hipStream_t s, const void* bnx, const float* coef);

// ---- conv3x3_c64.hip
bool conv3x3_c64_applies(int H, int W, int C, int Cout, int KH, int KW, int stride, int pad);
void conv3x3_c64_fwd_launch(int N, int H, int W, const void* x, const void* w, int ldw, void* y,
                            float* psum, float* psq, hipStream_t s, const float* coef, void* xo);
void conv3x3_c64_wgrad_launch(int N, int H, int W, const void* x, const void* dy, float* dw,
                              int ldw, float beta, hipStream_t s);
void conv3x3_c64_dgrad_launch(int N, int H, int W, const void* dy, const void* w, int ldw, void* dx,
                              const void* relu_y, const void* bn_x, const float* bn_mean,
                              const float* bn_rstd, float* psum, float* psq, void* wf,
                              hipStream_t s);

// ---- conv3x3_c128.hip
bool conv3x3_c128_applies(int H, int W, int C, int Cout, int KH, int KW, int stride, int pad);
void conv3x3_c128_launch(int mode, int N, int H, int W, const void* x, const void* w, int ldw,
                         void* y, void* wf, const void* relu_y, const void* bn_x,
                         const float* bn_mean, const float* bn_rstd, float* psum, float* psq,
                         hipStream_t s);

// ---- conv1x1.hip (its BnCoefSrc overload of conv1x1_pro_launch is internal to that file)
bool conv1x1_applies(int M, int K, int N);
int conv1x1_rows(int mode, int M, int K, int N);
void conv1x1_launch(int mode, int M, int K, int N, const void* x, const void* w, int ldw, void* y,
                    const void* res, const void* relu_y, const void* bn_x, const float* mean,
                    const float* rstd, float* ps, float* pq, void* wt, hipStream_t s);
bool conv1x1_pro_applies(int mode, int M, int K, int N);
void conv1x1_pro_launch(int mode, int M, int K, int N, const void* s0, const void* s1,
                        const float* coef, void* xo, const void* w, int ldw, void* y,
                        const void* res, const void* relu_y, const void* bn_x, const float* mean,
                        const float* rstd, float* ps, float* pq, void* wt, hipStream_t s,
                        int res_h, int res_w);
void conv1x1_pro_fwdbn_launch(int mode, int M, int K, int N, const void* s0, const void* s1,
                              long long Mst, const float* sum, const float* sq, float eps,
                              float* mean_out, float* rstd_out, float* run_mean, float* run_var,
                              float momentum, const float* gamma, const float* beta,
                              const float* sum2, const float* sq2, const float* g2, const float* b2,
                              float* mean2, float* rstd2, float* run_mean2, float* run_var2,
                              void* xo, const void* w, int ldw, void* y, float* ps, float* pq,
                              hipStream_t s);
void conv1x1_pro_bwdbn_launch(int M, int K, int N, const void* s0, const void* s1, long long Mst,
                              const float* bmean, const float* brstd, const float* gamma,
                              const float* sum_dy, const float* sum_dyxh, void* xo, const void* w,
                              int ldw, void* y, const void* res, const void* relu_y,
                              const void* bn_x, const float* mean, const float* rstd, float* ps,
                              float* pq, void* wt, hipStream_t s, int res_h, int res_w);
void transpose_bf16_batch_launch(const long long* tab, int n, int tiles, hipStream_t s);

}  // namespace dtfx
