// Host API of the GPU-resident parameter store's kernels (gpu_ps.hip), declared ONCE for that
// file and the store's host side (gpu_ps.cpp).  Plain C++: no kernel, no device code.  Pointers
// are device addresses (the store's allocation, possibly another GPU's over xGMI).
#pragma once
#include <hip/hip_runtime.h>

namespace dtfx {

void gps_pull_launch(float* dst, const float* src, long long n, hipStream_t s);
void gps_apply_launch(float* p, const float* g, float lr, long long n, bool locking, hipStream_t s);
void gps_fetch_add_launch(unsigned long long* ctr, long long delta, unsigned long long* out,
                          const float* extra, int nextra, hipStream_t s);
void gps_sync_join_launch(unsigned long long* round_word, unsigned local_step, unsigned R,
                          unsigned* dec, const float* extra, int nextra, hipStream_t s);
void gps_sync_push_launch(float* p, float* slots, long long slot_stride, const float* g,
                          const unsigned* dec, unsigned* arrivals, unsigned* chunks_done,
                          unsigned long long* round_word, unsigned long long* step_word, float lr,
                          unsigned R, long long n, int opt, float* opt0, float* opt1, float h0,
                          float h1, float h2, hipStream_t s);
void gps_apply_opt_launch(float* p, float* s0, float* s1, const float* g,
                          const unsigned long long* step_word, float lr, int opt, float h0,
                          float h1, float h2, long long n, hipStream_t s);

}  // namespace dtfx
