// Sum of squares of a flat f32 buffer, one partial per workgroup of 256 threads (1,024 elements,
// one float4 per thread): the pieces optim.hip's norm launches and the large-batch reduce launch
// (mlp_large_batch.hip, CLIP instantiation) share, so both leave the same bits for the same
// values.  Fixed order everywhere: a thread's four squares in element order, the wave's 64 lanes
// by the fixed DPP tree (wave_sum_n), the four waves in wave order through the LDS.  No atomics.
#pragma once
#include "common.h"

namespace dtfx {

// Sum of squares of a thread's values, in element order (dead lanes are +0).
__device__ __forceinline__ float lw_sq(float4 a) {
  float s = a.x * a.x;
  s = __fmaf_rn(a.y, a.y, s);
  s = __fmaf_rn(a.z, a.z, s);
  return __fmaf_rn(a.w, a.w, s);
}

// The workgroup's sum -> partials[block].  Every thread of the 256 calls it (one barrier).
__device__ __forceinline__ void gn_block_sum(float a, float* __restrict__ partials) {
  __shared__ float lds[4];
  const float s = wave_sum(a);
  if (lane_id() == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

}  // namespace dtfx
