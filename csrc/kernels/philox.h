// Philox4x32-10, the counter-based generator of the init kernels (optim.hip: philox_init_kernel)
// and of the fused MLP step's dropout mask (mlp_step_3launch.h: head_row<.., DROP>).
// tests/philox_reference.py is the same function in numpy.
#pragma once
#include <hip/hip_runtime.h>

namespace dtfx {

struct U4 { unsigned x, y, z, w; };

__device__ __forceinline__ U4 philox10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c.x;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c.z;
    const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0;
    const unsigned hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

}  // namespace dtfx
