// bf16 device helpers shared by the bf16 tier's kernel files: the vector typedefs, bf16 <-> f32,
// 8-wide pack / unpack, the 16-lane DPP reductions, the MFMA operand fragment reader and the MFMA
// itself.  One copy: a file that needs its own form of one of these says at that form which kernel
// symbol changed when it used the shared one.
#pragma once
#include "common.h"

namespace dtfx {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ float bf(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned short tobf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float tobf_round(float f) { return bf(tobf(f)); }
__device__ __forceinline__ void unpack8(const bf16x8& v, float* f) {
#pragma unroll
  for (int u = 0; u < 8; ++u) f[u] = bf((unsigned short)v[u]);
}
__device__ __forceinline__ bf16x8 pack8(const float* f) {
  bf16x8 v;
#pragma unroll
  for (int u = 0; u < 8; ++u) v[u] = (short)tobf(f[u]);
  return v;
}

// Reductions inside one 16-lane DPP row (the 16 lanes of an MFMA C/D tile that
// share a row group).  Not common.h's row_max16 / row_sum16: those are update_dpp with old = 0,
// these mov_dpp, and the attention kernels' code differs between the two.
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x124, 0xF, 0xF, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x128, 0xF, 0xF, false)));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x124, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x128, 0xF, 0xF, false));
  return v;
}

// MFMA 16x16x32 bf16 operand fragment from an LDS matrix with row pitch `ld`
// bytes: lane gets X[outer = o0 + (lane & 15)][k = k0 + 8 (lane >> 4) + j].
//  KC : element (outer, k) at base + outer*ld + 2k   (one ds_read_b128)
//  !KC: element (outer, k) at base + k*ld + 2*outer  (two ds_read_b64_tr_b16)
template <bool KC>
__device__ __forceinline__ bf16x8 lfrag(const char* base, int ld, int o0, int k0, int lane) {
  if (KC) {
    return *(const bf16x8*)(base + (o0 + (lane & 15)) * ld + (k0 + 8 * (lane >> 4)) * 2);
  } else {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const char* a = base + (k0 + 8 * g + q) * ld + (o0 + 4 * p) * 2;
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)a);
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(a + 4 * ld));
    bf16x8 v;
    v.lo = lo;
    v.hi = hi;
    return v;
  }
}
__device__ __forceinline__ f32x4 mma(const bf16x8& a, const bf16x8& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

}  // namespace dtfx
