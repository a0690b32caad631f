// Shared device helpers for the gfx950 (CDNA4) kernels of this framework.
//
// Everything here is written for a 64-lane wavefront and the f32-input MFMA
// (`v_mfma_f32_16x16x4_f32`): exact f32 products, f32 accumulate.  The
// reference (TF 1.x) computes its MNIST MLP in f32 (worker.py:47-66), so the
// flagship path keeps f32 numerics end to end.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dtfx {

constexpr int kWave = 64;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// 16x16x4 f32 MFMA.  Lane l supplies A[i = l&15][k = l>>4] and
// B[k = l>>4][j = l&15]; the 4-register accumulator holds
// C[row = (l>>4)*4 + r][col = l&15] for r = 0..3.
__device__ __forceinline__ f32x4 mfma16x16x4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float sigmoidf_(float z) {
  // Saturating, branch-free: exp of a non-positive argument never overflows;
  // v_rcp_f32 (1 ulp) instead of an IEEE division sequence.
  const float e = __expf(-fabsf(z));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  return z >= 0.f ? r : e * r;
}

// Hidden activations of the MNIST MLP (ops/hidden_act.py has the definition and these ids).
enum : int { HACT_SIGMOID = 0, HACT_RELU = 1, HACT_TANH = 2 };

__device__ __forceinline__ float tanhf_(float z) {
  // sigmoidf_'s shape: exp of a non-positive argument, v_rcp_f32, the sign restored by bits
  // (saturates at +-1, branch-free, no library call).  Near 0 the error is absolute, ~1e-7.
  const float e = __expf(-2.f * fabsf(z));
  const float t = (1.f - e) * __builtin_amdgcn_rcpf(1.f + e);
  return copysignf(t, z);
}

// h(z), and the derivative as a factor on the incoming gradient, from h alone: sigmoid
// h (1 - h), tanh 1 - h^2, ReLU [h > 0] (0 at z == 0; a select, so -0 and NaN give +0).
template <int ACT>
__device__ __forceinline__ float hidden_act(float z) {
  static_assert(ACT == HACT_SIGMOID || ACT == HACT_RELU || ACT == HACT_TANH, "unknown activation");
  if constexpr (ACT == HACT_RELU) return z > 0.f ? z : 0.f;
  else if constexpr (ACT == HACT_TANH) return tanhf_(z);
  else return sigmoidf_(z);
}
template <int ACT>
__device__ __forceinline__ float hidden_act_bwd(float dh, float h) {
  if constexpr (ACT == HACT_RELU) return h > 0.f ? dh : 0.f;
  else if constexpr (ACT == HACT_TANH) return dh * (1.f - h * h);
  else return dh * h * (1.f - h);
}

// DPP wave reductions (VALU lane moves, no LDS round trip as __shfl_xor's
// ds_bpermute needs): quad_perm xor1/xor2, row_ror 4/8 -> every lane holds its
// 16-lane row sum; row_bcast15/31 fold rows into lane 63; readlane -> SGPR.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}

// N independent wave sums, interleaved step by step so each DPP op's source
// was written N instructions earlier (the VALU->DPP wait states are filled by
// the other reductions, not s_nop).  Within a 16-lane row: quad_perm/row_ror
// adds with old=0 (the identity of +), which the DPP combiner folds into
// v_add_f32_dpp.  Across rows: gfx950 v_permlane16_swap / v_permlane32_swap,
// so every lane ends with the total in a VGPR (no row_bcast masks, no readlane).
template <int N>
__device__ __forceinline__ void wave_sum_n(float (&v)[N]) {
#define DTFX_STEP(CTRL)                                                                    \
  _Pragma("unroll") for (int i = 0; i < N; ++i) v[i] += __int_as_float(                     \
      __builtin_amdgcn_update_dpp(0, __float_as_int(v[i]), CTRL, 0xF, 0xF, false));
  DTFX_STEP(0xB1)
  DTFX_STEP(0x4E)
  DTFX_STEP(0x124)
  DTFX_STEP(0x128)
#undef DTFX_STEP
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int x = __float_as_int(v[i]);
    auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    v[i] = __int_as_float(r[0]) + __int_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int x = __float_as_int(v[i]);
    auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    v[i] = __int_as_float(r[0]) + __int_as_float(r[1]);
  }
}

__device__ __forceinline__ float wave_sum(float v) {
  float a[1] = {v};
  wave_sum_n(a);
  return a[0];
}

// Reduce-scatter of N <= 16 values per lane: returns, in EVERY lane l, the sum over all 64
// lanes of value (l & 15) (garbage where (l & 15) >= N).  Where wave_sum_n carries all N values
// through every step (8 N VALU ops), this halves the live values at each of the four DPP steps
// within the 16-lane row -- the lane's bit 3 / 2 / 1 / 0 selects which half of the value
// indices it keeps, and its partner (row_mirror l ^ 15, row_half_mirror l ^ 7, quad_perm l ^ 2,
// l ^ 1: all single full-rate DPP moves, and together they reach the whole row) supplies the
// other lane's partial of the kept half -- and then folds the four rows of the ONE remaining
// value with the two permlane swaps: 37 ops at N = 10.  A pair (k, k + h) whose upper index is
// >= N costs one add (the upper half's lanes then carry a value nobody reads).
// Fixed order: deterministic, the same bits in every run.
template <int N>
__device__ __forceinline__ float wave_reduce_scatter(const float (&v)[N], int lane) {
  static_assert(N >= 1 && N <= 16, "one value index per lane of a 16-lane row");
  float a[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = i < N ? v[i] : 0.f;
#define DTFX_RS_STEP(HALF, CTRL)                                                       \
  {                                                                                    \
    const bool up = (lane & HALF) != 0;                                                \
    _Pragma("unroll") for (int k = 0; k < HALF; ++k) {                                 \
      if (k < N) {                                                                     \
        const float lo = a[k] + dpp_f<CTRL>(a[k]);                                     \
        if (k + HALF < N) {                                                            \
          const float hi = a[k + HALF] + dpp_f<CTRL>(a[k + HALF]);                     \
          a[k] = up ? hi : lo;                                                         \
        } else {                                                                       \
          a[k] = lo;                                                                   \
        }                                                                              \
      }                                                                                \
    }                                                                                  \
  }
  DTFX_RS_STEP(8, 0x140)  // row_mirror
  DTFX_RS_STEP(4, 0x141)  // row_half_mirror
  DTFX_RS_STEP(2, 0x4E)   // quad_perm [2, 3, 0, 1]
  DTFX_RS_STEP(1, 0xB1)   // quad_perm [1, 0, 3, 2]
#undef DTFX_RS_STEP
  float s = a[0];
  {
    const int x = __float_as_int(s);
    auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    s = __int_as_float(r[0]) + __int_as_float(r[1]);
  }
  {
    const int x = __float_as_int(s);
    auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    s = __int_as_float(r[0]) + __int_as_float(r[1]);
  }
  return s;
}

// Sum / max over the 16-lane row of every lane (quad_perm xor 1 / xor 2, row_ror 4 / 8: every
// lane of the row ends with the result).
__device__ __forceinline__ float row_sum16(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x124>(v);
  v += dpp_f<0x128>(v);
  return v;
}
__device__ __forceinline__ float row_max16(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x124>(v));
  v = fmaxf(v, dpp_f<0x128>(v));
  return v;
}

__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// tanh(u) = 1 - 2 / (1 + e^{2u}): one v_exp_f32 + one v_rcp_f32 (libm tanhf is a long
// branchy sequence, and GEMM epilogues evaluate it per output element).  Saturates
// correctly (e^{2u} -> inf gives 1, -> 0 gives -1); absolute error ~1e-7.
__device__ __forceinline__ float fast_tanh(float u) {
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * u));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }

// Diagnostic stamps (trace builds only): 100 MHz constant-rate wall clock,
// comparable across CUs/XCDs.  STAMP waits for this wave's outstanding memory
// ops first, so each stamp marks "everything issued before has landed".
__device__ __forceinline__ void trace_stamp(unsigned long long* tr, int slot) {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  const unsigned long long t = __builtin_amdgcn_s_memrealtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) tr[slot] = t;
}

// Bijective XCD-aware remap of a 1-D block id (cdna_hip_programming.md §5,
// "XCD swizzle must be bijective"): blocks that the dispatcher deals to the
// same XCD (id % 8 equal) get a contiguous range of logical tile ids, so
// neighbouring tiles share that XCD's L2.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  constexpr int kXcd = 8;
  if (nwg <= kXcd) return orig;
  const int q = nwg / kXcd, r = nwg % kXcd;
  const int xcd = orig % kXcd, pos = orig / kXcd;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

}  // namespace dtfx

#define DTFX_HIP_CHECK(expr)                                                   \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      throw std::runtime_error(std::string("HIP error ") +                    \
                               hipGetErrorString(_e) + " at " + __FILE__ +    \
                               ":" + std::to_string(__LINE__));               \
    }                                                                          \
  } while (0)
