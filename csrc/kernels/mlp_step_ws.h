// Fused MLP step (mlp_step.hip): what every engine of the step shares -- the K slicing, the
// workspace (Bufs / ws_layout) and two small device helpers.
//
// All MFMA work is v_mfma_f32_16x16x4_f32 (exact f32).  Lane l supplies
// A[i = l&15][k = l>>4], B[k = l>>4][j = l&15]; C[row = (l>>4)*4 + r][col = l&15].
// A float4 load of k = 16g + 4q .. 16g + 4q + 3 feeds 4 MFMAs (element e is
// k = 16g + 4q + e on BOTH operands: a consistent permutation of the K sum).
#pragma once
#include "common.h"
#include "mlp_model.h"

namespace dtfx {
namespace mlp {

using namespace mlp_model;

constexpr int KS = 7;          // K slices of K1
constexpr int KW = D / KS;     // 112 = 7 groups of 16
constexpr int FT = D / 16;     // 49 feature tiles (dW1)
constexpr int KS2 = 14;        // K slices of the pipelined step's fused apply+forward launch
constexpr int KW2 = D / KS2;   // 56 features = 3.5 MFMA groups of 16
constexpr int KS3 = 28;        // ... the single-GPU form: 28 slices of 28 features (203 blocks)
constexpr int NSLAB_MAX = KS3; // slab planes in the workspace

static_assert(KW % 16 == 0 && KS * KW == D, "K slicing of 784");
static_assert(KS2 * KW2 == D && KW2 % 8 == 0, "K slicing of the pipelined step");

struct Bufs {            // workspace (zero-initialised once; padding stays 0)
  float* slab;           // [NSLAB_MAX][BP][HP]  partial z1 (KS or KS2 planes used)
  float* hbuf;           // [BP][HP]      h
  float* dz1T;           // [HP][BP]      dz1 transposed
  float* dlT;            // [16][BP]      dlogits transposed
  float* rowstat;        // [BP][2]       per-row (loss, correct)
  int* sync;             // [4] handoff words of mlp_head_flush_kernel (0 between launches):
                         //     [0] head rows done, [1] apply blocks done, [2] sticky timeout
  // the single-GPU two-launch step's factors, row-major: regions of their own AFTER the sync
  // words (StepWorkspace.buf ends at sync + 4: FusedMLPTrainer.check() and the tests' views
  // size that part; the allocation, mlp_workspace_floats, goes on)
  float* dz1R;           // [BP][HP]      dz1 row-major
  float* dlR;            // [BP][16]      dlogits row-major
};

// Float offsets of the workspace regions for a padded batch of BP rows: the ONE definition the
// host launchers (make_bufs, mlp_workspace_floats) and the lean step's kernels (which take the
// workspace base pointer alone) share.
struct WsLayout {
  long long hbuf, dz1T, dlT, rowstat, sync, dz1R, dlR, total;
};
__host__ __device__ constexpr WsLayout ws_layout(long long BP) {
  WsLayout o{};
  o.hbuf = (long long)NSLAB_MAX * BP * HP;
  o.dz1T = o.hbuf + BP * HP;
  o.dlT = o.dz1T + HP * BP;
  o.rowstat = o.dlT + 16 * BP;
  o.sync = o.rowstat + 2 * BP;
  o.dz1R = o.sync + 4;
  o.dlR = o.dz1R + BP * HP;
  o.total = o.dlR + 16 * BP;
  return o;
}
__host__ __device__ __forceinline__ Bufs ws_bufs(float* ws, int BP) {
  const WsLayout o = ws_layout(BP);
  Bufs b;
  b.slab = ws;
  b.hbuf = ws + o.hbuf;
  b.dz1T = ws + o.dz1T;
  b.dlT = ws + o.dlT;
  b.rowstat = ws + o.rowstat;
  b.sync = reinterpret_cast<int*>(ws + o.sync);
  b.dz1R = ws + o.dz1R;
  b.dlR = ws + o.dlR;
  return b;
}

__device__ __forceinline__ float4 f4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// trace_stamp (common.h) that leaves the wave's N most recent vector memory operations in
// flight: vector loads return in order, so it marks "everything but the last N has landed".
template <int N>
__device__ __forceinline__ void trace_stamp_vm(unsigned long long* tr, int slot) {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
  const unsigned long long t = __builtin_amdgcn_s_memrealtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) tr[slot] = t;
}

}  // namespace mlp
}  // namespace dtfx
