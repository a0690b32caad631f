// Fused evaluation of the reference's MNIST MLP (784 -> 100 sigmoid -> 10): one launch runs
// n rows through the network and leaves predictions, class probabilities (the reference's
// self.net), the summed softmax cross-entropy, the number of correct rows and a 10 x 10
// confusion matrix.  Reference: worker.py:87-90,150-154 (the 10,000-image test accuracy).
//
//   z1 = x . W1 + b1, h = act(z1), logits = h . W2 + b2, softmax, xent, arg-max
//
// act: sigmoid (the reference's), relu or tanh (ops/hidden_act.py; common.h: hidden_act<ACT>), one
// instantiation each; the sigmoid one is the kernel as it was.
//
// h and the logits never reach global memory; every element of x is loaded exactly once, by
// one lane.  All matrix work is v_mfma_f32_16x16x4_f32 (exact f32; lane layout and the
// float4-feeds-4-MFMAs K permutation as in mlp_step_ws.h).  Parameter layout: the flat
// 79,510-element buffer of mlp_model.h.
//
// Decomposition.  The arithmetic first: n = 10,000 rows x 784 x 112 (hidden width padded to 7
// tiles of 16) x 2 = 1.76 GFLOP of f32 MFMA, 11.2 us at the 157 TF peak if all 1024 SIMDs had
// equal work.  Unlike the training step (batch 100, bound by bytes per CU and launch
// boundaries) this is MFMA-issue bound, so the split is chosen by MFMA work per SIMD and by
// how often the 313 KB of W1 is re-read:
//
//   * one WAVE owns 16 rows and all 7 hidden tiles: its x float4 (one load) feeds 28 MFMAs,
//     the 16 x 112 tile of z1 stays in 28 accumulator registers, and x is read once.  That is
//     49 K groups x 28 = 1372 MFMAs of 32 cycles = 43.9 k cycles = 18.3 us at 2.4 GHz per wave:
//     the floor of this split (625 waves at n = 10,000, at most one per SIMD).  Splitting the
//     hidden tiles over more waves would lower it and read x once per split; splitting K
//     would need a cross-wave z1 sum.  Neither is taken: measured (profiles/eval/), the whole
//     evaluation is 43 us at n = 10,000 against 92 us for the two generic GEMM launches plus
//     ATen glue it replaces, and what separates it from the floor is not the split (below).
//   * one WORKGROUP is 4 waves = T = 64 rows, one wave per SIMD of its CU.  W1 does not fit
//     the LDS (351 KB padded), so it streams through it in 7 K chunks of 112 features
//     (49 KB each, double buffered: 98 KB), shared by the 4 waves: each workgroup pulls W1
//     once from its XCD's L2, 157 workgroups x 313 KB = 49 MB at n = 10,000, where 625
//     independent waves would pull 196 MB.  8 waves per pass would halve that again but
//     leave 79 workgroups for 256 CUs; 157 <= 256 keeps one workgroup per CU in one round.
//   * the chunk is staged in MFMA operand order: block (g, jt) of 64 float4, lane l's B
//     operand at l.  The staging wave loads W1t[jt * 16 + (l & 15)][16 g + 4 (l >> 4) ..]
//     (16 runs of 64 B per load, L2 resident) and writes lane-linear; the MFMA loop reads
//     lane-linear ds_read_b128: no bank conflict on either side.  Chunk c + 1 (and the wave's
//     next x float4s) are requested before chunk c's MFMAs and written to the other buffer
//     under the MFMAs of its sixth K group: one barrier per chunk.
//   * head: h goes through a wave-private LDS tile (C layout -> A operand layout), the
//     logits are 7 x 4 MFMAs against W2 (B operand straight from global, requested at kernel
//     start), and the softmax runs one class per lane with 16-lane DPP row reductions, four
//     rows per lane (the C layout's).
//
// Measured (profiles/eval/NOTES.md, in-kernel stamps of one workgroup at n = 10,000, 2.29 GHz):
// the first version spent 36 us per workgroup -- 2.2 us until the first chunk had landed,
// 7 x (4.0 us of MFMAs + 0.5 us staging the next chunk + barrier), 3 us of head -- i.e. ~48
// cycles per MFMA instead of 32, the B operands arriving from the LDS only 3-6 MFMAs ahead of
// their use.  Register double buffering of the B operands, the staging moved under the
// MFMAs and a wave-parallel final reduction took the evaluation from 47.4 to 43.4 us
// (n = 55,000: 176 -> 158 us); the memset node and the launch are ~15 us of that.  Still
// open: the MFMA stream is not at its 32-cycle issue rate, and one wave per SIMD hides
// nothing of the per-chunk barrier or the head.
//
// Reduction, no ticket and no fence: every workgroup sums its rows' losses in double over a
// fixed butterfly, converts the partial to 64-bit fixed point (2^-32 units) and adds it with ONE
// ordinary atomicAdd; counts and confusion cells are integer atomicAdds (pre-summed per
// workgroup in the LDS).  Integer addition is exact and commutes: the accumulator is bitwise
// reproducible for any arrival order.  The launcher zeroes the block with one hipMemsetAsync
// ahead of the kernel on the same stream (one more graph node under capture).
//
// Overflow bound: a row's loss enters the sum clamped to [0, 2^10] (a loss of 1024 nats is a
// probability no f32 softmax can represent; a NaN loss counts as 2^10, so a diverged model
// shows instead of hiding), so n rows sum to at most n * 2^42 units.  The sum is read back
// as a signed 64-bit integer: n <= 2^21 = kMaxRows rows cannot overflow it, and the launcher
// refuses more.
//
// Rows: a label outside [0, 10) still gets a prediction and probabilities and is counted in
// nothing.  labels == nullptr: predict only, the accumulator is neither zeroed nor written.
// Tail rows (any n >= 1) load row n - 1 instead and are never stored or counted.
#include "common.h"
#include "mlp_model.h"
#include "mlp_step_api.h"

#include <cmath>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace dtfx {
namespace mlpeval {

using namespace mlp_model;  // D, H, C, HT, OFF_*: the one definition (mlp_model.h)
constexpr int NW = 4;                 // waves per workgroup
constexpr int T = NW * 16;            // rows per workgroup
constexpr int KC = 112;               // features per staged W1 chunk
constexpr int NCH = D / KC;           // 7 chunks
constexpr int GPC = KC / 16;          // MFMA K groups (of 16) per chunk
constexpr int NBLK = GPC * HT;        // 49 operand blocks of 64 float4 per chunk
constexpr int WPT = (NBLK + NW - 1) / NW;  // blocks a wave stages per chunk (13)
constexpr int HS = 116;               // row stride of the h tile (116 = 4 mod 8: the C-layout
                                      // ds_write_b32 of lanes l, l + 16 fall on distinct banks)
constexpr int kMaxRows = 1 << 21;
constexpr float kLossCap = 1024.f;

static_assert(NCH * KC == D && KC % 16 == 0, "K chunking of 784");
static_assert(T == 64, "the workgroup's final reduction takes one row per lane of a wave");
static_assert(OFF_W2 % 4 == 0 && OFF_B1 % 4 == 0 && H % 4 == 0 && D % 4 == 0, "float4 loads");

// The accumulator block (zeroed by the launcher).  Python reads it as int32[104]:
// words 0-1 the loss sum (little-endian int64, 2^-32 units), 2 correct, 3 count, 4.. confusion.
struct EvalAcc {
  unsigned long long loss_fx;
  int correct;
  int count;
  int conf[C * C];  // [label][predicted]
};
static_assert(sizeof(EvalAcc) == 416, "accumulator layout shared with ops/mlp_eval.py");

__device__ __forceinline__ float4 f4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ int row_min16(int v) {
#define DTFX_MIN_STEP(CTRL) v = min(v, __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false));
  DTFX_MIN_STEP(0xB1)
  DTFX_MIN_STEP(0x4E)
  DTFX_MIN_STEP(0x124)
  DTFX_MIN_STEP(0x128)
#undef DTFX_MIN_STEP
  return v;
}

// Wave w's share of chunk c of W1 (blocks w, w + 4, ..; a block past the last is a clamped,
// unused load) and the wave's x float4s of the chunk.
__device__ __forceinline__ void load_chunk(const float* __restrict__ p, const float* __restrict__ xr,
                                           int c, int w, int r, int q, float4 (&wr)[WPT],
                                           float4 (&xa)[GPC]) {
#pragma unroll
  for (int t = 0; t < WPT; ++t) {
    const int b = min(w + NW * t, NBLK - 1);
    const int g = b / HT, jt = b % HT;
    const int j = min(jt * 16 + r, H - 1);
    wr[t] = f4(p + OFF_W1 + (size_t)j * D + c * KC + g * 16 + 4 * q);
  }
#pragma unroll
  for (int g = 0; g < GPC; ++g) xa[g] = f4(xr + c * KC + g * 16);
}

// Padded hidden units (tile 6, columns >= 4) are staged as copies of unit 99: column j of an
// MFMA result depends on column j of B alone, so they only fill z1 columns nobody reads.
__device__ __forceinline__ void store_chunk(float4* __restrict__ buf, int w, int lane,
                                            const float4 (&wr)[WPT]) {
#pragma unroll
  for (int t = 0; t < WPT; ++t) {
    const int b = w + NW * t;
    if (b < NBLK) buf[b * 64 + lane] = wr[t];  // (wave-uniform)
  }
}

template <int ACT>
__global__ __launch_bounds__(NW * 64) void mlp_eval_kernel(
    const float* __restrict__ p, const float* __restrict__ x, const int* __restrict__ labels,
    int n, EvalAcc* __restrict__ acc, int* __restrict__ pred, float* __restrict__ probs) {
  __shared__ float4 wbuf[2][NBLK * 64];  // W1 chunk in operand order, double buffered (98 KB)
  __shared__ float hs[NW][16 * HS];      // per-wave h tile [row][hidden]
  __shared__ float rloss[T];
  __shared__ int rlab[T], rpred[T];
  __shared__ int conf[C * C];

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: uniform staging branches)
  const int row0 = blockIdx.x * T + w * 16;
  if (tid < C * C) conf[tid] = 0;

  // the wave's A-operand row (clamped: a tail row re-reads row n - 1 and is never stored)
  const float* xr = x + (size_t)min(row0 + r, n - 1) * D + 4 * q;

  float4 wr[WPT], xa[GPC], xn[GPC];
  load_chunk(p, xr, 0, w, r, q, wr, xa);
  // head operands, requested now: b1 / W2 for this lane's columns, b2 and the labels of its
  // four C-layout rows
  float b1v[HT];
  float4 w2[HT];
#pragma unroll
  for (int jt = 0; jt < HT; ++jt) b1v[jt] = p[OFF_B1 + min(jt * 16 + r, H - 1)];
#pragma unroll
  for (int g = 0; g < HT; ++g)  // B[k = hidden 16 g + 4 q + e][class r]
    w2[g] = f4(p + OFF_W2 + min(r, C - 1) * H + min(g * 16 + 4 * q, H - 4));
  const float b2c = p[OFF_B2 + min(r, C - 1)];
  int yv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    yv[i] = labels ? labels[min(row0 + q * 4 + i, n - 1)] : -1;

  // every load so far has landed before the loop is entered (s_waitcnt vmcnt(0)): the compiler
  // then knows that chunk c's x registers are complete on both edges into the loop and puts
  // no vmcnt wait among its MFMAs (without this it waited there on the first loads of chunk
  // c + 1, conservatively, because of the head operands still in flight on the entry edge;
  // measured: no difference in time, the loads had landed -- kept for the cleaner stream)
  __builtin_amdgcn_s_waitcnt(0x0F70);
  store_chunk(wbuf[0], w, lane, wr);
  __syncthreads();

  f32x4 z[HT];
#pragma unroll
  for (int jt = 0; jt < HT; ++jt) z[jt] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int c = 0; c < NCH; ++c) {
    const bool more = c + 1 < NCH;
    if (more) load_chunk(p, xr, c + 1, w, r, q, wr, xn);
    __builtin_amdgcn_sched_barrier(0);  // the next chunk's loads stay ahead of this one's MFMAs
    const float4* wb = wbuf[c & 1] + lane;
    // B operands double buffered in registers: group g + 1's seven ds_read_b128 are issued
    // before group g's 28 MFMAs (fenced: left to itself the compiler reloads each register
    // right after its last use, 3-6 MFMAs ahead of the next one, and the MFMA stream then
    // ran at ~48 cycles per MFMA on LDS latency instead of 32)
    float4 b[2][HT];
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) b[0][jt] = wb[jt * 64];
#pragma unroll
    for (int g = 0; g < GPC; ++g) {
      if (g + 1 < GPC) {
#pragma unroll
        for (int jt = 0; jt < HT; ++jt) b[(g + 1) & 1][jt] = wb[((g + 1) * HT + jt) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
      // the next chunk goes to the other buffer under the MFMAs of group 5 (its loads were
      // issued five groups, ~2 us, ago; every wave left that buffer at the last barrier)
      if (g == GPC - 2 && more) store_chunk(wbuf[(c + 1) & 1], w, lane, wr);
      const float4(&bc)[HT] = b[g & 1];
      // element by element over the 7 tiles: 7 independent accumulators between two MFMAs
      // on the same one (40-cycle dependent latency against a 32-cycle issue)
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) z[jt] = mfma16x16x4(xa[g].x, bc[jt].x, z[jt]);
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) z[jt] = mfma16x16x4(xa[g].y, bc[jt].y, z[jt]);
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) z[jt] = mfma16x16x4(xa[g].z, bc[jt].z, z[jt]);
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) z[jt] = mfma16x16x4(xa[g].w, bc[jt].w, z[jt]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) {
#pragma unroll
      for (int g = 0; g < GPC; ++g) xa[g] = xn[g];
    }
    __syncthreads();
  }

  // h = act(z1 + b1) from the C layout (lane: column r of tile jt, rows 4 q + i) into the
  // wave's tile; padded hidden units are 0
  float* ht = hs[w];
#pragma unroll
  for (int jt = 0; jt < HT; ++jt) {
    const bool cv = jt * 16 + r < H;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      ht[(q * 4 + i) * HS + jt * 16 + r] = cv ? hidden_act<ACT>(z[jt][i] + b1v[jt]) : 0.f;
  }
  __syncthreads();
  // logits = h . W2: A[row r][k] from the tile, B from the registers requested at the start
  // (classes >= 10 and hidden units >= 100: zero operands)
  f32x4 lg0 = {0.f, 0.f, 0.f, 0.f}, lg1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < HT; ++g) {
    const float4 a = *reinterpret_cast<const float4*>(&ht[r * HS + g * 16 + 4 * q]);
    const bool bv = r < C && g * 16 + 4 * q < H;  // (H % 4 == 0: a float4 is whole or absent)
    float4 b = w2[g];
    b.x = bv ? b.x : 0.f;
    b.y = bv ? b.y : 0.f;
    b.z = bv ? b.z : 0.f;
    b.w = bv ? b.w : 0.f;
    lg0 = mfma16x16x4(a.x, b.x, lg0);
    lg1 = mfma16x16x4(a.y, b.y, lg1);
    lg0 = mfma16x16x4(a.z, b.z, lg0);
    lg1 = mfma16x16x4(a.w, b.w, lg1);
  }
  // softmax, xent and arg-max: class r per lane, the lane's four rows 4 q + i one after the
  // other (16-lane DPP row reductions; every DPP op runs with all lanes active)
  const bool clive = r < C;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lr = q * 4 + i, row = row0 + lr;
    const bool valid = row < n;
    const float v = lg0[i] + lg1[i] + b2c;
    const float m = row_max16(clive ? v : -INFINITY);
    // first max, like tf.argmax: the lowest class whose logit equals the max
    int am = row_min16((clive && v == m) ? r : 16);
    am = am < C ? am : 0;
    const float ec = clive ? __expf(v - m) : 0.f;
    const float se = row_sum16(ec);
    const float inv = fast_rcp(se);
    const int y = yv[i];
    const float ly = row_sum16((clive && r == y) ? v : 0.f);
    float loss = m + __logf(se) - ly;
    loss = loss >= 0.f ? loss : (loss < 0.f ? 0.f : kLossCap);  // NaN -> the cap
    loss = fminf(loss, kLossCap);
    if (probs && valid && clive) probs[(size_t)row * C + r] = ec * inv;
    if (r == 0) {
      if (pred && valid) pred[row] = am;
      const bool counted = valid && (unsigned)y < (unsigned)C;
      rloss[w * 16 + lr] = counted ? loss : 0.f;
      rlab[w * 16 + lr] = counted ? y : -1;
      rpred[w * 16 + lr] = am;
    }
  }
  __syncthreads();
  if (tid < T && labels) {
    const int lab = rlab[tid];
    if (lab >= 0) atomicAdd(&conf[lab * C + rpred[tid]], 1);
  }
  __syncthreads();
  if (!labels) return;
  if (tid < C * C) {
    const int v = conf[tid];
    if (v) atomicAdd(&acc->conf[tid], v);
  }
  if (w == 2) {  // (a wave other than the ones with the confusion cells): lane = row
    // fixed order: a butterfly over the 64 rows, the same tree in every run
    double s = (double)rloss[lane];
    const int lab = rlab[lane];
    const unsigned long long cm = __ballot(lab >= 0), km = __ballot(lab >= 0 && lab == rpred[lane]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0 && cm) {
      // s <= 64 * 2^10: s * 2^32 < 2^49, exact in a double up to the rounding to an integer
      atomicAdd(&acc->loss_fx, (unsigned long long)(long long)llrint(s * 4294967296.0));
      atomicAdd(&acc->count, __popcll(cm));
      if (km) atomicAdd(&acc->correct, __popcll(km));
    }
  }
}

}  // namespace mlpeval

int mlp_eval_acc_bytes() { return (int)sizeof(mlpeval::EvalAcc); }
int mlp_eval_row_tile() { return mlpeval::T; }
int mlp_eval_max_rows() { return mlpeval::kMaxRows; }

void mlp_eval_launch(const float* p, const float* x, const int* labels, int n, void* acc, int* pred,
                     float* probs, hipStream_t stream, int act) {
  using namespace mlpeval;
  if (act != HACT_SIGMOID && act != HACT_RELU && act != HACT_TANH)
    throw std::invalid_argument("mlp_eval: unknown hidden activation id " + std::to_string(act) +
                                " (0 sigmoid, 1 relu, 2 tanh)");
  if (n < 0 || n > kMaxRows)
    throw std::invalid_argument("mlp_eval: n must be in [0, " + std::to_string(kMaxRows) +
                                "] (the 64-bit fixed-point loss sum cannot overflow up to there)");
  if (labels != nullptr && acc == nullptr)
    throw std::invalid_argument("mlp_eval: labels need an accumulator block");
  if (labels != nullptr) DTFX_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(EvalAcc), stream));
  if (n == 0) return;
  const int grid = (n + T - 1) / T;
  auto launch = [&](auto ACT) {
    hipLaunchKernelGGL((mlp_eval_kernel<ACT()>), dim3(grid), dim3(NW * 64), 0, stream, p, x, labels,
                       n, static_cast<EvalAcc*>(acc), pred, probs);
  };
  if (act == HACT_RELU) launch(std::integral_constant<int, HACT_RELU>{});
  else if (act == HACT_TANH) launch(std::integral_constant<int, HACT_TANH>{});
  else launch(std::integral_constant<int, HACT_SIGMOID>{});
  DTFX_HIP_CHECK(hipGetLastError());
}

}  // namespace dtfx
