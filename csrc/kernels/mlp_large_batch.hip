// Large-batch gradient of the reference's MNIST MLP (784 -> 100 act -> 10): the fused step for
// 257 <= B <= 65,536 rows, where mlp_step.hip's launches (shaped for B <= 256: one-wave blocks
// with freshly loaded operands, one wave per row in the head, the whole batch as the K dimension
// of one block) stop.  Above 256 rows the step is a pair of real GEMMs, [B x 784] . [784 x 112]
// and [112 x B] . [B x 784]; these three launches produce the flat 79,510-element gradient of the
// batch mean loss, the recorded loss / accuracy and the global_step advance -- what mlp_wgrad's
// grad mode produces below 256 -- and the trainer's all-reduce engine applies it (ops/optim.py).
//
// f32 throughout; all matrix work is v_mfma_f32_16x16x4_f32 (lane layout and the
// float4-feeds-four-MFMAs K permutation as in mlp_step_ws.h); parameter layout of mlp_model.h;
// activations through common.h's hidden_act<ACT>, one instantiation each.  No atomics and a fixed
// summation order everywhere: the same inputs give the same bits on every run.  No host
// synchronisation, no allocation and no memset in a launcher: graph-capturable.
//
// The times below are arithmetic from the 32-cycle issue rate of the f32 MFMA at 2.4 GHz, not
// measurements (those are in profiles/large_batch/README.md).
//
// (a) mlp_lb_fwdhead<ACT>: rows -> factors.  One workgroup of 4 waves owns 16 batch rows; the
//     waves split K = 784 into quarters of 196 features (12 groups of 16 through the float4
//     permutation and one k = 4 MFMA step for the last 4 features).  A wave keeps all 7 hidden
//     tiles of its partial z1 in 28 accumulator registers, so one x float4 feeds 28 MFMAs; the W1
//     operands come straight from global memory (every wave has a K quarter of its own: nothing
//     to share through the LDS), requested one group ahead.  A wave's chain is 12 x 28 + 7 = 343
//     MFMAs = 4.6 us.  B / 16 workgroups: 32 at B = 512, 256 (one per CU) at B = 4096; x is
//     read once.  (A wave owning 16 rows over the whole K -- the evaluation kernel's split --
//     would need 1372 MFMAs and leave B / 64 workgroups.)
//     The four partial tiles are added in wave order through the LDS (4 x 7 KB); bias and
//     activation follow, split over the waves by hidden tile (wave w: tiles w and w + 4), which
//     leaves h in the C layout in that wave's registers and, through an LDS tile, in A-operand
//     layout.  The head is mlp_eval.hip's: logits as 7 x 4 MFMAs against W2, softmax one class
//     per lane with 16-lane DPP row reductions (formed by every wave: 28 MFMAs, no hand-off).
//     Training terms: dlogits = (p - onehot) / B goes through a wave-private LDS tile into
//     A-operand layout, dz1 = (dlogits . W2) * act'(h) is 4 MFMAs per hidden tile against W2,
//     the derivative formed from the h the wave holds.  Written row-major: h [BP][112], dz1
//     [BP][112], dlogits [BP][16], per-row (loss, correct).  Rows >= B load row B - 1 and write
//     zeros to every factor; padding columns 100..111 and 10..15 are zero.
//
// (b) mlp_lb_wgrad: factors -> split-K partial gradient planes.  The batch is cut into S slices
//     of R rows (lb_layout: R a multiple of 16 in [64, 256] chosen from B alone, about B / 19, so
//     the grid of 14 S workgroups is about one per CU where B allows; every supported B has
//     S >= 2).  Workgroup (feature block, slice): 4 waves, one 16-feature group each (49 groups:
//     13 blocks, the last with one live wave).  The slice's dz1 rows are staged once in the LDS
//     (R x 112 floats, at most 112 KB) as the A operand the four waves share; a wave's x value
//     (one per lane and 4 batch rows, requested two 16-row chunks ahead) feeds 7 MFMAs, one per
//     hidden tile, into 28 accumulator registers: R / 4 x 7 MFMAs per slice, 3 us at R = 128.
//     One further workgroup per slice forms the small parameters from global memory: dW2^T =
//     dl^T . h and db1 = column sums of dz1 (MFMA against ones) by hidden tile (wave w: tiles w
//     and w + 4), db2 = column sums of dl, and the slice's loss / correct sums (wave 0: lane-
//     strided partial sums, then the fixed DPP tree).  Every work item writes its tile of plane
//     [slice][79,512] in the parameter layout (hidden rows 100..111 dropped); the two words
//     behind b2 hold the slice's loss and correct sums.
//
// (c) mlp_lb_reduce: planes -> gradient.  One float4 per thread, the S planes (pointer and count
//     are arguments: mlp_large_batch_bf16.hip reduces its own planes with it) added in slice order.  The thread of the last float4 (b2[8], b2[9], loss sum, correct sum) stores the two
//     gradient words and writes mean loss and accuracy to stats[global_step % stats_ring], then
//     advances global_step: mlp_wgrad's contract (mlp_step_3launch.h), one thread, no other
//     launch touches the counter.  Folding this launch into the optimizer kernels is left open.
//     With a `partials` buffer (global-norm clipping) the CLIP instantiation also leaves each
//     workgroup's sum of squares of the gradient words it stored.
#include "common.h"
#include "gnorm.h"
#include "mlp_model.h"
#include "mlp_step_api.h"

#include <stdexcept>
#include <string>
#include <type_traits>

namespace dtfx {
namespace mlplb {

using namespace mlp_model;
constexpr int NW = 4;                  // waves per workgroup (all three kernels)
constexpr int KQ = D / NW;             // 196 features per wave of (a)
constexpr int GQ = KQ / 16;            // 12 whole groups of 16
constexpr int HS = 116;                // row stride of the h tile (mlp_eval.hip's)
constexpr int DLS = 20;                // row stride of a dl tile (80 B: float4 rows stay aligned)
constexpr int MINB = MAXB + 1, MAXLB = 65536;
constexpr int RMIN = 64, RMAX = 256;   // rows per slice of (b)
constexpr int FT = D / 16;             // 49 feature groups
constexpr int FB = (FT + NW - 1) / NW; // 13 feature blocks; block FB: the small parameters
constexpr int PLANE = NPARAM + 2;      // a slice's plane: the gradient, loss sum, correct sum
constexpr int NV4 = PLANE / 4;

static_assert(KQ * NW == D && KQ - GQ * 16 == 4 && KQ % 4 == 0,
              "K quarters: 12 groups + one k = 4 step");
static_assert(PLANE % 4 == 0 && OFF_W2 % 4 == 0 && H % 4 == 0, "float4 planes and W2 rows");
static_assert(RMAX * HP * 4 <= 112 * 1024, "the staged dz1 slice");

// Float offsets of the workspace regions and the slicing for a batch of B rows: the ONE definition
// the launchers, the kernels and (through mlp_lb_workspace_floats / mlp_lb_slices) Python share.
// The four zero hand-off words FusedMLPTrainer.check() reads close the buffer.
struct LbLayout {
  long long h, dz1, dl, rowstat, planes, sync, total;
  int BP, S, R;
};
__host__ __device__ constexpr LbLayout lb_layout(int B) {
  LbLayout o{};
  o.BP = (B + 15) / 16 * 16;
  int R = B / 19 / 16 * 16;  // 14 S workgroups: about 256 at S = 19
  o.R = R < RMIN ? RMIN : (R > RMAX ? RMAX : R);
  o.S = (o.BP + o.R - 1) / o.R;
  o.h = 0;
  o.dz1 = o.h + (long long)o.BP * HP;
  o.dl = o.dz1 + (long long)o.BP * HP;
  o.rowstat = o.dl + (long long)o.BP * 16;
  o.planes = o.rowstat + (long long)o.BP * 2;
  o.sync = o.planes + (long long)o.S * PLANE;
  o.total = o.sync + 4;
  return o;
}
static_assert(lb_layout(MINB).S >= 2 && lb_layout(MAXLB).S * lb_layout(MAXLB).R >= MAXLB, "slices");

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

// ---------------------------------------------------------------------------
// (a) rows -> factors
// ---------------------------------------------------------------------------
template <int ACT>
__global__ __launch_bounds__(NW * 64) void mlp_lb_fwdhead_kernel(
    const float* __restrict__ p, const float* __restrict__ x, const int* __restrict__ labels,
    float* __restrict__ ws, int B) {
  __shared__ float part[NW][HT * 4 * 64];  // partial z1 tiles, C layout, lane-linear (4 x 7 KB)
  __shared__ alignas(16) float hs[16 * HS];  // h tile [row][hidden]
  __shared__ alignas(16) float dls[NW][16 * DLS];  // per-wave dlogits tile [row][class]

  const LbLayout L = lb_layout(B);
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * 16;

  // the wave's A-operand row (clamped: a tail row re-reads row B - 1 and stores zeros) and its
  // B-operand rows of W1t, both at the wave's K quarter.  Padded hidden units are copies of unit
  // 99: column j of an MFMA result depends on column j of B alone, and those columns are masked.
  const float* xr = x + (size_t)min(row0 + r, B - 1) * D + w * KQ + 4 * q;
  const float* wp[HT];
#pragma unroll
  for (int jt = 0; jt < HT; ++jt)
    wp[jt] = p + OFF_W1 + (size_t)min(jt * 16 + r, H - 1) * D + w * KQ + 4 * q;

  float4 xa = f4(xr), wb[HT];
#pragma unroll
  for (int jt = 0; jt < HT; ++jt) wb[jt] = f4(wp[jt]);
  // the k = 4 tail of the quarter: lane group q supplies feature 192 + q of it on both operands
  const float xt = xr[GQ * 16 - 3 * q];
  float wt[HT];
#pragma unroll
  for (int jt = 0; jt < HT; ++jt) wt[jt] = wp[jt][GQ * 16 - 3 * q];
  // head operands, requested now: W2 as the logits' B operand (B[k = hidden 16 g + 4 q + e][class
  // r]) and as dz1's (B[k = class 4 q + e][hidden 16 jt + r], tiles w and w + 4), b1 of those
  // tiles, b2, and the labels of the lane's four C-layout rows
  const int t1 = min(w + 4, HT - 1);  // (wave 3 has one tile: its second is a masked copy)
  const bool two = w + 4 < HT;
  float4 w2[HT];
#pragma unroll
  for (int g = 0; g < HT; ++g)
    w2[g] = f4(p + OFF_W2 + min(r, C - 1) * H + min(g * 16 + 4 * q, H - 4));
  float w2d[2][4], b1v[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int j = min((t ? t1 : w) * 16 + r, H - 1);
    b1v[t] = p[OFF_B1 + j];
#pragma unroll
    for (int e = 0; e < 4; ++e) w2d[t][e] = p[OFF_W2 + min(4 * q + e, C - 1) * H + j];
  }
  const float b2c = p[OFF_B2 + min(r, C - 1)];
  int yv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) yv[i] = labels[min(row0 + q * 4 + i, B - 1)];

  f32x4 z[HT];
#pragma unroll
  for (int jt = 0; jt < HT; ++jt) z[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < GQ; ++g) {
    float4 xn = xa, wn[HT];
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) wn[jt] = wb[jt];
    if (g + 1 < GQ) {
      xn = f4(xr + (g + 1) * 16);
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) wn[jt] = f4(wp[jt] + (g + 1) * 16);
    }
    __builtin_amdgcn_sched_barrier(0);  // the next group's loads stay ahead of this one's MFMAs
    // element by element over the 7 tiles: 7 independent accumulators between two MFMAs on the
    // same one
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) z[jt] = mfma16x16x4(xa.x, wb[jt].x, z[jt]);
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) z[jt] = mfma16x16x4(xa.y, wb[jt].y, z[jt]);
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) z[jt] = mfma16x16x4(xa.z, wb[jt].z, z[jt]);
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) z[jt] = mfma16x16x4(xa.w, wb[jt].w, z[jt]);
    __builtin_amdgcn_sched_barrier(0);
    xa = xn;
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) wb[jt] = wn[jt];
  }
#pragma unroll
  for (int jt = 0; jt < HT; ++jt) z[jt] = mfma16x16x4(xt, wt[jt], z[jt]);

  // the four K quarters meet in the LDS (lane-linear: no bank conflict on either side)
#pragma unroll
  for (int jt = 0; jt < HT; ++jt)
#pragma unroll
    for (int i = 0; i < 4; ++i) part[w][(jt * 4 + i) * 64 + lane] = z[jt][i];
  __syncthreads();

  // z1 = quarters in wave order + b1, h = act(z1): wave w's tiles, C layout (column r of the tile,
  // rows 4 q + i).  h stays in the wave's registers for the derivative; padded units are 0.
  float* hg = ws + L.h;
  float hv[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int jt = t ? t1 : w;
    const bool cv = jt * 16 + r < H && (t == 0 || two);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = (jt * 4 + i) * 64 + lane;
      const float s = ((part[0][o] + part[1][o]) + part[2][o]) + part[3][o];
      hv[t][i] = cv ? hidden_act<ACT>(s + b1v[t]) : 0.f;
      if (t == 0 || two) {  // (wave-uniform)
        const int lr = q * 4 + i;
        hs[lr * HS + jt * 16 + r] = hv[t][i];
        hg[(size_t)(row0 + lr) * HP + jt * 16 + r] = row0 + lr < B ? hv[t][i] : 0.f;
      }
    }
  }
  __syncthreads();

  // logits = h . W2 (classes >= 10 and hidden units >= 100: zero operands), every wave
  f32x4 lg0 = {0.f, 0.f, 0.f, 0.f}, lg1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < HT; ++g) {
    const float4 a = *reinterpret_cast<const float4*>(&hs[r * HS + g * 16 + 4 * q]);
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
  // softmax, xent, arg-max and dlogits: class r per lane, the lane's four rows 4 q + i one after
  // the other (every DPP op runs with all lanes active)
  const bool clive = r < C;
  const float invB = 1.f / (float)B;
  float* dlg = ws + L.dl;
  float* rs = ws + L.rowstat;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lr = q * 4 + i, row = row0 + lr;
    const bool valid = row < B;
    const float v = lg0[i] + lg1[i] + b2c;
    const float m = row_max16(clive ? v : -INFINITY);
    // first max, like tf.argmax: the lowest class whose logit equals the max
    int am = row_min16((clive && v == m) ? r : 16);
    am = am < C ? am : 0;
    const float ec = clive ? __expf(v - m) : 0.f;
    const float se = row_sum16(ec);
    const float inv = fast_rcp(se);
    const int y = yv[i];
    const float ly = row_sum16((clive && r == y) ? v : 0.f);  // (0 for a label out of range)
    const float dl = (clive && valid) ? (ec * inv - (r == y ? 1.f : 0.f)) * invB : 0.f;
    dls[w][lr * DLS + r] = dl;
    if (w == 0) {
      dlg[(size_t)row * 16 + r] = dl;
      if (r == 0) {
        rs[2 * row] = valid ? m + __logf(se) - ly : 0.f;
        rs[2 * row + 1] = (valid && am == y) ? 1.f : 0.f;
      }
    }
  }
  __syncthreads();

  // dz1 = (dl . W2) * act'(h): A[row r][k = class 4 q + e] from the wave's dl tile, 4 MFMAs per
  // hidden tile; rows >= B have dl = 0 and padded units h = 0 and W2 = 0, so both come out 0
  const float4 da = *reinterpret_cast<const float4*>(&dls[w][r * DLS + 4 * q]);
  float* dzg = ws + L.dz1;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t == 1 && !two) break;  // (wave-uniform)
    const int jt = t ? t1 : w;
    const bool jv = jt * 16 + r < H;
    f32x4 dh = {0.f, 0.f, 0.f, 0.f};
    dh = mfma16x16x4(da.x, (jv && 4 * q + 0 < C) ? w2d[t][0] : 0.f, dh);
    dh = mfma16x16x4(da.y, (jv && 4 * q + 1 < C) ? w2d[t][1] : 0.f, dh);
    dh = mfma16x16x4(da.z, (jv && 4 * q + 2 < C) ? w2d[t][2] : 0.f, dh);
    dh = mfma16x16x4(da.w, (jv && 4 * q + 3 < C) ? w2d[t][3] : 0.f, dh);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dzg[(size_t)(row0 + q * 4 + i) * HP + jt * 16 + r] = hidden_act_bwd<ACT>(dh[i], hv[t][i]);
  }
}

// ---------------------------------------------------------------------------
// (b) factors -> split-K partial gradient planes
// ---------------------------------------------------------------------------
// The small parameters of one slice (rows b0 .. b0 + rows of the padded batch), from global memory.
__device__ __forceinline__ void lb_small(const float* ws, const LbLayout& L, float* plane, int b0,
                                         int rows, int w, int lane) {
  const int r = lane & 15, q = lane >> 4;
  const int t0 = w, t1 = min(w + 4, HT - 1);  // (wave 3: the second tile is a copy nobody stores)
  const float* dl = ws + L.dl + (size_t)(b0 + q) * 16 + r;
  const float* h0 = ws + L.h + (size_t)(b0 + q) * HP + r;
  const float* d0 = ws + L.dz1 + (size_t)(b0 + q) * HP + r;
  f32x4 aw[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 ab[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 ac = {0.f, 0.f, 0.f, 0.f};
  // K = batch rows, 4 per step (lane group q: row 4 t + q); padded rows hold zero factors
  // (16 rows per trip: its 20 loads are in flight together)
  for (int c = 0; c < rows / 16; ++c) {
    float dv[4], ha[4], hb[4], za[4], zb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t t = (size_t)c * 4 + e;
      dv[e] = dl[t * 4 * 16];
      ha[e] = h0[t * 4 * HP + t0 * 16];
      hb[e] = h0[t * 4 * HP + t1 * 16];
      za[e] = d0[t * 4 * HP + t0 * 16];
      zb[e] = d0[t * 4 * HP + t1 * 16];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      aw[0] = mfma16x16x4(dv[e], ha[e], aw[0]);  // dW2^T[c][j]: A[c = r][b], B[b][j = r]
      aw[1] = mfma16x16x4(dv[e], hb[e], aw[1]);
      ab[0] = mfma16x16x4(za[e], 1.f, ab[0]);    // db1[j]: A[j = r][b] against ones
      ab[1] = mfma16x16x4(zb[e], 1.f, ab[1]);
      ac = mfma16x16x4(dv[e], 1.f, ac);          // db2[c]: A[c = r][b] against ones
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t == 1 && w + 4 >= HT) break;  // (wave-uniform)
    const int jt = t ? t1 : t0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = q * 4 + i, j = jt * 16 + r, jb = jt * 16 + q * 4 + i;
      if (c < C && j < H) plane[OFF_W2 + c * H + j] = aw[t][i];
      if (r == 0 && jb < H) plane[OFF_B1 + jb] = ab[t][i];
    }
  }
  if (w == NW - 1 && r == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (q * 4 + i < C) plane[OFF_B2 + q * 4 + i] = ac[i];
  }
  if (w == 0) {  // the slice's loss / correct sums (rows >= B hold zeros)
    const float* rs = ws + L.rowstat + (size_t)b0 * 2;
    float l = 0.f, a = 0.f;
    for (int b = lane; b < rows; b += 64) {
      l += rs[2 * b];
      a += rs[2 * b + 1];
    }
    l = wave_sum(l);
    a = wave_sum(a);
    if (lane == 0) {
      plane[NPARAM] = l;
      plane[NPARAM + 1] = a;
    }
  }
}

__global__ __launch_bounds__(NW * 64) void mlp_lb_wgrad_kernel(const float* __restrict__ x,
                                                               float* ws, int B) {
  // the slice's dz1 rows, row-major: the A operand the four waves share
  __shared__ alignas(16) float dzs[RMAX * HP];
  const LbLayout L = lb_layout(B);
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fb = blockIdx.x, s = blockIdx.y;
  const int b0 = s * L.R, rows = min(L.R, L.BP - b0);  // (a multiple of 16, >= 16)
  float* plane = ws + L.planes + (size_t)s * PLANE;
  if (fb == FB) {
    lb_small(ws, L, plane, b0, rows, w, lane);
    return;
  }
  const int kt = min(fb * NW + w, FT - 1);  // (a wave past the last group: a clamped, unused copy)
  const bool live = fb * NW + w < FT;
  // x[b][16 kt + r] of chunk c (16 rows; step e of it: rows 4 e + q), clamped like (a)'s rows
  const float* xc = x + kt * 16 + r;
  auto ldx = [&](int c, float(&v)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = xc[(size_t)min(b0 + c * 16 + e * 4 + q, B - 1) * D];
  };
  const int nch = rows / 16;
  float x0[4], x1[4], x2[4];
  ldx(0, x0);
  ldx(min(1, nch - 1), x1);
  {
    const float4* src = reinterpret_cast<const float4*>(ws + L.dz1 + (size_t)b0 * HP);
    float4* dst = reinterpret_cast<float4*>(dzs);
    for (int i = tid; i < rows * (HP / 4); i += NW * 64) dst[i] = src[i];
  }
  __syncthreads();
  if (!live) return;

  f32x4 acc[HT];
#pragma unroll
  for (int jt = 0; jt < HT; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    ldx(min(c + 2, nch - 1), x2);
    __builtin_amdgcn_sched_barrier(0);  // chunk c + 2's loads stay ahead of chunk c's MFMAs
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // A[j = r][k = row 4 e + q] of the 7 hidden tiles; lanes 0..31 and 32..63 each cover the 32
      // banks once (row pitch 112 = 16 mod 32)
      const float* a = dzs + (c * 16 + e * 4 + q) * HP + r;
      float av[HT];
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) av[jt] = a[jt * 16];
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) acc[jt] = mfma16x16x4(av[jt], x0[e], acc[jt]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x0[e] = x1[e];
      x1[e] = x2[e];
    }
  }
  // C[j = 16 jt + 4 q + i][f = 16 kt + r] -> dW1t[j][f] of the slice's plane
#pragma unroll
  for (int jt = 0; jt < HT; ++jt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = jt * 16 + q * 4 + i;
      if (j < H) plane[OFF_W1 + (size_t)j * D + kt * 16 + r] = acc[jt][i];
    }
}

// ---------------------------------------------------------------------------
// (c) planes -> gradient, stats record, global_step
// ---------------------------------------------------------------------------
// Thread i's float4 of the gradient (i < NV4).  CLIP: returns the sum of squares of the gradient
// words it stored, in element order -- the loss and correct sums behind b2 are no gradient words.
template <bool CLIP>
__device__ __forceinline__ float lb_reduce_item(int i, const float* __restrict__ planes, int S,
                                                float* __restrict__ grad, int* __restrict__ ctr,
                                                float* __restrict__ stats, int stats_ring,
                                                int B) {
  const float* src = planes + (size_t)i * 4;
  float4 v = f4(src);
#pragma unroll 4
  for (int s = 1; s < S; ++s) {  // slice order
    const float4 u = f4(src + (size_t)s * PLANE);
    v.x += u.x;
    v.y += u.y;
    v.z += u.z;
    v.w += u.w;
  }
  if (i < NV4 - 1) {
    *reinterpret_cast<float4*>(grad + (size_t)i * 4) = v;
    return CLIP ? lw_sq(v) : 0.f;
  }
  grad[NPARAM - 2] = v.x;
  grad[NPARAM - 1] = v.y;
  const int step = *ctr;  // this thread is the only reader / writer of ctr
  if (stats) {
    float* st = stats + (size_t)(step % stats_ring) * 2;
    st[0] = v.z / (float)B;
    st[1] = v.w / (float)B;
  }
  *ctr = step + 1;
  return CLIP ? lw_sq(make_float4(v.x, v.y, 0.f, 0.f)) : 0.f;
}

// CLIP (global-norm clipping, ops/clip.py): every workgroup also writes the sum of squares of the
// 1,024 gradient words it stored to partials[block] -- optim.hip's gnorm_partials geometry and
// order (gnorm.h), taken from the registers that hold the sums, so the norm costs no second pass
// over the gradient.  Threads past the last float4 add +0 and stay for the barrier.
template <bool CLIP>
__global__ __launch_bounds__(256) void mlp_lb_reduce_kernel(const float* __restrict__ planes,
                                                            int S, float* __restrict__ grad,
                                                            int* __restrict__ ctr,
                                                            float* __restrict__ stats,
                                                            int stats_ring, int B,
                                                            float* __restrict__ partials) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if constexpr (!CLIP) {
    if (i >= NV4) return;
    lb_reduce_item<false>(i, planes, S, grad, ctr, stats, stats_ring, B);
  } else {
    const float sq =
        i < NV4 ? lb_reduce_item<true>(i, planes, S, grad, ctr, stats, stats_ring, B) : 0.f;
    gn_block_sum(sq, partials);
  }
}

static void check_batch(const char* who, int B) {
  if (B < MINB || B > MAXLB)
    throw std::runtime_error(std::string(who) + ": the large-batch step supports " +
                             std::to_string(MINB) + " <= batch <= " + std::to_string(MAXLB) +
                             ", got " + std::to_string(B));
}

}  // namespace mlplb

long long mlp_lb_workspace_floats(int B) {
  mlplb::check_batch("mlp_lb_workspace_floats", B);
  return mlplb::lb_layout(B).total;
}

void mlp_lb_slices(int B, int* S, int* R) {
  mlplb::check_batch("mlp_lb_slices", B);
  const mlplb::LbLayout L = mlplb::lb_layout(B);
  *S = L.S;
  *R = L.R;
}

void mlp_lb_fwdhead_launch(const float* p, const float* x, const int* labels, float* ws, int B,
                           int act, hipStream_t stream) {
  using namespace mlplb;
  check_batch("mlp_lb_fwdhead", B);
  if (act != HACT_SIGMOID && act != HACT_RELU && act != HACT_TANH)
    throw std::runtime_error("mlp_lb_fwdhead: unknown hidden activation id " + std::to_string(act) +
                             " (0 sigmoid, 1 relu, 2 tanh)");
  const int grid = lb_layout(B).BP / 16;
  auto launch = [&](auto ACT) {
    hipLaunchKernelGGL((mlp_lb_fwdhead_kernel<ACT()>), dim3(grid), dim3(NW * 64), 0, stream, p, x,
                       labels, ws, B);
  };
  if (act == HACT_RELU) launch(std::integral_constant<int, HACT_RELU>{});
  else if (act == HACT_TANH) launch(std::integral_constant<int, HACT_TANH>{});
  else launch(std::integral_constant<int, HACT_SIGMOID>{});
  DTFX_HIP_CHECK(hipGetLastError());
}

void mlp_lb_wgrad_launch(const float* x, float* ws, int B, hipStream_t stream) {
  using namespace mlplb;
  check_batch("mlp_lb_wgrad", B);
  hipLaunchKernelGGL(mlp_lb_wgrad_kernel, dim3(FB + 1, lb_layout(B).S), dim3(NW * 64), 0, stream,
                     x, ws, B);
  DTFX_HIP_CHECK(hipGetLastError());
}

int mlp_lb_reduce_partials(int B) {
  mlplb::check_batch("mlp_lb_reduce_partials", B);
  return (mlplb::NV4 + 255) / 256;
}

void mlp_lb_reduce_launch(const float* ws, float* grad, int* ctr, float* stats, int stats_ring,
                          int B, hipStream_t stream, float* partials) {
  using namespace mlplb;
  check_batch("mlp_lb_reduce", B);
  const LbLayout L = lb_layout(B);
  mlp_lb_reduce_planes_launch(ws + L.planes, L.S, grad, ctr, stats, stats_ring, B, stream,
                              partials);
}

void mlp_lb_reduce_planes_launch(const float* planes, int S, float* grad, int* ctr, float* stats,
                                 int stats_ring, int B, hipStream_t stream, float* partials) {
  using namespace mlplb;
  check_batch("mlp_lb_reduce", B);
  if (S < 1 || (reinterpret_cast<uintptr_t>(planes) & 15))
    throw std::runtime_error("mlp_lb_reduce: needs S >= 1 planes at a 16-byte aligned address");
  const dim3 grid((NV4 + 255) / 256);
  if (partials)
    hipLaunchKernelGGL(mlp_lb_reduce_kernel<true>, grid, dim3(256), 0, stream, planes, S, grad,
                       ctr, stats, stats_ring, B, partials);
  else
    hipLaunchKernelGGL(mlp_lb_reduce_kernel<false>, grid, dim3(256), 0, stream, planes, S, grad,
                       ctr, stats, stats_ring, B, partials);
  DTFX_HIP_CHECK(hipGetLastError());
}

}  // namespace dtfx
