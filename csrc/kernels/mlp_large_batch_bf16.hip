// Mixed-precision form of the large-batch gradient (mlp_large_batch.hip, 257 <= B <= 65,536): the
// two 784-wide GEMMs of the step, [B x 784] . [784 x 112] and [112 x B] . [B x 784], take bf16
// operands on v_mfma_f32_16x16x32_bf16 and accumulate in f32.  The weights stay the ONE f32
// parameter buffer (no bf16 shadow: W1 is rounded in registers on its way into the MFMA); the
// dataset comes as a row-major bf16 copy xh [n][784] (1568-byte rows, 16-byte aligned), half the
// bytes of the operand both GEMMs stream; labels are int32.  Outputs are mlp_lb_*'s contract, bit
// for bit in its layout: the flat 79,510-element f32 gradient of the batch mean loss, the step's
// loss / accuracy in the stats ring, global_step + 1.  Everything behind the first GEMM -- bias,
// activation, logits, softmax, loss, arg-max, dlogits, dz1, the small parameters, the reduce --
// is the f32 file's arithmetic on the f32 MFMA.  That code is copied here (the head from the LDS
// meeting on, lb_small) and not shared through a header: the f32 kernels stay byte-identical, and
// the copies differ only in the layout type they take.  The reduce launch IS shared
// (mlp_lb_reduce_planes_launch: planes pointer and S passed explicitly).
//
// No atomics, a fixed summation order everywhere (the same inputs give the same bits), no host
// synchronisation, allocation or memset in a launcher: graph-capturable.  lbh_layout(B) below is
// the one definition of the workspace regions and the slicing; it shares nothing with lb_layout.
//
// bf16 MFMA lane layout (bf16.h): A lane holds A[row = lane & 15][k = 8 (lane >> 4) + 0..7], B
// lane holds B[k = 8 (lane >> 4) + 0..7][col = lane & 15], C is the f32 MFMA's: C[row = 4 (lane
// >> 4) + i][col = lane & 15].  So both kernels leave their accumulators exactly where the f32
// kernels' epilogues expect them.
//
// (a) mlp_lbh_fwdhead<ACT>: rows -> factors.  16 batch rows per workgroup, 4 waves split K:
//     784 = 24 steps of k = 32 + 16 features; wave w takes steps 6 w .. 6 w + 5, and wave 3 one
//     more k = 32 step for features 768..783 whose upper half (lane groups 2, 3) is zero on both
//     operands (those lanes re-load the lower half's addresses: nothing is read past a row).  Per
//     step a lane loads its A fragment as ONE 16-byte load (8 consecutive bf16 features of its
//     row, clamped to row B - 1) and, per hidden tile, W1t row min(16 jt + r, 99) at the same 8
//     features as two float4 of the f32 master, packed to bf16 round-to-nearest-even in registers
//     (pack8).  One x fragment feeds 7 MFMAs into 28 accumulator registers; the next step's 15
//     loads are requested before this step's MFMAs.  A wave's chain is 6 x 7 (+ 7) MFMAs where
//     the f32 kernel's is 343.  The four partial tiles meet in the LDS in wave order; from there
//     on the kernel is mlp_lb_fwdhead's.  It writes h, dz1, dl and the row stats in f32 where the
//     f32 kernel does, and dz1 once more as bf16 [BP32][112] (BP32: B rounded up to 32), each
//     value the RNE rounding of the f32 value the same lane stores; rows B .. BP16 are stored as
//     zeros, rows BP16 .. BP32 are never written (the workspace is zeroed once at construction).
//
// (b) mlp_lbh_wgrad: factors -> split-K partial planes.  dW1t[j][f] = sum_b dz1[b][j] x[b][f]: K
//     is the batch, and BOTH operands are stored with K as the strided dimension, so both go
//     through the LDS row-major and are read with the transposing read (lfrag<false>, two
//     ds_read_b64_tr_b16 per fragment).  Slices of R rows (R a multiple of 32 in [64, 256] chosen
//     from B alone, about B / 19; S >= 2 for every supported B).  Workgroup (feature block of 64,
//     slice): 4 waves, one 16-feature group each; 13 blocks, the last with one live wave (all
//     four still stage).  The slice's bf16 dz1 rows are staged once (R x 224 B, at most 56 KB); x
//     is staged in chunks of 32 rows x 64 features, one 16-byte global load per thread (128-byte
//     contiguous row pieces), double-buffered in the LDS with two more chunks in registers: chunk
//     c + 1 is written to the other buffer after chunk c's MFMAs, one barrier per chunk.  Per
//     chunk a wave reads one x fragment and 7 dz1 fragments and issues 7 MFMAs into 28
//     accumulator registers: R / 32 x 7 MFMAs per slice (the f32 kernel: R / 4 x 7).  Rows >= B
//     carry zero dz1 and clamp their x row to B - 1 (the dataset is finite: 0 x finite = 0).  The
//     last block has 16 features: its staging lanes of segments 2..7 re-load segments 0 / 1.
//     LDS pitches.  A transposing read's 16-lane group touches 4 consecutive K rows x 32
//     contiguous bytes.  With a row pitch of 32 or 96 mod 128 bytes those four pieces tile one
//     128-byte window of the banks, so a group's read is conflict-free.  dz1 rows are 224 B = 96
//     mod 128 as they are (staging is a straight copy); x chunk rows are 128 B and are padded to
//     160 B = 32 mod 128 (16-byte aligned for the staging stores).  LDS: 56 KB + 2 x 5 KB.
//     One further workgroup per slice forms dW2, db1, db2 and the loss / correct sums from the f32
//     factors: lb_small's arithmetic.  Planes as in the f32 file: [slice][79,512] f32, the loss
//     and correct sums behind b2.
//
// (c) reduce: mlp_lb_reduce_kernel through mlp_lb_reduce_planes_launch.
#include "bf16.h"
#include "mlp_model.h"
#include "mlp_step_api.h"

#include <stdexcept>
#include <string>
#include <type_traits>

namespace dtfx {
namespace mlplbh {

using namespace mlp_model;
constexpr int NW = 4;                  // waves per workgroup
constexpr int NS = 6;                  // k = 32 steps per wave of (a); wave 3: one more, half empty
constexpr int KW = NS * 32;            // 192 features per wave
constexpr int HS = 116;                // row stride of the h tile (mlp_lb_fwdhead's)
constexpr int DLS = 20;                // row stride of a dl tile
constexpr int MINB = MAXB + 1, MAXLB = 65536;
constexpr int RMIN = 64, RMAX = 256;   // rows per slice of (b)
constexpr int CH = 32;                 // batch rows per staged x chunk: one MFMA's K
constexpr int FBW = 64;                // features per block of (b): 16 per wave
constexpr int FB = (D + FBW - 1) / FBW;  // 13 feature blocks; block FB: the small parameters
constexpr int DZP = HP * 2;            // LDS row pitch of the bf16 dz1 slice: 224 B (96 mod 128)
constexpr int XP = FBW * 2 + 32;       // LDS row pitch of an x chunk: 160 B (32 mod 128)
constexpr int PLANE = NPARAM + 2;      // a slice's plane: the gradient, loss sum, correct sum

static_assert(NW * KW + 16 == D, "K: 24 steps of 32 + 16 features");
static_assert((FB - 1) * FBW + 16 == D, "the last feature block holds one 16-feature group");
static_assert(DZP % 128 == 96 && XP % 128 == 32 && XP % 16 == 0, "bank layout of the LDS pitches");
static_assert(RMAX * DZP <= 56 * 1024 && NW * 64 == CH * (FBW / 8), "staging: one load per thread");
static_assert(D % 8 == 0 && PLANE % 4 == 0, "16-byte bf16 rows, float4 planes");

// Float offsets of the workspace regions and the slicing for a batch of B rows: the ONE definition
// the launchers, the kernels and (through mlp_lbh_workspace_floats / mlp_lbh_slices /
// mlp_lbh_offsets) Python share.  h, dz1, dl, rowstat: the f32 factors, BP = B rounded up to 16
// rows, as the f32 step keeps them; dz1h: the bf16 dz1 plane [BP32][112] (two values per float
// word); the four zero hand-off words FusedMLPTrainer.check() reads close the buffer.
struct LbhLayout {
  long long h, dz1, dl, rowstat, dz1h, planes, sync, total;
  int BP, BP32, S, R;
};
__host__ __device__ constexpr LbhLayout lbh_layout(int B) {
  LbhLayout o{};
  o.BP = (B + 15) / 16 * 16;
  o.BP32 = (B + 31) / 32 * 32;
  int R = B / 19 / 32 * 32;  // 14 S workgroups: about 256 at S = 19
  o.R = R < RMIN ? RMIN : (R > RMAX ? RMAX : R);
  o.S = (o.BP32 + o.R - 1) / o.R;
  o.h = 0;
  o.dz1 = o.h + (long long)o.BP * HP;
  o.dl = o.dz1 + (long long)o.BP * HP;
  o.rowstat = o.dl + (long long)o.BP * 16;
  o.dz1h = o.rowstat + (long long)o.BP * 2;
  o.planes = o.dz1h + (long long)o.BP32 * (HP / 2);
  o.sync = o.planes + (long long)o.S * PLANE;
  o.total = o.sync + 4;
  return o;
}
static_assert(lbh_layout(MINB).S >= 2 && lbh_layout(MAXLB).S * lbh_layout(MAXLB).R >= MAXLB,
              "slices");
static_assert(lbh_layout(MINB).dz1h % 4 == 0 && lbh_layout(MINB).planes % 4 == 0,
              "16-byte aligned bf16 plane and gradient planes");

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
__global__ __launch_bounds__(NW * 64) void mlp_lbh_fwdhead_kernel(
    const float* __restrict__ p, const unsigned short* __restrict__ xh,
    const int* __restrict__ labels, float* __restrict__ ws, int B) {
  __shared__ float part[NW][HT * 4 * 64];  // partial z1 tiles, C layout, lane-linear (4 x 7 KB)
  __shared__ alignas(16) float hs[16 * HS];  // h tile [row][hidden]
  __shared__ alignas(16) float dls[NW][16 * DLS];  // per-wave dlogits tile [row][class]

  const LbhLayout L = lbh_layout(B);
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * 16;
  const bool tail = w == NW - 1;  // (wave-uniform) the wave with the 16-feature step

  // the wave's A-operand row (clamped: a tail row re-reads row B - 1 and stores zeros) and its
  // B-operand rows of W1t, both at the wave's K range.  Padded hidden units are copies of unit
  // 99: column j of an MFMA result depends on column j of B alone, and those columns are masked.
  const unsigned short* xr = xh + (size_t)min(row0 + r, B - 1) * D + w * KW;
  const float* wp[HT];
#pragma unroll
  for (int jt = 0; jt < HT; ++jt)
    wp[jt] = p + OFF_W1 + (size_t)min(jt * 16 + r, H - 1) * D + w * KW;
  // step s of the wave: features 32 s + 8 q + 0..7 on both operands; step NS (wave 3 only) has 16
  // features, and its lane groups 2, 3 re-load groups 0, 1 (zeroed before the MFMA)
  auto ld = [&](int s, bf16x8& xv, float4(&wv)[HT][2]) {
    const int o = s * 32 + 8 * (s == NS ? (q & 1) : q);
    xv = *reinterpret_cast<const bf16x8*>(xr + o);
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) {
      wv[jt][0] = f4(wp[jt] + o);
      wv[jt][1] = f4(wp[jt] + o + 4);
    }
  };
  bf16x8 xa;
  float4 wr[HT][2];
  ld(0, xa, wr);
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
  for (int s = 0; s <= NS; ++s) {
    if (s == NS && !tail) break;  // (wave-uniform)
    bf16x8 xn = xa;
    float4 wn[HT][2];
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) {
      wn[jt][0] = wr[jt][0];
      wn[jt][1] = wr[jt][1];
    }
    if (s + 1 < NS || (s + 1 == NS && tail)) ld(s + 1, xn, wn);
    __builtin_amdgcn_sched_barrier(0);  // the next step's loads stay ahead of this one's MFMAs
    // W1 -> bf16, round-to-nearest-even, in registers; the half-empty step: zero upper K half
    const bool kv = s < NS || q < 2;
    bf16x8 wb[HT];
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) {
      const float f[8] = {wr[jt][0].x, wr[jt][0].y, wr[jt][0].z, wr[jt][0].w,
                          wr[jt][1].x, wr[jt][1].y, wr[jt][1].z, wr[jt][1].w};
      wb[jt] = pack8(f);
#pragma unroll
      for (int u = 0; u < 8; ++u) wb[jt][u] = kv ? wb[jt][u] : (short)0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) xa[u] = kv ? xa[u] : (short)0;
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) z[jt] = mma(xa, wb[jt], z[jt]);
    __builtin_amdgcn_sched_barrier(0);
    xa = xn;
#pragma unroll
    for (int jt = 0; jt < HT; ++jt) {
      wr[jt][0] = wn[jt][0];
      wr[jt][1] = wn[jt][1];
    }
  }

  // ---- from here on: mlp_lb_fwdhead's code (plus the bf16 dz1 store) ----
  // the four K ranges meet in the LDS (lane-linear: no bank conflict on either side)
#pragma unroll
  for (int jt = 0; jt < HT; ++jt)
#pragma unroll
    for (int i = 0; i < 4; ++i) part[w][(jt * 4 + i) * 64 + lane] = z[jt][i];
  __syncthreads();

  // z1 = ranges in wave order + b1, h = act(z1): wave w's tiles, C layout (column r of the tile,
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
  // hidden tile; rows >= B have dl = 0 and padded units h = 0 and W2 = 0, so both come out 0.
  // Stored twice: f32 for the small parameters, bf16 (RNE of that f32 value) for (b)'s GEMM.
  const float4 da = *reinterpret_cast<const float4*>(&dls[w][r * DLS + 4 * q]);
  float* dzg = ws + L.dz1;
  unsigned short* dzh = reinterpret_cast<unsigned short*>(ws + L.dz1h);
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
    for (int i = 0; i < 4; ++i) {
      const size_t o = (size_t)(row0 + q * 4 + i) * HP + jt * 16 + r;
      const float d = hidden_act_bwd<ACT>(dh[i], hv[t][i]);
      dzg[o] = d;
      dzh[o] = tobf(d);
    }
  }
}

// ---------------------------------------------------------------------------
// (b) factors -> split-K partial gradient planes
// ---------------------------------------------------------------------------
// The small parameters of one slice (rows b0 .. b0 + rows of the 16-padded batch), from the f32
// factors in global memory: mlp_large_batch.hip's lb_small.
__device__ __forceinline__ void lbh_small(const float* ws, const LbhLayout& L, float* plane,
                                          int b0, int rows, int w, int lane) {
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

__global__ __launch_bounds__(NW * 64) void mlp_lbh_wgrad_kernel(
    const unsigned short* __restrict__ xh, float* ws, int B) {
  // the slice's bf16 dz1 rows [row][112] and two x chunks [32 rows][64 features (+ pad)], both
  // row-major with the batch (the MFMA's K) as the strided dimension
  __shared__ alignas(16) char dzs[RMAX * DZP];
  __shared__ alignas(16) char xs[2][CH * XP];
  const LbhLayout L = lbh_layout(B);
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fb = blockIdx.x, s = blockIdx.y;
  const int b0 = s * L.R;
  float* plane = ws + L.planes + (size_t)s * PLANE;
  if (fb == FB) {
    lbh_small(ws, L, plane, b0, min(L.R, L.BP - b0), w, lane);  // (a multiple of 16, >= 16)
    return;
  }
  const int rows = min(L.R, L.BP32 - b0);  // (a multiple of 32, >= 32)
  const int nch = rows / CH;
  // staging: thread -> (row tid / 8 of the chunk, 16-byte segment tid % 8 of its 64 features);
  // the last block has two live segments, the others re-load them (a row is never overrun)
  const int srow = tid >> 3, sseg = tid & 7;
  const unsigned short* xg = xh + fb * FBW + (fb == FB - 1 ? (sseg & 1) : sseg) * 8;
  auto ldx = [&](int c) {
    const int row = min(b0 + min(c, nch - 1) * CH + srow, B - 1);
    return *reinterpret_cast<const bf16x8*>(xg + (size_t)row * D);
  };
  char* xdst = &xs[0][0] + srow * XP + sseg * 16;
  bf16x8 n1 = ldx(0), n2 = ldx(1), n3 = ldx(2);
  {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(
        reinterpret_cast<const unsigned short*>(ws + L.dz1h) + (size_t)b0 * HP);
    bf16x8* dst = reinterpret_cast<bf16x8*>(dzs);
    for (int i = tid; i < rows * (DZP / 16); i += NW * 64) dst[i] = src[i];
  }
  *reinterpret_cast<bf16x8*>(xdst) = n1;
  n1 = n2;
  n2 = n3;
  __syncthreads();

  const bool live = fb * NW + w < D / 16;  // (wave-uniform; every wave stages and meets the barriers)
  f32x4 acc[HT];
#pragma unroll
  for (int jt = 0; jt < HT; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    n3 = ldx(c + 3);
    __builtin_amdgcn_sched_barrier(0);  // chunk c + 3's load stays ahead of chunk c's MFMAs
    if (live) {
      // B[k = row][f = 16 w + (lane & 15)] of the chunk, A[j = 16 jt + (lane & 15)][k = row] of
      // the 7 hidden tiles: both through the transposing read
      const bf16x8 xb = lfrag<false>(xs[c & 1], XP, 16 * w, 0, lane);
      bf16x8 av[HT];
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) av[jt] = lfrag<false>(dzs, DZP, 16 * jt, c * CH, lane);
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) acc[jt] = mma(av[jt], xb, acc[jt]);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (c + 1 < nch) *reinterpret_cast<bf16x8*>(xdst + ((c + 1) & 1) * (CH * XP)) = n1;
    n1 = n2;
    n2 = n3;
    __syncthreads();  // chunk c + 1 is staged, and chunk c's buffer is free for chunk c + 2
  }
  if (!live) return;
  // C[j = 16 jt + 4 q + i][f = 64 fb + 16 w + r] -> dW1t[j][f] of the slice's plane
#pragma unroll
  for (int jt = 0; jt < HT; ++jt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = jt * 16 + q * 4 + i;
      if (j < H) plane[OFF_W1 + (size_t)j * D + fb * FBW + 16 * w + r] = acc[jt][i];
    }
}

static void check_batch(const char* who, int B) {
  if (B < MINB || B > MAXLB)
    throw std::runtime_error(std::string(who) + ": the large-batch step supports " +
                             std::to_string(MINB) + " <= batch <= " + std::to_string(MAXLB) +
                             ", got " + std::to_string(B));
}

}  // namespace mlplbh

long long mlp_lbh_workspace_floats(int B) {
  mlplbh::check_batch("mlp_lbh_workspace_floats", B);
  return mlplbh::lbh_layout(B).total;
}

void mlp_lbh_slices(int B, int* S, int* R) {
  mlplbh::check_batch("mlp_lbh_slices", B);
  const mlplbh::LbhLayout L = mlplbh::lbh_layout(B);
  *S = L.S;
  *R = L.R;
}

void mlp_lbh_offsets(int B, long long* off) {
  mlplbh::check_batch("mlp_lbh_offsets", B);
  const mlplbh::LbhLayout L = mlplbh::lbh_layout(B);
  off[0] = L.h;
  off[1] = L.dz1;
  off[2] = L.dl;
  off[3] = L.rowstat;
  off[4] = L.dz1h;
  off[5] = L.planes;
  off[6] = L.BP;
  off[7] = L.BP32;
}

void mlp_lbh_fwdhead_launch(const float* p, const unsigned short* xh, const int* labels, float* ws,
                            int B, int act, hipStream_t stream) {
  using namespace mlplbh;
  check_batch("mlp_lbh_fwdhead", B);
  if (act != HACT_SIGMOID && act != HACT_RELU && act != HACT_TANH)
    throw std::runtime_error("mlp_lbh_fwdhead: unknown hidden activation id " +
                             std::to_string(act) + " (0 sigmoid, 1 relu, 2 tanh)");
  const int grid = lbh_layout(B).BP / 16;
  auto launch = [&](auto ACT) {
    hipLaunchKernelGGL((mlp_lbh_fwdhead_kernel<ACT()>), dim3(grid), dim3(NW * 64), 0, stream, p,
                       xh, labels, ws, B);
  };
  if (act == HACT_RELU) launch(std::integral_constant<int, HACT_RELU>{});
  else if (act == HACT_TANH) launch(std::integral_constant<int, HACT_TANH>{});
  else launch(std::integral_constant<int, HACT_SIGMOID>{});
  DTFX_HIP_CHECK(hipGetLastError());
}

void mlp_lbh_wgrad_launch(const unsigned short* xh, float* ws, int B, hipStream_t stream) {
  using namespace mlplbh;
  check_batch("mlp_lbh_wgrad", B);
  hipLaunchKernelGGL(mlp_lbh_wgrad_kernel, dim3(FB + 1, lbh_layout(B).S), dim3(NW * 64), 0, stream,
                     xh, ws, B);
  DTFX_HIP_CHECK(hipGetLastError());
}

void mlp_lbh_reduce_launch(const float* ws, float* grad, int* ctr, float* stats, int stats_ring,
                           int B, hipStream_t stream, float* partials) {
  using namespace mlplbh;
  check_batch("mlp_lbh_reduce", B);
  const LbhLayout L = lbh_layout(B);
  mlp_lb_reduce_planes_launch(ws + L.planes, L.S, grad, ctr, stats, stats_ring, B, stream,
                              partials);
}

}  // namespace dtfx
