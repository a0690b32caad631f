// LARS on the mixed-precision flat buffer of the ResNet-50 trainer (f32 master + bf16 working
// copy): every tensor of the buffer in two launches, whatever their number.
//
// The rule (ops/layerwise.py: lars_mixed_update is the float64 definition): g = gscale * G per
// tensor, G its gradient range -- or, for a tensor whose weight gradient was left as S split-K
// planes (conv_bf16 defer_reduce), the sum of the planes in plane order.  Adapted tensors
// (convolution / fc weights): r = eta |p| / (|g| + wd |p|) when |p| > 0 and the denominator is
// > 0, else 1, and g' = r (g + wd p).  Excluded tensors (BatchNorm scales / offsets, biases):
// g' = g.  Then sgd_momentum_mixed's arithmetic on g': v = mu v + g'; p -= lr v; pb = bf16(p).
//
// optim.hip's lars kernels pass their segment table by value (8 segments) and know neither the
// bf16 copy, the planes nor an exclusion list.  Here the table lives in device memory:
//
//   tensor record (8 x int64): start, len (elements; the tensors tile [0, n) in order), flags
//     (bit 0: adapted), planes (f32 address, 0: not folded), plane stride (elements), S, first
//     workgroup (= index of its first pair of partials), plane length (elements the planes
//     cover; the record's padding behind them takes G from the gradient range).
//   workgroup record (1 x int64, after the tensor records): tensor | chunk << 32.
//
// A workgroup of 256 threads owns one chunk = 1,024 consecutive elements (one float4 per thread)
// of ONE tensor; starts and lengths are multiples of 4, so every access is a whole float4.
//
//   launch 1 (norms): G (planes summed in plane order, four loads in flight), p; the thread adds
//     its squares in element order, the wave by the fixed DPP tree, the four waves in wave order
//     through the LDS; thread 0 stores partials[workgroup] = (sum p^2, sum g^2).  No atomics.
//     Workgroups of an excluded, unfolded tensor have nothing to do and leave.
//   launch 2 (apply): an adapted tensor's workgroup adds the tensor's pairs itself -- thread t
//     takes chunks t, t + 256, ... in that order (the largest ResNet-50 tensor has 2,304), then
//     the same tree -- so the order depends on the table alone; r is formed once, in f32; the
//     update moves p, g, v as float4 and pb as four bf16 (8 bytes).
//
// Folded tensors: launch 1 STORES the plane sum (unscaled, what ResNet50.materialize_grads
// writes) into the gradient range and launch 2 reads that one stream, instead of summing the
// planes a second time.  In units of the tensor's size (3x3x512x512: 9.4 MB of f32), with S
// planes: storing moves S + 1 (planes, p) + 1 (store) in launch 1 and 3 + 2.5 in launch 2 =
// S + 7.5; summing twice moves S + 1 and S + 2 + 2.5 = 2 S + 5.5.  Storing is less for S > 2 and
// the wgrad workspace path splits deeper than that (20 planes on average over ResNet-50 at batch
// 256; S = 8: 146 MB against 203 MB for this tensor).  The planes themselves are only read, as sgd_momentum_mixed's
// segments leave them: the next step's weight gradient overwrites every plane, and the
// gradient range is cleared by the next backward like the rest of the gradient buffer.
//
// Launchers allocate nothing, clear nothing and never synchronise; lr and gscale are kernel
// arguments as in sgd_momentum_mixed; every result is bit-reproducible and graph-capturable.
#include <stdexcept>
#include <string>

#include "bf16.h"
#include "common.h"
#include "nn_api.h"

namespace dtfx {

constexpr int kLmChunk = 1024;  // elements per workgroup
constexpr int kLmRec = 8;       // int64 words per tensor record
enum : int { LM_START = 0, LM_LEN, LM_FLAGS, LM_PLANES, LM_PSTRIDE, LM_S, LM_WG0, LM_PLEN };

struct LmWork {        // what one thread owns (everything but `i` and `live` is wave-uniform)
  long long i;         // its first element in the flat buffer
  long long rel;       // ... relative to its tensor's start
  bool live;           // inside the tensor
  bool adapted;
  const float* planes; // null: G is the gradient range
  long long pstride, plen;
  int S;
  int wg0, nchunk;     // the tensor's workgroups [wg0, wg0 + nchunk)
};

__device__ __forceinline__ LmWork lm_work(const long long* __restrict__ tab, int ntensor) {
  const long long rec = tab[(long long)kLmRec * ntensor + blockIdx.x];
  const int t = (int)(rec & 0xffffffffLL), c = (int)(rec >> 32);
  const long long* T = tab + (long long)kLmRec * t;
  const long long len = T[LM_LEN];
  LmWork w;
  w.rel = (long long)c * kLmChunk + 4 * (int)threadIdx.x;
  w.i = T[LM_START] + w.rel;
  w.live = w.rel < len;
  w.adapted = (T[LM_FLAGS] & 1) != 0;
  w.planes = reinterpret_cast<const float*>(T[LM_PLANES]);
  w.pstride = T[LM_PSTRIDE];
  w.plen = T[LM_PLEN];
  w.S = (int)T[LM_S];
  w.wg0 = (int)T[LM_WG0];
  w.nchunk = (int)((len + kLmChunk - 1) / kLmChunk);
  return w;
}

// The thread's float4 of a folded tensor: the planes added in plane order, four loads in flight
// (sgd_momentum_mixed_segs_kernel's order and grouping).
__device__ __forceinline__ f32x4 lm_plane_sum(const LmWork& w) {
  const f32x4* q = reinterpret_cast<const f32x4*>(w.planes + w.rel);
  const long long pl = w.pstride >> 2;
  f32x4 gv = __builtin_nontemporal_load(q);
  int s = 1;
  for (; s + 3 < w.S; s += 4) {
    const f32x4 a0 = __builtin_nontemporal_load(q + s * pl),
                a1 = __builtin_nontemporal_load(q + (s + 1) * pl),
                a2 = __builtin_nontemporal_load(q + (s + 2) * pl),
                a3 = __builtin_nontemporal_load(q + (s + 3) * pl);
    gv += a0;
    gv += a1;
    gv += a2;
    gv += a3;
  }
  for (; s < w.S; ++s) gv += __builtin_nontemporal_load(q + s * pl);
  return gv;
}

__device__ __forceinline__ float lm_sq(const f32x4& x) {  // element order, no contraction
  float s = __fmul_rn(x[0], x[0]);
  s = __fmaf_rn(x[1], x[1], s);
  s = __fmaf_rn(x[2], x[2], s);
  return __fmaf_rn(x[3], x[3], s);
}

// A pair of sums over the workgroup, in every thread: DPP tree per wave, waves in wave order.
__device__ __forceinline__ void lm_block_sums(float& a, float& b) {
  __shared__ float lds[4][2];
  float s[2] = {a, b};
  wave_sum_n(s);
  if (lane_id() == 0) {
    lds[threadIdx.x >> 6][0] = s[0];
    lds[threadIdx.x >> 6][1] = s[1];
  }
  __syncthreads();
  a = ((lds[0][0] + lds[1][0]) + lds[2][0]) + lds[3][0];
  b = ((lds[0][1] + lds[1][1]) + lds[2][1]) + lds[3][1];
}

__global__ __launch_bounds__(256) void lars_mixed_norms_kernel(
    const long long* __restrict__ tab, int ntensor, const float* __restrict__ p,
    float* __restrict__ g, float* __restrict__ partials, float gscale) {
  const LmWork w = lm_work(tab, ntensor);
  if (!w.adapted && !w.planes) return;  // (uniform) no norm to take, nothing to fold
  float sp = 0.f, sg = 0.f;
  if (w.live) {
    f32x4 gv;
    if (w.planes && w.rel < w.plen) {
      gv = lm_plane_sum(w);
      *reinterpret_cast<f32x4*>(g + w.i) = gv;  // launch 2 (and nobody else) reads it back
    } else {
      gv = *reinterpret_cast<const f32x4*>(g + w.i);
    }
    const f32x4 pv = *reinterpret_cast<const f32x4*>(p + w.i);
    sp = lm_sq(pv);
    sg = lm_sq(gv * gscale);
  }
  if (!w.adapted) return;  // (uniform)
  lm_block_sums(sp, sg);
  if (threadIdx.x == 0)
    *reinterpret_cast<float2*>(partials + 2 * (long long)blockIdx.x) = make_float2(sp, sg);
}

__global__ __launch_bounds__(256) void lars_mixed_apply_kernel(
    const long long* __restrict__ tab, int ntensor, float* __restrict__ p,
    const float* __restrict__ g, float* __restrict__ v, unsigned short* __restrict__ pb,
    const float* __restrict__ partials, float lr, float mu, float wd, float eta, float gscale) {
  const LmWork w = lm_work(tab, ntensor);
  float r = 1.f;
  if (w.adapted) {  // (uniform: the barrier inside is reached by the whole workgroup)
    float sp = 0.f, sg = 0.f;
    for (int j = threadIdx.x; j < w.nchunk; j += 256) {
      const float2 q = *reinterpret_cast<const float2*>(partials + 2 * (long long)(w.wg0 + j));
      sp += q.x;
      sg += q.y;
    }
    lm_block_sums(sp, sg);
    const float pn = sqrtf(sp);
    const float den = __fmaf_rn(wd, pn, sqrtf(sg));
    if (pn > 0.f && den > 0.f) r = eta * pn / den;
  }
  if (!w.live) return;
  f32x4 pv = *reinterpret_cast<const f32x4*>(p + w.i), vv = *reinterpret_cast<const f32x4*>(v + w.i);
  const f32x4 gv = *reinterpret_cast<const f32x4*>(g + w.i);
  ushort4 o;
  unsigned short* op = (unsigned short*)&o;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float gs = gv[u] * gscale;
    const float g1 = w.adapted ? r * (gs + wd * pv[u]) : gs;
    vv[u] = mu * vv[u] + g1;
    pv[u] -= lr * vv[u];
    op[u] = tobf(pv[u]);
  }
  __builtin_nontemporal_store(pv, reinterpret_cast<f32x4*>(p + w.i));
  __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(v + w.i));
  if (pb) *reinterpret_cast<ushort4*>(pb + w.i) = o;
}

int lars_mixed_chunk() { return kLmChunk; }

// The table as the kernels will read it, checked on the host's copy: the tensors tile [0, n) in
// order on float4 boundaries, a folded tensor has planes that cover it, and workgroup record w
// is chunk c of tensor t exactly where the tensor records say so.
static void lars_mixed_check(long long n, const long long* tab, int ntensor, int nwg) {
  auto bad = [](const std::string& m) { throw std::runtime_error("lars_momentum_mixed: " + m); };
  if (n <= 0 || n % 4) bad("n must be a positive multiple of 4");
  if (!tab || ntensor < 1 || nwg < 1) bad("a table of at least one tensor and one workgroup");
  long long at = 0, wg = 0;
  const long long* W = tab + (long long)kLmRec * ntensor;
  for (int t = 0; t < ntensor; ++t) {
    const long long* T = tab + (long long)kLmRec * t;
    const std::string who = "tensor " + std::to_string(t);
    if (T[LM_START] != at)
      bad(who + " starts at " + std::to_string(T[LM_START]) + ", the one before it ends at " +
          std::to_string(at) + " (starts must increase and tile the buffer)");
    if (T[LM_START] % 4 || T[LM_LEN] <= 0 || T[LM_LEN] % 4)
      bad(who + ": start and length must be multiples of 4 elements (float4 alignment)");
    if (T[LM_FLAGS] & ~1LL) bad(who + ": unknown flags");
    if (T[LM_S] < 0 || T[LM_S] > 4096) bad(who + ": 0..4096 planes");
    if (T[LM_S] > 0) {
      if (!T[LM_PLANES] || (T[LM_PLANES] & 15)) bad(who + ": folded, but its planes are null or not 16-byte aligned");
      if (T[LM_PLEN] <= 0 || T[LM_PLEN] % 4 || T[LM_PLEN] > T[LM_LEN] ||
          T[LM_PSTRIDE] % 4 || T[LM_PSTRIDE] < T[LM_PLEN])
        bad(who + ": plane length / stride must be multiples of 4 with length <= stride and <= the tensor");
    } else if (T[LM_PLANES] || T[LM_PLEN] || T[LM_PSTRIDE]) {
      bad(who + ": planes without a plane count");
    }
    if (T[LM_WG0] != wg) bad(who + ": first workgroup does not follow the tensor before it");
    const long long nc = (T[LM_LEN] + kLmChunk - 1) / kLmChunk;
    if (wg + nc > nwg) bad("the workgroup records end before " + who + " does");
    for (long long c = 0; c < nc; ++c)
      if (W[wg + c] != ((long long)t | (c << 32)))
        bad("workgroup record " + std::to_string(wg + c) + " is not chunk " + std::to_string(c) +
            " of " + who);
    wg += nc;
    at += T[LM_LEN];
  }
  if (at != n)
    bad("the tensors end at " + std::to_string(at) + ", the buffer has " + std::to_string(n) +
        " elements");
  if (wg != nwg) bad("the table has " + std::to_string(nwg) + " workgroup records, its tensors need " + std::to_string(wg));
}

void lars_momentum_mixed_launch(long long n, float* p, float* g, float* v, void* pb, float lr,
                                float mu, float wd, float eta, float gscale,
                                const long long* tab_host, const long long* tab_dev, int ntensor,
                                int nwg, float* partials, hipStream_t st) {
  if (!p || !g || !v || !partials || !tab_dev) throw std::runtime_error("lars_momentum_mixed: null buffer");
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) |
       reinterpret_cast<uintptr_t>(v)) & 15)
    throw std::runtime_error("lars_momentum_mixed: p, g, v must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(pb) | reinterpret_cast<uintptr_t>(partials) |
       reinterpret_cast<uintptr_t>(tab_dev) | reinterpret_cast<uintptr_t>(tab_host)) & 7)
    throw std::runtime_error("lars_momentum_mixed: pb, partials and the table must be 8-byte aligned");
  lars_mixed_check(n, tab_host, ntensor, nwg);
  hipLaunchKernelGGL(lars_mixed_norms_kernel, dim3((unsigned)nwg), dim3(256), 0, st, tab_dev,
                     ntensor, p, g, partials, gscale);
  hipLaunchKernelGGL(lars_mixed_apply_kernel, dim3((unsigned)nwg), dim3(256), 0, st, tab_dev,
                     ntensor, p, g, v, (unsigned short*)pb, partials, lr, mu, wd, eta, gscale);
  DTFX_HIP_CHECK(hipGetLastError());
}

}  // namespace dtfx
