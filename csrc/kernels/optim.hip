// Multi-tensor optimizers over ONE flat f32 parameter buffer (every model
// parameter is a view into it), so a single launch updates all tensors.
//
//   sgd      : p -= lr * (g + wd * p)            (GradientDescentOptimizer,
//                                                 worker.py:71, ApplyGradientDescent)
//   momentum : v = mu * v + g' ; p -= lr * (nesterov ? g' + mu * v : v)
//   adam(w)  : bias-corrected Adam; decoupled weight decay when adamw
//   scale    : x *= alpha                        (gradient averaging)
//   ema      : shadow -= (1 - d_t) * (shadow - p) (tf.train.ExponentialMovingAverage;
//                                                 ops/ema.py is the definition)
//   lars     : momentum on g' = r_k (g + wd * p), r_k the segment's trust ratio
//   lamb     : Adam's direction u, p -= lr * r_k * u   (two launches each, see below;
//                                                 ops/layerwise.py is the definition)
//   clip     : g *= pre * clip / max(pre |g|, clip)   (tf.clip_by_global_norm; norm partials
//                                                 and scale, see below; ops/clip.py)
//
// The streaming loops are grid-stride over float4 (dwordx4) with a scalar tail.
// `lr_ptr` / `step_ptr` (optional) let a captured hipGraph pick up a device-side
// learning-rate schedule / step count instead of a frozen kernel argument.
#include "common.h"
#include "f32_api.h"
#include "gnorm.h"
#include "philox.h"

#include <cmath>
#include <stdexcept>

namespace dtfx {

static inline dim3 stream_grid(long long n4) {
  long long b = (n4 + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

__global__ __launch_bounds__(256) void sgd_kernel(long long n, float* __restrict__ p,
                                                  const float* __restrict__ g, float lr,
                                                  const float* __restrict__ lr_ptr, float wd) {
  const float l = lr_ptr ? *lr_ptr : lr;
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    pv.x -= l * (gv.x + wd * pv.x);
    pv.y -= l * (gv.y + wd * pv.y);
    pv.z -= l * (gv.z + wd * pv.z);
    pv.w -= l * (gv.w + wd * pv.w);
    reinterpret_cast<float4*>(p)[i] = pv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    p[i] -= l * (g[i] + wd * p[i]);
  }
}

__global__ __launch_bounds__(256) void momentum_kernel(long long n, float* __restrict__ p,
                                                       const float* __restrict__ g,
                                                       float* __restrict__ v, float lr,
                                                       const float* __restrict__ lr_ptr,
                                                       float mu, float wd, int nesterov) {
  const float l = lr_ptr ? *lr_ptr : lr;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gg = g[i] + wd * p[i];
    const float vv = mu * v[i] + gg;
    v[i] = vv;
    p[i] -= l * (nesterov ? gg + mu * vv : vv);
  }
}

__global__ __launch_bounds__(256) void adam_kernel(long long n, float* __restrict__ p,
                                                   const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   float lr, const float* __restrict__ lr_ptr,
                                                   float b1, float b2, float eps, float wd,
                                                   int adamw, int step,
                                                   const int* __restrict__ step_ptr) {
  const float l = lr_ptr ? *lr_ptr : lr;
  const int t = (step_ptr ? *step_ptr : step);
  const float bc1 = 1.f - powf(b1, (float)t);
  const float bc2 = 1.f - powf(b2, (float)t);
  const float step_size = l / bc1;
  const float rbc2 = rsqrtf(bc2);
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  auto upd = [&](float& pp, float gg, float& mm, float& vv) {
    if (!adamw) gg += wd * pp;
    mm = b1 * mm + (1.f - b1) * gg;
    vv = b2 * vv + (1.f - b2) * gg * gg;
    const float denom = sqrtf(vv) * rbc2 + eps;
    if (adamw) pp -= l * wd * pp;
    pp -= step_size * mm / denom;
  };
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    upd(pv.x, gv.x, mv.x, vv.x);
    upd(pv.y, gv.y, mv.y, vv.y);
    upd(pv.z, gv.z, mv.z, vv.z);
    upd(pv.w, gv.w, mv.w, vv.w);
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    upd(p[i], g[i], m[i], v[i]);
  }
}

__global__ __launch_bounds__(256) void scale_kernel(long long n, float* __restrict__ x, float a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] *= a;
}

// shadow -= (1 - d_t) * (shadow - p), in place on the shadow.  omd = 1 - decay; nu: d_t =
// min(decay, (1 + t) / (10 + t)), i.e. 1 - d_t = max(omd, 9 / (10 + t)) -- the fused step's
// arithmetic (mlp_step_opt.h: ema_omd), t = *step_ptr (a device counter, so a captured graph picks
// up the step) or `step`.  vec == 0 (a buffer that is not 16-byte aligned): the scalar loop alone.
__global__ __launch_bounds__(256) void ema_kernel(long long n, float* __restrict__ e,
                                                  const float* __restrict__ p, float omd, int nu,
                                                  int step, const int* __restrict__ step_ptr,
                                                  int vec) {
  float om = omd;
  if (nu) {  // (uniform: a kernel argument)
    const float t = (float)(step_ptr ? *step_ptr : step);
    om = fmaxf(omd, 9.f / (10.f + t));
  }
  const long long n4 = vec ? n >> 2 : 0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = i0; i < n4; i += stride) {
    float4 ev = reinterpret_cast<float4*>(e)[i];
    const float4 pv = reinterpret_cast<const float4*>(p)[i];
    ev.x -= om * (ev.x - pv.x);
    ev.y -= om * (ev.y - pv.y);
    ev.z -= om * (ev.z - pv.z);
    ev.w -= om * (ev.w - pv.w);
    reinterpret_cast<float4*>(e)[i] = ev;
  }
  for (long long i = (n4 << 2) + i0; i < n; i += stride) e[i] -= om * (e[i] - p[i]);
}

__global__ void counter_add_kernel(int* c, int d) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *c += d;
}

static void check_align(const void* p, const char* what) {
  if (reinterpret_cast<uintptr_t>(p) & 15)
    throw std::runtime_error(std::string(what) + ": buffer must be 16-byte aligned");
}

void sgd_launch(long long n, float* p, const float* g, float lr, const float* lr_ptr, float wd,
                hipStream_t s) {
  if (n <= 0) return;
  check_align(p, "sgd");
  check_align(g, "sgd");
  hipLaunchKernelGGL(sgd_kernel, stream_grid(n >> 2), dim3(256), 0, s, n, p, g, lr, lr_ptr, wd);
  DTFX_HIP_CHECK(hipGetLastError());
}

void momentum_launch(long long n, float* p, const float* g, float* v, float lr,
                     const float* lr_ptr, float mu, float wd, bool nesterov, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(momentum_kernel, stream_grid(n), dim3(256), 0, s, n, p, g, v, lr, lr_ptr, mu,
                     wd, nesterov ? 1 : 0);
  DTFX_HIP_CHECK(hipGetLastError());
}

void adam_launch(long long n, float* p, const float* g, float* m, float* v, float lr,
                 const float* lr_ptr, float b1, float b2, float eps, float wd, bool adamw,
                 int step, const int* step_ptr, hipStream_t s) {
  if (n <= 0) return;
  check_align(p, "adam");
  check_align(g, "adam");
  check_align(m, "adam");
  check_align(v, "adam");
  hipLaunchKernelGGL(adam_kernel, stream_grid(n >> 2), dim3(256), 0, s, n, p, g, m, v, lr, lr_ptr,
                     b1, b2, eps, wd, adamw ? 1 : 0, step, step_ptr);
  DTFX_HIP_CHECK(hipGetLastError());
}

void ema_launch(long long n, float* shadow, const float* p, float omd, bool num_updates, int step,
                const int* step_ptr, hipStream_t s) {
  if (n <= 0) return;
  if (!shadow || !p) throw std::runtime_error("ema: null buffer");
  if (!(omd > 0.f && omd < 1.f)) throw std::runtime_error("ema: decay must lie in (0, 1)");
  const bool vec =
      ((reinterpret_cast<uintptr_t>(shadow) | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
  hipLaunchKernelGGL(ema_kernel, stream_grid(vec ? n >> 2 : n), dim3(256), 0, s, n, shadow, p, omd,
                     num_updates ? 1 : 0, step, step_ptr, vec ? 1 : 0);
  DTFX_HIP_CHECK(hipGetLastError());
}

void scale_launch(long long n, float* x, float a, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(scale_kernel, stream_grid(n), dim3(256), 0, s, n, x, a);
  DTFX_HIP_CHECK(hipGetLastError());
}

void counter_add_launch(int* c, int d, hipStream_t s) {
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(64), 0, s, c, d);
  DTFX_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Layer-wise adaptive rates: LARS and LAMB (ops/layerwise.py has the definition).
//
// Both rules need the Euclidean norm of every parameter tensor (a *segment* of the flat buffer)
// between forming the update direction and applying it, so each is two launches over ONE
// segment-aligned grid: a workgroup of 256 threads owns 1,024 consecutive elements (one float4 per
// thread) of ONE segment -- segment k owns ceil(len_k / 1024) consecutive workgroups, none
// straddles two segments, and a workgroup finds its segment by a wave-uniform scan of the (at
// most 8) block-count prefixes in the by-value LwSegs.
//
//   launch 1 (norms): every thread squares its float4 of the two vectors whose norms the rule
//     takes (lars: p, g; lamb: p, u -- lamb also writes the new m, v here), adds the four squares
//     in element order, the wave adds its 64 lanes by the fixed DPP tree (wave_sum_n), the four
//     waves meet in the LDS and are added in wave order, and thread 0 stores the pair to
//     partials[block][2].  No atomics; elements past the segment's end contribute +0.
//   launch 2 (apply): every WAVE of a workgroup adds its segment's partial pairs itself --
//     lane-strided in block order, then the same fixed tree -- so the order is a function of the
//     segment table alone, every wave of the segment sees the same bits, and no LDS or barrier is
//     needed (the MLP's largest segment has 77 pairs: two 8-byte loads per lane, where a serial
//     uniform loop is 77 dependent scalar loads).  It forms the trust ratio r_k once (f32 sqrtf,
//     one division) and applies the update.  lamb recomputes u from the stored m, v and the
//     still-unchanged p through lamb_u(), the function launch 1 used, so both launches see the
//     same bits and no 318 KB scratch plane of u is written and read back.
//
// Launchers allocate nothing, clear nothing and never synchronise: `partials` is the caller's
// (2 floats per workgroup), lr_ptr / step_ptr are read on the device as adam_kernel reads them,
// and every result is bit-reproducible and graph-capturable.
// ---------------------------------------------------------------------------
constexpr int kLwBlock = 1024;  // elements per workgroup

struct LwWork {   // what one thread owns
  int seg;        // its segment
  int blk0, blk1; // the segment's workgroups [blk0, blk1)
  long long i;    // its first element
  int nv;         // live elements of its float4: 0..4 (< 4 only at the buffer's ragged end)
};

__device__ __forceinline__ LwWork lw_work(const LwSegs& sg) {
  const int b = blockIdx.x;
  int k = 0;
#pragma unroll
  for (int i = 1; i < kLwMaxSegments; ++i)  // (uniform: blockIdx and kernel arguments only)
    if (i < sg.nseg && b >= sg.blk[i]) k = i;
  int off0 = sg.off[0], off1 = sg.off[1], blk0 = sg.blk[0], blk1 = sg.blk[1];
#pragma unroll
  for (int i = 1; i < kLwMaxSegments; ++i)  // (selects with constant indices: no private array)
    if (k == i) { off0 = sg.off[i]; off1 = sg.off[i + 1]; blk0 = sg.blk[i]; blk1 = sg.blk[i + 1]; }
  LwWork w;
  w.seg = k;
  w.blk0 = blk0;
  w.blk1 = blk1;
  w.i = (long long)off0 + (long long)(b - blk0) * kLwBlock + 4 * (int)threadIdx.x;
  const long long left = (long long)off1 - w.i;
  w.nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  return w;
}

// A thread's up-to-four values: one dwordx4 when whole, the scalar tail otherwise (dead lanes 0).
__device__ __forceinline__ float4 lw_load(const float* __restrict__ x, const LwWork& w) {
  if (w.nv == 4) return *reinterpret_cast<const float4*>(x + w.i);
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (w.nv > 0) r.x = x[w.i];
  if (w.nv > 1) r.y = x[w.i + 1];
  if (w.nv > 2) r.z = x[w.i + 2];
  return r;
}
__device__ __forceinline__ void lw_store(float* __restrict__ x, const LwWork& w, float4 r) {
  if (w.nv == 4) {
    *reinterpret_cast<float4*>(x + w.i) = r;
    return;
  }
  if (w.nv > 0) x[w.i] = r.x;
  if (w.nv > 1) x[w.i + 1] = r.y;
  if (w.nv > 2) x[w.i + 2] = r.z;
}

// (lw_sq, the sum of squares of a thread's values in element order: gnorm.h)

// The workgroup's pair of sums -> partials[block][2]: DPP tree per wave, waves in wave order.
__device__ __forceinline__ void lw_block_sums(float a, float b, float* __restrict__ partials) {
  __shared__ float lds[4][2];
  float s[2] = {a, b};
  wave_sum_n(s);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) {
    lds[wave][0] = s[0];
    lds[wave][1] = s[1];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s0 = ((lds[0][0] + lds[1][0]) + lds[2][0]) + lds[3][0];
    const float s1 = ((lds[0][1] + lds[1][1]) + lds[2][1]) + lds[3][1];
    *reinterpret_cast<float2*>(partials + 2 * (long long)blockIdx.x) = make_float2(s0, s1);
  }
}

// The segment's pair of sums, in every lane of the calling wave: lane l adds the pairs of blocks
// blk0 + l, blk0 + l + 64, ... in that order, then the fixed tree.
__device__ __forceinline__ void lw_segment_sums(const float* __restrict__ partials,
                                                const LwWork& w, float& a, float& b) {
  float s[2] = {0.f, 0.f};
  for (int j = w.blk0 + lane_id(); j < w.blk1; j += kWave) {
    const float2 v = *reinterpret_cast<const float2*>(partials + 2 * (long long)j);
    s[0] += v.x;
    s[1] += v.y;
  }
  wave_sum_n(s);
  a = s[0];
  b = s[1];
}

// LAMB's bias corrections and update direction: ONE definition for both launches (explicit fma /
// mul, so no contraction choice can differ between them).  lb = log(beta), rounded once from the
// host's double: 1 - beta^t = -expm1(t log beta) keeps its relative accuracy at small t, where
// 1.f - powf(0.999f, t) loses five digits to the rounding of beta -- a segment with r = 1 (no
// norm to cancel a common factor of u) shows it.
__device__ __forceinline__ void lamb_corr(float lb1, float lb2, int t, float& rbc1, float& rbc2) {
  rbc1 = 1.f / -expm1f((float)t * lb1);
  rbc2 = rsqrtf(-expm1f((float)t * lb2));
}
__device__ __forceinline__ float lamb_u(float p, float m, float v, float rbc1, float rbc2,
                                        float eps, float wd) {
  const float q = __fmul_rn(m, rbc1) / __fmaf_rn(sqrtf(v), rbc2, eps);
  return __fmaf_rn(wd, p, q);
}

__global__ __launch_bounds__(256) void lars_norms_kernel(LwSegs sg, const float* __restrict__ p,
                                                         const float* __restrict__ g,
                                                         float* __restrict__ partials) {
  const LwWork w = lw_work(sg);
  lw_block_sums(lw_sq(lw_load(p, w)), lw_sq(lw_load(g, w)), partials);
}

__global__ __launch_bounds__(256) void lars_apply_kernel(LwSegs sg, float* __restrict__ p,
                                                         const float* __restrict__ g,
                                                         float* __restrict__ v,
                                                         const float* __restrict__ partials,
                                                         float lr, const float* __restrict__ lr_ptr,
                                                         float mu, float eta, float wd) {
  const LwWork w = lw_work(sg);
  const float l = lr_ptr ? *lr_ptr : lr;
  float sp, sgg;
  lw_segment_sums(partials, w, sp, sgg);
  const float pn = sqrtf(sp);
  const float den = __fmaf_rn(wd, pn, sqrtf(sgg));
  const float r = (pn > 0.f && den > 0.f) ? eta * pn / den : 1.f;
  if (w.nv == 0) return;
  float4 pv = lw_load(p, w), vv = lw_load(v, w);
  const float4 gv = lw_load(g, w);
  auto upd = [&](float& pp, float gg, float& ac) {  // momentum_kernel's arithmetic on g'
    const float g1 = r * (gg + wd * pp);
    ac = mu * ac + g1;
    pp -= l * ac;
  };
  upd(pv.x, gv.x, vv.x);
  upd(pv.y, gv.y, vv.y);
  upd(pv.z, gv.z, vv.z);
  upd(pv.w, gv.w, vv.w);
  lw_store(p, w, pv);
  lw_store(v, w, vv);
}

__global__ __launch_bounds__(256) void lamb_norms_kernel(LwSegs sg, const float* __restrict__ p,
                                                         const float* __restrict__ g,
                                                         float* __restrict__ m,
                                                         float* __restrict__ v,
                                                         float* __restrict__ partials, float b1,
                                                         float b2, float omb1, float omb2,
                                                         float lb1, float lb2, float eps,
                                                         float wd, int step,
                                                         const int* __restrict__ step_ptr) {
  const LwWork w = lw_work(sg);
  float rbc1, rbc2;
  lamb_corr(lb1, lb2, step_ptr ? *step_ptr : step, rbc1, rbc2);
  const float4 pv = lw_load(p, w), gv = lw_load(g, w);
  float4 mv = lw_load(m, w), vv = lw_load(v, w), u;
  // omb1 / omb2: 1 - beta rounded ONCE from the host's double (1.f - 0.999f is off by 1.3e-5 of
  // itself, which a second moment of large gradients shows)
  auto mom = [&](float pp, float gg, float& mm, float& v2) {
    mm = b1 * mm + omb1 * gg;
    v2 = b2 * v2 + omb2 * gg * gg;
    return lamb_u(pp, mm, v2, rbc1, rbc2, eps, wd);
  };
  u.x = mom(pv.x, gv.x, mv.x, vv.x);
  u.y = mom(pv.y, gv.y, mv.y, vv.y);
  u.z = mom(pv.z, gv.z, mv.z, vv.z);
  u.w = mom(pv.w, gv.w, mv.w, vv.w);
  // (dead lanes add +0 like everything else, also where eps = 0 makes their 0 / 0 a NaN)
  if (w.nv < 4) u.w = 0.f;
  if (w.nv < 3) u.z = 0.f;
  if (w.nv < 2) u.y = 0.f;
  if (w.nv < 1) u.x = 0.f;
  lw_store(m, w, mv);
  lw_store(v, w, vv);
  lw_block_sums(lw_sq(pv), lw_sq(u), partials);
}

__global__ __launch_bounds__(256) void lamb_apply_kernel(LwSegs sg, float* __restrict__ p,
                                                         const float* __restrict__ m,
                                                         const float* __restrict__ v,
                                                         const float* __restrict__ partials,
                                                         float lr, const float* __restrict__ lr_ptr,
                                                         float lb1, float lb2, float eps,
                                                         float wd, int step,
                                                         const int* __restrict__ step_ptr) {
  const LwWork w = lw_work(sg);
  const float l = lr_ptr ? *lr_ptr : lr;
  float rbc1, rbc2;
  lamb_corr(lb1, lb2, step_ptr ? *step_ptr : step, rbc1, rbc2);
  float sp, su;
  lw_segment_sums(partials, w, sp, su);
  const float pn = sqrtf(sp), un = sqrtf(su);
  const float lr_r = (pn > 0.f && un > 0.f) ? l * (pn / un) : l;
  if (w.nv == 0) return;
  float4 pv = lw_load(p, w);
  const float4 mv = lw_load(m, w), vv = lw_load(v, w);
  pv.x -= lr_r * lamb_u(pv.x, mv.x, vv.x, rbc1, rbc2, eps, wd);
  pv.y -= lr_r * lamb_u(pv.y, mv.y, vv.y, rbc1, rbc2, eps, wd);
  pv.z -= lr_r * lamb_u(pv.z, mv.z, vv.z, rbc1, rbc2, eps, wd);
  pv.w -= lr_r * lamb_u(pv.w, mv.w, vv.w, rbc1, rbc2, eps, wd);
  lw_store(p, w, pv);
}

// The segment table of a flat buffer of n elements cut at offsets[0..nseg] (offsets[0] = 0,
// offsets[nseg] = n): throws unless there are 1..8 non-empty segments, every start a multiple of
// 4 elements (only the buffer's end may be ragged) and the buffers are 16-byte aligned.
LwSegs layerwise_segments(const long long* offsets, int nseg) {
  if (nseg < 1 || nseg > kLwMaxSegments)
    throw std::runtime_error("layerwise: 1.." + std::to_string(kLwMaxSegments) +
                             " segments, got " + std::to_string(nseg));
  if (offsets[0] != 0) throw std::runtime_error("layerwise: the first segment starts at 0");
  LwSegs sg = {};
  sg.nseg = nseg;
  long long blocks = 0;
  for (int k = 0; k < nseg; ++k) {
    const long long a = offsets[k], b = offsets[k + 1];
    if (b <= a) throw std::runtime_error("layerwise: segment offsets must increase");
    if (a & 3)
      throw std::runtime_error("layerwise: every segment must start at a multiple of 4 elements "
                               "(got " + std::to_string(a) + ")");
    if (b > 0x7fffffffLL - kLwBlock || blocks + (b - a + kLwBlock - 1) / kLwBlock > 0x3fffffffLL)
      throw std::runtime_error("layerwise: buffer too large");
    sg.off[k] = (int)a;
    sg.blk[k] = (int)blocks;
    blocks += (b - a + kLwBlock - 1) / kLwBlock;
  }
  for (int k = nseg; k <= kLwMaxSegments; ++k) {  // (unused entries: the end, so any scan is safe)
    sg.off[k] = (int)offsets[nseg];
    sg.blk[k] = (int)blocks;
  }
  return sg;
}

int layerwise_blocks(const LwSegs& sg) { return sg.blk[sg.nseg]; }

void lars_launch(const LwSegs& sg, float* p, const float* g, float* v, float* partials, float lr,
                 const float* lr_ptr, float mu, float eta, float wd, hipStream_t s) {
  if (!p || !g || !v || !partials) throw std::runtime_error("lars: null buffer");
  check_align(p, "lars");
  check_align(g, "lars");
  check_align(v, "lars");
  if (reinterpret_cast<uintptr_t>(partials) & 7)
    throw std::runtime_error("lars: partials must be 8-byte aligned");
  const dim3 grid((unsigned)layerwise_blocks(sg));
  hipLaunchKernelGGL(lars_norms_kernel, grid, dim3(256), 0, s, sg, p, g, partials);
  hipLaunchKernelGGL(lars_apply_kernel, grid, dim3(256), 0, s, sg, p, g, v, partials, lr, lr_ptr,
                     mu, eta, wd);
  DTFX_HIP_CHECK(hipGetLastError());
}

void lamb_launch(const LwSegs& sg, float* p, const float* g, float* m, float* v, float* partials,
                 float lr, const float* lr_ptr, double beta1, double beta2, float eps, float wd,
                 int step, const int* step_ptr, hipStream_t s) {
  if (!p || !g || !m || !v || !partials) throw std::runtime_error("lamb: null buffer");
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0))
    throw std::runtime_error("lamb: beta1 and beta2 must lie in [0, 1)");
  const float b1 = (float)beta1, b2 = (float)beta2;
  const float lb1 = (float)std::log(beta1), lb2 = (float)std::log(beta2);  // (-inf at 0: bc = 1)
  check_align(p, "lamb");
  check_align(g, "lamb");
  check_align(m, "lamb");
  check_align(v, "lamb");
  if (reinterpret_cast<uintptr_t>(partials) & 7)
    throw std::runtime_error("lamb: partials must be 8-byte aligned");
  const dim3 grid((unsigned)layerwise_blocks(sg));
  hipLaunchKernelGGL(lamb_norms_kernel, grid, dim3(256), 0, s, sg, p, g, m, v, partials, b1, b2,
                     (float)(1.0 - beta1), (float)(1.0 - beta2), lb1, lb2, eps, wd, step,
                     step_ptr);
  hipLaunchKernelGGL(lamb_apply_kernel, grid, dim3(256), 0, s, sg, p, m, v, partials, lr, lr_ptr,
                     lb1, lb2, eps, wd, step, step_ptr);
  DTFX_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Clipping by the global norm (ops/clip.py has the definition): g *= clip / max(|g|, clip), |g|
// the Euclidean norm of the WHOLE flat gradient, fused with the gradient averaging the
// all-reduce engine does anyway (`pre` = 1 / world): the norm of pre * g is pre * |g|, so the
// partial sums may be taken from the unscaled buffer and ONE multiplier does both.
//
// The layer-wise geometry with the buffer as one segment: a workgroup of 256 threads owns 1,024
// consecutive elements, one float4 per thread, the ragged end through lw_load / lw_store.
//
//   gnorm_partials : sum of squares per workgroup -> partials[block] (gnorm.h: element order,
//     fixed DPP tree, waves in wave order; elements past n contribute +0).  The large-batch
//     reduce launch writes the same partials for the gradient it stores (mlp_large_batch.hip,
//     CLIP instantiation: the same geometry, the same bits), and this launch is then skipped.
//   clip_scale : every WAVE re-adds all nblk partials itself -- lane-strided in block order, then
//     the fixed tree, as lw_segment_sums does (the MLP's gradient has 78: a second trip for 14
//     lanes) -- and forms norm = pre * sqrtf(sum) and the multiplier f = pre * clip / max(norm,
//     clip) once: one IEEE division, so pre = 1 and norm <= clip give exactly 1.0f and the
//     gradient's bits do not move.  A NaN norm takes max()'s other operand (f = pre): the
//     non-finite elements stay non-finite, no special case.  One lane stores the norm.
//
// The re-add is O(nblk) loads per wave: meant for gradients of up to a few million elements.
// Launchers allocate nothing, clear nothing and never synchronise.
// ---------------------------------------------------------------------------
__device__ __forceinline__ LwWork gn_work(long long n) {
  LwWork w;
  w.seg = 0;
  w.blk0 = 0;
  w.blk1 = (int)gridDim.x;
  w.i = (long long)blockIdx.x * kLwBlock + 4 * (int)threadIdx.x;
  const long long left = n - w.i;
  w.nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  return w;
}

__global__ __launch_bounds__(256) void gnorm_partials_kernel(long long n,
                                                             const float* __restrict__ g,
                                                             float* __restrict__ partials) {
  gn_block_sum(lw_sq(lw_load(g, gn_work(n))), partials);
}

__global__ __launch_bounds__(256) void clip_scale_kernel(long long n, float* __restrict__ g,
                                                         const float* __restrict__ partials,
                                                         int nblk, float clip, float pre,
                                                         float* __restrict__ gnorm_out) {
  const LwWork w = gn_work(n);
  float s = 0.f;
  for (int j = lane_id(); j < nblk; j += kWave) s += partials[j];  // block order per lane
  s = wave_sum(s);
  const float norm = __fmul_rn(pre, sqrtf(s));
  const float f = __fdiv_rn(__fmul_rn(pre, clip), fmaxf(norm, clip));
  if (gnorm_out && blockIdx.x == 0 && threadIdx.x == 0) *gnorm_out = norm;
  if (w.nv == 0) return;
  float4 v = lw_load(g, w);
  v.x *= f;
  v.y *= f;
  v.z *= f;
  v.w *= f;
  lw_store(g, w, v);
}

int gnorm_blocks(long long n) {
  if (n < 1 || n > 0x7fffffffLL - kLwBlock)
    throw std::runtime_error("gnorm: the buffer must have 1 .. 2^31 - 1025 elements, got " +
                             std::to_string(n));
  return (int)((n + kLwBlock - 1) / kLwBlock);
}

void gnorm_partials_launch(long long n, const float* g, float* partials, hipStream_t s) {
  const int nblk = gnorm_blocks(n);
  if (!g || !partials) throw std::runtime_error("gnorm_partials: null buffer");
  check_align(g, "gnorm_partials");
  hipLaunchKernelGGL(gnorm_partials_kernel, dim3((unsigned)nblk), dim3(256), 0, s, n, g, partials);
  DTFX_HIP_CHECK(hipGetLastError());
}

void clip_scale_launch(long long n, float* g, const float* partials, int nblk, float clip,
                       float pre, float* gnorm_out, hipStream_t s) {
  if (nblk != gnorm_blocks(n))
    throw std::runtime_error("clip_scale: " + std::to_string(n) + " elements have " +
                             std::to_string(gnorm_blocks(n)) + " partial sums, got " +
                             std::to_string(nblk));
  if (!g || !partials) throw std::runtime_error("clip_scale: null buffer");
  if (!(clip > 0.f) || !std::isfinite(clip))
    throw std::runtime_error("clip_scale: clip_norm must be finite and > 0");
  if (!(pre > 0.f) || !std::isfinite(pre))
    throw std::runtime_error("clip_scale: the pre-scale must be finite and > 0");
  check_align(g, "clip_scale");
  hipLaunchKernelGGL(clip_scale_kernel, dim3((unsigned)nblk), dim3(256), 0, s, n, g, partials,
                     nblk, clip, pre, gnorm_out);
  DTFX_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Philox4x32-10 counter-based RNG init (tf.random_normal_initializer,
// worker.py:51,53; truncated normal / uniform for the extension models).
// mode 0: normal(a = mean, b = std)   1: uniform[a, b)
// mode 2: truncated normal (|z| <= 2, redrawn), mean a, std b
// ---------------------------------------------------------------------------
__device__ __forceinline__ float u01(unsigned x) {  // (0, 1]
  return ((float)(x >> 8) + 1.f) * (1.f / 16777216.f);
}

__global__ __launch_bounds__(256) void philox_init_kernel(long long n, float* __restrict__ out,
                                                          unsigned long long seed,
                                                          unsigned long long offset, int mode,
                                                          float a, float b) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i * 4 < n; i += stride) {
    float v[4];
    bool done[4] = {false, false, false, false};
    for (int round = 0; round < (mode == 2 ? 16 : 1); ++round) {
      const unsigned long long ctr = (unsigned long long)i;
      const U4 r = philox10(U4{(unsigned)ctr, (unsigned)(ctr >> 32),
                               (unsigned)offset + (unsigned)round, (unsigned)(offset >> 32)},
                            k0, k1);
      float z[4];
      if (mode == 1) {
        z[0] = u01(r.x); z[1] = u01(r.y); z[2] = u01(r.z); z[3] = u01(r.w);
      } else {
        const float r0 = sqrtf(-2.f * __logf(u01(r.x))), t0 = 6.283185307179586f * u01(r.y);
        const float r1 = sqrtf(-2.f * __logf(u01(r.z))), t1 = 6.283185307179586f * u01(r.w);
        z[0] = r0 * __cosf(t0); z[1] = r0 * __sinf(t0);
        z[2] = r1 * __cosf(t1); z[3] = r1 * __sinf(t1);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (done[e]) continue;
        if (mode == 2 && fabsf(z[e]) > 2.f && round < 15) continue;
        if (mode == 2 && fabsf(z[e]) > 2.f) z[e] = copysignf(2.f, z[e]);
        v[e] = (mode == 1) ? (a + (b - a) * (1.f - z[e])) : (a + b * z[e]);
        done[e] = true;
      }
      if (done[0] && done[1] && done[2] && done[3]) break;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i * 4 + e < n) out[i * 4 + e] = v[e];
  }
}

void philox_init_launch(long long n, float* out, unsigned long long seed,
                        unsigned long long offset, int mode, float a, float b, hipStream_t s) {
  if (n <= 0) return;
  if (mode < 0 || mode > 2) throw std::runtime_error("philox_init: mode must be 0, 1 or 2");
  hipLaunchKernelGGL(philox_init_kernel, stream_grid((n + 3) >> 2), dim3(256), 0, s, n, out, seed,
                     offset, mode, a, b);
  DTFX_HIP_CHECK(hipGetLastError());
}

}  // namespace dtfx
