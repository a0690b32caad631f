// Per-epoch reshuffle of the device-resident MNIST batches (train/fused_mlp.py, shuffle=True):
// the reference's next_batch reshuffles the training set at every epoch boundary (worker.py:133,
// TF DataSet.next_batch); here the next epoch's order is WRITTEN between epochs, so the step
// kernels keep reading plain contiguous batches and no index load joins a step's critical path.
//
//   shuffle_rows : dst[w][j][:] = src[w][perm(seed, epoch, n)[j]][:]   (W planes of [n, 784] f32)
//                  dst_labels[j] = src_labels[perm(seed, epoch, n)[j]]
//
// perm is a stateless bijection of [0, n) (no permutation array, no sort, no RNG state): a
// balanced 4-round Feistel network over 2k bits, k = ceil(max(bitlen(n - 1), 2) / 2), whose
// round function is murmur3's fmix32 of (R ^ key_r) masked to k bits, cycle-walked into
// [0, n) (re-applied while the value is >= n: the walk ends, the start lies on the cycle).
// 32-bit unsigned arithmetic only: ops/shuffle.py computes the same values in numpy, bit for
// bit -- that function is the CPU reference and the order a resumed run reproduces.
//
// One wave per destination row: the row index is wave-uniform, so the source index is computed
// once per row on the scalar unit.  A row is 3,136 B = 196 x 16 B = 3 x 64 + 4 chunks: three
// full-wave 16-byte loads and a 4-lane tail, all issued before the first store.  Source rows are
// read once (non-temporal loads); destination rows are what the next epoch's steps read (plain
// stores).  The grid is capped and strides over the rows.
#include "common.h"
#include "f32_api.h"

#include <stdexcept>

namespace dtfx {

namespace shuffle {
constexpr int D = 784;             // floats per row
constexpr int CH = D / 4;          // 16-byte chunks per row (196)
constexpr int WAVES = 4;           // rows in flight per block
constexpr int MAX_BLOCKS = 2048;

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

struct Perm {
  uint32_t key[4];
  uint32_t k, mask, n;
};

// round keys of (seed, epoch) and the half width of n's domain (host side, once per launch)
static Perm make_perm(uint32_t seed, uint32_t epoch, uint32_t n) {
  Perm p;
  uint32_t bits = 0;
  for (uint32_t v = n - 1; v; v >>= 1) ++bits;
  if (bits < 2) bits = 2;
  p.k = (bits + 1) / 2;
  p.mask = (1u << p.k) - 1u;
  p.n = n;
  const uint32_t base = fmix32(fmix32(seed ^ 0x9E3779B9u) + epoch);
  for (uint32_t r = 0; r < 4; ++r) p.key[r] = fmix32(base + r + 1u);
  return p;
}

__host__ __device__ __forceinline__ uint32_t perm_index(const Perm& p, uint32_t j) {
  uint32_t v = j;
  do {
    uint32_t L = v >> p.k, R = v & p.mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t t = L ^ (fmix32(R ^ p.key[r]) & p.mask);
      L = R;
      R = t;
    }
    v = (L << p.k) | R;
  } while (v >= p.n);
  return v;
}
}  // namespace shuffle

__global__ __launch_bounds__(256) void shuffle_rows_kernel(
    float* __restrict__ dst, const float* __restrict__ src, int* __restrict__ dst_labels,
    const int* __restrict__ src_labels, shuffle::Perm perm, int planes, size_t dst_stride,
    size_t src_stride) {
  using namespace shuffle;
  const int lane = threadIdx.x & 63;
  // wave-uniform row index (kept in a scalar register: perm_index then runs on the scalar unit)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * WAVES;
  for (uint32_t j = blockIdx.x * WAVES + wave; j < perm.n; j += nwaves) {
    const uint32_t sj = perm_index(perm, j);
    if (dst_labels && lane == 0) dst_labels[j] = src_labels[sj];
    for (int w = 0; w < planes; ++w) {
      const f32x4* s = reinterpret_cast<const f32x4*>(src + (size_t)w * src_stride + (size_t)sj * D);
      f32x4* d = reinterpret_cast<f32x4*>(dst + (size_t)w * dst_stride + (size_t)j * D);
      const f32x4 a = __builtin_nontemporal_load(s + lane);
      const f32x4 b = __builtin_nontemporal_load(s + 64 + lane);
      const f32x4 c = __builtin_nontemporal_load(s + 128 + lane);
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (lane < CH - 192) t = __builtin_nontemporal_load(s + 192 + lane);
      d[lane] = a;
      d[64 + lane] = b;
      d[128 + lane] = c;
      if (lane < CH - 192) d[192 + lane] = t;
    }
  }
}

// dst / src: `planes` planes of [n, 784] f32, plane p at base + p * stride (strides in floats);
// labels: int32 [n] (both or neither).  The same permutation moves every plane and the labels.
void shuffle_rows_launch(float* dst, const float* src, int* dst_labels, const int* src_labels,
                         long long n, int planes, long long dst_stride, long long src_stride,
                         unsigned seed, unsigned epoch, hipStream_t stream) {
  using namespace shuffle;
  if (!dst || !src || n < 1 || n > 0x7fffffffLL || planes < 1)
    throw std::runtime_error("shuffle_rows: needs buffers, 1 <= n < 2^31 rows, planes >= 1");
  if ((dst_labels == nullptr) != (src_labels == nullptr))
    throw std::runtime_error("shuffle_rows: both label buffers or neither");
  const long long plane = n * D;
  if (planes > 1 && (dst_stride < plane || src_stride < plane))
    throw std::runtime_error("shuffle_rows: plane stride smaller than a plane");
  if (((uintptr_t)dst | (uintptr_t)src) % 16 ||
      (planes > 1 && ((dst_stride | src_stride) % 4)))
    throw std::runtime_error("shuffle_rows: bases and plane strides must be 16-byte aligned");
  // extents [base, base + (planes - 1) * stride + n * 784) must be disjoint
  const uintptr_t d0 = (uintptr_t)dst, s0 = (uintptr_t)src;
  const uintptr_t d1 = d0 + sizeof(float) * (size_t)((planes - 1) * dst_stride + plane);
  const uintptr_t s1 = s0 + sizeof(float) * (size_t)((planes - 1) * src_stride + plane);
  if (d0 < s1 && s0 < d1) throw std::runtime_error("shuffle_rows: dst and src overlap");
  if (dst_labels) {
    const uintptr_t a = (uintptr_t)dst_labels, b = (uintptr_t)src_labels;
    if (a < b + sizeof(int) * (size_t)n && b < a + sizeof(int) * (size_t)n)
      throw std::runtime_error("shuffle_rows: dst and src labels overlap");
  }
  const Perm perm = make_perm(seed, epoch, (uint32_t)n);
  long long blocks = (n + WAVES - 1) / WAVES;
  if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
  hipLaunchKernelGGL(shuffle_rows_kernel, dim3((unsigned)blocks), dim3(64 * WAVES), 0, stream, dst,
                     src, dst_labels, src_labels, perm, planes, (size_t)dst_stride,
                     (size_t)src_stride);
  DTFX_HIP_CHECK(hipGetLastError());
}

}  // namespace dtfx
