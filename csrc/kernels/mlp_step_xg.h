// Fused MLP step (mlp_step.hip): the xGMI exchange engines -- the LL-word gradient exchanges a
// wave runs in its epilogue (xg_exchange, xg_exchange16, xg_exchange2p, xg_exchange2) and the
// factor engines' dz1 all-gather of one head row (head_allgather).  Protocol words: xgmi_ll.h.
#pragma once
#include "mlp_step_ws.h"
#include "xgmi_ll.h"

namespace dtfx {
namespace mlp {

// 16-byte LL layout of the one-shot split exchange (mlp_fwdapply_kernel<.., XW, .., TWO =
// false> with DTFX_XG_SPLIT bit 0): word pair of (exchange slot, K-split wave, lane) at
// XG_W1_BASE + ((eslot * 2 + sp) * 64 + lane) * 2 -- past the parameter-offset region of
// the small parameters; a communicator needs XG_SLOT_WORDS words per slot for it.
constexpr long long XG_W1_BASE = 79616;
constexpr long long XG_SLOT_WORDS = XG_W1_BASE + (long long)HT * KS3 * 2 * 2 * 64 * 2;

// The factor engines' dz1 all-gather of one head row (mlp_head_kernel<.., XW>): BL = polls as
// 16-byte buffer loads and pushes as global stores (DTFX_XG_SPLIT bit 4, as xg_exchange2p).
template <int XW, bool BL>
__device__ __forceinline__ void head_allgather(const MlpXg& xg, unsigned ep, int row, int lane,
                                               int BP, const float (&dzv)[2],
                                               float* __restrict__ dz1A, bool& fail) {
  {
    // the row's 100 factors travel as 50 16-byte word pairs {dz(2l), ep, dz(2l+1), ep} at
    // word row * HP + 2l of slot (parity, me) -- a wave's pushes and polls are contiguous
    // 800-B runs, one store / load per lane and peer -- and land in dz1A [XW][BP][HP] row-major
    // (one 8-byte store per lane and rank).  Each 8-byte half carries the epoch (as
    // xg_exchange16); every poll is issued before the pushes (xgll::first_loads).
    using xgll::u64;
    using xgll::u32x4;
    const long long par = ep & 1u, plane = (long long)HP * BP;
    const int me = xgll::uniform(xg.rank);
    const bool act = lane < H / 2;
    const long long woff = (long long)row * HP + 2 * (act ? lane : 0);
    auto slot = [&](int dst, int src) {
      return xgll::uniform_ptr((u64*)xg.peers.data[dst]) + (par * XW + src) * xg.S + woff;
    };
    const xgll::OwnPoll pr(BL ? xgll::uniform_ptr((const u64*)xg.peers.data[me]) : nullptr);
    auto poll = [&](int q) {
      if constexpr (BL) return pr.pair((par * XW + q) * xg.S, woff);
      else return xgll::load_pair(slot(me, q));
    };
    u32x4 wq[XW];
#pragma unroll
    for (int q = 0; q < XW; ++q)
      if (act && q != me) wq[q] = poll(q);
    if (act) {
      const u32x4 out = {__float_as_uint(dzv[0]), ep, __float_as_uint(dzv[1]), ep};
#pragma unroll
      for (int d = 0; d < XW; ++d)
        if (d != me) {
          if constexpr (BL) xgll::store_pair_g(slot(d, me), out);
          else *(u32x4*)slot(d, me) = out;
        }
    }
    if (act) {
      const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
      for (;;) {
        bool ready = true;
#pragma unroll
        for (int q = 0; q < XW; ++q)
          if (q != me && (wq[q].y != ep || wq[q].w != ep)) {
            ready = false;
            wq[q] = poll(q);
          }
        if (ready) break;
        if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > xg.ticks) {
          fail = true;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
#pragma unroll
      for (int q = 0; q < XW; ++q) {
        const float2 v = q == me ? make_float2(dzv[0], dzv[1])
                                 : make_float2(__uint_as_float(wq[q].x), __uint_as_float(wq[q].z));
        *reinterpret_cast<float2*>(&dz1A[q * plane + woff]) = v;
      }
    }
  }
}

// Fused xGMI gradient exchange over XW ranks (mlp_wgrad_kernel<.., XW>, wgrad_small,
// fwdapply_block<.., XW>): a lane's N elements, summed in rank order.
template <int XW, int N = 4>
__device__ __forceinline__ void xg_exchange(const MlpXg& xg, unsigned ep, const size_t (&off)[N],
                                            const bool (&ok)[N], float (&v)[N], bool& fail) {
  using xgll::u64;
  const long long par = ep & 1u;
  const int me = xgll::uniform(xg.rank);
  auto local = [&](int j) { return (const u64*)xg.peers.data[me] + (par * XW + j) * xg.S; };
  u64 w[N][XW];  // first polls before the pushes (xgll::first_loads: one vmcnt for both)
  xgll::first_loads<XW, N>(local, off, ok, me, ep, w);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (!ok[i]) continue;
    const u64 wd = xgll::word(v[i], ep);
#pragma unroll
    for (int d = 0; d < XW; ++d)
      if (d != me) xgll::store((u64*)xg.peers.data[d] + (par * XW + me) * xg.S + off[i], wd);
  }
  if (!fail) xgll::finish_sum_n<XW, N>(local, off, ok, me, ep, w, v, xg.ticks, fail);
}

// Two-shot form of xg_exchange (reduce-scatter + all-gather inside the wave): element i of
// lane l (hidden row 4 q + i of the tile, q = l / 16) is owned by rank (q + 4 i) % XW -- the
// same on every rank, and one owner per 16-lane row segment, so every push below writes whole
// 128-byte runs.  (1) a non-owned value goes to its owner only (slot (par, me) of the owner),
// (2) the owner sums the XW contributions in rank order and pushes the sum into every peer's
// result region (2 XW + par) -- the push layout's last two slots --, (3) a non-owned element
// waits for its owner's sum.  Per rank 2 (XW-1)/XW words per element cross the links instead
// of XW-1 (at 8 ranks 1.75 vs 7), for one more dependent hop.  Every rank pushes before it
// waits in each phase: no wait cycle.
// Tried (round 4, tools/probes/engine_trace.py): wave-uniform owners ((eslot * 4 + i) % XW,
// every owned set's gather in full 64-lane instructions, 4x fewer load instructions).  The
// median wave's exchange at 8 ranks fell 4.7 -> 1.8 us, but the owning waves then carried all
// of the gather transactions, the launch's span grew 8.2 -> 9.0 us and the step's local cost
// 11.8 -> 12.6 us (W = 4: 10.1 -> 10.7): the per-lane owners keep every wave's share of the
// uncached-memory transactions equal, which is what bounds the phase.
// One-shot exchange of a lane's TWO elements as one 16-byte word pair {v0, epoch, v1, epoch}
// per peer (a single dwordx4 store / load instead of two 8-byte LL accesses: half the memory
// instructions and requests of the wave, and 16-byte fabric writes on real xGMI).  Each 8-byte
// half still carries its own epoch, so a reader never accepts a value of another epoch even if
// the pair were observed as two 8-byte halves.  `woff`: this (slot, wave, lane)'s pair in the
// XG_W1_BASE layout -- the same on every rank.  `live` = false (a pair of padding columns /
// hidden rows, the same on every rank): neither pushed nor gathered -- 22 % of the layout's
// pairs, so the links carry live parameters only (78,400 of 100,352 words).
// BL: polls as 16-byte buffer loads, pushes as global stores (as xg_exchange2p<XW, true>).
template <int XW, bool BL = false>
__device__ __forceinline__ void xg_exchange16(const MlpXg& xg, unsigned ep, long long woff,
                                              float (&v)[2], bool& fail, bool live = true) {
  using xgll::u64;
  using xgll::u32x4;
  const long long par = ep & 1u;
  const int me = xgll::uniform(xg.rank);
  const u64* mine = xgll::uniform_ptr((const u64*)xg.peers.data[me]) + woff;
  const xgll::OwnPoll pr(BL ? mine - woff : nullptr);
  auto poll = [&](int j) {
    if constexpr (BL) return pr.pair((par * XW + j) * xg.S, woff);
    else return xgll::load_pair(mine + (par * XW + j) * xg.S);
  };
  const u32x4 out = {__float_as_uint(v[0]), ep, __float_as_uint(v[1]), ep};
  u32x4 w[XW];  // first polls before the pushes (xgll::first_loads: one vmcnt for both)
#pragma unroll
  for (int j = 0; j < XW; ++j) {
    w[j] = u32x4{0u, ep, 0u, ep};
    if (live && j != me) w[j] = poll(j);
  }
#pragma unroll
  for (int d = 0; d < XW; ++d)
    if (live && d != me) {
      u64* dst = xgll::uniform_ptr((u64*)xg.peers.data[d]) + (par * XW + me) * xg.S + woff;
      if constexpr (BL) xgll::store_pair_g(dst, out);
      else *(u32x4*)dst = out;
    }
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  for (;;) {
    bool ready = true;
#pragma unroll
    for (int j = 0; j < XW; ++j)
      if (j != me && (w[j].y != ep || w[j].w != ep)) {
        ready = false;
        w[j] = poll(j);
      }
    if (ready) break;
    if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > xg.ticks) {
      fail = true;
      return;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  float a0 = 0.f, a1 = 0.f;  // rank-ordered sums: the same bits on every rank
#pragma unroll
  for (int j = 0; j < XW; ++j) {
    a0 += j == me ? v[0] : __uint_as_float(w[j].x);
    a1 += j == me ? v[1] : __uint_as_float(w[j].z);
  }
  v[0] = a0;
  v[1] = a1;
}

// Two-shot form of xg_exchange16 (fused2x, round 5): a lane's TWO elements travel as one
// 16-byte word pair in the XG_W1_BASE layout (`woff`, as the one-shot) and the PAIR has one
// owner rank, (q + 4 sp) % XW -- the same on every rank; at 8 ranks the 8 (q, sp) classes of a
// column group are the 8 owners.  (1) a non-owner lane pushes its pair to the owner's slot
// (parity, me); (2) an owner lane gathers the XW - 1 peers' pairs, sums each element in rank
// order and pushes the sums into every peer's result region (2 XW + parity); (3) a non-owner
// lane waits for its owner's sums.  Per hop one 16-byte store / load per lane and peer instead
// of two 8-byte LL accesses to two owners (per-element owners, xg_exchange2), and every poll
// is issued before the hop's own pushes (xgll::first_loads: stores and loads share one
// in-order vmcnt).  Each 8-byte half carries the epoch, as in xg_exchange16.
// `live` as in xg_exchange16: a dead pair is neither pushed, gathered nor broadcast.
// BL (DTFX_XG_SPLIT bit 4, round 6): the polls of the own slot region as 16-byte raw buffer
// loads and the pushes as GLOBAL stores (xgll::OwnPoll / store_pair_g) instead of FLAT
// accesses -- same words, same coherence bits.
template <int XW, bool BL = false>
__device__ __forceinline__ void xg_exchange2p(const MlpXg& xg, unsigned ep, long long woff,
                                              float (&v)[2], bool& fail, int lane, int sp,
                                              unsigned long long* trw = nullptr,
                                              bool live = true) {
  using xgll::u64;
  using xgll::u32x4;
  const long long par = ep & 1u;
  const int me = xgll::uniform(xg.rank);
  // owner class of the pair: (q + 4 sp) % XW -- at 8 ranks one rank owns one (q, sp) row of
  // a column group.  DTFX_XG_SPLIT bit 3 (A/B runs): (q + 4 (sp ^ h)) % XW, h = the lane's half
  // of its 16-lane row, so a rank owns half a row in EACH of the two waves
  const int h = (xg.split & 8) ? ((lane >> 3) & 1) : 0;
  const int own = ((lane >> 4) + 4 * (sp ^ h)) % XW;
  const bool mine = live && own == me, other = live && own != me;
  auto base = [&](int dst) { return xgll::uniform_ptr((u64*)xg.peers.data[dst]); };
  auto slot = [&](int dst, int src) { return base(dst) + (par * XW + src) * xg.S + woff; };
  auto result = [&](int dst) { return base(dst) + (2 * XW + par) * xg.S + woff; };
  auto ready2 = [&](const u32x4& w) { return w.y == ep && w.w == ep; };
  const xgll::OwnPoll pr(BL ? base(me) : nullptr);
  auto poll_slot = [&](int j) {
    if constexpr (BL) return pr.pair((par * XW + j) * xg.S, woff);
    else return xgll::load_pair(slot(me, j));
  };
  auto poll_result = [&]() {
    if constexpr (BL) return pr.pair((2 * XW + par) * xg.S, woff);
    else return xgll::load_pair(result(me));
  };
  auto put = [&](u64* p, const u32x4& w) {
    if constexpr (BL) xgll::store_pair_g(p, w);
    else *(u32x4*)p = w;
  };
  // ---- hop 1: owners' first polls, then the non-owners' push to their owner
  u32x4 w[XW];
#pragma unroll
  for (int j = 0; j < XW; ++j)
    if (mine && j != me) w[j] = poll_slot(j);
  const u32x4 out = {__float_as_uint(v[0]), ep, __float_as_uint(v[1]), ep};
  // uniform loop over destinations, per-lane predicate: a per-lane peer index would turn the
  // kernel-argument pointer table into a private (scratch) array
#pragma unroll
  for (int d = 0; d < XW; ++d)
    if (other && own == d) put(slot(d, me), out);
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  if (mine) {
    for (;;) {
      bool ready = true;
#pragma unroll
      for (int j = 0; j < XW; ++j)
        if (j != me && !ready2(w[j])) {
          ready = false;
          w[j] = poll_slot(j);
        }
      if (ready) break;
      if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > xg.ticks) {
        fail = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    float a0 = 0.f, a1 = 0.f;  // rank-ordered sums: the same bits on every rank
#pragma unroll
    for (int j = 0; j < XW; ++j) {
      a0 += j == me ? v[0] : __uint_as_float(w[j].x);
      a1 += j == me ? v[1] : __uint_as_float(w[j].z);
    }
    v[0] = a0;
    v[1] = a1;
  }
  if (trw) trace_stamp(trw, 5);  // probe builds: the owned sums are complete
  // ---- hop 2: non-owners' first poll of the result, then the owners' broadcast
  u32x4 r = {0u, 0u, 0u, 0u};
  if (other) r = poll_result();
  if (mine && !fail) {
    const u32x4 sum = {__float_as_uint(v[0]), ep, __float_as_uint(v[1]), ep};
#pragma unroll
    for (int d = 0; d < XW; ++d)
      if (d != me) put(result(d), sum);
  }
  if (other) {
    const long long t1 = (long long)__builtin_amdgcn_s_memrealtime();
    while (!ready2(r)) {
      if ((long long)__builtin_amdgcn_s_memrealtime() - t1 > xg.ticks) {
        fail = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      r = poll_result();
    }
    v[0] = __uint_as_float(r.x);
    v[1] = __uint_as_float(r.z);
  }
}

// N < 4: the lane's elements i0 .. i0 + N - 1 of the four (the exchange split over the
// K-split waves of mlp_fwdapply_kernel); ownership is by the element index i either way.
template <int XW, int N = 4>
__device__ __forceinline__ void xg_exchange2(const MlpXg& xg, unsigned ep, const size_t (&off)[N],
                                             const bool (&ok)[N], float (&v)[N], bool& fail,
                                             int lane, unsigned long long* trw = nullptr,
                                             int i0 = 0) {
  using xgll::u64;
  const long long par = ep & 1u;
  const int me = xgll::uniform(xg.rank);
  const int q = lane >> 4;
  int own[N];
  bool mine[N], other[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    own[i] = (q + 4 * (i0 + i)) % XW;
    mine[i] = ok[i] && own[i] == me;
    other[i] = ok[i] && own[i] != me;
  }
  auto slot = [&](int dst, int src) {
    return xgll::uniform_ptr((u64*)xg.peers.data[dst]) + (par * XW + src) * xg.S;
  };
  auto result = [&](int dst) {
    return xgll::uniform_ptr((u64*)xg.peers.data[dst]) + (2 * XW + par) * xg.S;
  };
  auto local = [&](int j) { return (const u64*)slot(me, j); };
  // each hop issues its first polls before its pushes (xgll::first_loads: one vmcnt for both)
  u64 w1[N][XW];
  xgll::first_loads<XW, N>(local, off, mine, me, ep, w1);
  // uniform loop over destinations, per-lane predicate: a per-lane peer index would turn the
  // kernel-argument pointer table into a private (scratch) array
#pragma unroll
  for (int d = 0; d < XW; ++d) {
    if (d == me) continue;
    u64* dst = slot(d, me);
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (other[i] && own[i] == d) xgll::store(dst + off[i], xgll::word(v[i], ep));
  }
  if (!fail) xgll::finish_sum_n<XW, N>(local, off, mine, me, ep, w1, v, xg.ticks, fail);
  if (trw) trace_stamp(trw, 5);  // probe builds: the owned sums are complete
  u64 w2[N];
  xgll::first_loads1<N>(result(me), off, other, ep, w2);
#pragma unroll
  for (int d = 0; d < XW; ++d) {
    if (d == me) continue;
    u64* dst = result(d);
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (mine[i]) xgll::store(dst + off[i], xgll::word(v[i], ep));
  }
  if (!fail) xgll::finish_wait_n<N>(result(me), off, other, ep, w2, v, xg.ticks, fail);
}

}  // namespace mlp
}  // namespace dtfx
