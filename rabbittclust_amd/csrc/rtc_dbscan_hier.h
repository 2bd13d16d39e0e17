// rtc_dbscan_hier.h -- clust-dbscan --hierarchy: the maximum spanning forest of the mutual-reachability relation over the
// pairs kept at eps_max, included by rtc_dbscan_sweep.hip whose pair phase and k-distance selection it shares.
//
//   * hier_filter_kernel: rtc_dbscan's predicate at eps_max in both orientations on a chunk of candidates; the passing pairs
//     are appended as (p < q, common) by wave ballot with one atomic per wave;
//   * hier_weight_kernel (after the last chunk, when every point's core triple is final): per kept pair the limiting triple of
//     m = min(j(p, q), jcore(p), jcore(q)); pairs with an end that has no core level are dropped by the same ballot compaction;
//   * rocprim::merge_sort with the exact cross-multiplying comparator puts the weighted edges into the total order (larger m,
//     then smaller p, then smaller q).  An edge's position IS its key from here on: unique, so the forest is unique;
//   * Boruvka rounds: every component takes the smallest position among the edges leaving it (atomicMin, no value returned),
//     hooks along it (two components that chose each other chose the same edge: the smaller stays the root), pointer jumping;
//   * the flagged edges compacted in position order (rocprim::select) are the forest, already sorted.
// Everything is integer arithmetic: products of a 31-bit count and a 32-bit denominator in 64 bits.
#pragma once
#include "rtc_dbscan_common.h"

namespace {

constexpr unsigned long long HB_NONE = ~0ull;

// j_a < j_b for j = c / d, d > 0 (c <= 2^31 - 1, d < 2^32: the products stay below 2^63)
__host__ __device__ __forceinline__ bool hj_less(uint32_t ca, uint32_t da, uint32_t cb, uint32_t db) {
  return (uint64_t)ca * db < (uint64_t)cb * da;
}
// the total order of the hierarchy's edges; a zero denominator (two empty u64 sketches, host side only) is j = 1
struct HedgeBefore {
  __host__ __device__ __forceinline__ bool operator()(const rtc_hedge& a, const rtc_hedge& b) const {
    uint32_t ca = a.common, da = a.size_p + a.size_q - a.common, cb = b.common, db = b.size_p + b.size_q - b.common;
    if (!da) ca = da = 1;
    if (!db) cb = db = 1;
    if (hj_less(cb, db, ca, da)) return true;
    if (hj_less(ca, da, cb, db)) return false;
    if (a.p != b.p) return a.p < b.p;
    return a.q < b.q;
  }
};

// The filter of the hierarchy's one level (lv level 0, n_lv = 1): eps_mask_kernel's predicate block and append, but the record
// is (p < q, the count the predicate saw), which the forest's weights need.  cnt: as eps_mask_kernel's.
__global__ __launch_bounds__(256) void hier_filter_kernel(const rtc_cedge* __restrict__ cand, uint64_t m, const uint32_t* __restrict__ len,
                                                          EpsLevels lv, uint32_t n_lv, uint32_t sat, rtc_cedge* __restrict__ kept,
                                                          uint64_t cap, unsigned long long* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += stride) {  // uniform per wave
    const uint64_t e = base + threadIdx.x;
    bool keep = false;
    rtc_cedge c{0, 0, 0};
    if (e < m) {
      c = cand[e];
      uint32_t common;
      keep = eps_level_mask(c, len, lv, n_lv, sat, &common, cnt) != 0;
      c = rtc_cedge{c.i < c.j ? c.i : c.j, c.i < c.j ? c.j : c.i, common};
    }
    wave_append(keep, c, kept, cap, &cnt[0]);
  }
}

// cnt[0]: weighted edges written.  `out` has room for m records.
__global__ __launch_bounds__(256) void hier_weight_kernel(const rtc_cedge* __restrict__ kept, uint64_t m, const uint32_t* __restrict__ len,
                                                          const rtc_kdist* __restrict__ core, rtc_hedge* __restrict__ out,
                                                          unsigned long long* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += stride) {  // uniform per wave
    const uint64_t e = base + threadIdx.x;
    bool keep = false;
    rtc_hedge h{0, 0, 0, 0, 0};
    if (e < m) {
      const rtc_cedge c = kept[e];
      const rtc_kdist cp = core[c.i], cq = core[c.j];
      keep = cp.neighbour != 0xffffffffu && cq.neighbour != 0xffffffffu;
      h = rtc_hedge{c.i, c.j, c.common, len[c.i], len[c.j]};
      uint32_t d = h.size_p + h.size_q - h.common;
      const uint32_t dp = cp.size_p + cp.size_q - cp.common, dq = cq.size_p + cq.size_q - cq.common;
      if (keep && hj_less(cp.common, dp, h.common, d)) { h.common = cp.common; h.size_p = cp.size_p; h.size_q = cp.size_q; d = dp; }
      if (keep && hj_less(cq.common, dq, h.common, d)) { h.common = cq.common; h.size_p = cq.size_p; h.size_q = cq.size_q; }
    }
    wave_append(keep, h, out, m, &cnt[0]);
  }
}

__global__ __launch_bounds__(256) void hb_begin_kernel(uint32_t* __restrict__ comp, unsigned long long* __restrict__ best, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) { comp[v] = v; best[v] = HB_NONE; }
}
// best[c] = the first (in the total order) edge that leaves component c.  The look before the atomic goes to the L2 and only
// ever sees a value at or above the final minimum, so no edge that could still win is dropped; the atomic returns nothing.
__global__ __launch_bounds__(256) void hb_minedge_kernel(const rtc_hedge* __restrict__ edges, uint64_t m, const uint32_t* __restrict__ comp,
                                                         unsigned long long* __restrict__ best) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t cp = comp[edges[e].p], cq = comp[edges[e].q];
    if (cp == cq) continue;
    if (e < __hip_atomic_load(&best[cp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&best[cp], (unsigned long long)e);
    if (e < __hip_atomic_load(&best[cq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&best[cq], (unsigned long long)e);
  }
}
// Every root with an edge hooks onto the component at its other end and flags the edge.  Two roots that chose each other chose
// the same edge (the positions are unique): the smaller one stays a root.  *added counts the edges of the round, one atomic per wave.
__global__ __launch_bounds__(256) void hb_hook_kernel(const rtc_hedge* __restrict__ edges, uint64_t m, const uint32_t* __restrict__ comp,
                                                      const unsigned long long* __restrict__ best, uint32_t n, uint32_t* __restrict__ succ,
                                                      uint8_t* __restrict__ flag, unsigned long long* __restrict__ added) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t v0 = blockIdx.x * blockDim.x; v0 < n; v0 += gridDim.x * blockDim.x) {  // whole waves stay together
    const uint32_t v = v0 + threadIdx.x;
    uint32_t s = v;
    bool append = false;
    if (v < n && comp[v] == v) {
      const unsigned long long e = best[v];
      if (e < m) {
        const uint32_t cp = comp[edges[e].p], cq = comp[edges[e].q];
        const uint32_t d = cp == v ? cq : cp;
        const bool mutual = best[d] == e;
        if (mutual && v < d) { s = v; append = true; flag[e] = 1; }
        else { s = d; append = !mutual; if (append) flag[e] = 1; }
      }
    }
    if (v < n) succ[v] = s;
    const uint64_t bal = __ballot(append);
    if (lane == 0 && bal) atomicAdd(added, (unsigned long long)__popcll(bal));
  }
}
// comp[v] <- the root of comp[v] in the hooked forest (chains end in a root with succ[r] == r); the keys of the next round
__global__ __launch_bounds__(256) void hb_relabel_kernel(uint32_t* __restrict__ comp, const uint32_t* __restrict__ succ,
                                                         unsigned long long* __restrict__ best, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    uint32_t r = comp[v];
    for (;;) { const uint32_t nx = succ[r]; if (nx == r) break; r = nx; }
    comp[v] = r;
    best[v] = HB_NONE;
  }
}

struct HierStats { uint64_t m_weighted = 0, n_forest = 0, rounds = 0, rank_ns = 0, forest_ns = 0; };

// The forest of the kept pairs (d_kept, m_kept; p < q) under the core triples h_core, into h_forest (n - 1 slots, sorted).
int hier_forest(rtc_ctx* ctx, DevBuf& db, const char* who, const rtc_cedge* d_kept, uint64_t m_kept, const uint32_t* d_len, uint32_t n,
                const rtc_kdist* h_core, rtc_hedge* h_forest, HierStats* st) {
  hipStream_t s = ctx->stream;
  if (!m_kept) return RTC_OK;
  const uint64_t t0 = now_ns();
  rtc_kdist* d_core = nullptr;
  rtc_hedge *d_w = nullptr, *d_sorted = nullptr;
  unsigned long long* d_cnt = nullptr;
  RTC_TRY(db.get(ctx, n, &d_core));
  RTC_TRY(db.get(ctx, m_kept, &d_w));
  RTC_TRY(db.get(ctx, 8, &d_cnt));
  RTC_HIP(ctx, hipMemcpyAsync(d_core, h_core, (size_t)n * sizeof(rtc_kdist), hipMemcpyHostToDevice, s));
  RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 64, s));
  const dim3 b(256);
  hipLaunchKernelGGL(hier_weight_kernel, dim3(blocks_for(m_kept, ctx->num_cu)), b, 0, s, d_kept, m_kept, d_len, (const rtc_kdist*)d_core, d_w, d_cnt);
  RTC_CHECK_LAUNCH(ctx);
  unsigned long long m = 0;
  RTC_HIP(ctx, hipMemcpyAsync(&m, d_cnt, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  if (m > m_kept) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu weighted edges from %llu pairs", who, m, (unsigned long long)m_kept);
  db.release(d_core);
  st->m_weighted = m;
  if (!m) { st->rank_ns = now_ns() - t0; return RTC_OK; }
  RTC_TRY(db.get(ctx, m, &d_sorted));
  size_t tb = 0;
  RTC_HIP(ctx, rocprim::merge_sort(nullptr, tb, (rtc_hedge*)nullptr, (rtc_hedge*)nullptr, (size_t)m, HedgeBefore(), s));
  void* tmp = nullptr;
  RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
  RTC_HIP(ctx, rocprim::merge_sort(tmp, tb, d_w, d_sorted, (size_t)m, HedgeBefore(), s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  st->rank_ns = now_ns() - t0;

  const uint64_t t1 = now_ns();
  uint32_t *d_comp = nullptr, *d_succ = nullptr;
  unsigned long long* d_best = nullptr;
  uint8_t* d_flag = nullptr;
  RTC_TRY(db.get(ctx, n, &d_comp));
  RTC_TRY(db.get(ctx, n, &d_succ));
  RTC_TRY(db.get(ctx, n, &d_best));
  RTC_TRY(db.get(ctx, m, &d_flag));
  RTC_HIP(ctx, hipMemsetAsync(d_flag, 0, m, s));
  const dim3 gv(blocks_for(n, ctx->num_cu)), ge(blocks_for(m, ctx->num_cu));
  hipLaunchKernelGGL(hb_begin_kernel, gv, b, 0, s, d_comp, d_best, n);
  RTC_CHECK_LAUNCH(ctx);
  uint64_t total = 0;
  for (;;) {
    RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 8, s));
    hipLaunchKernelGGL(hb_minedge_kernel, ge, b, 0, s, (const rtc_hedge*)d_sorted, (uint64_t)m, (const uint32_t*)d_comp, d_best);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(hb_hook_kernel, gv, b, 0, s, (const rtc_hedge*)d_sorted, (uint64_t)m, (const uint32_t*)d_comp,
                       (const unsigned long long*)d_best, n, d_succ, d_flag, d_cnt);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(hb_relabel_kernel, gv, b, 0, s, d_comp, (const uint32_t*)d_succ, d_best, n);
    RTC_CHECK_LAUNCH(ctx);
    unsigned long long added = 0;
    RTC_HIP(ctx, hipMemcpyAsync(&added, d_cnt, 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    if (!added) break;
    st->rounds++;
    total += added;
    if (total >= n || st->rounds > 64)
      return rtc_fail(ctx, RTC_ERR_HIP, "%s: %llu forest edges of %u points after %llu rounds", who, (unsigned long long)total, n,
                      (unsigned long long)st->rounds);
  }
  // the flagged edges in position order: the forest, sorted (d_w is free again and holds at least m records)
  if (total) {
    RTC_HIP(ctx, rocprim::select(nullptr, tb, (rtc_hedge*)nullptr, (uint8_t*)nullptr, (rtc_hedge*)nullptr, (unsigned long long*)nullptr, (size_t)m, s));
    RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
    RTC_HIP(ctx, rocprim::select(tmp, tb, d_sorted, d_flag, d_w, d_cnt, (size_t)m, s));
    unsigned long long got = 0;
    RTC_HIP(ctx, hipMemcpyAsync(&got, d_cnt, 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    if (got != total) return rtc_fail(ctx, RTC_ERR_HIP, "%s: %llu edges flagged, %llu counted", who, got, (unsigned long long)total);
    RTC_HIP(ctx, hipMemcpyAsync(h_forest, d_w, (size_t)total * sizeof(rtc_hedge), hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
  }
  st->n_forest = total;
  db.release(d_w); db.release(d_sorted); db.release(d_comp); db.release(d_succ); db.release(d_best); db.release(d_flag); db.release(d_cnt);
  st->forest_ns = now_ns() - t1;
  return RTC_OK;
}

}  // namespace
