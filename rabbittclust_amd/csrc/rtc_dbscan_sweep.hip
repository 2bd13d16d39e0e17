// rtc_dbscan_sweep.hip -- clust-dbscan on one GPU: KssdDBSCAN (src/dbscan.cpp:725-985 in the reference tree) for up to 32 eps
// values ("levels"), every point's distance to its (minPts - 1)-th nearest candidate and the density hierarchy
// (rtc_dbscan_hier.h), all from ONE pair phase and ONE implementation (dbscan_run).  rtc_dbscan is its one-level case,
// rtc_dbscan_sweep its levels and curve, rtc_dbscan_hierarchy its hierarchy alone.
//
// The reference walks the points in index order and expands every new cluster breadth-first.  With a symmetric neighbour
// relation that walk has a closed form: a cluster is a connected component of the core points over core-core
// eps edges, numbered by its smallest core index; a non-core point with a core neighbour joins the lowest-numbered cluster
// among its core neighbours; every other point is noise.  The candidates -- every pair sharing a hash -- do not depend on eps;
// the predicate, the degrees, the components and the border pass do.  So:
//   * candidates: every pair sharing a hash, from the pair phase (rtc_pair_edges_dev, radio < 0) over row chunks
//     (dbscan_pair_chunks), the overflow protocol of rtc_candidate_edges_device.  Every chunk goes through
//   * eps_mask_kernel: the neighbour predicate of findNeighborsKSSDWithIndex (:366-612, eps_pred) in both orientations for every
//     level, one bit per level; the pairs with a non-zero mask are appended as (u, v, mask) by wave ballot with one atomic per
//     wave.  The levels are not assumed to be nested: the mask is the truth.  A pair whose orientations disagree at some level
//     fails the call;
//   * the k-distance bucket: both orientations of the chunk's candidates, together with every point's running top-k of
//     the chunks before, are bucketed by point (count, scan, scatter) and the segmented selection of rtc_topk_select.h keeps
//     the k best by the exact rational order of common / (|p| + |q| - common), lower index first among equals.
// After the last chunk every step of the closed form reads the kept list once and acts on each level whose bit is set:
//   * degrees [L][n] (atomics) and a core mask per point;
//   * hook_kernel / compress_kernel over parents [L][n]: core-core edges hooked towards the smaller root (atomicMin), pointer
//     jumping, repeated with a mask of the levels that still change -- the root of a component is its smallest core index;
//   * one exclusive scan over the L x n root flags numbers the clusters of every level in index order; border_kernel takes,
//     for every non-core point, the minimum cluster number over its core neighbours (atomicMin).
// --max-posting (u32 sketches): the hashes that more than M sketches hold are dropped before the pair phase
// (buildInvertedIndexCSR32, :95-130) -- a sorted copy of all hashes gives every hash its run length; the pair phase
// then counts over the pruned sketches while the predicate keeps the unpruned sizes.
//
// Memory: the kept list (12 B per pair that passes at some level; doubled when short, so up to twice that), one candidate
// chunk (RTC_EDGE_BUDGET), four words per point and level and one mask word per point, one byte per point and level where the
// core flags are asked for, and for the curve 32 B per candidate of one chunk plus 16 B x k per point.  Past that: RTC_ERR_NOMEM.
//
// rtc_dbscan_mash (clust-dbscan --minhash) is MinHashDBSCAN (:685-720, :987-1096) through the same dbscan_run: the
// pair phase and everything from the kept list onward are shared; its predicate (rtc_dbscan_mash.h) takes eps_mask_kernel's
// place and its core rule counts the neighbours alone (|N(v)| >= minPts, :1017, :1050) where KssdDBSCAN's counts the point too.
//
// rtc_dbscan_update (clust-dbscan --db --update) is one level of either kind through the same dbscan_run with an
// UpdReq: the pair phase runs over the new rows and then over a view of the old noise and border rows that can change
// (rtc_dbscan_update.h), the old core-core edges are seeds of the union-find, and everything from the kept list onward is shared.
#include "rtc_dbscan_common.h"
#include "rtc_topk_select.h"
#include "rtc_dbscan_hier.h"
#include "rtc_dbscan_mash.h"
#include "rtc_dbscan_update.h"

namespace {

// The curve's order compares common_a * denom_b with common_b * denom_a in 64 bits, denom = |p| + |q| - common in 32 bits:
// with every sketch of at most 2^31 - 1 hashes denom < 2^32 and the products stay below 2^63.
constexpr uint32_t SW_KDIST_MAX_LEN = 0x7fffffffu;

// cnt[0]: pairs kept (u64), cnt[1..3]: eps_level_mask's
__global__ __launch_bounds__(256) void eps_mask_kernel(const rtc_cedge* __restrict__ cand, uint64_t m, const uint32_t* __restrict__ len,
                                                       EpsLevels lv, uint32_t n_lv, uint32_t sat, rtc_cedge* __restrict__ kept,
                                                       uint64_t cap, unsigned long long* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += stride) {  // uniform per wave
    const uint64_t e = base + threadIdx.x;
    rtc_cedge c{0, 0, 0};
    if (e < m) {
      c = cand[e];
      uint32_t common;
      c.common = eps_level_mask(c, len, lv, n_lv, sat, &common, cnt);
    }
    wave_append(c.common != 0, c, kept, cap, &cnt[0]);
  }
}

// ---- the levels, one pass over the kept list per step (arrays [L][n], row l at l * n) ----
// deg[l][v] = the eps edges at v at level l, plus the empty-sketch clique of the u64 path (dbscan_run)
__global__ __launch_bounds__(256) void degree_init_kernel(const uint32_t* __restrict__ len, uint32_t n, uint32_t n_lv, uint32_t empty_deg,
                                                          uint32_t* __restrict__ deg) {
  const uint64_t total = (uint64_t)n * n_lv;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x)
    deg[x] = len[x % n] == 0 ? empty_deg : 0;
}
__global__ __launch_bounds__(256) void degree_kernel(const rtc_cedge* __restrict__ kept, uint64_t m, uint32_t n, uint32_t* __restrict__ deg) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_cedge c = kept[e];
    for (uint32_t mk = c.common; mk; mk &= mk - 1) {
      const uint64_t row = (uint64_t)__builtin_ctz(mk) * n;
      atomicAdd(&deg[row + c.i], 1u);
      atomicAdd(&deg[row + c.j], 1u);
    }
  }
}
// coremask[v] bit l: v is a core point at level l, |N(v)| + self >= minPts -- self = 1 for KssdDBSCAN, which counts the point
// (:845, :906), 0 for MinHashDBSCAN (:1017, :1050); parent[l][v] = v, or the first empty sketch for a core empty sketch of the
// u64 path; *n_core0: the core points of level 0 (one atomic per wave)
__global__ __launch_bounds__(256) void core_init_kernel(const uint32_t* __restrict__ deg, const uint32_t* __restrict__ len, uint32_t n,
                                                        uint32_t n_lv, long long min_pts, long long self, uint32_t empty_root,
                                                        uint32_t* __restrict__ coremask, uint32_t* __restrict__ parent,
                                                        unsigned long long* __restrict__ n_core0) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {  // uniform per wave
    const uint32_t v = base + threadIdx.x;
    uint32_t cm = 0;
    if (v < n) {
      const bool empty = len[v] == 0 && empty_root != 0xffffffffu;
      for (uint32_t l = 0; l < n_lv; l++) {
        const bool c = (long long)deg[(uint64_t)l * n + v] + self >= min_pts;
        if (c) cm |= 1u << l;
        parent[(uint64_t)l * n + v] = (c && empty) ? empty_root : v;
      }
      coremask[v] = cm;
    }
    const uint64_t bal = __ballot(cm & 1u);
    if (lane == 0 && bal) atomicAdd(n_core0, (unsigned long long)__popcll(bal));
  }
}
// One hooking pass, for every level in `active` whose bit the edge carries: a core-core edge whose ends sit in different trees
// hangs the larger root under the smaller one.  parent[v] <= v holds throughout, so no cycle can form; roots only ever
// decrease.  *changed gathers the levels that need another round (one atomic per wave).
__global__ __launch_bounds__(256) void hook_kernel(const rtc_cedge* __restrict__ kept, uint64_t m, uint32_t n,
                                                   const uint32_t* __restrict__ coremask, uint32_t active,
                                                   uint32_t* __restrict__ parent, uint32_t* __restrict__ changed) {
  uint32_t ch = 0;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_cedge c = kept[e];
    for (uint32_t mk = c.common & active & coremask[c.i] & coremask[c.j]; mk; mk &= mk - 1) {
      const uint32_t l = __builtin_ctz(mk);
      uint32_t* p = parent + (uint64_t)l * n;
      const uint32_t ri = __hip_atomic_load(&p[c.i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t rj = __hip_atomic_load(&p[c.j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (ri == rj) continue;
      // the ends were seen in different trees: another round follows whether or not this atomic lowers anything (a smaller
      // value already there leaves the two trees apart until the next pass)
      const uint32_t lo = ri < rj ? ri : rj, hi = ri < rj ? rj : ri;
      atomicMin(&p[hi], lo);
      ch |= 1u << l;
    }
  }
  for (int d = 32; d; d >>= 1) ch |= __shfl_xor(ch, d);
  if ((threadIdx.x & 63) == 0 && ch) atomicOr(changed, ch);
}
// pointer jumping: every vertex of an active level points at its root afterwards (no hook runs meanwhile, so roots stay put)
__global__ __launch_bounds__(256) void compress_kernel(uint32_t* __restrict__ parent, uint32_t n, uint32_t n_lv, uint32_t active) {
  const uint64_t total = (uint64_t)n * n_lv;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t l = (uint32_t)(x / n);
    if (!((active >> l) & 1u)) continue;
    uint32_t* p = parent + (uint64_t)l * n;
    uint32_t r = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
      const uint32_t q = __hip_atomic_load(&p[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (q == r) break;
      r = q;
    }
    __hip_atomic_store(&parent[x], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
__global__ __launch_bounds__(256) void root_flags_kernel(const uint32_t* __restrict__ coremask, const uint32_t* __restrict__ parent,
                                                         uint32_t n, uint32_t n_lv, uint32_t* __restrict__ is_root) {
  const uint64_t total = (uint64_t)n * n_lv;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = (uint32_t)(x % n), l = (uint32_t)(x / n);
    is_root[x] = ((coremask[v] >> l) & 1u) && parent[x] == v;
  }
}
// core points take their root's number; everything else starts as noise (~0u = -1).  cid: the exclusive scan over all L x n
// root flags; a level's numbers start at cid[l * n] (the difference is exact modulo 2^32).  core (may be null): the flags [L][n]
__global__ __launch_bounds__(256) void label_init_kernel(const uint32_t* __restrict__ coremask, const uint32_t* __restrict__ parent,
                                                         const uint32_t* __restrict__ cid, uint32_t n, uint32_t n_lv,
                                                         uint32_t* __restrict__ label, uint8_t* __restrict__ core) {
  const uint64_t total = (uint64_t)n * n_lv;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = (uint32_t)(x % n), l = (uint32_t)(x / n);
    const uint64_t row = (uint64_t)l * n;
    const bool c = (coremask[v] >> l) & 1u;
    label[x] = c ? cid[row + parent[x]] - cid[row] : 0xffffffffu;
    if (core) core[x] = c;
  }
}
// a border point joins the first cluster to reach it: the smallest number among its core neighbours'
__global__ __launch_bounds__(256) void border_kernel(const rtc_cedge* __restrict__ kept, uint64_t m, uint32_t n,
                                                     const uint32_t* __restrict__ coremask, const uint32_t* __restrict__ parent,
                                                     const uint32_t* __restrict__ cid, uint32_t* __restrict__ label) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_cedge c = kept[e];
    const uint32_t cmi = coremask[c.i], cmj = coremask[c.j];
    for (uint32_t mk = c.common & (cmi ^ cmj); mk; mk &= mk - 1) {  // exactly one end is a core point at these levels
      const uint32_t l = __builtin_ctz(mk);
      const uint64_t row = (uint64_t)l * n;
      const uint32_t from = ((cmi >> l) & 1u) ? c.i : c.j, to = from == c.i ? c.j : c.i;
      atomicMin(&label[row + to], cid[row + parent[row + from]] - cid[row]);
    }
  }
}

// ---- the k-distance buckets ----
// cnt[p] = cursor[p] = the records point p keeps from the chunks before
__global__ __launch_bounds__(256) void kd_count_init_kernel(const uint64_t* __restrict__ prev_koff, uint32_t n, uint32_t* __restrict__ cnt,
                                                            uint32_t* __restrict__ cursor) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x)
    cnt[p] = cursor[p] = (uint32_t)(prev_koff[p + 1] - prev_koff[p]);
}
__global__ __launch_bounds__(256) void kd_count_kernel(const rtc_cedge* __restrict__ cand, uint64_t m, uint32_t* __restrict__ cnt) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    atomicAdd(&cnt[cand[e].i], 1u);
    atomicAdd(&cnt[cand[e].j], 1u);
  }
}
// the kept records of the chunks before open every segment
__global__ __launch_bounds__(256) void kd_carry_kernel(const rtc_rep_hit* __restrict__ prev, const uint64_t* __restrict__ prev_koff,
                                                       uint64_t n_prev, const uint64_t* __restrict__ off, TkRec* __restrict__ seg) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_prev; x += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_rep_hit h = prev[x];
    seg[off[h.query] + (x - prev_koff[h.query])] = TkRec{h.slot, h.common, h.denom, 0};
  }
}
__global__ __launch_bounds__(256) void kd_scatter_kernel(const rtc_cedge* __restrict__ cand, uint64_t m, const uint32_t* __restrict__ len,
                                                         uint32_t sat, const uint64_t* __restrict__ off, uint32_t* __restrict__ cursor,
                                                         TkRec* __restrict__ seg) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_cedge c = cand[e];
    const uint32_t common = c.common < sat ? c.common : sat;
    const uint32_t denom = len[c.i] + len[c.j] - common;
    const uint32_t pi = atomicAdd(&cursor[c.i], 1u), pj = atomicAdd(&cursor[c.j], 1u);
    if (off[c.i] + pi < off[c.i + 1]) seg[off[c.i] + pi] = TkRec{c.j, common, denom, 0};
    if (off[c.j] + pj < off[c.j + 1]) seg[off[c.j] + pj] = TkRec{c.i, common, denom, 0};
  }
}
// the k-th record of every point that kept k of them
__global__ __launch_bounds__(256) void kd_pick_kernel(const rtc_rep_hit* __restrict__ hits, const uint64_t* __restrict__ koff,
                                                      const uint32_t* __restrict__ len, uint32_t n, uint32_t k, rtc_kdist* __restrict__ out) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
    rtc_kdist r{0, len[p], 0, 0xffffffffu};
    if (koff[p + 1] - koff[p] >= k) {
      const rtc_rep_hit h = hits[koff[p] + k - 1];
      r.common = h.common; r.size_q = len[h.slot]; r.neighbour = h.slot;
    }
    out[p] = r;
  }
}

// The curve's running state: every point's best min(seen, k) candidates so far, in rank order (hits[koff[p] .. koff[p + 1])).
struct KdState {
  uint32_t k = 0;
  rtc_rep_hit* d_hits = nullptr;
  uint64_t* d_koff = nullptr;  // n + 1
  uint64_t n_hits = 0;
  std::vector<std::vector<TkRec>> host;  // k > TK_KMAX: the selection on the host
};

int kdist_chunk_device(rtc_ctx* ctx, DevBuf& db, KdState& K, const rtc_cedge* d_cand, uint64_t m, const uint32_t* d_len, uint32_t n, uint32_t sat) {
  hipStream_t s = ctx->stream;
  uint32_t *d_c = nullptr, *d_cur = nullptr;
  uint64_t *d_off = nullptr, *d_koff = nullptr;
  RTC_TRY(db.get(ctx, n, &d_c));
  RTC_TRY(db.get(ctx, n, &d_cur));
  RTC_TRY(db.get(ctx, (size_t)n + 1, &d_off));
  RTC_TRY(db.get(ctx, (size_t)n + 1, &d_koff));
  const dim3 gv(blocks_for(n, ctx->num_cu)), ge(blocks_for(m, ctx->num_cu)), b(256);
  hipLaunchKernelGGL(kd_count_init_kernel, gv, b, 0, s, (const uint64_t*)K.d_koff, n, d_c, d_cur);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(kd_count_kernel, ge, b, 0, s, d_cand, m, d_c);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(tk_scan_kernel, dim3(1), dim3(TK_SCAN_THREADS), 0, s, (const uint32_t*)d_c, n, K.k, d_off, d_koff);
  RTC_CHECK_LAUNCH(ctx);
  uint64_t tot[2] = {0, 0};
  RTC_HIP(ctx, hipMemcpyAsync(&tot[0], d_off + n, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(&tot[1], d_koff + n, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint64_t T = tot[0], M = tot[1];
  if (T != K.n_hits + 2 * m) return rtc_fail(ctx, RTC_ERR_HIP, "rtc_dbscan_sweep: k-distance buckets hold %llu records, expected %llu",
                                            (unsigned long long)T, (unsigned long long)(K.n_hits + 2 * m));
  TkRec* d_seg = nullptr;
  rtc_rep_hit* d_hits = nullptr;
  RTC_TRY(db.get(ctx, T, &d_seg));
  RTC_TRY(db.get(ctx, M, &d_hits));
  if (K.n_hits) {
    hipLaunchKernelGGL(kd_carry_kernel, dim3(blocks_for(K.n_hits, ctx->num_cu)), b, 0, s, (const rtc_rep_hit*)K.d_hits, (const uint64_t*)K.d_koff,
                       K.n_hits, (const uint64_t*)d_off, d_seg);
    RTC_CHECK_LAUNCH(ctx);
  }
  hipLaunchKernelGGL(kd_scatter_kernel, ge, b, 0, s, d_cand, m, d_len, sat, (const uint64_t*)d_off, d_cur, d_seg);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(tk_select_kernel<64>, dim3(n), dim3(64), 0, s, (const TkRec*)d_seg, (const uint64_t*)d_off, (const uint64_t*)d_koff, n, 0u,
                     K.k, 1u, TK_LONG, d_hits);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(tk_select_kernel<256>, dim3(n), dim3(256), 0, s, (const TkRec*)d_seg, (const uint64_t*)d_off, (const uint64_t*)d_koff, n, 0u,
                     K.k, TK_LONG + 1, 0xffffffffu, d_hits);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipStreamSynchronize(s));
  db.release(d_seg); db.release(d_c); db.release(d_cur); db.release(d_off);
  db.release(K.d_hits); db.release(K.d_koff);
  K.d_hits = d_hits; K.d_koff = d_koff; K.n_hits = M;
  return RTC_OK;
}

int kdist_chunk_host(rtc_ctx* ctx, KdState& K, const rtc_cedge* d_cand, uint64_t m, const std::vector<uint32_t>& h_len, uint32_t sat) {
  std::vector<rtc_cedge> h(m);
  RTC_HIP(ctx, hipMemcpyAsync(h.data(), d_cand, m * sizeof(rtc_cedge), hipMemcpyDeviceToHost, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (const rtc_cedge& c : h) {
    const uint32_t common = std::min(c.common, sat), denom = h_len[c.i] + h_len[c.j] - common;
    K.host[c.i].push_back(TkRec{c.j, common, denom, 0});
    K.host[c.j].push_back(TkRec{c.i, common, denom, 0});
  }
  for (auto& v : K.host)  // the running top-k: nothing past the k-th can become the k-th later
    if (v.size() > 2 * (size_t)K.k) { std::nth_element(v.begin(), v.begin() + (K.k - 1), v.end(), tk_beats_host); v.resize(K.k); }
  return RTC_OK;
}

}  // namespace

// What a hierarchy call adds to the pair phase (rtc_dbscan_hier.h): the level it keeps pairs at, and where its results go.
struct HierReq { double eps_max; rtc_hedge* h_forest; uint64_t* h_n_forest; rtc_kdist* h_core; };
// What makes a call MinHashDBSCAN: the estimator's sketch size.  The levels' predicate is then rtc_dbscan_mash.h's, the core
// rule |N(v)| >= minPts, and the empty sketches are plain points (distance 1 to everything).
struct MashReq { uint32_t sketch_size; };
// What makes a call an update (rtc_dbscan_update): rows [0, n_old) carry a clustering -- that of this very call on them alone,
// which the entry point has checked as far as the host can -- and only the rows that can change anything are joined: stage 1
// the new rows against everything below them, stage 2 the old noise points that stage 1 touched and the old border points
// against the old rows.  The old core-core edges are the seeds (rtc_dbscan_update.h).  One level, no curve, no hierarchy.
struct UpdReq { uint32_t n_old; const int32_t* h_labels_old; const uint8_t* h_core_old; uint32_t n_clusters_old; uint64_t rows2; };

// What one call did.  Every entry point maps it onto its own counter array and touches no other.
struct DbscanStats {
  bool began = false;  // past the argument checks: from here on the entry point's counters are this call's
  uint64_t chunks = 0, candidates = 0, kept = 0, core0 = 0, asym = 0, rounds = 0;  // core0: the core points of level 0
  uint64_t merged = 0;  // MinHash: the candidates past the prefilter
  uint64_t pair_ns = 0, filter_ns = 0, components_ns = 0, kdist_ns = 0, total_ns = 0;
  uint64_t h_kept = 0, h_forest = 0, h_rounds = 0, h_rank_ns = 0, h_forest_ns = 0, h_total_ns = 0;  // the hierarchy's
};

// The one implementation: the levels h_eps[0 .. n_eps), the curve (h_kdist) and with hq the hierarchy, from one pair phase.
// who: the entry point, for the messages; single: rtc_dbscan, whose one level the messages do not name.
static int dbscan_run(rtc_ctx* ctx, const char* who, bool single, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                      uint32_t n, const double* h_eps, uint32_t n_eps, int min_pts, int kmer_size, int max_posting, int32_t* h_labels,
                      uint8_t* h_core, uint32_t* h_n_clusters, uint32_t* h_n_noise, rtc_kdist* h_kdist, const HierReq* hq, DbscanStats* st,
                      const MashReq* mq = nullptr, UpdReq* uq = nullptr) {
  if (!ctx || (n && (!d_hashes || !d_start || !d_len)) || (width != 4 && width != 8)) return RTC_ERR_ARG;
  if (n_eps > DB_MAX_LEVELS) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u eps values, at most %u", who, n_eps, DB_MAX_LEVELS);
  if (n_eps == 0 && !h_kdist && !hq) return rtc_fail(ctx, RTC_ERR_ARG, "%s: no eps value and no k-distance curve asked for", who);
  if (hq && (!hq->h_n_forest || (n && !hq->h_core) || (n > 1 && !hq->h_forest))) return RTC_ERR_ARG;
  if (n_eps && (!h_eps || (n && !h_labels))) return RTC_ERR_ARG;
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u points", who, n);
  if (mq) {  // 0 <= eps < 1: from 1 on the pairs without a common hash (distance 1) are neighbours, and no candidate list holds them
    if (mq->sketch_size == 0 || mq->sketch_size >= (1u << 28)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: sketch size %u", who, mq->sketch_size);
    if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: k-mer size %d", who, kmer_size);
    for (uint32_t e = 0; e < n_eps; e++)
      if (!(h_eps[e] >= 0.0)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: eps %g (value %u of the list) is not in [0, 1)", who, h_eps[e], e);
    for (uint32_t e = 0; e < n_eps; e++)
      if (h_eps[e] >= 1.0)
        return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: eps %g (value %u of the list): from 1 on, pairs without a common hash are neighbours", who,
                        h_eps[e], e);
  }
  st->began = true;
  if (hq) *hq->h_n_forest = 0;
  for (uint32_t e = 0; e < n_eps; e++) {
    if (h_n_clusters) h_n_clusters[e] = 0;
    if (h_n_noise) h_n_noise[e] = 0;
  }
  if (n == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  // How a message names the level it is about (at < 0: the hierarchy's): `name` is its eps, with its place in the list where it
  // comes from one; `about` opens a message on something found at the level, and is empty at rtc_dbscan's only level.
  struct LevelName { char name[96], about[100]; };
  auto level = [&](int at) {
    LevelName m;
    if (at < 0 || single) snprintf(m.name, sizeof m.name, "eps %g", at < 0 ? hq->eps_max : h_eps[at]);
    else snprintf(m.name, sizeof m.name, "eps %g (value %d of the list)", h_eps[at], at);
    m.about[0] = 0;
    if (at < 0 || !single) snprintf(m.about, sizeof m.about, "%s: ", m.name);
    return m;
  };
  // every level's t, the hierarchy's likewise, and the two refusals (eps_to_t, u32_size_bound_fits)
  EpsLevels lv, hlv;
  memset(&lv, 0, sizeof lv);
  memset(&hlv, 0, sizeof hlv);
  for (uint32_t e = 0; e < n_eps && !mq; e++)
    if (!eps_to_t(h_eps[e], kmer_size, &lv.t[e], &lv.one_plus_t[e]))
      return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: %s with k %d gives jaccard_min %g <= 1e-12", who, level((int)e).name, kmer_size, lv.t[e]);
  if (hq && !eps_to_t(hq->eps_max, kmer_size, &hlv.t[0], &hlv.one_plus_t[0]))
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: %s with k %d gives jaccard_min %g <= 1e-12", who, level(-1).name, kmer_size, hlv.t[0]);
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  uint32_t max_len = 0;
  std::vector<uint32_t> empties;
  for (uint32_t g = 0; g < n; g++) {
    max_len = std::max(max_len, h_len[g]);
    if (!h_len[g]) empties.push_back(g);
  }
  if (width == 4 && !mq) {
    for (uint32_t e = 0; e < n_eps; e++)
      if (!u32_size_bound_fits(max_len, lv.t[e]))
        return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: %ssize bound ceil(%u / %g) past INT_MAX", who, level((int)e).about, max_len, lv.t[e]);
    if (hq && !u32_size_bound_fits(max_len, hlv.t[0]))
      return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: %ssize bound ceil(%u / %g) past INT_MAX", who, level(-1).about, max_len, hlv.t[0]);
  }
  rtc_kdist* const kd_out = hq ? hq->h_core : h_kdist;  // the hierarchy's core triples ARE the curve
  if (kd_out && max_len > SW_KDIST_MAX_LEN)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: a sketch of %u hashes, the k-distance order is exact up to %u", who, max_len, SW_KDIST_MAX_LEN);
  // The u64 brute force (:383-445) has no emptiness test: two empty sketches pass its size filter (0 <= 0) and its inequality
  // (0 + 1e-12 < 0 fails), so the empty sketches are neighbours of each other.  The u32 path skips them (:470-473, :564).
  const uint32_t n_empty = (uint32_t)empties.size();
  const uint32_t empty_deg = (width == 8 && n_empty && !mq) ? n_empty - 1 : 0;
  const uint32_t empty_root = (width == 8 && n_empty && !mq) ? empties[0] : 0xffffffffu;
  const long long kth = (long long)min_pts - 1;
  const bool curve = kd_out && kth >= 1;  // k <= 0: every point is its own k-th neighbour, no candidates needed

  DevBuf db;
  const void* ph = d_hashes;
  const uint64_t* pstart = d_start;
  const uint32_t* plen = d_len;
  if (width == 4 && max_posting > 0 && (n_eps || curve || hq)) {
    uint32_t *d_ph = nullptr, *d_plen = nullptr;
    uint64_t* d_pstart = nullptr;
    RTC_TRY(prune_postings(ctx, db, (const uint32_t*)d_hashes, d_start, d_len, n, h_len, (uint64_t)max_posting, &d_ph, &d_pstart, &d_plen));
    ph = d_ph; pstart = d_pstart; plen = d_plen;
  }
  const uint32_t sat = width == 4 ? 65535u : 0xffffffffu;

  // ---- one pair phase: every chunk gives its level masks, the hierarchy's pairs and its share of the curve ----
  // The candidate chunk and the kept lists are separate buffers, so memory is bounded by the kept pairs plus one chunk.
  unsigned long long* d_cnt = nullptr;  // [0] pair count, [1..4] the counters of the filter in flight
  RTC_TRY(db.get(ctx, 8, &d_cnt));
  KeptList kept, hkept;  // the levels' (u, v, mask), and the hierarchy's own list: the pairs kept at eps_max as (p < q, common)
  kept.cap = hkept.cap = std::max<uint64_t>((uint64_t)1 << 16, (uint64_t)n * 16);
  if (n_eps) RTC_TRY(db.get(ctx, kept.cap, &kept.d));
  if (hq) RTC_TRY(db.get(ctx, hkept.cap, &hkept.d));
  KdState K;
  if (curve) {
    K.k = (uint32_t)std::min<long long>(kth, 0xffffffffll);
    if (K.k <= TK_KMAX) {
      RTC_TRY(db.get(ctx, (size_t)n + 1, &K.d_koff));
      RTC_HIP(ctx, hipMemsetAsync(K.d_koff, 0, ((size_t)n + 1) * 8, s));
    } else {
      K.host.resize(n);
    }
  }
  MashTables mt;
  if (mq && n_eps) RTC_TRY(mash_tables(ctx, db, mq->sketch_size, max_len, kmer_size, h_eps, n_eps, &mt));
  PairPhase pp;
  auto on_chunk = [&](const rtc_cedge* d_cand, uint64_t cnt) -> int {
      if (!cnt) return RTC_OK;
      if (n_eps && mq)
        RTC_TRY(mash_filter_chunk(ctx, db, who, d_hashes, width, d_start, d_len, mq->sketch_size, d_cand, cnt, mt, n_eps, d_cnt + 1, &kept, &st->merged));
      else if (n_eps) RTC_TRY(filter_chunk(ctx, db, who, eps_mask_kernel, d_cand, cnt, d_len, lv, n_eps, sat, d_cnt + 1, &kept));
      if (hq) RTC_TRY(filter_chunk(ctx, db, who, hier_filter_kernel, d_cand, cnt, d_len, hlv, 1, sat, d_cnt + 1, &hkept));
      if (curve) {
        const uint64_t tk = now_ns();
        if (K.k <= TK_KMAX) RTC_TRY(kdist_chunk_device(ctx, db, K, d_cand, cnt, d_len, n, sat));
        else RTC_TRY(kdist_chunk_host(ctx, K, d_cand, cnt, h_len, sat));
        st->kdist_ns += now_ns() - tk;
      }
      return RTC_OK;
  };
  int32_t* d_lab_old = nullptr;
  uint8_t* d_core_old = nullptr;
  if (uq) {
    const uint32_t n_old = uq->n_old;
    // ---- stage 1: the new rows against everything below them; no view, the rows are last already ----
    RTC_TRY(dbscan_pair_chunks(ctx, db, ph, width, pstart, plen, n, n_old, d_cnt, &pp, on_chunk));
    // ---- T u B: the old border points (from the host) and the old noise points at the old end of a kept pair ----
    uint32_t *d_flag = nullptr, *d_pos = nullptr, *d_perm = nullptr, *d_vlen = nullptr;
    uint64_t* d_vstart = nullptr;
    RTC_TRY(db.get(ctx, n_old, &d_lab_old));
    RTC_TRY(db.get(ctx, n_old, &d_core_old));
    RTC_TRY(db.get(ctx, n_old, &d_flag));
    RTC_TRY(db.get(ctx, n_old, &d_pos));
    std::vector<uint32_t> h_flag(n_old);
    for (uint32_t v = 0; v < n_old; v++) h_flag[v] = !uq->h_core_old[v] && uq->h_labels_old[v] >= 0;
    RTC_HIP(ctx, hipMemcpyAsync(d_lab_old, uq->h_labels_old, (size_t)n_old * 4, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemcpyAsync(d_core_old, uq->h_core_old, n_old, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemcpyAsync(d_flag, h_flag.data(), (size_t)n_old * 4, hipMemcpyHostToDevice, s));
    const dim3 go(blocks_for(n_old, ctx->num_cu)), b(256);
    if (kept.used) {
      hipLaunchKernelGGL(upd_touch_kernel, dim3(blocks_for(kept.used, ctx->num_cu)), b, 0, s, (const rtc_cedge*)kept.d, kept.used, n_old,
                         (const int32_t*)d_lab_old, d_flag);
      RTC_CHECK_LAUNCH(ctx);
    }
    bool new_empty = false;
    for (uint32_t g = n_old; g < n; g++) new_empty |= h_len[g] == 0;
    if (empty_root != 0xffffffffu && new_empty) {
      hipLaunchKernelGGL(upd_touch_empty_kernel, go, b, 0, s, d_len, n_old, (const int32_t*)d_lab_old, d_flag);
      RTC_CHECK_LAUNCH(ctx);
    }
    size_t tb = 0;
    RTC_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n_old, rocprim::plus<uint32_t>(), s));
    void* tmp = nullptr;
    RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
    RTC_HIP(ctx, rocprim::exclusive_scan(tmp, tb, (const uint32_t*)d_flag, d_pos, 0u, (size_t)n_old, rocprim::plus<uint32_t>(), s));
    uint32_t last[2] = {0, 0};
    RTC_HIP(ctx, hipMemcpyAsync(&last[0], d_pos + (n_old - 1), 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipMemcpyAsync(&last[1], d_flag + (n_old - 1), 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));  // (h_flag goes away below)
    const uint32_t k2 = last[0] + last[1];
    if (k2 > n_old) return rtc_fail(ctx, RTC_ERR_HIP, "%s: %u rows flagged among %u", who, k2, n_old);
    uq->rows2 = k2;
    // ---- stage 2: those rows against the old rows, on a view that places them last; its pairs come back in the original numbering ----
    if (k2 && n_old > 1) {
      RTC_TRY(db.get(ctx, n_old, &d_perm));
      RTC_TRY(db.get(ctx, n_old, &d_vlen));
      RTC_TRY(db.get(ctx, n_old, &d_vstart));
      hipLaunchKernelGGL(upd_view_kernel, go, b, 0, s, (const uint32_t*)d_flag, (const uint32_t*)d_pos, n_old, k2, pstart, plen, d_vstart, d_vlen, d_perm);
      RTC_CHECK_LAUNCH(ctx);
      auto on_view_chunk = [&](rtc_cedge* d_cand, uint64_t cnt) -> int {
        if (!cnt) return RTC_OK;
        hipLaunchKernelGGL(upd_unview_kernel, dim3(blocks_for(cnt, ctx->num_cu)), dim3(256), 0, s, d_cand, cnt, n_old, (const uint32_t*)d_perm);
        RTC_CHECK_LAUNCH(ctx);
        return on_chunk(d_cand, cnt);
      };
      // the join's note of a dense tile is keyed by the hash buffer and the tile, not by start / len: none from another
      // arrangement of these hashes may speak for the view, and none from the view for a later call
      ctx->join_dense.hashes = nullptr;
      const int rc2 = dbscan_pair_chunks(ctx, db, ph, width, (const uint64_t*)d_vstart, (const uint32_t*)d_vlen, n_old, n_old - k2, d_cnt, &pp, on_view_chunk);
      ctx->join_dense.hashes = nullptr;
      RTC_TRY(rc2);
      db.release(d_perm); db.release(d_vlen); db.release(d_vstart);
    }
    db.release(d_flag); db.release(d_pos);
  } else if (n_eps || curve || hq) {
    RTC_TRY(dbscan_pair_chunks(ctx, db, ph, width, pstart, plen, n, 1, d_cnt, &pp, on_chunk));
  }
  st->chunks = pp.chunks;
  st->candidates = pp.cand_total;
  st->pair_ns = pp.pair_ns;
  st->kept = kept.used;
  st->asym = kept.asym;
  st->filter_ns = kept.ns;
  st->h_kept = hkept.used;
  if (hkept.asym)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: %s%llu pairs whose eps test depends on the orientation, e.g. (%u, %u)", who, level(-1).about,
                    (unsigned long long)hkept.asym, (uint32_t)(hkept.first_asym >> 32), (uint32_t)hkept.first_asym);
  if (kept.asym)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: %s%llu pairs whose eps test depends on the orientation, e.g. (%u, %u)", who,
                    level(__builtin_ctzll(kept.asym_levels)).about, (unsigned long long)kept.asym, (uint32_t)(kept.first_asym >> 32),
                    (uint32_t)kept.first_asym);

  // ---- the curve: the k-th record of every point, the empty sketches of the u64 path, k <= 0 ----
  if (kd_out) {
    const uint64_t tk = now_ns();
    if (!curve) {
      for (uint32_t p = 0; p < n; p++) kd_out[p] = rtc_kdist{h_len[p], h_len[p], h_len[p], p};
    } else if (K.k <= TK_KMAX) {
      rtc_kdist* d_out = nullptr;
      RTC_TRY(db.get(ctx, n, &d_out));
      hipLaunchKernelGGL(kd_pick_kernel, dim3(blocks_for(n, ctx->num_cu)), dim3(256), 0, s, (const rtc_rep_hit*)K.d_hits, (const uint64_t*)K.d_koff,
                         d_len, n, K.k, d_out);
      RTC_CHECK_LAUNCH(ctx);
      RTC_HIP(ctx, hipMemcpyAsync(kd_out, d_out, (size_t)n * sizeof(rtc_kdist), hipMemcpyDeviceToHost, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
      db.release(d_out); db.release(K.d_hits); db.release(K.d_koff);
    } else {
      for (uint32_t p = 0; p < n; p++) {
        std::vector<TkRec>& v = K.host[p];
        kd_out[p] = rtc_kdist{0, h_len[p], 0, 0xffffffffu};
        if (v.size() < K.k) continue;
        std::nth_element(v.begin(), v.begin() + (K.k - 1), v.end(), tk_beats_host);
        const TkRec& r = v[K.k - 1];
        kd_out[p] = rtc_kdist{r.common, h_len[p], h_len[r.slot], r.slot};
      }
    }
    if (curve && width == 8)  // the brute force accepts two empty sketches at every eps: j = 1 among them, the lower index first
      for (uint32_t r = 0; r < n_empty; r++) {
        const uint64_t at = (uint64_t)K.k - 1 < r ? (uint64_t)K.k - 1 : K.k;  // the k-th of the empties without r
        kd_out[empties[r]] = rtc_kdist{0, 0, 0, at < n_empty ? empties[at] : 0xffffffffu};
      }
    st->kdist_ns += now_ns() - tk;
  }
  if (hq && h_kdist) memcpy(h_kdist, kd_out, (size_t)n * sizeof(rtc_kdist));

  // ---- the hierarchy: weights, ranking and the forest on the device; the clique of empty u64 sketches is a star on the host ----
  if (hq) {
    HierStats hs;
    RTC_TRY(hier_forest(ctx, db, who, (const rtc_cedge*)hkept.d, hkept.used, d_len, n, (const rtc_kdist*)kd_out, hq->h_forest, &hs));
    db.release(hkept.d);
    uint64_t nf = hs.n_forest;
    if (width == 8 && n_empty >= 2 && kd_out[empties[0]].neighbour != 0xffffffffu) {
      // every pair of empty sketches has m = 1: the order takes (e0, e1), (e0, e2), ... first, and those already span them
      for (uint32_t r = 1; r < n_empty; r++) hq->h_forest[nf++] = rtc_hedge{empties[0], empties[r], 0, 0, 0};
      std::sort(hq->h_forest, hq->h_forest + nf, HedgeBefore());
    }
    *hq->h_n_forest = nf;
    st->h_forest = nf;
    st->h_rounds = hs.rounds;
    st->h_rank_ns = hkept.ns + hs.rank_ns;
    st->h_forest_ns = hs.forest_ns;
    st->h_total_ns = now_ns() - t_begin;
  }
  if (!n_eps) { st->total_ns = now_ns() - t_begin; return RTC_OK; }

  // ---- core points, components, cluster numbers, border points: every level in one pass per step ----
  const uint64_t tc = now_ns();
  const uint32_t L = n_eps;
  const uint64_t LN = (uint64_t)L * n, m_kept = kept.used;
  const rtc_cedge* d_kept = kept.d;
  uint32_t *d_deg = nullptr, *d_parent = nullptr, *d_cid = nullptr, *d_label = nullptr, *d_coremask = nullptr, *d_changed = nullptr;
  uint8_t* d_core = nullptr;
  RTC_TRY(db.get(ctx, LN, &d_deg));  // the degrees, then the root flags
  RTC_TRY(db.get(ctx, LN, &d_parent));
  RTC_TRY(db.get(ctx, LN, &d_cid));
  RTC_TRY(db.get(ctx, LN, &d_label));
  RTC_TRY(db.get(ctx, n, &d_coremask));
  RTC_TRY(db.get(ctx, 64, &d_changed));  // [0] the levels a round changed, [2..3] level 0's core points (u64)
  if (h_core) RTC_TRY(db.get(ctx, LN, &d_core));
  const dim3 gv(blocks_for(n, ctx->num_cu)), gl(blocks_for(LN, ctx->num_cu)), ge(blocks_for(std::max<uint64_t>(m_kept, 1), ctx->num_cu)), b(256);
  hipLaunchKernelGGL(degree_init_kernel, gl, b, 0, s, d_len, n, L, empty_deg, d_deg);
  RTC_CHECK_LAUNCH(ctx);
  if (m_kept) hipLaunchKernelGGL(degree_kernel, ge, b, 0, s, d_kept, m_kept, n, d_deg);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipMemsetAsync(d_changed, 0, 16, s));
  hipLaunchKernelGGL(core_init_kernel, gv, b, 0, s, (const uint32_t*)d_deg, d_len, n, L, (long long)min_pts, mq ? 0ll : 1ll, empty_root, d_coremask, d_parent,
                     (unsigned long long*)(d_changed + 2));
  RTC_CHECK_LAUNCH(ctx);
  if (uq) {  // the seeds: every old core point stays one and hangs under its old cluster's smallest core index
    uint32_t* d_tab = nullptr;
    const uint32_t nc = uq->n_clusters_old;
    RTC_TRY(db.get(ctx, std::max<uint32_t>(nc, 1), &d_tab));
    RTC_HIP(ctx, hipMemsetAsync(d_tab, 0xff, (size_t)std::max<uint32_t>(nc, 1) * 4, s));
    const dim3 go(blocks_for(uq->n_old, ctx->num_cu));
    hipLaunchKernelGGL(upd_seed_min_kernel, go, b, 0, s, (const int32_t*)d_lab_old, (const uint8_t*)d_core_old, uq->n_old, nc, d_tab);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(upd_seed_kernel, go, b, 0, s, (const int32_t*)d_lab_old, (const uint8_t*)d_core_old, uq->n_old, nc, (const uint32_t*)d_tab,
                       d_coremask, d_parent);
    RTC_CHECK_LAUNCH(ctx);
  }
  uint32_t* h_changed = nullptr;
  RTC_TRY(rtc_pinned(ctx, 64, (void**)&h_changed));
  uint64_t rounds = 0;
  uint32_t active = L == 32 ? 0xffffffffu : (1u << L) - 1u;  // the levels whose last round still moved a root
  while (active) {
    if (rounds) RTC_HIP(ctx, hipMemsetAsync(d_changed, 0, 4, s));
    if (m_kept) hipLaunchKernelGGL(hook_kernel, ge, b, 0, s, d_kept, m_kept, n, (const uint32_t*)d_coremask, active, d_parent, d_changed);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(compress_kernel, gl, b, 0, s, d_parent, n, L, active);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemcpyAsync(h_changed, d_changed, 16, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    rounds++;
    active = h_changed[0];
    if (active && rounds > 256) return rtc_fail(ctx, RTC_ERR_HIP, "%s: components not settled after %llu rounds", who, (unsigned long long)rounds);
  }
  hipLaunchKernelGGL(root_flags_kernel, gl, b, 0, s, (const uint32_t*)d_coremask, (const uint32_t*)d_parent, n, L, d_deg);
  RTC_CHECK_LAUNCH(ctx);
  size_t tb = 0;
  RTC_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)LN, rocprim::plus<uint32_t>(), s));
  void* tmp = nullptr;
  RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
  RTC_HIP(ctx, rocprim::exclusive_scan(tmp, tb, (const uint32_t*)d_deg, d_cid, 0u, (size_t)LN, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(label_init_kernel, gl, b, 0, s, (const uint32_t*)d_coremask, (const uint32_t*)d_parent, (const uint32_t*)d_cid, n, L, d_label, d_core);
  RTC_CHECK_LAUNCH(ctx);
  if (m_kept) hipLaunchKernelGGL(border_kernel, ge, b, 0, s, d_kept, m_kept, n, (const uint32_t*)d_coremask, (const uint32_t*)d_parent,
                                 (const uint32_t*)d_cid, d_label);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipMemcpyAsync(h_labels, d_label, (size_t)LN * 4, hipMemcpyDeviceToHost, s));
  if (h_core) RTC_HIP(ctx, hipMemcpyAsync(h_core, d_core, (size_t)LN, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  for (uint32_t e = 0; e < L; e++) {
    const int32_t* lab = h_labels + (size_t)e * n;
    int32_t max_label = -1;
    uint32_t noise = 0;
    for (uint32_t v = 0; v < n; v++) {
      if (lab[v] < 0) noise++;
      else max_label = std::max(max_label, lab[v]);
    }
    if (h_n_clusters) h_n_clusters[e] = (uint32_t)(max_label + 1);
    if (h_n_noise) h_n_noise[e] = noise;
  }
  st->core0 = (uint64_t)h_changed[2] | (uint64_t)h_changed[3] << 32;  // as the last round's copy brought it
  st->rounds = rounds;
  st->components_ns = now_ns() - tc;
  st->total_ns = now_ns() - t_begin;
  return RTC_OK;
}

// rtc_dbscan: the one-level case.  Its argument checks are dbscan_run's for one level (h_labels is needed as soon as n > 0):
// RTC_ERR_ARG before the counters are touched.
extern "C" int rtc_dbscan(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                          double eps, int min_pts, int kmer_size, int max_posting, int32_t* h_labels, uint8_t* h_core,
                          uint32_t* h_n_clusters, uint32_t* h_n_noise) {
  DbscanStats st;
  const int rc = dbscan_run(ctx, "rtc_dbscan", true, d_hashes, width, d_start, d_len, n, &eps, 1, min_pts, kmer_size, max_posting, h_labels, h_core,
                            h_n_clusters, h_n_noise, nullptr, nullptr, &st);
  if (st.began) {
    const uint64_t c[10] = {st.chunks, st.candidates, st.kept, st.core0, st.asym, st.rounds, st.pair_ns, st.filter_ns, st.components_ns, st.total_ns};
    std::copy(c, c + 10, ctx->dbscan);
  }
  return rc;
}

static void put_sweep_counters(rtc_ctx* ctx, const DbscanStats& st, uint32_t n_eps) {
  const uint64_t c[10] = {st.chunks, st.candidates, st.kept, n_eps, st.rounds, st.pair_ns, st.filter_ns, st.components_ns, st.kdist_ns, st.total_ns};
  if (st.began) std::copy(c, c + 10, ctx->dbscan_sweep);
}
static void put_hierarchy_counters(rtc_ctx* ctx, const DbscanStats& st) {
  const uint64_t c[10] = {st.chunks, st.candidates, st.h_kept, st.h_forest, st.h_rounds, st.pair_ns, st.kdist_ns, st.h_rank_ns, st.h_forest_ns,
                          st.h_total_ns};
  if (st.began) std::copy(c, c + 10, ctx->dbscan_hier);
}

extern "C" int rtc_dbscan_sweep(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                const double* h_eps, uint32_t n_eps, int min_pts, int kmer_size, int max_posting, int32_t* h_labels,
                                uint8_t* h_core, uint32_t* h_n_clusters, uint32_t* h_n_noise, rtc_kdist* h_kdist) {
  DbscanStats st;
  const int rc = dbscan_run(ctx, "rtc_dbscan_sweep", false, d_hashes, width, d_start, d_len, n, h_eps, n_eps, min_pts, kmer_size, max_posting, h_labels,
                            h_core, h_n_clusters, h_n_noise, h_kdist, nullptr, &st);
  put_sweep_counters(ctx, st, n_eps);
  return rc;
}

extern "C" int rtc_dbscan_sweep_hierarchy(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                                          uint32_t n, const double* h_eps, uint32_t n_eps, int min_pts, int kmer_size, int max_posting,
                                          int32_t* h_labels, uint8_t* h_core_flags, uint32_t* h_n_clusters, uint32_t* h_n_noise,
                                          rtc_kdist* h_kdist, double eps_max, rtc_hedge* h_forest, uint64_t* h_n_forest, rtc_kdist* h_core) {
  const HierReq hq{eps_max, h_forest, h_n_forest, h_core};
  DbscanStats st;
  const int rc = dbscan_run(ctx, "rtc_dbscan_sweep_hierarchy", false, d_hashes, width, d_start, d_len, n, h_eps, n_eps, min_pts, kmer_size, max_posting,
                            h_labels, h_core_flags, h_n_clusters, h_n_noise, h_kdist, &hq, &st);
  put_sweep_counters(ctx, st, n_eps);
  put_hierarchy_counters(ctx, st);
  return rc;
}

extern "C" int rtc_dbscan_hierarchy(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                    double eps_max, int min_pts, int kmer_size, int max_posting, rtc_hedge* h_forest, uint64_t* h_n_forest,
                                    rtc_kdist* h_core) {
  const HierReq hq{eps_max, h_forest, h_n_forest, h_core};
  DbscanStats st;
  const int rc = dbscan_run(ctx, "rtc_dbscan_hierarchy", false, d_hashes, width, d_start, d_len, n, nullptr, 0, min_pts, kmer_size, max_posting, nullptr,
                            nullptr, nullptr, nullptr, nullptr, &hq, &st);
  put_hierarchy_counters(ctx, st);
  return rc;
}

// rtc_dbscan_mash: MinHashDBSCAN for the levels h_eps.  A negative minPts is 0: every point is a core point.
extern "C" int rtc_dbscan_mash(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                               uint32_t sketch_size, const double* h_eps, uint32_t n_eps, int min_pts, int kmer_size, int32_t* h_labels,
                               uint8_t* h_core, uint32_t* h_n_clusters, uint32_t* h_n_noise) {
  if (ctx && n_eps == 0) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_dbscan_mash: no eps value");
  const MashReq mq{sketch_size};
  DbscanStats st;
  const int rc = dbscan_run(ctx, "rtc_dbscan_mash", false, d_hashes, width, d_start, d_len, n, h_eps, n_eps, std::max(min_pts, 0), kmer_size, 0,
                            h_labels, h_core, h_n_clusters, h_n_noise, nullptr, nullptr, &st, &mq);
  if (st.began) {
    const uint64_t c[10] = {st.chunks, st.candidates, st.merged, st.kept, n_eps, st.rounds, st.pair_ns, st.filter_ns, st.components_ns, st.total_ns};
    std::copy(c, c + 10, ctx->dbscan_mash);
  }
  return rc;
}

// rtc_dbscan_update: include/rtclust.h is the definition.  The old clustering is checked as far as the host can (RTC_ERR_ARG),
// then the call is dbscan_run's one level of the model's kind with an UpdReq.
extern "C" int rtc_dbscan_update(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n_old,
                                 uint32_t n_new, const int32_t* h_labels_old, const uint8_t* h_core_old, int is_minhash, uint32_t sketch_size,
                                 double eps, int min_pts, int kmer_size, int32_t* h_labels, uint8_t* h_core, uint32_t* h_n_clusters,
                                 uint32_t* h_n_noise) {
  const char* who = "rtc_dbscan_update";
  if (!ctx) return RTC_ERR_ARG;
  if ((uint64_t)n_old + n_new >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u + %u points", who, n_old, n_new);
  const uint32_t n = n_old + n_new;
  if (n_old && (!h_labels_old || !h_core_old)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: the model's labels or core flags are missing", who);
  if (n && !h_labels) return rtc_fail(ctx, RTC_ERR_ARG, "%s: no room for the labels", who);
  // the old clustering: noise is -1, a core point has a cluster, the clusters are 0 .. max and each has a core point
  int32_t max_label = -1;
  for (uint32_t v = 0; v < n_old; v++) {
    if (h_labels_old[v] < -1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: old label %d of point %u", who, h_labels_old[v], v);
    if (h_core_old[v] && h_labels_old[v] < 0) return rtc_fail(ctx, RTC_ERR_ARG, "%s: old point %u is a core point without a cluster", who, v);
    max_label = std::max(max_label, h_labels_old[v]);
  }
  const uint32_t nc_old = (uint32_t)(max_label + 1);
  uint32_t noise_old = 0;
  {
    std::vector<uint8_t> has_core(nc_old, 0);
    for (uint32_t v = 0; v < n_old; v++) {
      if (h_core_old[v]) has_core[h_labels_old[v]] = 1;
      noise_old += h_labels_old[v] < 0;
    }
    for (uint32_t c = 0; c < nc_old; c++)
      if (!has_core[c]) return rtc_fail(ctx, RTC_ERR_ARG, "%s: old cluster %u of %u has no core point", who, c, nc_old);
  }
  const MashReq mq{sketch_size};
  const int mp = is_minhash ? std::max(min_pts, 0) : min_pts;
  DbscanStats st;
  UpdReq uq{n_old, h_labels_old, h_core_old, nc_old, 0};
  uint64_t rows1 = n_new, promoted = 0, merged = 0;
  int rc = RTC_OK;
  if (n_new == 0) {  // the model as it is (after the kind's own argument checks: an empty set passes them alone)
    rc = dbscan_run(ctx, who, true, nullptr, width, nullptr, nullptr, 0, &eps, 1, mp, kmer_size, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                    &st, is_minhash ? &mq : nullptr);
    if (rc != RTC_OK) return rc;
    if (n_old) memcpy(h_labels, h_labels_old, (size_t)n_old * 4);
    if (n_old && h_core) memcpy(h_core, h_core_old, n_old);
    if (h_n_clusters) *h_n_clusters = nc_old;
    if (h_n_noise) *h_n_noise = noise_old;
    st.total_ns = 0;
  } else {
    std::vector<uint8_t> core_own;
    if (!h_core) { core_own.resize(n); h_core = core_own.data(); }
    rc = dbscan_run(ctx, who, true, d_hashes, width, d_start, d_len, n, &eps, 1, mp, kmer_size, 0, h_labels, h_core, h_n_clusters, h_n_noise, nullptr,
                    nullptr, &st, is_minhash ? &mq : nullptr, n_old ? &uq : nullptr);
    if (rc == RTC_OK && n_old) {
      std::vector<uint8_t> seen(nc_old ? (size_t)n : 0, 0);  // final labels that old core points carry
      uint64_t distinct = 0;
      for (uint32_t v = 0; v < n_old; v++) {
        promoted += h_core[v] && !h_core_old[v];
        if (h_core_old[v] && h_labels[v] >= 0 && !seen[h_labels[v]]) { seen[h_labels[v]] = 1; distinct++; }
      }
      merged = nc_old - distinct;
    }
    if (!n_old) rows1 = n_new ? n_new - 1 : 0;  // the plain call: row 0 has nothing below it
  }
  if (st.began) {
    const uint64_t c[12] = {rows1, uq.rows2, st.chunks, st.candidates, st.kept, promoted, merged, st.rounds, st.pair_ns, st.filter_ns,
                            st.components_ns, st.total_ns};
    std::copy(c, c + 12, ctx->dbscan_update);
  }
  return rc;
}

extern "C" int rtc_dbscan_update_counters(const rtc_ctx* ctx, uint64_t out[12]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 12; i++) out[i] = ctx->dbscan_update[i];
  return RTC_OK;
}

extern "C" int rtc_dbscan_mash_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->dbscan_mash[i];
  return RTC_OK;
}

// rtc_dbscan_mash's table for one eps, on the host alone: out[d] for d = 0 .. sketch_size
extern "C" int rtc_dbscan_mash_table(uint32_t sketch_size, int kmer_size, double eps, uint32_t* out) {
  if (!out || sketch_size == 0 || sketch_size >= (1u << 28) || kmer_size < 1 || !(eps >= 0.0) || eps >= 1.0) return RTC_ERR_ARG;
  mash_cmin_row(sketch_size, sketch_size, kmer_size, eps, out);
  return RTC_OK;
}

extern "C" double rtc_mash_distance(uint32_t common, uint32_t denom, uint32_t sketch_size, int kmer_size) {
  return rtc_mash_distance_host(common, denom, sketch_size, kmer_size);
}

// The recount on its own: the truncated (common, denom) of m given pairs, by the kernel rtc_dbscan_mash runs (the cooperative
// merge, or the per-thread one under RTC_DBSCAN_MASH_SERIAL).  Context stream, asynchronous.
extern "C" int rtc_pair_mash_edges_dev(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                       uint32_t sketch_size, const rtc_cedge* d_edges, uint64_t m, uint32_t* d_common, uint32_t* d_denom) {
  if (!ctx || !d_start || !d_len || (m && (!d_edges || !d_common || !d_denom))) return RTC_ERR_ARG;
  if (width != 4 && width != 8) return rtc_fail(ctx, RTC_ERR_ARG, "width must be 4 or 8");
  if (m == 0 || n == 0) return m ? rtc_fail(ctx, RTC_ERR_ARG, "rtc_pair_mash_edges_dev: pairs of an empty set") : RTC_OK;
  if (!d_hashes) return RTC_ERR_ARG;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const MashParams P{nullptr, nullptr, 0, 0};
  if (ctx->opt.dbscan_mash_serial)
    mash_edges_launch<true>(ctx, d_hashes, width, d_start, d_len, sketch_size, d_edges, m, P, d_common, d_denom, (rtc_cedge*)nullptr, 0, nullptr);
  else
    mash_edges_launch<false>(ctx, d_hashes, width, d_start, d_len, sketch_size, d_edges, m, P, d_common, d_denom, (rtc_cedge*)nullptr, 0, nullptr);
  RTC_CHECK_LAUNCH(ctx);
  return RTC_OK;
}

extern "C" int rtc_dbscan_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->dbscan[i];
  return RTC_OK;
}

extern "C" int rtc_dbscan_hierarchy_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->dbscan_hier[i];
  return RTC_OK;
}

extern "C" int rtc_dbscan_sweep_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->dbscan_sweep[i];
  return RTC_OK;
}
