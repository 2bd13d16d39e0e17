// rtc_dbscan_sweep.hip -- clust-dbscan --eps-sweep / --kdist: KssdDBSCAN (rtc_dbscan.hip) for up to 32 eps values, and every
// point's distance to its (minPts - 1)-th nearest candidate, from ONE pair phase.
//
// The candidates -- every pair sharing a hash -- do not depend on eps; the predicate, the degrees, the components and the
// border pass do.  So the pair phase of rtc_dbscan runs once (dbscan_pair_chunks) and every chunk goes through
//   * eps_mask_kernel: the predicate of rtc_dbscan (eps_pred, both orientations) for every level, one bit per level; the
//     pairs with a non-zero mask are appended as (u, v, mask) by wave ballot with one atomic per wave.  The levels are not
//     assumed to be nested: the mask is the truth.  A pair whose orientations disagree at some level fails the call;
//   * the k-distance bucket: both orientations of the chunk's candidates, together with every point's running top-k of
//     the chunks before, are bucketed by point (count, scan, scatter) and the segmented selection of rtc_topk_select.h keeps
//     the k best by the exact rational order of common / (|p| + |q| - common), lower index first among equals.
// After the last chunk every step of rtc_dbscan's closed form reads the kept list once and acts on each level whose bit is
// set: degrees [L][n], a core mask per point, hook / compress over parents [L][n] with a mask of the levels that still
// change, one scan over the L x n root flags for the numbering, and the border pass.
//
// Memory: the kept list (12 B per pair that passes at some level), one candidate chunk (RTC_EDGE_BUDGET), four words per
// point and level, and for the curve 32 B per candidate of one chunk plus 16 B x k per point.  Past that: RTC_ERR_NOMEM.
#include "rtc_dbscan_common.h"
#include "rtc_topk_select.h"
#include "rtc_dbscan_hier.h"

namespace {

constexpr uint32_t SW_MAX_LEVELS = 32;
// The curve's order compares common_a * denom_b with common_b * denom_a in 64 bits, denom = |p| + |q| - common in 32 bits:
// with every sketch of at most 2^31 - 1 hashes denom < 2^32 and the products stay below 2^63.
constexpr uint32_t SW_KDIST_MAX_LEN = 0x7fffffffu;

struct SweepLevels { double t[SW_MAX_LEVELS], one_plus_t[SW_MAX_LEVELS]; };

// cnt[0]: pairs kept (u64), cnt[1]: pairs whose orientations disagree at some level, cnt[2]: the smallest such pair (i << 32 | j),
// cnt[3]: the levels at which one did
__global__ __launch_bounds__(256) void eps_mask_kernel(const rtc_cedge* __restrict__ cand, uint64_t m, const uint32_t* __restrict__ len,
                                                       SweepLevels lv, uint32_t n_lv, uint32_t sat, rtc_cedge* __restrict__ kept,
                                                       uint64_t cap, unsigned long long* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += stride) {  // uniform per wave
    const uint64_t e = base + threadIdx.x;
    rtc_cedge c{0, 0, 0};
    uint32_t mask = 0;
    if (e < m) {
      c = cand[e];
      const uint32_t common = c.common < sat ? c.common : sat;
      const uint32_t a = len[c.i], b = len[c.j];
      uint32_t asym = 0;
      for (uint32_t l = 0; l < n_lv; l++) {
        const bool fwd = eps_pred(a, b, common, lv.t[l], lv.one_plus_t[l]), bwd = eps_pred(b, a, common, lv.t[l], lv.one_plus_t[l]);
        if (fwd != bwd) asym |= 1u << l;
        if (fwd && bwd) mask |= 1u << l;
      }
      if (asym) {
        atomicAdd(&cnt[1], 1ull);
        atomicMin(&cnt[2], ((unsigned long long)c.i << 32) | c.j);
        atomicOr(&cnt[3], (unsigned long long)asym);
      }
    }
    const bool keep = mask != 0;
    const uint64_t bal = __ballot(keep);
    if (bal) {
      unsigned long long at = 0;
      if (lane == 0) at = atomicAdd(&cnt[0], (unsigned long long)__popcll(bal));
      at = __shfl(at, 0);
      const uint64_t idx = at + (uint64_t)__popcll(bal & ((1ULL << lane) - 1ULL));
      if (keep && idx < cap) kept[idx] = rtc_cedge{c.i, c.j, mask};
    }
  }
}

// ---- the levels, one pass over the kept list per step (arrays [L][n], row l at l * n) ----
__global__ __launch_bounds__(256) void sw_degree_init_kernel(const uint32_t* __restrict__ len, uint32_t n, uint32_t n_lv, uint32_t empty_deg,
                                                             uint32_t* __restrict__ deg) {
  const uint64_t total = (uint64_t)n * n_lv;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x)
    deg[x] = len[x % n] == 0 ? empty_deg : 0;
}
__global__ __launch_bounds__(256) void sw_degree_kernel(const rtc_cedge* __restrict__ kept, uint64_t m, uint32_t n, uint32_t* __restrict__ deg) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_cedge c = kept[e];
    for (uint32_t mk = c.common; mk; mk &= mk - 1) {
      const uint64_t row = (uint64_t)__builtin_ctz(mk) * n;
      atomicAdd(&deg[row + c.i], 1u);
      atomicAdd(&deg[row + c.j], 1u);
    }
  }
}
// coremask[v] bit l: v is a core point at level l; parent as core_init_kernel sets it
__global__ __launch_bounds__(256) void sw_core_init_kernel(const uint32_t* __restrict__ deg, const uint32_t* __restrict__ len, uint32_t n,
                                                           uint32_t n_lv, long long min_pts, uint32_t empty_root,
                                                           uint32_t* __restrict__ coremask, uint32_t* __restrict__ parent) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    uint32_t cm = 0;
    const bool empty = len[v] == 0 && empty_root != 0xffffffffu;
    for (uint32_t l = 0; l < n_lv; l++) {
      const bool c = (long long)deg[(uint64_t)l * n + v] + 1 >= min_pts;
      if (c) cm |= 1u << l;
      parent[(uint64_t)l * n + v] = (c && empty) ? empty_root : v;
    }
    coremask[v] = cm;
  }
}
// hook_kernel of rtc_dbscan.hip for every level in `active` whose bit the edge carries; *changed gathers the levels that need
// another round (one atomic per wave)
__global__ __launch_bounds__(256) void sw_hook_kernel(const rtc_cedge* __restrict__ kept, uint64_t m, uint32_t n,
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
      const uint32_t lo = ri < rj ? ri : rj, hi = ri < rj ? rj : ri;
      atomicMin(&p[hi], lo);
      ch |= 1u << l;
    }
  }
  for (int d = 32; d; d >>= 1) ch |= __shfl_xor(ch, d);
  if ((threadIdx.x & 63) == 0 && ch) atomicOr(changed, ch);
}
__global__ __launch_bounds__(256) void sw_compress_kernel(uint32_t* __restrict__ parent, uint32_t n, uint32_t n_lv, uint32_t active) {
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
__global__ __launch_bounds__(256) void sw_root_flags_kernel(const uint32_t* __restrict__ coremask, const uint32_t* __restrict__ parent,
                                                            uint32_t n, uint32_t n_lv, uint32_t* __restrict__ is_root) {
  const uint64_t total = (uint64_t)n * n_lv;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = (uint32_t)(x % n), l = (uint32_t)(x / n);
    is_root[x] = ((coremask[v] >> l) & 1u) && parent[x] == v;
  }
}
// cid: the exclusive scan over all L x n root flags; a level's numbers start at cid[l * n] (the difference is exact modulo 2^32)
__global__ __launch_bounds__(256) void sw_label_init_kernel(const uint32_t* __restrict__ coremask, const uint32_t* __restrict__ parent,
                                                            const uint32_t* __restrict__ cid, uint32_t n, uint32_t n_lv,
                                                            uint32_t* __restrict__ label) {
  const uint64_t total = (uint64_t)n * n_lv;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = (uint32_t)(x % n), l = (uint32_t)(x / n);
    const uint64_t row = (uint64_t)l * n;
    label[x] = ((coremask[v] >> l) & 1u) ? cid[row + parent[x]] - cid[row] : 0xffffffffu;
  }
}
__global__ __launch_bounds__(256) void sw_border_kernel(const rtc_cedge* __restrict__ kept, uint64_t m, uint32_t n,
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

// What a hierarchy call adds to the sweep's pair phase (rtc_dbscan_hier.h): the level it keeps pairs at, and where its results go.
struct HierReq { double eps_max; rtc_hedge* h_forest; uint64_t* h_n_forest; rtc_kdist* h_core; };

// rtc_dbscan_sweep, and with hq the hierarchy from the same pair phase.  who: the entry point, for the messages.
static int sweep_impl(rtc_ctx* ctx, const char* who, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
               const double* h_eps, uint32_t n_eps, int min_pts, int kmer_size, int max_posting, int32_t* h_labels,
               uint8_t* h_core, uint32_t* h_n_clusters, uint32_t* h_n_noise, rtc_kdist* h_kdist, const HierReq* hq) {
  if (!ctx || (n && (!d_hashes || !d_start || !d_len)) || (width != 4 && width != 8)) return RTC_ERR_ARG;
  if (n_eps > SW_MAX_LEVELS) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u eps values, at most %u", who, n_eps, SW_MAX_LEVELS);
  if (n_eps == 0 && !h_kdist && !hq) return rtc_fail(ctx, RTC_ERR_ARG, "%s: no eps value and no k-distance curve asked for", who);
  if (hq && (!hq->h_n_forest || (n && !hq->h_core) || (n > 1 && !hq->h_forest))) return RTC_ERR_ARG;
  if (n_eps && (!h_eps || (n && !h_labels))) return RTC_ERR_ARG;
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u points", who, n);
  for (int i = 0; i < 10; i++) ctx->dbscan_sweep[i] = 0;
  ctx->dbscan_sweep[3] = n_eps;
  if (hq) {
    for (int i = 0; i < 10; i++) ctx->dbscan_hier[i] = 0;
    *hq->h_n_forest = 0;
  }
  for (uint32_t e = 0; e < n_eps; e++) {
    if (h_n_clusters) h_n_clusters[e] = 0;
    if (h_n_noise) h_n_noise[e] = 0;
  }
  if (n == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  // every level's x and t on the host with libm, as rtc_dbscan forms them, and its two refusals
  SweepLevels lv;
  memset(&lv, 0, sizeof lv);
  for (uint32_t e = 0; e < n_eps; e++) {
    const double x = exp(-h_eps[e] * kmer_size);
    lv.t[e] = x / (2.0 - x);
    lv.one_plus_t[e] = 1.0 + lv.t[e];
    if (!(lv.t[e] > 1e-12))
      return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: eps %g (value %u of the list) with k %d gives jaccard_min %g <= 1e-12", who, h_eps[e], e,
                      kmer_size, lv.t[e]);
  }
  // the hierarchy's level: the same x, t and refusals
  double ht = 0.0;
  if (hq) {
    const double x = exp(-hq->eps_max * kmer_size);
    ht = x / (2.0 - x);
    if (!(ht > 1e-12))
      return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: eps %g with k %d gives jaccard_min %g <= 1e-12", who, hq->eps_max, kmer_size, ht);
  }
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  uint32_t max_len = 0;
  std::vector<uint32_t> empties;
  for (uint32_t g = 0; g < n; g++) {
    max_len = std::max(max_len, h_len[g]);
    if (!h_len[g]) empties.push_back(g);
  }
  if (width == 4)
    for (uint32_t e = 0; e < n_eps; e++)
      if (ceil((double)max_len / lv.t[e]) > 2147483647.0)
        return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: eps %g (value %u of the list): size bound ceil(%u / %g) past INT_MAX", who, h_eps[e], e,
                        max_len, lv.t[e]);
  if (hq && width == 4 && ceil((double)max_len / ht) > 2147483647.0)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: eps %g: size bound ceil(%u / %g) past INT_MAX", who, hq->eps_max, max_len, ht);
  rtc_kdist* const kd_out = hq ? hq->h_core : h_kdist;  // the hierarchy's core triples ARE the curve
  if (kd_out && max_len > SW_KDIST_MAX_LEN)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: a sketch of %u hashes, the k-distance order is exact up to %u", who, max_len, SW_KDIST_MAX_LEN);
  const uint32_t n_empty = (uint32_t)empties.size();
  const uint32_t empty_deg = (width == 8 && n_empty) ? n_empty - 1 : 0;  // the u64 brute force's clique of empty sketches (rtc_dbscan.hip)
  const uint32_t empty_root = (width == 8 && n_empty) ? empties[0] : 0xffffffffu;
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

  // ---- one pair phase: every chunk gives its level masks and its share of the curve ----
  rtc_cedge* d_kept = nullptr;
  uint64_t kept_cap = std::max<uint64_t>((uint64_t)1 << 16, (uint64_t)n * 16);
  unsigned long long* d_cnt = nullptr;  // [0] pair count, [1..4] mask counters, [5..7] the hierarchy filter's
  RTC_TRY(db.get(ctx, 8, &d_cnt));
  if (n_eps) RTC_TRY(db.get(ctx, kept_cap, &d_kept));
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
  uint64_t m_kept = 0, asym = 0, first_asym = ~0ull, asym_levels = 0, mask_ns = 0, kdist_ns = 0;
  rtc_cedge* d_hkept = nullptr;  // the hierarchy's own list: the pairs kept at eps_max, p < q
  uint64_t hkept_cap = std::max<uint64_t>((uint64_t)1 << 16, (uint64_t)n * 16);
  uint64_t m_hkept = 0, h_asym = 0, h_first_asym = ~0ull, hfilter_ns = 0;
  if (hq) RTC_TRY(db.get(ctx, hkept_cap, &d_hkept));
  PairPhase pp;
  // a kept list moved into `want` records (the filter kernels never write past a list that holds used + the chunk's candidates)
  auto regrow = [&](rtc_cedge*& d_list, uint64_t& cap, uint64_t used, uint64_t want) -> int {
      rtc_cedge* nd = nullptr;
      RTC_TRY(db.get(ctx, want, &nd));
      if (used) RTC_HIP(ctx, hipMemcpyAsync(nd, d_list, used * sizeof(rtc_cedge), hipMemcpyDeviceToDevice, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
      db.release(d_list);
      d_list = nd; cap = want;
      return RTC_OK;
  };
  auto on_chunk = [&](const rtc_cedge* d_cand, uint64_t cnt) -> int {
      if (!cnt) return RTC_OK;
      if (n_eps) {
        const uint64_t tf = now_ns();
        // at most every candidate is kept: the mask kernel never runs past the list
        if (m_kept + cnt > kept_cap) RTC_TRY(regrow(d_kept, kept_cap, m_kept, m_kept + cnt));
        unsigned long long fc[4] = {(unsigned long long)m_kept, 0ull, ~0ull, 0ull};
        RTC_HIP(ctx, hipMemcpyAsync(d_cnt + 1, fc, sizeof fc, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(eps_mask_kernel, dim3(blocks_for(cnt, ctx->num_cu)), dim3(256), 0, s, d_cand, cnt, d_len, lv, n_eps, sat, d_kept,
                           kept_cap, d_cnt + 1);
        RTC_CHECK_LAUNCH(ctx);
        RTC_HIP(ctx, hipMemcpyAsync(fc, d_cnt + 1, sizeof fc, hipMemcpyDeviceToHost, s));
        RTC_HIP(ctx, hipStreamSynchronize(s));
        if (fc[0] > kept_cap) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu pairs kept, room for %llu", who, fc[0], (unsigned long long)kept_cap);
        m_kept = fc[0];
        asym += fc[1];
        first_asym = std::min<uint64_t>(first_asym, fc[2]);
        asym_levels |= fc[3];
        mask_ns += now_ns() - tf;
      }
      if (hq) {
        const uint64_t tf = now_ns();
        // room for the kept pairs and every candidate of the chunk; doubled when short, so many row chunks move the list a few times
        if (m_hkept + cnt > hkept_cap) {
          const uint64_t need = m_hkept + cnt;
          if (2 * hkept_cap <= need || regrow(d_hkept, hkept_cap, m_hkept, 2 * hkept_cap) != RTC_OK) {
            (void)hipGetLastError();  // a doubled list that did not fit is no failure yet: the exact size may
            RTC_TRY(regrow(d_hkept, hkept_cap, m_hkept, need));
          }
        }
        unsigned long long fc[3] = {(unsigned long long)m_hkept, 0ull, ~0ull};
        RTC_HIP(ctx, hipMemcpyAsync(d_cnt + 5, fc, sizeof fc, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(hier_filter_kernel, dim3(blocks_for(cnt, ctx->num_cu)), dim3(256), 0, s, d_cand, cnt, d_len, ht, 1.0 + ht, sat, d_hkept,
                           hkept_cap, d_cnt + 5);
        RTC_CHECK_LAUNCH(ctx);
        RTC_HIP(ctx, hipMemcpyAsync(fc, d_cnt + 5, sizeof fc, hipMemcpyDeviceToHost, s));
        RTC_HIP(ctx, hipStreamSynchronize(s));
        if (fc[0] > hkept_cap) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu pairs kept, room for %llu", who, fc[0], (unsigned long long)hkept_cap);
        m_hkept = fc[0];
        h_asym += fc[1];
        h_first_asym = std::min<uint64_t>(h_first_asym, fc[2]);
        hfilter_ns += now_ns() - tf;
      }
      if (curve) {
        const uint64_t tk = now_ns();
        if (K.k <= TK_KMAX) RTC_TRY(kdist_chunk_device(ctx, db, K, d_cand, cnt, d_len, n, sat));
        else RTC_TRY(kdist_chunk_host(ctx, K, d_cand, cnt, h_len, sat));
        kdist_ns += now_ns() - tk;
      }
      return RTC_OK;
  };
  if (n_eps || curve || hq) RTC_TRY(dbscan_pair_chunks(ctx, db, ph, width, pstart, plen, n, d_cnt, &pp, on_chunk));
  ctx->dbscan_sweep[0] = pp.chunks;
  ctx->dbscan_sweep[1] = pp.cand_total;
  ctx->dbscan_sweep[2] = m_kept;
  ctx->dbscan_sweep[5] = pp.pair_ns;
  ctx->dbscan_sweep[6] = mask_ns;
  if (hq) {
    ctx->dbscan_hier[0] = pp.chunks;
    ctx->dbscan_hier[1] = pp.cand_total;
    ctx->dbscan_hier[2] = m_hkept;
    ctx->dbscan_hier[5] = pp.pair_ns;
    if (h_asym)
      return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: eps %g: %llu pairs whose eps test depends on the orientation, e.g. (%u, %u)", who, hq->eps_max,
                      (unsigned long long)h_asym, (uint32_t)(h_first_asym >> 32), (uint32_t)h_first_asym);
  }
  if (asym) {
    const uint32_t e = (uint32_t)__builtin_ctzll(asym_levels);
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: eps %g (value %u of the list): %llu pairs whose eps test depends on the orientation, e.g. (%u, %u)", who,
                    h_eps[e], e, (unsigned long long)asym, (uint32_t)(first_asym >> 32), (uint32_t)first_asym);
  }

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
    kdist_ns += now_ns() - tk;
  }
  ctx->dbscan_sweep[8] = kdist_ns;
  if (hq && h_kdist) memcpy(h_kdist, kd_out, (size_t)n * sizeof(rtc_kdist));

  // ---- the hierarchy: weights, ranking and the forest on the device; the clique of empty u64 sketches is a star on the host ----
  if (hq) {
    HierStats hs;
    RTC_TRY(hier_forest(ctx, db, who, (const rtc_cedge*)d_hkept, m_hkept, d_len, n, (const rtc_kdist*)kd_out, hq->h_forest, &hs));
    db.release(d_hkept);
    uint64_t nf = hs.n_forest;
    if (width == 8 && n_empty >= 2 && kd_out[empties[0]].neighbour != 0xffffffffu) {
      // every pair of empty sketches has m = 1: the order takes (e0, e1), (e0, e2), ... first, and those already span them
      for (uint32_t r = 1; r < n_empty; r++) hq->h_forest[nf++] = rtc_hedge{empties[0], empties[r], 0, 0, 0};
      std::sort(hq->h_forest, hq->h_forest + nf, HedgeBefore());
    }
    *hq->h_n_forest = nf;
    ctx->dbscan_hier[3] = nf;
    ctx->dbscan_hier[4] = hs.rounds;
    ctx->dbscan_hier[6] = kdist_ns;
    ctx->dbscan_hier[7] = hfilter_ns + hs.rank_ns;
    ctx->dbscan_hier[8] = hs.forest_ns;
    ctx->dbscan_hier[9] = now_ns() - t_begin;
  }
  if (!n_eps) { ctx->dbscan_sweep[9] = now_ns() - t_begin; return RTC_OK; }

  // ---- core points, components, cluster numbers, border points: every level in one pass per step ----
  const uint64_t tc = now_ns();
  const uint32_t L = n_eps;
  const uint64_t LN = (uint64_t)L * n;
  uint32_t *d_deg = nullptr, *d_parent = nullptr, *d_cid = nullptr, *d_label = nullptr, *d_coremask = nullptr, *d_changed = nullptr;
  RTC_TRY(db.get(ctx, LN, &d_deg));  // the degrees, then the root flags
  RTC_TRY(db.get(ctx, LN, &d_parent));
  RTC_TRY(db.get(ctx, LN, &d_cid));
  RTC_TRY(db.get(ctx, LN, &d_label));
  RTC_TRY(db.get(ctx, n, &d_coremask));
  RTC_TRY(db.get(ctx, 64, &d_changed));
  const dim3 gv(blocks_for(n, ctx->num_cu)), gl(blocks_for(LN, ctx->num_cu)), ge(blocks_for(std::max<uint64_t>(m_kept, 1), ctx->num_cu)), b(256);
  hipLaunchKernelGGL(sw_degree_init_kernel, gl, b, 0, s, d_len, n, L, empty_deg, d_deg);
  RTC_CHECK_LAUNCH(ctx);
  if (m_kept) hipLaunchKernelGGL(sw_degree_kernel, ge, b, 0, s, (const rtc_cedge*)d_kept, m_kept, n, d_deg);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(sw_core_init_kernel, gv, b, 0, s, (const uint32_t*)d_deg, d_len, n, L, (long long)min_pts, empty_root, d_coremask, d_parent);
  RTC_CHECK_LAUNCH(ctx);
  uint32_t* h_changed = nullptr;
  RTC_TRY(rtc_pinned(ctx, 64, (void**)&h_changed));
  uint64_t rounds = 0;
  uint32_t active = L == 32 ? 0xffffffffu : (1u << L) - 1u;  // the levels whose last round still moved a root
  while (active) {
    RTC_HIP(ctx, hipMemsetAsync(d_changed, 0, 4, s));
    if (m_kept) hipLaunchKernelGGL(sw_hook_kernel, ge, b, 0, s, (const rtc_cedge*)d_kept, m_kept, n, (const uint32_t*)d_coremask, active, d_parent, d_changed);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(sw_compress_kernel, gl, b, 0, s, d_parent, n, L, active);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemcpyAsync(h_changed, d_changed, 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    rounds++;
    active = *h_changed;
    if (active && rounds > 256) return rtc_fail(ctx, RTC_ERR_HIP, "%s: components not settled after %llu rounds", who, (unsigned long long)rounds);
  }
  hipLaunchKernelGGL(sw_root_flags_kernel, gl, b, 0, s, (const uint32_t*)d_coremask, (const uint32_t*)d_parent, n, L, d_deg);
  RTC_CHECK_LAUNCH(ctx);
  size_t tb = 0;
  RTC_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)LN, rocprim::plus<uint32_t>(), s));
  void* tmp = nullptr;
  RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
  RTC_HIP(ctx, rocprim::exclusive_scan(tmp, tb, (const uint32_t*)d_deg, d_cid, 0u, (size_t)LN, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(sw_label_init_kernel, gl, b, 0, s, (const uint32_t*)d_coremask, (const uint32_t*)d_parent, (const uint32_t*)d_cid, n, L, d_label);
  RTC_CHECK_LAUNCH(ctx);
  if (m_kept) hipLaunchKernelGGL(sw_border_kernel, ge, b, 0, s, (const rtc_cedge*)d_kept, m_kept, n, (const uint32_t*)d_coremask,
                                 (const uint32_t*)d_parent, (const uint32_t*)d_cid, d_label);
  RTC_CHECK_LAUNCH(ctx);
  std::vector<uint32_t> h_coremask(h_core ? n : 0);
  RTC_HIP(ctx, hipMemcpyAsync(h_labels, d_label, (size_t)LN * 4, hipMemcpyDeviceToHost, s));
  if (h_core) RTC_HIP(ctx, hipMemcpyAsync(h_coremask.data(), d_coremask, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  for (uint32_t e = 0; e < L; e++) {
    const int32_t* lab = h_labels + (size_t)e * n;
    int32_t max_label = -1;
    uint32_t noise = 0;
    for (uint32_t v = 0; v < n; v++) {
      if (lab[v] < 0) noise++;
      else max_label = std::max(max_label, lab[v]);
      if (h_core) h_core[(size_t)e * n + v] = (h_coremask[v] >> e) & 1u;
    }
    if (h_n_clusters) h_n_clusters[e] = (uint32_t)(max_label + 1);
    if (h_n_noise) h_n_noise[e] = noise;
  }
  ctx->dbscan_sweep[4] = rounds;
  ctx->dbscan_sweep[7] = now_ns() - tc;
  ctx->dbscan_sweep[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_dbscan_sweep(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                const double* h_eps, uint32_t n_eps, int min_pts, int kmer_size, int max_posting, int32_t* h_labels,
                                uint8_t* h_core, uint32_t* h_n_clusters, uint32_t* h_n_noise, rtc_kdist* h_kdist) {
  return sweep_impl(ctx, "rtc_dbscan_sweep", d_hashes, width, d_start, d_len, n, h_eps, n_eps, min_pts, kmer_size, max_posting, h_labels, h_core,
                    h_n_clusters, h_n_noise, h_kdist, nullptr);
}

extern "C" int rtc_dbscan_sweep_hierarchy(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                                          uint32_t n, const double* h_eps, uint32_t n_eps, int min_pts, int kmer_size, int max_posting,
                                          int32_t* h_labels, uint8_t* h_core_flags, uint32_t* h_n_clusters, uint32_t* h_n_noise,
                                          rtc_kdist* h_kdist, double eps_max, rtc_hedge* h_forest, uint64_t* h_n_forest, rtc_kdist* h_core) {
  const HierReq hq{eps_max, h_forest, h_n_forest, h_core};
  return sweep_impl(ctx, "rtc_dbscan_sweep_hierarchy", d_hashes, width, d_start, d_len, n, h_eps, n_eps, min_pts, kmer_size, max_posting, h_labels,
                    h_core_flags, h_n_clusters, h_n_noise, h_kdist, &hq);
}

extern "C" int rtc_dbscan_hierarchy(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                    double eps_max, int min_pts, int kmer_size, int max_posting, rtc_hedge* h_forest, uint64_t* h_n_forest,
                                    rtc_kdist* h_core) {
  if (!ctx) return RTC_ERR_ARG;
  uint64_t sweep[10];  // the last sweep's counters stay the last sweep's
  memcpy(sweep, ctx->dbscan_sweep, sizeof sweep);
  const HierReq hq{eps_max, h_forest, h_n_forest, h_core};
  const int st = sweep_impl(ctx, "rtc_dbscan_hierarchy", d_hashes, width, d_start, d_len, n, nullptr, 0, min_pts, kmer_size, max_posting, nullptr,
                            nullptr, nullptr, nullptr, nullptr, &hq);
  memcpy(ctx->dbscan_sweep, sweep, sizeof sweep);
  return st;
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
