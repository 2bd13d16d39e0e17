// rtc_dbscan.hip -- KssdDBSCAN (src/dbscan.cpp:725-985 in the reference tree) on one GPU.
//
// The reference walks the points in index order and expands every new cluster breadth-first.  With a symmetric
// neighbour relation that walk has a closed form: a cluster is a connected component of the core points
// over core-core eps edges, numbered by its smallest core index; a non-core point with a core neighbour joins the
// lowest-numbered cluster among its core neighbours; every other point is noise.  So:
//   * candidates: every pair sharing a hash, from the pair phase (rtc_pair_edges_dev, radio < 0) over row chunks, the
//     overflow protocol of rtc_candidate_edges_device;
//   * eps_filter_kernel: the neighbour predicate of findNeighborsKSSDWithIndex (:366-612) in both orientations, the
//     passing pairs appended to the eps list (wave ballot + one atomic per wave), disagreeing orientations counted;
//   * hook_kernel / compress_kernel: core-core edges hooked towards the smaller root (atomicMin), pointer jumping,
//     repeated until a device flag stays down -- the root of a component is its smallest core index;
//   * an exclusive scan over the roots in index order numbers the clusters; border_kernel takes, for every non-core
//     point, the minimum cluster number over its core neighbours (atomicMin).
// --max-posting (u32 sketches): the hashes that more than M sketches hold are dropped before the pair phase
// (buildInvertedIndexCSR32, :95-130) -- a sorted copy of all hashes gives every hash its run length; the pair phase
// then counts over the pruned sketches while the predicate keeps the unpruned sizes.
#include "rtc_dbscan_common.h"

namespace {

// cnt[0]: eps edges appended (u64), cnt[1]: pairs whose two orientations disagree, cnt[2]: the smallest such pair (i << 32 | j)
__global__ __launch_bounds__(256) void eps_filter_kernel(const rtc_cedge* __restrict__ cand, uint64_t m, const uint32_t* __restrict__ len,
                                                         double t, double one_plus_t, uint32_t sat, rtc_cedge* __restrict__ eps,
                                                         uint64_t cap, unsigned long long* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += stride) {  // uniform per wave
    const uint64_t e = base + threadIdx.x;
    bool keep = false;
    rtc_cedge c{0, 0, 0};
    if (e < m) {
      c = cand[e];
      const uint32_t common = c.common < sat ? c.common : sat;  // MarkCnt's u16 count (:75-80, :496-506); sat = ~0u for u64
      const uint32_t a = len[c.i], b = len[c.j];
      const bool fwd = eps_pred(a, b, common, t, one_plus_t), bwd = eps_pred(b, a, common, t, one_plus_t);
      if (fwd != bwd) {
        atomicAdd(&cnt[1], 1ull);
        atomicMin(&cnt[2], ((unsigned long long)c.i << 32) | c.j);
      }
      keep = fwd && bwd;
    }
    const uint64_t bal = __ballot(keep);
    if (bal) {
      unsigned long long at = 0;
      if (lane == 0) at = atomicAdd(&cnt[0], (unsigned long long)__popcll(bal));
      at = __shfl(at, 0);
      const uint64_t idx = at + (uint64_t)__popcll(bal & ((1ULL << lane) - 1ULL));
      if (keep && idx < cap) eps[idx] = c;
    }
  }
}

// deg[v] = the eps edges at v, plus the empty-sketch clique of the u64 path (below)
__global__ __launch_bounds__(256) void degree_init_kernel(const uint32_t* __restrict__ len, uint32_t n, uint32_t empty_deg,
                                                          uint32_t* __restrict__ deg) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) deg[v] = len[v] == 0 ? empty_deg : 0;
}
__global__ __launch_bounds__(256) void degree_kernel(const rtc_cedge* __restrict__ eps, uint64_t m, uint32_t* __restrict__ deg) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    atomicAdd(&deg[eps[e].i], 1u);
    atomicAdd(&deg[eps[e].j], 1u);
  }
}
// core[v] = |N(v)| + 1 >= minPts (:845, :906); parent[v] = v, or the first empty sketch for a core empty sketch of the u64 path
__global__ __launch_bounds__(256) void core_init_kernel(const uint32_t* __restrict__ deg, const uint32_t* __restrict__ len, uint32_t n,
                                                        long long min_pts, uint32_t empty_root, uint8_t* __restrict__ core,
                                                        uint32_t* __restrict__ parent, unsigned long long* __restrict__ n_core) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
    const uint32_t v = base + threadIdx.x;
    bool c = false;
    if (v < n) {
      c = (long long)deg[v] + 1 >= min_pts;
      core[v] = c;
      parent[v] = (c && len[v] == 0 && empty_root != 0xffffffffu) ? empty_root : v;
    }
    const uint64_t bal = __ballot(c);
    if (lane == 0 && bal) atomicAdd(n_core, (unsigned long long)__popcll(bal));
  }
}
// One hooking pass: every core-core edge whose ends sit in different trees hangs the larger root under the smaller one.
// parent[v] <= v holds throughout, so no cycle can form; roots only ever decrease.
__global__ __launch_bounds__(256) void hook_kernel(const rtc_cedge* __restrict__ eps, uint64_t m, const uint8_t* __restrict__ core,
                                                   uint32_t* __restrict__ parent, uint32_t* __restrict__ changed) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_cedge c = eps[e];
    if (!core[c.i] || !core[c.j]) continue;
    const uint32_t ri = __hip_atomic_load(&parent[c.i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t rj = __hip_atomic_load(&parent[c.j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ri == rj) continue;
    // the ends were seen in different trees: another round follows whether or not this atomic lowers anything (a smaller
    // value already there leaves the two trees apart until the next pass)
    const uint32_t lo = ri < rj ? ri : rj, hi = ri < rj ? rj : ri;
    atomicMin(&parent[hi], lo);
    *changed = 1u;
  }
}
// pointer jumping: every vertex points at its root afterwards (no hook runs meanwhile, so roots stay put)
__global__ __launch_bounds__(256) void compress_kernel(uint32_t* __restrict__ parent, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    uint32_t r = __hip_atomic_load(&parent[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
      const uint32_t p = __hip_atomic_load(&parent[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (p == r) break;
      r = p;
    }
    __hip_atomic_store(&parent[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
__global__ __launch_bounds__(256) void root_flags_kernel(const uint8_t* __restrict__ core, const uint32_t* __restrict__ parent, uint32_t n,
                                                         uint32_t* __restrict__ is_root) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) is_root[v] = core[v] && parent[v] == v;
}
// core points take their root's number; everything else starts as noise (~0u = -1)
__global__ __launch_bounds__(256) void label_init_kernel(const uint8_t* __restrict__ core, const uint32_t* __restrict__ parent,
                                                         const uint32_t* __restrict__ cid, uint32_t n, uint32_t* __restrict__ label) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) label[v] = core[v] ? cid[parent[v]] : 0xffffffffu;
}
// a border point joins the first cluster to reach it: the smallest number among its core neighbours'
__global__ __launch_bounds__(256) void border_kernel(const rtc_cedge* __restrict__ eps, uint64_t m, const uint8_t* __restrict__ core,
                                                     const uint32_t* __restrict__ parent, const uint32_t* __restrict__ cid,
                                                     uint32_t* __restrict__ label) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_cedge c = eps[e];
    const bool ci = core[c.i], cj = core[c.j];
    if (ci && !cj) atomicMin(&label[c.j], cid[parent[c.i]]);
    else if (cj && !ci) atomicMin(&label[c.i], cid[parent[c.j]]);
  }
}

}  // namespace

extern "C" int rtc_dbscan(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                          double eps, int min_pts, int kmer_size, int max_posting, int32_t* h_labels, uint8_t* h_core,
                          uint32_t* h_n_clusters, uint32_t* h_n_noise) {
  if (!ctx || (n && (!d_hashes || !d_start || !d_len || !h_labels)) || (width != 4 && width != 8)) return RTC_ERR_ARG;
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_dbscan: %u points", n);
  for (int i = 0; i < 10; i++) ctx->dbscan[i] = 0;
  if (h_n_clusters) *h_n_clusters = 0;
  if (h_n_noise) *h_n_noise = 0;
  if (n == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  // x and t on the host with libm (:751-752)
  const double x = exp(-eps * kmer_size);
  const double t = x / (2.0 - x);
  const double one_plus_t = 1.0 + t;
  // Outside this range the reference's relation is not the one the closed form needs: with t <= 1e-12 pairs without a common
  // hash pass the test (the u64 brute force lists them, the u32 index never sees them), and a u32 bound ceil(a / t) past
  // INT_MAX is an undefined int conversion (:514).
  if (!(t > 1e-12)) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "rtc_dbscan: eps %g with k %d gives jaccard_min %g <= 1e-12", eps, kmer_size, t);
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  uint32_t max_len = 0, n_empty = 0, first_empty = 0xffffffffu;
  for (uint32_t g = 0; g < n; g++) {
    max_len = std::max(max_len, h_len[g]);
    if (!h_len[g]) { n_empty++; if (first_empty == 0xffffffffu) first_empty = g; }
  }
  if (width == 4 && ceil((double)max_len / t) > 2147483647.0)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "rtc_dbscan: size bound ceil(%u / %g) past INT_MAX", max_len, t);
  // The u64 brute force (:383-445) has no emptiness test: two empty sketches pass its size filter (0 <= 0) and its inequality
  // (0 + 1e-12 < 0 fails), so the empty sketches are neighbours of each other.  The u32 path skips them (:470-473, :564).
  const uint32_t empty_deg = (width == 8 && n_empty) ? n_empty - 1 : 0;
  const uint32_t empty_root = (width == 8 && n_empty) ? first_empty : 0xffffffffu;

  DevBuf db;
  const void* ph = d_hashes;
  const uint64_t* pstart = d_start;
  const uint32_t* plen = d_len;
  if (width == 4 && max_posting > 0) {
    uint32_t *d_ph = nullptr, *d_plen = nullptr;
    uint64_t* d_pstart = nullptr;
    RTC_TRY(prune_postings(ctx, db, (const uint32_t*)d_hashes, d_start, d_len, n, h_len, (uint64_t)max_posting, &d_ph, &d_pstart, &d_plen));
    ph = d_ph; pstart = d_pstart; plen = d_plen;
  }
  const uint32_t sat = width == 4 ? 65535u : 0xffffffffu;

  // ---- candidates over row chunks, each filtered down to its eps edges before the next one is produced ----
  rtc_cedge* d_eps = nullptr;
  uint64_t eps_cap = std::max<uint64_t>((uint64_t)1 << 16, (uint64_t)n * 16);
  unsigned long long* d_cnt = nullptr;  // [0] pair count, [1..3] filter counters
  RTC_TRY(db.get(ctx, eps_cap, &d_eps));
  RTC_TRY(db.get(ctx, 8, &d_cnt));
  uint64_t m_eps = 0, asym = 0, first_asym = ~0ull, filter_ns = 0;
  PairPhase pp;
  auto on_chunk = [&](const rtc_cedge* d_cand, uint64_t cnt) -> int {
    // eps filter of the chunk, appended to the eps list.  The list is grown first to hold the whole chunk (at most every candidate
    // passes), so the filter runs once; the loop's regrow-and-filter-again is a guard on that bound.
    const uint64_t tf = now_ns();
    if (m_eps + cnt > eps_cap) {
      rtc_cedge* nd = nullptr;
      const uint64_t want = m_eps + cnt;
      RTC_TRY(db.get(ctx, want, &nd));
      if (m_eps) RTC_HIP(ctx, hipMemcpyAsync(nd, d_eps, m_eps * sizeof(rtc_cedge), hipMemcpyDeviceToDevice, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
      db.release(d_eps);
      d_eps = nd; eps_cap = want;
    }
    for (;;) {
      unsigned long long fc[3] = {(unsigned long long)m_eps, 0ull, ~0ull};
      RTC_HIP(ctx, hipMemcpyAsync(d_cnt + 1, fc, sizeof fc, hipMemcpyHostToDevice, s));
      if (cnt)
        hipLaunchKernelGGL(eps_filter_kernel, dim3(blocks_for(cnt, ctx->num_cu)), dim3(256), 0, s, d_cand, cnt,
                           d_len, t, one_plus_t, sat, d_eps, eps_cap, d_cnt + 1);
      RTC_CHECK_LAUNCH(ctx);
      RTC_HIP(ctx, hipMemcpyAsync(fc, d_cnt + 1, sizeof fc, hipMemcpyDeviceToHost, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
      if (fc[0] <= eps_cap) {
        m_eps = fc[0];
        asym += fc[1];
        first_asym = std::min<uint64_t>(first_asym, fc[2]);
        break;
      }
      rtc_cedge* nd = nullptr;
      const uint64_t want = fc[0] + fc[0] / 4;
      RTC_TRY(db.get(ctx, want, &nd));
      if (m_eps) RTC_HIP(ctx, hipMemcpyAsync(nd, d_eps, m_eps * sizeof(rtc_cedge), hipMemcpyDeviceToDevice, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
      db.release(d_eps);
      d_eps = nd; eps_cap = want;
    }
    filter_ns += now_ns() - tf;
    return RTC_OK;
  };
  RTC_TRY(dbscan_pair_chunks(ctx, db, ph, width, pstart, plen, n, d_cnt, &pp, on_chunk));
  const uint64_t chunks = pp.chunks, cand_total = pp.cand_total, pair_ns = pp.pair_ns;
  ctx->dbscan[0] = chunks;
  ctx->dbscan[1] = cand_total;
  ctx->dbscan[2] = m_eps;
  ctx->dbscan[4] = asym;
  ctx->dbscan[6] = pair_ns;
  ctx->dbscan[7] = filter_ns;
  if (asym)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "rtc_dbscan: %llu pairs whose eps test depends on the orientation, e.g. (%u, %u)",
                    (unsigned long long)asym, (uint32_t)(first_asym >> 32), (uint32_t)first_asym);

  // ---- core points, components, cluster numbers, border points ----
  const uint64_t tc = now_ns();
  uint32_t *d_deg = nullptr, *d_parent = nullptr, *d_flag = nullptr, *d_cid = nullptr, *d_label = nullptr, *d_changed = nullptr;
  uint8_t* d_core = nullptr;
  RTC_TRY(db.get(ctx, n, &d_deg));
  RTC_TRY(db.get(ctx, n, &d_parent));
  RTC_TRY(db.get(ctx, n, &d_flag));
  RTC_TRY(db.get(ctx, n, &d_cid));
  RTC_TRY(db.get(ctx, n, &d_label));
  RTC_TRY(db.get(ctx, n, &d_core));
  RTC_TRY(db.get(ctx, 64, &d_changed));
  const dim3 gv(blocks_for(n, ctx->num_cu)), ge(blocks_for(std::max<uint64_t>(m_eps, 1), ctx->num_cu)), b(256);
  hipLaunchKernelGGL(degree_init_kernel, gv, b, 0, s, d_len, n, empty_deg, d_deg);
  RTC_CHECK_LAUNCH(ctx);
  if (m_eps) hipLaunchKernelGGL(degree_kernel, ge, b, 0, s, (const rtc_cedge*)d_eps, m_eps, d_deg);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 8, s));
  hipLaunchKernelGGL(core_init_kernel, gv, b, 0, s, (const uint32_t*)d_deg, d_len, n, (long long)min_pts, empty_root, d_core, d_parent, d_cnt);
  RTC_CHECK_LAUNCH(ctx);
  uint32_t* h_changed = nullptr;
  RTC_TRY(rtc_pinned(ctx, 64, (void**)&h_changed));
  uint64_t rounds = 0;
  for (;;) {
    RTC_HIP(ctx, hipMemsetAsync(d_changed, 0, 4, s));
    if (m_eps) hipLaunchKernelGGL(hook_kernel, ge, b, 0, s, (const rtc_cedge*)d_eps, m_eps, (const uint8_t*)d_core, d_parent, d_changed);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(compress_kernel, gv, b, 0, s, d_parent, n);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemcpyAsync(h_changed, d_changed, 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    rounds++;
    if (!*h_changed) break;
    if (rounds > 256) return rtc_fail(ctx, RTC_ERR_HIP, "rtc_dbscan: components not settled after %llu rounds", (unsigned long long)rounds);
  }
  hipLaunchKernelGGL(root_flags_kernel, gv, b, 0, s, (const uint8_t*)d_core, (const uint32_t*)d_parent, n, d_flag);
  RTC_CHECK_LAUNCH(ctx);
  size_t tb = 0;
  RTC_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(), s));
  void* tmp = nullptr;
  RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
  RTC_HIP(ctx, rocprim::exclusive_scan(tmp, tb, (const uint32_t*)d_flag, d_cid, 0u, (size_t)n, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(label_init_kernel, gv, b, 0, s, (const uint8_t*)d_core, (const uint32_t*)d_parent, (const uint32_t*)d_cid, n, d_label);
  RTC_CHECK_LAUNCH(ctx);
  if (m_eps) hipLaunchKernelGGL(border_kernel, ge, b, 0, s, (const rtc_cedge*)d_eps, m_eps, (const uint8_t*)d_core, (const uint32_t*)d_parent,
                                (const uint32_t*)d_cid, d_label);
  RTC_CHECK_LAUNCH(ctx);
  unsigned long long n_core = 0;
  RTC_HIP(ctx, hipMemcpyAsync(h_labels, d_label, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(&n_core, d_cnt, 8, hipMemcpyDeviceToHost, s));
  if (h_core) RTC_HIP(ctx, hipMemcpyAsync(h_core, d_core, n, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  int32_t max_label = -1;
  uint32_t noise = 0;
  for (uint32_t v = 0; v < n; v++) {
    if (h_labels[v] < 0) noise++;
    else max_label = std::max(max_label, h_labels[v]);
  }
  if (h_n_clusters) *h_n_clusters = (uint32_t)(max_label + 1);
  if (h_n_noise) *h_n_noise = noise;
  ctx->dbscan[3] = n_core;
  ctx->dbscan[5] = rounds;
  ctx->dbscan[8] = now_ns() - tc;
  ctx->dbscan[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_dbscan_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->dbscan[i];
  return RTC_OK;
}
