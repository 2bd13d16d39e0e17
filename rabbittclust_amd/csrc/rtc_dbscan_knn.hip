// rtc_dbscan_knn.hip -- clust-dbscan --knn on one GPU: KssdDBSCAN (src/dbscan.cpp:725-982 in the reference tree) over the k-NN
// graph of buildKNNForPoint (:221-360), read through the k-NN branch of findNeighborsKSSDWithIndex (:444-454).  DESIGN 3.4c-knn.
//
// Truncating every row to its k best passers makes the neighbour relation directed, so nothing of dbscan_run's closed form
// (undirected components plus a border rule) applies.  The reference's two order-dependent steps have closed forms of their own:
//   * the selection: a min-heap of (score, id) of capacity k fed in arrival order ends as every passer above s* (the k-th
//     largest score) plus, of the passers AT s* that arrive no later than T (the arrival of the k-th passer at or above s*), all but
//     the h lowest ids, h = the passers above s* that arrive after T.  With exactly k passers at or above s* that is those k;
//   * the walk: v's cluster is the rank of m(v), the smallest core index with a path to v whose inner vertices are all core.
// The pair phase and the candidate records are dbscan_run's (dbscan_pair_chunks, rtc_cedge {i, j, common}); its kernels are not
// touched.  Across the row chunks only the pairs passing the predicate in at least one orientation are kept (knn_keep_kernel).
// Then, all on the device:
//   (a) knn_expand_kernel: the kept pairs as directed passers (row, score bits, id), the predicate evaluated per orientation;
//       score = (float)common / (float)(|p| + |c| - common), one correctly rounded binary32 division, whose bit pattern orders
//       as an unsigned integer;
//   (b) one merge sort by (row, score descending, id), then knn_select_kernel, one wave per row: rows of at most k passers keep
//       them all; otherwise s* = the k-th record's score, G = the passers above it, Q = those at or above it; Q == k keeps the
//       first k; Q > k keeps the first G and lists its first Q records for
//   (c) knn_first_shared_kernel, one wave per listed passer: the smallest index in p's list of a hash that c holds too (over
//       the pruned sketches when max_posting > 0) -- the arrival order is ascending by (that index, c); a second merge sort by
//       (row, index, id) puts every such row in arrival order and knn_ties_kernel keeps the k - G highest ids among the tied
//       passers within the first k positions;
//   (d) knn_neighbour_kernel: of the kept passers those with (double)score >= t stay neighbours, the rest lose their id; degrees,
//       core flags, m[v] = v for core points;
//   (e) knn_propagate_kernel, one wave per frontier point: m[q] = min(m[q], m[p]) over p's neighbours (atomicMin); a core q
//       whose m fell joins the next frontier once (a round stamp).  Until a round lowers nothing: the fixpoint is unique;
//   (f) the core points with m[v] == v are the distinct values of m; an exclusive scan ranks them, label[v] = rank of m[v].
// Memory: the kept list (12 B a pair), its directed passers (12 B each, twice during the sort), 24 B per listed passer of a row that
// needs arrival keys (twice during its sort), six words per point.  Past that: RTC_ERR_NOMEM, no fallback.
#include "rtc_dbscan_common.h"

namespace {

struct KnnRec { uint32_t row, score, id; };             // score: the binary32 bit pattern; id = KNN_NONE: no neighbour (after (d))
struct KnnArr { uint32_t row, first, id, tie; uint64_t src; };  // first: the arrival key; tie: score == s*; src: its KnnRec
constexpr uint32_t KNN_NONE = 0xffffffffu;

__device__ __forceinline__ uint32_t knn_sat(uint32_t common, uint32_t sat) { return common < sat ? common : sat; }

// the pairs that pass in at least one orientation, with the count the predicate saw (FilterKernel's signature; one level)
__global__ __launch_bounds__(256) void knn_keep_kernel(const rtc_cedge* __restrict__ cand, uint64_t m, const uint32_t* __restrict__ len,
                                                       EpsLevels lv, uint32_t, uint32_t sat, rtc_cedge* __restrict__ kept, uint64_t cap,
                                                       unsigned long long* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += stride) {  // uniform per wave
    const uint64_t e = base + threadIdx.x;
    rtc_cedge c{0, 0, 0};
    bool keep = false;
    if (e < m) {
      c = cand[e];
      c.common = knn_sat(c.common, sat);
      const uint32_t a = len[c.i], b = len[c.j];
      keep = eps_pred(a, b, c.common, lv.t[0], lv.one_plus_t[0]) || eps_pred(b, a, c.common, lv.t[0], lv.one_plus_t[0]);
    }
    wave_append(keep, c, kept, cap, &cnt[0]);
  }
}

// (a) cnt[0]: directed passers; rowcnt[p]: those of row p
__global__ __launch_bounds__(256) void knn_expand_kernel(const rtc_cedge* __restrict__ kept, uint64_t m, const uint32_t* __restrict__ len, double t,
                                                         double one_plus_t, KnnRec* __restrict__ out, uint64_t cap,
                                                         uint32_t* __restrict__ rowcnt, unsigned long long* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += stride) {  // uniform per wave
    const uint64_t e = base + threadIdx.x;
    bool fwd = false, bwd = false;
    KnnRec rf{0, 0, 0}, rb{0, 0, 0};
    if (e < m) {
      const rtc_cedge c = kept[e];
      const uint32_t a = len[c.i], b = len[c.j];
      fwd = eps_pred(a, b, c.common, t, one_plus_t);
      bwd = eps_pred(b, a, c.common, t, one_plus_t);
      const unsigned long long uni = (unsigned long long)a + b - c.common;
      const uint32_t score = __float_as_uint(__fdiv_rn(__uint2float_rn(c.common), __ull2float_rn(uni)));
      rf = KnnRec{c.i, score, c.j};
      rb = KnnRec{c.j, score, c.i};
      if (fwd) atomicAdd(&rowcnt[c.i], 1u);
      if (bwd) atomicAdd(&rowcnt[c.j], 1u);
    }
    wave_append(fwd, rf, out, cap, &cnt[0]);
    wave_append(bwd, rb, out, cap, &cnt[0]);
  }
}

struct KnnRecLess {
  __device__ bool operator()(const KnnRec& x, const KnnRec& y) const {
    if (x.row != y.row) return x.row < y.row;
    if (x.score != y.score) return x.score > y.score;
    return x.id < y.id;
  }
};
struct KnnArrLess {
  __device__ bool operator()(const KnnArr& x, const KnnArr& y) const {
    if (x.row != y.row) return x.row < y.row;
    if (x.first != y.first) return x.first < y.first;
    return x.id < y.id;
  }
};

// (b) one wave per row of the sorted passers [off[p], off[p + 1]).  keep[e] = 1 for the records decided here.  ties[p] = k - G
// for a row that needs arrival keys (0 otherwise), whose first Q records go to arr (first = KNN_NONE until (c)).
// cnt[0]: records listed, cnt[1]: rows truncated, cnt[2]: rows that need arrival keys
__global__ __launch_bounds__(256) void knn_select_kernel(const KnnRec* __restrict__ rec, const uint64_t* __restrict__ off, uint32_t n, uint32_t k,
                                                         uint8_t* __restrict__ keep, uint32_t* __restrict__ ties, KnnArr* __restrict__ arr,
                                                         uint64_t arr_cap, unsigned long long* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t p = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; p < n; p += waves) {  // uniform per wave
    const uint64_t a = off[p], P = off[p + 1] - a;
    if (lane == 0) ties[p] = 0;
    if (P <= k) {
      for (uint64_t e = lane; e < P; e += 64) keep[a + e] = 1;
      continue;
    }
    const uint32_t sstar = rec[a + k - 1].score;
    uint32_t g = 0, q = 0;  // the lane's share of G and Q
    for (uint64_t e = lane; e < P; e += 64) {
      const uint32_t sc = rec[a + e].score;
      g += sc > sstar;
      q += sc >= sstar;
    }
    for (int d = 32; d; d >>= 1) { g += __shfl_xor(g, d); q += __shfl_xor(q, d); }
    const uint64_t G = g, Q = q;
    if (lane == 0) atomicAdd(&cnt[1], 1ull);
    if (Q == k) {
      for (uint64_t e = lane; e < P; e += 64) keep[a + e] = e < k;
      continue;
    }
    // Q > k: the records above s* stay, the tied ones wait for the arrival order
    for (uint64_t e = lane; e < P; e += 64) keep[a + e] = e < G;
    unsigned long long at = 0;
    if (lane == 0) {
      ties[p] = (uint32_t)(k - G);
      atomicAdd(&cnt[2], 1ull);
      at = atomicAdd(&cnt[0], (unsigned long long)Q);
    }
    at = __shfl(at, 0);
    for (uint64_t e = lane; e < Q; e += 64)
      if (at + e < arr_cap) arr[at + e] = KnnArr{p, KNN_NONE, rec[a + e].id, e >= G ? 1u : 0u, a + e};
  }
}

// (c) one wave per listed passer (p, c): the smallest index in p's list of a hash that c's list holds.  Every lane takes one
// of p's hashes and searches c's ascending list for it; the first lane that finds one gives the index.
__global__ __launch_bounds__(256) void knn_first_shared_kernel(const uint32_t* __restrict__ h, const uint64_t* __restrict__ start,
                                                               const uint32_t* __restrict__ len, KnnArr* __restrict__ arr, uint64_t m) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64);
  for (uint64_t x = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; x < m; x += waves) {  // uniform per wave
    const uint32_t p = arr[x].row, c = arr[x].id;
    const uint32_t* hp = h + start[p];
    const uint32_t* hc = h + start[c];
    const uint32_t lp = len[p], lc = len[c];
    uint32_t found = KNN_NONE;
    for (uint32_t base = 0; base < lp && found == KNN_NONE; base += 64) {  // uniform per wave
      bool hit = false;
      if (base + lane < lp) {
        const uint32_t v = hp[base + lane];
        uint32_t lo = 0, hi = lc;  // the first element of hc not below v
        while (lo < hi) {
          const uint32_t mid = lo + (hi - lo) / 2;
          if (hc[mid] < v) lo = mid + 1; else hi = mid;
        }
        hit = lo < lc && hc[lo] == v;
      }
      const uint64_t bal = __ballot(hit);
      if (bal) found = base + (uint32_t)__builtin_ctzll(bal);
    }
    if (lane == 0) arr[x].first = found;
  }
}

// where every row of a list sorted by row starts: head[row] = the index of its first record (rows without one are not read)
__global__ __launch_bounds__(256) void knn_arr_heads_kernel(const KnnArr* __restrict__ arr, uint64_t m, uint64_t* __restrict__ head) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < m; x += (uint64_t)gridDim.x * blockDim.x)
    if (x == 0 || arr[x - 1].row != arr[x].row) head[arr[x].row] = x;
}

// The rows in arrival order: E = the tied records within the first k positions; of E the ties[p] = k - G highest ids stay.
// One wave per row; every lane ranks its members of E against all of E (at most k of them).
__global__ __launch_bounds__(256) void knn_ties_kernel(const KnnArr* __restrict__ arr, const uint64_t* __restrict__ head,
                                                       const uint32_t* __restrict__ ties, uint32_t n, uint32_t k, uint8_t* __restrict__ keep) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t p = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; p < n; p += waves) {  // uniform per wave
    const uint32_t want = ties[p];
    if (!want) continue;
    const KnnArr* a = arr + head[p];  // Q > k records of row p
    for (uint32_t e = lane; e < k; e += 64) {
      if (!a[e].tie) continue;
      uint32_t above = 0;  // the members of E with a higher id
      for (uint32_t f = 0; f < k; f++) above += a[f].tie && a[f].id > a[e].id;
      if (above < want) keep[a[e].src] = 1;
    }
  }
}

// (d) the kept passers with (double)score >= t are the neighbours; every other record loses its id.  deg[p] counts them.
__global__ __launch_bounds__(256) void knn_neighbour_kernel(KnnRec* __restrict__ rec, const uint8_t* __restrict__ keep, uint64_t m, double t,
                                                            uint32_t* __restrict__ deg) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const KnnRec r = rec[e];
    if (keep[e] && (double)__uint_as_float(r.score) >= t) atomicAdd(&deg[r.row], 1u);
    else rec[e].id = KNN_NONE;
  }
}
// core[v], m[v] = v for a core point and KNN_NONE otherwise, the core points as the first frontier (stamp 0 = never listed)
// cnt[0]: the frontier's length, cnt[1]: neighbour edges
__global__ __launch_bounds__(256) void knn_core_kernel(const uint32_t* __restrict__ deg, uint32_t n, long long min_pts, uint8_t* __restrict__ core,
                                                       uint32_t* __restrict__ m, uint32_t* __restrict__ stamp, uint32_t* __restrict__ frontier,
                                                       unsigned long long* __restrict__ cnt) {
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {  // uniform per wave
    const uint32_t v = base + threadIdx.x;
    bool c = false;
    if (v < n) {
      c = (long long)deg[v] + 1 >= min_pts;
      core[v] = c;
      m[v] = c ? v : KNN_NONE;
      stamp[v] = 0;
      if (deg[v]) atomicAdd(&cnt[1], (unsigned long long)deg[v]);
    }
    wave_append(c, v, frontier, (uint64_t)n, &cnt[0]);
  }
}

// (e) one round: every frontier point hands its m to its neighbours; a core neighbour whose m fell is listed for the next round
// once (stamp[q] = round).  m only ever falls, and a point whose m falls after it was read here is listed again by whoever
// lowered it, so no update is lost.
__global__ __launch_bounds__(256) void knn_propagate_kernel(const KnnRec* __restrict__ rec, const uint64_t* __restrict__ off,
                                                            const uint8_t* __restrict__ core, const uint32_t* __restrict__ frontier, uint32_t nf,
                                                            uint32_t round, uint32_t n, uint32_t* __restrict__ m, uint32_t* __restrict__ stamp,
                                                            uint32_t* __restrict__ next, unsigned long long* __restrict__ n_next) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t x = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; x < nf; x += waves) {  // uniform per wave
    const uint32_t p = frontier[x];
    const uint32_t mp = __hip_atomic_load(&m[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t a = off[p], P = off[p + 1] - a;
    for (uint64_t base = 0; base < P; base += 64) {  // uniform per wave
      bool list = false;
      uint32_t q = 0;
      if (base + lane < P) {
        q = rec[a + base + lane].id;
        if (q != KNN_NONE && atomicMin(&m[q], mp) > mp && core[q]) list = atomicExch(&stamp[q], round) != round;
      }
      wave_append(list, q, next, (uint64_t)n, n_next);
    }
  }
}

// (f)
__global__ __launch_bounds__(256) void knn_root_kernel(const uint8_t* __restrict__ core, const uint32_t* __restrict__ m, uint32_t n,
                                                       uint32_t* __restrict__ is_root) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) is_root[v] = core[v] && m[v] == v;
}
__global__ __launch_bounds__(256) void knn_label_kernel(const uint32_t* __restrict__ m, const uint32_t* __restrict__ cid, uint32_t n,
                                                        uint32_t* __restrict__ label) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
    label[v] = m[v] == KNN_NONE ? KNN_NONE : cid[m[v]];
}

template <class T, class Less>
int knn_sort(rtc_ctx* ctx, DevBuf& db, T** list, uint64_t m, Less less) {
  if (m < 2) return RTC_OK;
  size_t tb = 0;
  RTC_HIP(ctx, rocprim::merge_sort(nullptr, tb, (T*)nullptr, (T*)nullptr, (size_t)m, less, ctx->stream));
  char* tmp = nullptr;
  T* d_sorted = nullptr;
  RTC_TRY(db.get(ctx, tb, &tmp));
  RTC_TRY(db.get(ctx, m, &d_sorted));
  RTC_HIP(ctx, rocprim::merge_sort(tmp, tb, *list, d_sorted, (size_t)m, less, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  db.release(tmp);
  db.release(*list);
  *list = d_sorted;
  return RTC_OK;
}

inline uint32_t wave_blocks_for(uint64_t waves, int num_cu) {  // blocks of four waves
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((waves + 3) / 4, (uint64_t)num_cu * 16));
}

}  // namespace

extern "C" int rtc_dbscan_knn(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                              double eps, int min_pts, int kmer_size, int max_posting, int knn_k, int32_t* h_labels, uint8_t* h_core,
                              uint32_t* h_n_clusters, uint32_t* h_n_noise) {
  const char* who = "rtc_dbscan_knn";
  if (!ctx || (n && (!d_hashes || !d_start || !d_len || !h_labels)) || (width != 4 && width != 8)) return RTC_ERR_ARG;
  memset(ctx->dbscan_knn, 0, sizeof ctx->dbscan_knn);
  ctx->dbscan_knn_propagate_ns = 0;
  // the u64 brute force never reads the k-NN graph (:384-442), and k <= 0 builds none (:240-243)
  if (knn_k <= 0 || width == 8)
    return rtc_dbscan(ctx, d_hashes, width, d_start, d_len, n, eps, min_pts, kmer_size, max_posting, h_labels, h_core, h_n_clusters, h_n_noise);
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u points", who, n);
  if (h_n_clusters) *h_n_clusters = 0;
  if (h_n_noise) *h_n_noise = 0;
  if (n == 0) return RTC_OK;
  if ((long long)knn_k < (long long)min_pts - 1) knn_k = min_pts - 1;  // :754-757
  const uint32_t k = (uint32_t)knn_k;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  uint64_t* out = ctx->dbscan_knn;
  EpsLevels lv;
  memset(&lv, 0, sizeof lv);
  if (!eps_to_t(eps, kmer_size, &lv.t[0], &lv.one_plus_t[0]))
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: eps %g with k %d gives jaccard_min %g <= 1e-12", who, eps, kmer_size, lv.t[0]);
  const double t = lv.t[0], one_plus_t = lv.one_plus_t[0];
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t max_len = *std::max_element(h_len.begin(), h_len.end());
  if (!u32_size_bound_fits(max_len, t)) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: size bound ceil(%u / %g) past INT_MAX", who, max_len, t);

  DevBuf db;
  const uint32_t* ph = (const uint32_t*)d_hashes;
  const uint64_t* pstart = d_start;
  const uint32_t* plen = d_len;
  if (max_posting > 0) {
    uint32_t *d_ph = nullptr, *d_plen = nullptr;
    uint64_t* d_pstart = nullptr;
    RTC_TRY(prune_postings(ctx, db, (const uint32_t*)d_hashes, d_start, d_len, n, h_len, (uint64_t)max_posting, &d_ph, &d_pstart, &d_plen));
    ph = d_ph; pstart = d_pstart; plen = d_plen;
  }

  // ---- the pair phase: the pairs that pass in some orientation, with MarkCnt's u16 count ----
  unsigned long long* d_cnt = nullptr;  // [0] pair count, [1..4] the counters of the kernel in flight
  RTC_TRY(db.get(ctx, 8, &d_cnt));
  KeptList kept;
  kept.cap = std::max<uint64_t>((uint64_t)1 << 16, (uint64_t)n * 16);
  RTC_TRY(db.get(ctx, kept.cap, &kept.d));
  PairPhase pp;
  auto on_chunk = [&](const rtc_cedge* d_cand, uint64_t cnt) -> int {
    if (!cnt) return RTC_OK;
    return filter_chunk(ctx, db, who, knn_keep_kernel, d_cand, cnt, d_len, lv, 1, 65535u, d_cnt + 1, &kept);
  };
  RTC_TRY(dbscan_pair_chunks(ctx, db, ph, 4, pstart, plen, n, 1, d_cnt, &pp, on_chunk));
  out[0] = pp.chunks; out[1] = pp.cand_total;

  // ---- (a) directed passers, (b) the selection, (c) arrival keys where a row needs them ----
  const uint64_t t_sel = now_ns();
  const uint64_t m_kept = kept.used, rec_cap = std::max<uint64_t>(2 * m_kept, 1);
  const dim3 b(256), gv(blocks_for(n, ctx->num_cu)), gw(wave_blocks_for(n, ctx->num_cu));
  KnnRec* d_rec = nullptr;
  uint32_t *d_rowcnt = nullptr, *d_ties = nullptr;
  uint64_t* d_off = nullptr;
  RTC_TRY(db.get(ctx, rec_cap, &d_rec));
  RTC_TRY(db.get(ctx, (size_t)n + 1, &d_rowcnt));  // the passers of every row, then its neighbours
  RTC_TRY(db.get(ctx, (size_t)n + 1, &d_off));
  RTC_TRY(db.get(ctx, n, &d_ties));
  RTC_HIP(ctx, hipMemsetAsync(d_rowcnt, 0, ((size_t)n + 1) * 4, s));
  RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 64, s));
  if (m_kept) {
    hipLaunchKernelGGL(knn_expand_kernel, dim3(blocks_for(m_kept, ctx->num_cu)), b, 0, s, (const rtc_cedge*)kept.d, m_kept, d_len, t, one_plus_t, d_rec,
                       rec_cap, d_rowcnt, d_cnt);
    RTC_CHECK_LAUNCH(ctx);
  }
  size_t tb = 0;
  RTC_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, (const uint32_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), s));
  void* tmp = nullptr;
  RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
  RTC_HIP(ctx, rocprim::exclusive_scan(tmp, tb, (const uint32_t*)d_rowcnt, d_off, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), s));
  unsigned long long fc[3] = {0, 0, 0};
  RTC_HIP(ctx, hipMemcpyAsync(fc, d_cnt, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint64_t m_rec = fc[0];
  if (m_rec > rec_cap) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu directed passers of %llu pairs", who, fc[0], (unsigned long long)m_kept);
  db.release(kept.d);
  out[2] = m_rec;
  RTC_TRY(knn_sort(ctx, db, &d_rec, m_rec, KnnRecLess{}));
  uint8_t* d_keep = nullptr;
  KnnArr* d_arr = nullptr;
  RTC_TRY(db.get(ctx, std::max<uint64_t>(m_rec, 1), &d_keep));
  // Every row's share of the list is known only after its selection: the rows are selected once to count (no list), the list is
  // sized, and they are selected again into it.
  uint64_t m_arr = 0;
  for (int pass = 0; pass < 2; pass++) {
    RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 64, s));
    hipLaunchKernelGGL(knn_select_kernel, gw, b, 0, s, (const KnnRec*)d_rec, (const uint64_t*)d_off, n, k, d_keep, d_ties, d_arr, pass ? m_arr : 0, d_cnt);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemcpyAsync(fc, d_cnt, sizeof fc, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    if (pass == 0) {
      m_arr = fc[0];
      if (!m_arr) break;
      RTC_TRY(db.get(ctx, m_arr, &d_arr));
    } else if (fc[0] != m_arr) {
      return rtc_fail(ctx, RTC_ERR_HIP, "%s: %llu passers need arrival keys, %llu at the first count", who, fc[0], (unsigned long long)m_arr);
    }
  }
  out[3] = fc[1]; out[4] = fc[2];
  if (m_arr) {
    uint64_t* d_head = nullptr;
    RTC_TRY(db.get(ctx, n, &d_head));
    hipLaunchKernelGGL(knn_first_shared_kernel, dim3(wave_blocks_for(m_arr, ctx->num_cu)), b, 0, s, ph, pstart, plen, d_arr, m_arr);
    RTC_CHECK_LAUNCH(ctx);
    RTC_TRY(knn_sort(ctx, db, &d_arr, m_arr, KnnArrLess{}));
    hipLaunchKernelGGL(knn_arr_heads_kernel, dim3(blocks_for(m_arr, ctx->num_cu)), b, 0, s, (const KnnArr*)d_arr, m_arr, d_head);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(knn_ties_kernel, gw, b, 0, s, (const KnnArr*)d_arr, (const uint64_t*)d_head, (const uint32_t*)d_ties, n, k, d_keep);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipStreamSynchronize(s));
    db.release(d_arr); db.release(d_head);
  }

  // ---- (d) neighbours, degrees, core points ----
  uint32_t *d_m = nullptr, *d_stamp = nullptr, *d_fa = nullptr, *d_fb = nullptr, *d_cid = nullptr;
  uint8_t* d_core = nullptr;
  RTC_TRY(db.get(ctx, n, &d_m));
  RTC_TRY(db.get(ctx, n, &d_stamp));  // the round stamps, then the root flags
  RTC_TRY(db.get(ctx, n, &d_fa));
  RTC_TRY(db.get(ctx, n, &d_fb));     // the second frontier, then the labels
  RTC_TRY(db.get(ctx, n, &d_cid));
  RTC_TRY(db.get(ctx, n, &d_core));
  RTC_HIP(ctx, hipMemsetAsync(d_rowcnt, 0, ((size_t)n + 1) * 4, s));
  RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 64, s));
  if (m_rec) {
    hipLaunchKernelGGL(knn_neighbour_kernel, dim3(blocks_for(m_rec, ctx->num_cu)), b, 0, s, d_rec, (const uint8_t*)d_keep, m_rec, t, d_rowcnt);
    RTC_CHECK_LAUNCH(ctx);
  }
  hipLaunchKernelGGL(knn_core_kernel, gv, b, 0, s, (const uint32_t*)d_rowcnt, n, (long long)min_pts, d_core, d_m, d_stamp, d_fa, d_cnt);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipMemcpyAsync(fc, d_cnt, 16, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  out[5] = fc[1]; out[6] = fc[0];
  const uint64_t t_prop = now_ns();
  out[8] = t_prop - t_sel;

  // ---- (e) min-propagation from the core points, frontier by frontier ----
  uint64_t nf = fc[0], rounds = 0;
  while (nf) {
    rounds++;
    if (rounds > (uint64_t)n + 1) return rtc_fail(ctx, RTC_ERR_HIP, "%s: propagation not settled after %llu rounds", who, (unsigned long long)rounds);
    RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 8, s));
    hipLaunchKernelGGL(knn_propagate_kernel, dim3(wave_blocks_for(nf, ctx->num_cu)), b, 0, s, (const KnnRec*)d_rec, (const uint64_t*)d_off,
                       (const uint8_t*)d_core, (const uint32_t*)d_fa, (uint32_t)nf, (uint32_t)rounds, n, d_m, d_stamp, d_fb, d_cnt);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemcpyAsync(fc, d_cnt, 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    if (fc[0] > n) return rtc_fail(ctx, RTC_ERR_HIP, "%s: a frontier of %llu points", who, fc[0]);
    nf = fc[0];
    std::swap(d_fa, d_fb);
  }
  out[7] = rounds;

  // ---- (f) the distinct values of m ranked into cluster numbers ----
  hipLaunchKernelGGL(knn_root_kernel, gv, b, 0, s, (const uint8_t*)d_core, (const uint32_t*)d_m, n, d_stamp);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(), s));
  RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
  RTC_HIP(ctx, rocprim::exclusive_scan(tmp, tb, (const uint32_t*)d_stamp, d_cid, 0u, (size_t)n, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(knn_label_kernel, gv, b, 0, s, (const uint32_t*)d_m, (const uint32_t*)d_cid, n, d_fb);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipMemcpyAsync(h_labels, d_fb, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  if (h_core) RTC_HIP(ctx, hipMemcpyAsync(h_core, d_core, (size_t)n, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  int32_t max_label = -1;
  uint32_t noise = 0;
  for (uint32_t v = 0; v < n; v++) {
    if (h_labels[v] < 0) noise++;
    else max_label = std::max(max_label, h_labels[v]);
  }
  if (h_n_clusters) *h_n_clusters = (uint32_t)(max_label + 1);
  if (h_n_noise) *h_n_noise = noise;
  const uint64_t t_end = now_ns();
  ctx->dbscan_knn_propagate_ns = t_end - t_prop;
  out[9] = t_end - t_begin;
  return RTC_OK;
}

extern "C" uint64_t rtc_dbscan_knn_propagate_ns(const rtc_ctx* ctx) { return ctx ? ctx->dbscan_knn_propagate_ns : 0; }

extern "C" int rtc_dbscan_knn_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->dbscan_knn[i];
  return RTC_OK;
}
