// rtc_graph.hip -- rtc_graph_build: the similarity graph of clust-leiden (the reference's KssdLeidenCluster, src/leiden.cpp:168-293)
// on the GPU.  One pair phase in row chunks (dbscan_pair_chunks), a filter kernel that appends the passing pairs to a growing
// list (filter_chunk's protocol), one rocPRIM merge sort by (u, rank, v) with an exact comparator and a segment-position kernel
// for the per-node top-k, and a final sort by (u, v).  The device forms no distance: the host bisects the least Jaccard value
// that passes through the very host function (graph_jstar) and the kernel compares one IEEE quotient with it.
// rtc_graph_build_mash (clust-leiden --minhash) is the same graph over MinHash sketches: the candidates of
// the same pair phase go through the union-truncated merge of rtc_dbscan_mash.h, the rule is rtc_mash_distance < threshold
// decided by one host-built table of counts, and the kept record carries (common, denom); kept list, top-k and sorts are shared.
#include "rtc_dbscan_mash.h"

namespace {

// calculate_mash_distance_fast (:109-121) from the quotient on: the reference forms jaccard = (double)common / union and goes on
// with it alone.  Host libm; the unit is built with -ffp-contract=off.
inline double dist_of_jaccard(double jaccard, int k) {
  if (jaccard <= 0.0) return 1.0;
  if (jaccard >= 1.0) return 0.0;
  const double mash_dist = -1.0 / k * log(2.0 * jaccard / (1.0 + jaccard));
  return std::max(0.0, std::min(1.0, mash_dist));
}

inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
inline uint64_t to_bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

// J*: the least double j with dist_of_jaccard(j) < threshold, threshold > 0.  Non-negative doubles order as their bit patterns.
// dist(1.0) = 0 passes; where dist(0.0) = 1 passes too (threshold > 1) every sharing pair is an edge and J* = 0.  The bisection
// keeps lo failing and hi passing -- mash_cmin_row's argument: the distance does not increase with j, log being monotone.  The
// rounding of 2j / (1 + j) can still turn the order of two doubles a few ulps apart, so the flip the bisection ends on is
// moved past the largest failing double within 64 ulps above it: a quotient that fails is then never kept, and one that passes
// could be dropped only within 64 ulps of a failing one -- the quotients of two pairs with unions below 2^22 differ by more
// than 256 ulps.
double graph_jstar(double threshold, int k) {
  if (dist_of_jaccard(0.0, k) < threshold) return 0.0;
  uint64_t lo = to_bits(0.0), hi = to_bits(1.0);
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (dist_of_jaccard(from_bits(mid), k) < threshold) hi = mid; else lo = mid;
  }
  const uint64_t top = std::min<uint64_t>(hi + 64, to_bits(1.0));
  for (uint64_t b = top; b > hi; b--)
    if (!(dist_of_jaccard(from_bits(b), k) < threshold)) { hi = b + 1; break; }
  return from_bits(hi);
}

// The edge rule for candidate (i > j, common >= 1): u = j, v = i.
//   - the size ratio: the reference skips the pair when (double)small / large < 0.5.  0.5 is a double and the quotient is
//     correctly rounded, so it is below 0.5 exactly when small / large is (a true quotient below 1/2 lies at least 1 / (2 large)
//     > 2^-34 under it, far more than half an ulp): the integer test 2 small < large is the same test.
//   - (double)common / (double)union >= J* (lv.t[0]), the reference's own quotient: the sketches are shorter than 2^31 hashes, so
//     its int union does not wrap.
// The kept record stays a rtc_cedge (i = v, j = u): the sorts and the top-k read it, the host turns it into rtc_gedge.
__global__ __launch_bounds__(256) void graph_filter_kernel(const rtc_cedge* __restrict__ cand, uint64_t m, const uint32_t* __restrict__ len,
                                                           EpsLevels lv, uint32_t, uint32_t, rtc_cedge* __restrict__ out, uint64_t cap,
                                                           unsigned long long* __restrict__ cnt) {
  const double jstar = lv.t[0];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t rounds = (m + stride - 1) / stride;  // every lane of a wave reaches wave_append
  for (uint64_t r = 0; r < rounds; r++) {
    const uint64_t idx = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    rtc_cedge c{0, 0, 0};
    if (idx < m) {
      c = cand[idx];
      const uint64_t a = len[c.j], b = len[c.i];
      const uint64_t small = a < b ? a : b, large = a < b ? b : a;
      if (c.common && a && b && !(2 * small < large))
        keep = (double)c.common / (double)(a + b - c.common) >= jstar;
    }
    wave_append(keep, c, out, cap, cnt);
  }
}

// (u, rank, v): u ascending, then common / union descending -- compared exactly, common_a union_b against common_b union_a in
// 64 bits (common < 2^31, union < 2^32) -- then v ascending
struct RankLess {
  const uint32_t* len;
  __device__ bool operator()(const rtc_cedge& x, const rtc_cedge& y) const {
    if (x.j != y.j) return x.j < y.j;
    const uint64_t lu = len[x.j];
    const uint64_t ux = lu + len[x.i] - x.common, uy = lu + len[y.i] - y.common;
    const uint64_t l = (uint64_t)x.common * uy, r = (uint64_t)y.common * ux;
    if (l != r) return l > r;
    return x.i < y.i;
  }
};
// the MinHash graph's rank: common / denom of the truncated merge, both at most sketch_size < 2^32
struct MashRankLess {
  __device__ bool operator()(const rtc_medge& x, const rtc_medge& y) const {
    if (x.j != y.j) return x.j < y.j;
    const uint64_t l = (uint64_t)x.common * y.denom, r = (uint64_t)y.common * x.denom;
    if (l != r) return l > r;
    return x.i < y.i;
  }
};
struct PairLess {
  template <class R>
  __device__ bool operator()(const R& x, const R& y) const { return x.j != y.j ? x.j < y.j : x.i < y.i; }
};

// The list sorted by RankLess: record idx is kept when fewer than knn_k records of its u come before it.  The segment's start
// is the lower bound of u in the list.  cnt[0]: kept so far (wave_append), cnt[1]: nodes that lost an edge.
template <class R>
__global__ __launch_bounds__(256) void graph_topk_kernel(const R* __restrict__ sorted, uint64_t m, uint32_t knn_k,
                                                         R* __restrict__ out, uint64_t cap, unsigned long long* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t rounds = (m + stride - 1) / stride;
  for (uint64_t r = 0; r < rounds; r++) {
    const uint64_t idx = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    R c{};
    if (idx < m) {
      c = sorted[idx];
      uint64_t lo = 0, hi = idx;  // first record of u: sorted[lo - 1].j < u <= sorted[hi].j
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (sorted[mid].j < c.j) lo = mid + 1; else hi = mid;
      }
      keep = idx - lo < knn_k;
      if (idx - lo == knn_k) atomicAdd(&cnt[1], 1ull);
    }
    wave_append(keep, c, out, cap, cnt);
  }
}

// *list sorted by `less` into a list of its own; the unsorted one is released
template <class R, class Less>
int sort_kept(rtc_ctx* ctx, DevBuf& db, R** list, uint64_t m, Less less) {
  if (m < 2) return RTC_OK;
  size_t tb = 0;
  RTC_HIP(ctx, rocprim::merge_sort(nullptr, tb, (R*)nullptr, (R*)nullptr, (size_t)m, less, ctx->stream));
  char* tmp = nullptr;
  R* d_sorted = nullptr;
  RTC_TRY(db.get(ctx, tb, &tmp));
  RTC_TRY(db.get(ctx, m, &d_sorted));
  RTC_HIP(ctx, rocprim::merge_sort(tmp, tb, *list, d_sorted, (size_t)m, less, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  db.release(tmp);
  db.release(*list);
  *list = d_sorted;
  return RTC_OK;
}

// The kept list to the call's edges: with knn_k > 0 the sort by `rank` and the position test, then the sort by (u, v).  The
// list passed in is released or handed on in *d_final.  d_fc: two device counters.
template <class R, class Rank>
int select_edges(rtc_ctx* ctx, DevBuf& db, R* d_kept, uint64_t used, uint32_t knn_k, Rank rank, unsigned long long* d_fc, R** d_final,
                 uint64_t* n_final, uint64_t* cut) {
  hipStream_t s = ctx->stream;
  *d_final = d_kept; *n_final = used; *cut = 0;
  if (knn_k > 0 && used) {
    RTC_TRY(sort_kept(ctx, db, &d_kept, used, rank));
    R* d_top = nullptr;
    RTC_TRY(db.get(ctx, used, &d_top));
    unsigned long long fc[2] = {0ull, 0ull};
    RTC_HIP(ctx, hipMemcpyAsync(d_fc, fc, sizeof fc, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(graph_topk_kernel<R>, dim3(blocks_for(used, ctx->num_cu)), dim3(256), 0, s, (const R*)d_kept, used, knn_k, d_top, used, d_fc);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemcpyAsync(fc, d_fc, sizeof fc, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    db.release(d_kept);
    *d_final = d_top; *n_final = fc[0]; *cut = fc[1];
  }
  return sort_kept(ctx, db, d_final, *n_final, PairLess{});
}

}  // namespace

double rtc_graph_jstar(double threshold, int kmer_size) { return graph_jstar(threshold, kmer_size); }

extern "C" double rtc_graph_weight(uint32_t common, uint32_t size_u, uint32_t size_v, int kmer_size) {
  if (common == 0) return 0.0;  // distance 1
  const uint64_t union_size = (uint64_t)size_u + size_v - common;
  if (union_size == 0) return 0.0;
  return 1.0 - dist_of_jaccard((double)common / (double)union_size, kmer_size);
}

extern "C" int rtc_graph_build(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                               double threshold, int kmer_size, uint32_t knn_k, rtc_gedge* h_edges, uint64_t cap, uint64_t* h_n_edges) {
  const char* who = "rtc_graph_build";
  if (!ctx || !h_n_edges || (n && (!d_hashes || !d_start || !d_len)) || (width != 4 && width != 8) || (cap && !h_edges)) return RTC_ERR_ARG;
  if (!(threshold > 0.0)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: threshold %g", who, threshold);
  if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: k-mer size %d", who, kmer_size);
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u points", who, n);
  *h_n_edges = 0;
  memset(ctx->graph, 0, sizeof ctx->graph);
  if (n < 2) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t max_len = *std::max_element(h_len.begin(), h_len.end());
  if (max_len >= 0x80000000u)  // the reference's int sizes, and the ranker's 64-bit products
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: a sketch of %u hashes, the edge rule is exact below 2^31", who, max_len);
  EpsLevels lv;
  memset(&lv, 0, sizeof lv);
  lv.t[0] = graph_jstar(threshold, kmer_size);

  DevBuf db;
  unsigned long long* d_cnt = nullptr;  // [0] pair count, [1..4] the counters of the kernel in flight
  RTC_TRY(db.get(ctx, 8, &d_cnt));
  KeptList kept;
  kept.cap = std::max<uint64_t>((uint64_t)1 << 16, (uint64_t)n * 16);
  RTC_TRY(db.get(ctx, kept.cap, &kept.d));
  PairPhase pp;
  auto on_chunk = [&](const rtc_cedge* d_cand, uint64_t cnt) -> int {
    if (!cnt) return RTC_OK;
    return filter_chunk(ctx, db, who, graph_filter_kernel, d_cand, cnt, d_len, lv, 1, 0xffffffffu, d_cnt + 1, &kept);
  };
  RTC_TRY(dbscan_pair_chunks(ctx, db, d_hashes, width, d_start, d_len, n, 1, d_cnt, &pp, on_chunk));

  const uint64_t t_sel = now_ns();
  rtc_cedge* d_final = nullptr;
  uint64_t n_final = 0, cut = 0;
  RTC_TRY(select_edges(ctx, db, kept.d, kept.used, knn_k, RankLess{d_len}, d_cnt + 1, &d_final, &n_final, &cut));
  const uint64_t t_out = now_ns();
  *h_n_edges = n_final;
  uint64_t* g = ctx->graph;
  g[0] = pp.chunks; g[1] = pp.cand_total; g[2] = kept.used; g[3] = n_final; g[4] = cut;
  g[5] = pp.pair_ns; g[6] = kept.ns; g[7] = t_out - t_sel;
  if (n_final > cap) {
    g[9] = now_ns() - t_begin;
    return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu edges, room for %llu", who, (unsigned long long)n_final, (unsigned long long)cap);
  }
  std::vector<rtc_cedge> h(n_final);
  if (n_final) {
    RTC_HIP(ctx, hipMemcpyAsync(h.data(), d_final, n_final * sizeof(rtc_cedge), hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
  }
  for (uint64_t e = 0; e < n_final; e++) h_edges[e] = rtc_gedge{h[e].j, h[e].i, h[e].common, 0};
  g[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" double rtc_graph_weight_mash(uint32_t common, uint32_t denom, uint32_t sketch_size, int kmer_size) {
  return 1.0 - rtc_mash_distance_host(common, denom, sketch_size, kmer_size);
}

// rtc_graph_build_mash's table for one threshold, on the host alone: out[d] for d = 0 .. sketch_size
extern "C" int rtc_graph_mash_table(uint32_t sketch_size, int kmer_size, double threshold, uint32_t* out) {
  if (!out || sketch_size == 0 || kmer_size < 1 || !(threshold > 0.0) || threshold > 1.0) return RTC_ERR_ARG;
  mash_cmin_row<true>(sketch_size, sketch_size, kmer_size, threshold, out);
  return RTC_OK;
}

extern "C" int rtc_graph_build_mash(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                    uint32_t sketch_size, double threshold, int kmer_size, uint32_t knn_k, rtc_gedge* h_edges, uint64_t cap,
                                    uint64_t* h_n_edges) {
  const char* who = "rtc_graph_build_mash";
  if (!ctx || !h_n_edges || (n && (!d_hashes || !d_start || !d_len)) || (width != 4 && width != 8) || (cap && !h_edges)) return RTC_ERR_ARG;
  if (!(threshold > 0.0)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: threshold %g", who, threshold);
  if (threshold > 1.0)  // pairs without a shared hash have distance 1 and no candidate list holds them
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: threshold %g above 1 would make edges of pairs that share no hash", who, threshold);
  if (sketch_size == 0) return rtc_fail(ctx, RTC_ERR_ARG, "%s: sketch size 0", who);
  if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: k-mer size %d", who, kmer_size);
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u points", who, n);
  *h_n_edges = 0;
  memset(ctx->graph, 0, sizeof ctx->graph);
  if (n < 2) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t max_len = *std::max_element(h_len.begin(), h_len.end());

  DevBuf db;
  MashTables mt;
  RTC_TRY(mash_tables<true>(ctx, db, sketch_size, max_len, kmer_size, &threshold, 1, &mt));
  unsigned long long* d_cnt = nullptr;  // [0] pair count, [1..2] the counters of the kernel in flight
  RTC_TRY(db.get(ctx, 8, &d_cnt));
  KeptListOf<rtc_medge> kept;
  kept.cap = std::max<uint64_t>((uint64_t)1 << 16, (uint64_t)n * 16);
  RTC_TRY(db.get(ctx, kept.cap, &kept.d));
  PairPhase pp;
  uint64_t merged = 0;
  auto on_chunk = [&](const rtc_cedge* d_cand, uint64_t cnt) -> int {
    if (!cnt) return RTC_OK;
    return mash_filter_chunk(ctx, db, who, d_hashes, width, d_start, d_len, sketch_size, d_cand, cnt, mt, 1, d_cnt + 1, &kept, &merged);
  };
  RTC_TRY(dbscan_pair_chunks(ctx, db, d_hashes, width, d_start, d_len, n, 1, d_cnt, &pp, on_chunk));

  const uint64_t t_sel = now_ns();
  rtc_medge* d_final = nullptr;
  uint64_t n_final = 0, cut = 0;
  RTC_TRY(select_edges(ctx, db, kept.d, kept.used, knn_k, MashRankLess{}, d_cnt + 1, &d_final, &n_final, &cut));
  const uint64_t t_out = now_ns();
  *h_n_edges = n_final;
  uint64_t* g = ctx->graph;
  g[0] = pp.chunks; g[1] = pp.cand_total; g[2] = kept.used; g[3] = n_final; g[4] = cut;
  g[5] = pp.pair_ns; g[6] = kept.ns; g[7] = t_out - t_sel; g[8] = merged;
  if (n_final > cap) {
    g[9] = now_ns() - t_begin;
    return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu edges, room for %llu", who, (unsigned long long)n_final, (unsigned long long)cap);
  }
  std::vector<rtc_medge> h(n_final);
  if (n_final) {
    RTC_HIP(ctx, hipMemcpyAsync(h.data(), d_final, n_final * sizeof(rtc_medge), hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
  }
  for (uint64_t e = 0; e < n_final; e++) h_edges[e] = rtc_gedge{h[e].j, h[e].i, h[e].common, h[e].denom};
  g[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_graph_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->graph[i];
  return RTC_OK;
}
