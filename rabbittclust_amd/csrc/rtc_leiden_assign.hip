// rtc_leiden_assign.hip -- clust-leiden --db --assign: new genomes placed into the communities of a finished run
// (include/rtclust.h defines the placement).  Two calls with the host's weights between them, as the build goes
// rtc_graph_build, weights, rtc_louvain.
//
// rtc_graph_query: the set on the device is the model's rows [0, n_db) followed by the queries' rows, the layout of
// rtc_rep_topk.  A chunk of queries (for_query_chunks, rtc_query_chunks.h) goes through five steps on the device:
//   1. join     query_candidates: rtc_pair_edges_join with the columns [0, n_db) only.
//   2. bucket   query_segments: the segment of every query.
//   3. scatter  a lane per candidate evaluates rtc_graph_build's edge rule, writes (p, common, union, pass) into the query's
//               segment and appends the passing ones, with their query, to one list (wave_append).  A workgroup per query then
//               folds the segment -- one wave up to TK_LONG records, 256 lanes beyond -- into the passing count and the nearest
//               candidate by cross-lane shuffles (tk_fold_segment over LqFold, as as_fold_kernel over AsFold): no atomics on a
//               query's record.
//   4. select   knn_k is typically 500 or 1 000, past what the running selection of rtc_topk_select.h holds (TK_KMAX = 256: two
//               tables and a tile of 16-byte records in LDS, and every survivor of a tile ranked against every other one, k
//               comparisons a record).  So the passing list is sorted once by (q, rank, p) with the exact comparator -- the
//               rocPRIM merge sort rtc_graph_build uses -- and a record is kept when fewer than knn_k records of its query come
//               before it, the position test of graph_topk_kernel.  No cap on knn_k, no LDS, and the cost does not grow with it.
//   5. output   a sort by (q, p) and the read-back.
// A chunk whose candidates exceed the edge budget or whose join scratch does not fit is halved; RTC_ERR_NOMEM past one query.
//
// rtc_leiden_place: the records (query, model genome, q) become a CSR by one radix sort and one reduce_by_key (equal pairs
// summed), the rows are split by length as a level's rows are (RowPaths) and row_kernel under place_rule (rtc_community.h)
// scores them.
#include "rtc_community.h"
#include "rtc_query_chunks.h"

namespace {

constexpr uint32_t LQ_NONE = 0xffffffffu;

// rtc_graph_build's edge rule (graph_filter_kernel) for candidate (row0 + q, p, common).  cnt[0]: the passing list's length.
__global__ __launch_bounds__(256) void lq_scatter_kernel(const rtc_cedge* __restrict__ e, uint64_t m, uint32_t row0, uint32_t nq, uint32_t q_first,
                                                         uint32_t n_db, const uint32_t* __restrict__ len, double jstar,
                                                         const uint64_t* __restrict__ off, uint32_t* __restrict__ cursor, TkRec* __restrict__ seg,
                                                         rtc_qedge* __restrict__ pass, uint64_t cap, unsigned long long* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t rounds = (m + stride - 1) / stride;  // every lane of a wave reaches wave_append
  for (uint64_t r = 0; r < rounds; r++) {
    const uint64_t idx = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    rtc_qedge k{0, 0, 0, 0};
    if (idx < m) {
      const rtc_cedge c = e[idx];
      const uint32_t q = c.i - row0;
      if (q < nq && c.j < n_db) {
        const uint64_t a = len[c.j], b = len[c.i];
        const uint64_t small = a < b ? a : b, large = a < b ? b : a;
        const uint64_t uni = a + b - c.common;
        if (c.common && a && b && !(2 * small < large)) keep = (double)c.common / (double)uni >= jstar;
        TkRec t;
        t.slot = c.j; t.common = c.common; t.denom = (uint32_t)uni; t.pad = keep ? 1u : 0u;
        const uint32_t p = atomicAdd(&cursor[q], 1u);
        if (off[q] + p < off[q + 1]) seg[off[q] + p] = t;
        k.q = q_first + q; k.p = c.j; k.common = c.common; k.pad = (uint32_t)uni;  // pad: the union until the output
      }
    }
    wave_append(keep, k, pass, cap, cnt);
  }
}

// What a lane, a wave and then the workgroup hold of a query's segment (tk_fold_segment's F)
struct LqFold {
  TkRec best;   // over every candidate
  uint32_t np;  // the passing ones
  __device__ __forceinline__ void take(const TkRec& x) {
    np += x.pad & 1u;
    if (tk_beats(x, best)) best = x;
  }
  __device__ __forceinline__ void merge(const LqFold& b) {
    np += b.np;
    if (tk_beats(b.best, best)) best = b.best;
  }
};

// a workgroup of B lanes per query whose segment length lies in [lo, hi]
template <int B>
__global__ __launch_bounds__(B) void lq_fold_kernel(const TkRec* __restrict__ seg, const uint64_t* __restrict__ off, uint32_t nq, uint32_t lo,
                                                    uint32_t hi, rtc_graph_near* __restrict__ out) {
  __shared__ LqFold part[B > 64 ? B / 64 : 1];
  const uint32_t q = blockIdx.x;
  if (q >= nq) return;
  const uint64_t s0 = off[q], s1 = off[q + 1];
  if (s1 - s0 < lo || s1 - s0 > hi) return;  // uniform across the workgroup
  // key 0 / 1: below every candidate's, each shares a hash
  const LqFold f = tk_fold_segment<B>(seg, s0, s1, LqFold{TkRec{LQ_NONE, 0, 1, 0}, 0}, part);
  if (threadIdx.x == 0) {
    const bool none = f.best.slot == LQ_NONE;
    rtc_graph_near r;
    r.nearest = f.best.slot; r.common = none ? 0u : f.best.common; r.denom = none ? 0u : f.best.denom;
    r.n_candidates = (uint32_t)(s1 - s0); r.n_passing = f.np; r.n_kept = f.np;
    out[q] = r;
  }
}

// (q, rank, p): RankLess of rtc_graph.hip with the union carried in the record
struct QRankLess {
  __device__ bool operator()(const rtc_qedge& x, const rtc_qedge& y) const {
    if (x.q != y.q) return x.q < y.q;
    const uint64_t l = (uint64_t)x.common * y.pad, r = (uint64_t)y.common * x.pad;
    if (l != r) return l > r;
    return x.p < y.p;
  }
};
struct QPairLess {
  __device__ bool operator()(const rtc_qedge& x, const rtc_qedge& y) const { return x.q != y.q ? x.q < y.q : x.p < y.p; }
};

// graph_topk_kernel's position test on the list sorted by QRankLess.  cnt[0]: kept so far, cnt[1]: queries that lost a record.
__global__ __launch_bounds__(256) void lq_topk_kernel(const rtc_qedge* __restrict__ sorted, uint64_t m, uint32_t knn_k, rtc_qedge* __restrict__ out,
                                                      uint64_t cap, unsigned long long* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t rounds = (m + stride - 1) / stride;
  for (uint64_t r = 0; r < rounds; r++) {
    const uint64_t idx = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    rtc_qedge c{0, 0, 0, 0};
    if (idx < m) {
      c = sorted[idx];
      uint64_t lo = 0, hi = idx;  // first record of q
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (sorted[mid].q < c.q) lo = mid + 1; else hi = mid;
      }
      keep = idx - lo < knn_k;
      if (idx - lo == knn_k) atomicAdd(&cnt[1], 1ull);
    }
    wave_append(keep, c, out, cap, cnt);
  }
}

// *list sorted by `less` into a list of its own; the unsorted one is released
template <class Less>
int lq_sort(rtc_ctx* ctx, DevBuf& db, rtc_qedge** list, uint64_t m, Less less) {
  if (m < 2) return RTC_OK;
  size_t tb = 0;
  RTC_HIP(ctx, rocprim::merge_sort(nullptr, tb, (rtc_qedge*)nullptr, (rtc_qedge*)nullptr, (size_t)m, less, ctx->stream));
  char* tmp = nullptr;
  rtc_qedge* d_sorted = nullptr;
  RTC_TRY(db.get(ctx, tb, &tmp));
  RTC_TRY(db.get(ctx, m, &d_sorted));
  RTC_HIP(ctx, rocprim::merge_sort(tmp, tb, *list, d_sorted, (size_t)m, less, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  db.release(tmp);
  db.release(*list);
  *list = d_sorted;
  return RTC_OK;
}

struct LqArgs {
  const void* d_hashes; int width; const uint64_t* d_start; const uint32_t* d_len; uint32_t n, n_db;
  double jstar; uint32_t knn_k; uint64_t budget;
  unsigned long long* d_fc;  // [0] list length (wave_append), [1] queries cut
};
struct LqStats { uint64_t candidates = 0, passing = 0, kept = 0, cut = 0, join_ns = 0, bucket_ns = 0, select_ns = 0; };

// queries [q0, q1): h_near[0 .. q1 - q0) holds the defaults and keeps them where nothing can share a hash; the chunk's records
// are appended to *edges in (q, p) order.  RTC_ERR_NOMEM: the candidates are past the budget or the join's scratch did not fit.
int query_chunk_run(rtc_ctx* ctx, const LqArgs& A, const std::vector<uint32_t>& h_len, uint32_t q0, uint32_t q1, rtc_graph_near* h_near,
                    std::vector<rtc_qedge>* edges, LqStats* st) {
  const char* who = "rtc_graph_query";
  const uint32_t R = A.n_db, row0 = R + q0, row1 = R + q1, nq = q1 - q0;
  if (query_rows_alone(h_len, R, row0, row1)) return RTC_OK;
  hipStream_t s = ctx->stream;
  DevBuf db;
  const uint64_t t0 = now_ns();
  // ---- 1. candidates (row, p, common) from the join ----
  rtc_cedge* d_edges = nullptr;
  uint64_t m = 0;
  RTC_TRY(query_candidates(ctx, db, who, A.d_hashes, A.width, A.d_start, A.d_len, A.n, row0, row1, R, A.budget, &d_edges, &m));
  const uint64_t t1 = now_ns();
  st->join_ns += t1 - t0;
  if (m == 0) return RTC_OK;
  // ---- 2. count, scan; 3. edge rule + scatter, fold ----
  QuerySegments S;
  RTC_TRY(query_segments(ctx, db, d_edges, m, row0, nq, R, nullptr, 0u, &S));
  const uint64_t T = S.T;
  st->candidates += T;
  if (T == 0) return RTC_OK;
  TkRec* d_seg = nullptr;
  rtc_qedge* d_pass = nullptr;
  RTC_TRY(db.get(ctx, T, &d_seg));
  RTC_TRY(db.get(ctx, T, &d_pass));
  unsigned long long fc[2] = {0ull, 0ull};
  RTC_HIP(ctx, hipMemcpyAsync(A.d_fc, fc, sizeof fc, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(lq_scatter_kernel, dim3(blocks_for(m, ctx->num_cu)), dim3(256), 0, s, (const rtc_cedge*)d_edges, m, row0, nq, q0, R, A.d_len,
                     A.jstar, (const uint64_t*)S.d_off, S.d_cur, d_seg, d_pass, T, A.d_fc);
  RTC_CHECK_LAUNCH(ctx);
  uint64_t n_long = 0;
  for (uint32_t q = 0; q < nq; q++) n_long += S.h_cnt[q] > TK_LONG;
  rtc_graph_near* d_near = nullptr;
  RTC_TRY(db.get(ctx, nq, &d_near));
  if (n_long < nq) {
    hipLaunchKernelGGL(lq_fold_kernel<64>, dim3(nq), dim3(64), 0, s, (const TkRec*)d_seg, (const uint64_t*)S.d_off, nq, 0u, TK_LONG, d_near);
    RTC_CHECK_LAUNCH(ctx);
  }
  if (n_long) {
    hipLaunchKernelGGL(lq_fold_kernel<256>, dim3(nq), dim3(256), 0, s, (const TkRec*)d_seg, (const uint64_t*)S.d_off, nq, TK_LONG + 1, 0xffffffffu,
                       d_near);
    RTC_CHECK_LAUNCH(ctx);
  }
  RTC_HIP(ctx, hipMemcpyAsync(h_near, d_near, (size_t)nq * sizeof(rtc_graph_near), hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(fc, A.d_fc, sizeof fc, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  db.release(d_edges);
  db.release(d_seg);
  const uint64_t n_pass = fc[0];
  if (n_pass > T) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu passing of %llu candidates", who, (unsigned long long)n_pass, (unsigned long long)T);
  st->passing += n_pass;
  const uint64_t t2 = now_ns();
  st->bucket_ns += t2 - t1;
  // ---- 4. the knn_k best of every query, 5. (q, p) order and the read-back ----
  rtc_qedge* d_final = d_pass;
  uint64_t n_final = n_pass;
  if (A.knn_k > 0 && n_pass) {
    RTC_TRY(lq_sort(ctx, db, &d_pass, n_pass, QRankLess{}));
    rtc_qedge* d_top = nullptr;
    RTC_TRY(db.get(ctx, n_pass, &d_top));
    fc[0] = fc[1] = 0ull;
    RTC_HIP(ctx, hipMemcpyAsync(A.d_fc, fc, sizeof fc, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(lq_topk_kernel, dim3(blocks_for(n_pass, ctx->num_cu)), dim3(256), 0, s, (const rtc_qedge*)d_pass, n_pass, A.knn_k, d_top,
                       n_pass, A.d_fc);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemcpyAsync(fc, A.d_fc, sizeof fc, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    db.release(d_pass);
    d_final = d_top; n_final = fc[0];
    st->cut += fc[1];
  }
  RTC_TRY(lq_sort(ctx, db, &d_final, n_final, QPairLess{}));
  if (n_final) {
    const size_t at = edges->size();
    edges->resize(at + n_final);
    RTC_HIP(ctx, hipMemcpyAsync(edges->data() + at, d_final, n_final * sizeof(rtc_qedge), hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    for (size_t e = at; e < edges->size(); e++) (*edges)[e].pad = 0;
  }
  st->kept += n_final;
  for (uint32_t q = 0; q < nq; q++)
    if (A.knn_k && h_near[q].n_passing > A.knn_k) h_near[q].n_kept = A.knn_k;
  st->select_ns += now_ns() - t2;
  return RTC_OK;
}

}  // namespace

extern "C" int rtc_graph_query(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n_db,
                               uint32_t n_queries, double threshold, int kmer_size, uint32_t knn_k, uint32_t query_chunk, rtc_qedge* h_edges,
                               uint64_t cap, uint64_t* h_n_edges, rtc_graph_near* h_near) {
  const char* who = "rtc_graph_query";
  if (!ctx || !h_n_edges || (width != 4 && width != 8) || (cap && !h_edges)) return RTC_ERR_ARG;
  if ((uint64_t)n_db + n_queries >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u + %u points", who, n_db, n_queries);
  const uint32_t n = n_db + n_queries;
  if (n && (!d_hashes || !d_start || !d_len)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: no sketches", who);
  if (n_queries && !h_near) return rtc_fail(ctx, RTC_ERR_ARG, "%s: no room for the queries' records (h_near)", who);
  if (!(threshold > 0.0)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: threshold %g", who, threshold);
  if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: k-mer size %d", who, kmer_size);
  *h_n_edges = 0;
  memset(ctx->graph_query, 0, sizeof ctx->graph_query);
  if (n_queries == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t max_len = *std::max_element(h_len.begin(), h_len.end());
  if (max_len >= 0x80000000u)  // the reference's int sizes, and the ranker's 64-bit products
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: a sketch of %u hashes, the edge rule is exact below 2^31", who, max_len);
  LqArgs A;
  A.d_hashes = d_hashes; A.width = width; A.d_start = d_start; A.d_len = d_len; A.n = n; A.n_db = n_db;
  A.jstar = rtc_graph_jstar(threshold, kmer_size);
  A.knn_k = knn_k;
  A.budget = ctx->opt.edge_budget ? ctx->opt.edge_budget : (uint64_t)256 << 20;
  A.budget = std::max<uint64_t>(A.budget, (uint64_t)n_db + 1024);  // one query's candidates always fit
  const rtc_graph_near none{LQ_NONE, 0, 0, 0, 0, 0};
  std::fill(h_near, h_near + n_queries, none);
  DevBuf db;
  RTC_TRY(db.get(ctx, 2, &A.d_fc));
  LqStats st;
  std::vector<rtc_qedge> edges;
  LqStats before;
  size_t had = 0;
  uint64_t chunks = 0;
  RTC_TRY(for_query_chunks(
      ctx, n_queries, query_chunk,
      [&](uint32_t q0, uint32_t q1) {
        before = st;
        had = edges.size();
        return query_chunk_run(ctx, A, h_len, q0, q1, h_near + q0, &edges, &st);
      },
      [&](uint32_t q0, uint32_t q1) {
        st = before;
        edges.resize(had);
        std::fill(h_near + q0, h_near + q1, none);
      },
      &chunks));
  uint64_t lonely = 0;
  for (uint32_t q = 0; q < n_queries; q++) lonely += h_near[q].n_candidates == 0;
  *h_n_edges = edges.size();
  const uint64_t c[10] = {chunks, st.candidates, st.passing, st.kept, st.cut, lonely, st.join_ns, st.bucket_ns, st.select_ns, 0};
  std::copy(c, c + 10, ctx->graph_query);
  if (edges.size() > cap) {
    ctx->graph_query[9] = now_ns() - t_begin;
    return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu edges, room for %llu", who, (unsigned long long)edges.size(), (unsigned long long)cap);
  }
  if (!edges.empty()) memcpy(h_edges, edges.data(), edges.size() * sizeof(rtc_qedge));
  ctx->graph_query[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_graph_query_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->graph_query[i];
  return RTC_OK;
}

namespace {
// the CSR's keys: query << 32 | model genome
__global__ __launch_bounds__(256) void place_entries_kernel(const rtc_wedge* __restrict__ edges, uint64_t m, uint64_t* __restrict__ key,
                                                            uint64_t* __restrict__ w) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_wedge r = edges[e];
    key[e] = ((uint64_t)r.u << 32) | r.v;
    w[e] = r.q;
  }
}
}  // namespace

extern "C" int rtc_leiden_place(rtc_ctx* ctx, uint32_t n_db, const int32_t* h_labels, uint32_t n_clusters, const uint64_t* h_tot, uint64_t m2,
                                double resolution, int objective, uint32_t n_queries, const rtc_wedge* h_edges, uint64_t m,
                                rtc_leiden_placement* h_out) {
  const char* who = "rtc_leiden_place";
  if (!ctx || (n_db && !h_labels) || (m && !h_edges) || (n_queries && !h_out)) return RTC_ERR_ARG;
  if (objective != RTC_LEIDEN_CPM && objective != RTC_LEIDEN_MODULARITY) return rtc_fail(ctx, RTC_ERR_ARG, "%s: objective %d", who, objective);
  const bool modularity = objective == RTC_LEIDEN_MODULARITY;
  if (modularity && n_clusters && !h_tot) return rtc_fail(ctx, RTC_ERR_ARG, "%s: the model's community totals (h_tot) are missing", who);
  if (!(resolution > 0.0) || !(resolution * 65536.0 < 4294967295.5)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: resolution %g", who, resolution);
  const uint64_t g = (uint64_t)llround(resolution * 65536.0);
  if (g == 0 || g >= (1ull << 32)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: resolution %g", who, resolution);
  if (n_db >= 0x7fffffffu || n_queries >= 0x7fffffffu || n_clusters >= 0x7fffffffu)
    return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u genomes, %u clusters, %u queries", who, n_db, n_clusters, n_queries);
  std::vector<uint64_t> tot(std::max<uint32_t>(n_clusters, 1), 0);
  for (uint32_t p = 0; p < n_db; p++) {
    if (h_labels[p] < 0 || (uint32_t)h_labels[p] >= n_clusters)
      return rtc_fail(ctx, RTC_ERR_ARG, "%s: genome %u has label %d with %u clusters", who, p, h_labels[p], n_clusters);
    if (!modularity) tot[h_labels[p]]++;
  }
  if (modularity) std::copy(h_tot, h_tot + n_clusters, tot.begin());
  if (modularity && m2 >= (1ull << 46)) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: total weight past 2^46 units", who);
  std::vector<uint64_t> kx(n_queries, 0);
  for (uint64_t e = 0; e < m; e++) {
    if (h_edges[e].u >= n_queries || h_edges[e].v >= n_db || h_edges[e].q == 0)
      return rtc_fail(ctx, RTC_ERR_ARG, "%s: record %llu is (%u, %u, %u) with %u queries and %u genomes", who, (unsigned long long)e, h_edges[e].u,
                      h_edges[e].v, h_edges[e].q, n_queries, n_db);
    kx[h_edges[e].u] += h_edges[e].q;
    if (modularity && m2 + 2 * kx[h_edges[e].u] >= (1ull << 46))
      return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: total weight past 2^46 units with query %u", who, h_edges[e].u);
    if (kx[h_edges[e].u] >= (1ull << 62)) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: query %u's weight past 2^62 units", who, h_edges[e].u);
  }
  memset(ctx->leiden_place, 0, sizeof ctx->leiden_place);
  ctx->leiden_place_path = 0;
  const rtc_leiden_placement none{-1, -1, 0, 0, 0, 0, 0};
  std::fill(h_out, h_out + n_queries, none);
  if (m == 0 || n_queries == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();

  Louvain L{ctx};  // its scratch list and, for RowPaths, the row offsets
  uint64_t *key_in = nullptr, *key_sorted = nullptr, *key = nullptr, *w_in = nullptr, *w_sorted = nullptr, *w = nullptr, *d_tot = nullptr;
  int32_t* d_labels = nullptr;
  rtc_leiden_placement* d_out = nullptr;
  unsigned long long* d_cnt = nullptr;
  for (uint64_t** p : {&key_in, &key_sorted, &key, &w_in, &w_sorted, &w}) RTC_TRY(L.db.get(ctx, m, p));
  RTC_TRY(L.db.get(ctx, (size_t)n_queries + 1, &L.row_off));
  RTC_TRY(L.db.get(ctx, tot.size(), &d_tot));
  RTC_TRY(L.db.get(ctx, n_db, &d_labels));
  RTC_TRY(L.db.get(ctx, n_queries, &d_out));
  RTC_TRY(L.db.get(ctx, 2, &d_cnt));
  {
    rtc_wedge* d_edges = nullptr;
    RTC_TRY(L.db.get(ctx, m, &d_edges));
    RTC_HIP(ctx, hipMemcpyAsync(d_edges, h_edges, m * sizeof(rtc_wedge), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(place_entries_kernel, dim3(blocks_for(m, ctx->num_cu)), dim3(256), 0, s, (const rtc_wedge*)d_edges, m, key_in, w_in);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemcpyAsync(d_tot, tot.data(), tot.size() * 8, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemcpyAsync(d_labels, h_labels, (size_t)n_db * 4, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemcpyAsync(d_out, h_out, (size_t)n_queries * sizeof(rtc_leiden_placement), hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    L.db.release(d_edges);
  }
  const uint64_t t0 = now_ns();
  size_t a = 0, b = 0;
  RTC_HIP(ctx, rocprim::radix_sort_pairs(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                         (size_t)m, 0u, 64u, s));
  RTC_HIP(ctx, rocprim::reduce_by_key(nullptr, b, (const uint64_t*)nullptr, (const uint64_t*)nullptr, (size_t)m, (uint64_t*)nullptr,
                                      (uint64_t*)nullptr, (unsigned long long*)nullptr, rocprim::plus<uint64_t>(), rocprim::equal_to<uint64_t>(),
                                      s));
  size_t tmp_bytes = std::max(a, b) + 256, tb = tmp_bytes;
  char* tmp = nullptr;
  RTC_TRY(L.db.get(ctx, tmp_bytes, &tmp));
  RTC_HIP(ctx, rocprim::radix_sort_pairs(tmp, tb, (const uint64_t*)key_in, key_sorted, (const uint64_t*)w_in, w_sorted, (size_t)m, 0u, 64u, s));
  tb = tmp_bytes;
  RTC_HIP(ctx, rocprim::reduce_by_key(tmp, tb, (const uint64_t*)key_sorted, (const uint64_t*)w_sorted, (size_t)m, key, w, d_cnt,
                                      rocprim::plus<uint64_t>(), rocprim::equal_to<uint64_t>(), s));
  unsigned long long E = 0;
  RTC_HIP(ctx, hipMemcpyAsync(&E, d_cnt, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  hipLaunchKernelGGL(louvain_rows_kernel, dim3(blocks_for((uint64_t)n_queries + 1, ctx->num_cu)), dim3(256), 0, s, (const uint64_t*)key, (uint64_t)E,
                     n_queries, L.row_off);
  RTC_CHECK_LAUNCH(ctx);
  RowPaths<lv_shape> P;
  RTC_TRY(P.prepare(ctx, L.db, L.row_off, n_queries, who));
  RTC_TRY(P.launch<place_rule>(ctx, PlaceArgs{L.row_off, key, w, d_tot, d_labels, modularity ? 1 : 0, g, m2, d_out}));
  RTC_HIP(ctx, hipMemcpyAsync(h_out, d_out, (size_t)n_queries * sizeof(rtc_leiden_placement), hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  uint64_t placed = 0, with = 0;
  for (uint32_t q = 0; q < n_queries; q++) { placed += h_out[q].label >= 0; with += h_out[q].n_edges > 0; }
  const uint64_t t1 = now_ns();
  const uint64_t c[10] = {m, E, with, placed, n_queries - placed, P.lists[0].size(), P.lists[1].size(), P.lists[2].size(), t1 - t0, t1 - t_begin};
  std::copy(c, c + 10, ctx->leiden_place);
  ctx->leiden_place_path = P.path_mask();
  return RTC_OK;
}

extern "C" int rtc_leiden_place_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->leiden_place[i];
  return RTC_OK;
}

extern "C" int rtc_leiden_place_last_path(const rtc_ctx* ctx) { return ctx ? ctx->leiden_place_path : 0; }
