// rtc_dbscan_assign.hip -- clust-dbscan --db --assign: new points placed into a clustered sketch set by DBSCAN's border rule
// (include/rtclust.h defines the rule).  The set on the device is the model's rows [0, n_db) followed by the
// queries' rows, the layout of rtc_rep_topk.  A chunk of queries (for_query_chunks, rtc_query_chunks.h) goes through four steps
// on the device:
//   1. join     query_candidates: rtc_pair_edges_join with the columns [0, n_db) only, (n_db + q, p, common) for every pair that
//               shares a hash.  Queries never see each other.
//   2. bucket   query_segments (count, scan), then the scatter: a record (p, common, denom, in N(q)) per candidate into
//               its query's segment.  The scatter evaluates the model's predicate -- KSSD: eps_level_mask at one level, the
//               predicate block of rtc_dbscan's filter; MinHash: the wave-cooperative truncated merge (mash_merge_wave) and one
//               level's cmin table, without a prefilter because `nearest` needs every candidate's counts.  The atomic order of
//               the scatter is not fixed; nothing below depends on it.
//   3. fold     a workgroup per query -- one wave for segments of up to AS_WAVE_TILE records, 256 lanes for the longer ones --
//               strides over the segment; every lane keeps the neighbour count, the core count, min / max label over the core
//               neighbours and its best record under rtc_rep_topk's exact order, and cross-lane shuffles (then four partials in
//               LDS) reduce them: tk_fold_segment (rtc_topk_select.h) over AsFold.  No atomics on a query's record: a query
//               inside a family of 1 000 would serialise them.  min / max / sum are order-free and the order of the records
//               is total, so the result is the same for every scatter order.
//   4. read     the chunk's fixed-size records.
// A chunk whose candidates exceed the edge budget or whose join scratch does not fit is halved; RTC_ERR_NOMEM past one query.
#include "rtc_dbscan_mash.h"
#include "rtc_query_chunks.h"

namespace {

constexpr uint32_t AS_WAVE_TILE = 4096;  // segments longer than this take the 256-lane workgroup
constexpr uint32_t AS_NONE = 0xffffffffu;

// cnt[1..3]: eps_level_mask's.  TkRec.pad bit 0: the candidate is in N(q).
__global__ __launch_bounds__(256) void as_kssd_scatter_kernel(const rtc_cedge* __restrict__ e, uint64_t m, uint32_t row0, uint32_t nq,
                                                              uint32_t n_db, const uint32_t* __restrict__ len, EpsLevels lv, uint32_t sat,
                                                              const uint64_t* __restrict__ off, uint32_t* __restrict__ cursor,
                                                              TkRec* __restrict__ out, unsigned long long* __restrict__ cnt) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const rtc_cedge c = e[a];
  const uint32_t q = c.i - row0;
  if (q >= nq || c.j >= n_db) return;
  uint32_t common;
  const uint32_t mask = eps_level_mask(c, len, lv, 1, sat, &common, cnt);
  TkRec r;
  r.slot = c.j; r.common = common; r.denom = len[c.i] + len[c.j] - common; r.pad = mask & 1u;
  const uint32_t p = atomicAdd(&cursor[q], 1u);
  if (off[q] + p < off[q + 1]) out[off[q] + p] = r;
}

// One wave per block, 64 candidates per wave and round, as mash_edges_kernel: the wave merges one candidate at a time, lane k
// then holds candidate k's truncated counts and the epilogue is lane-parallel.  cnt[0]: candidates merged.
template <typename T>
__global__ __launch_bounds__(64) void as_mash_scatter_kernel(const T* __restrict__ hashes, const uint64_t* __restrict__ start,
                                                             const uint32_t* __restrict__ len, uint32_t sketch_size,
                                                             const rtc_cedge* __restrict__ cand, uint64_t m, uint32_t row0, uint32_t nq,
                                                             uint32_t n_db, const uint32_t* __restrict__ cmin, uint32_t D,
                                                             const uint64_t* __restrict__ off, uint32_t* __restrict__ cursor,
                                                             TkRec* __restrict__ out, unsigned long long* __restrict__ cnt) {
  __shared__ T sb[MASH_LDS_ELEMS];
  const uint32_t lane = threadIdx.x;
  for (uint64_t base = (uint64_t)blockIdx.x * 64; base < m; base += (uint64_t)gridDim.x * 64) {  // uniform
    const uint64_t e = base + lane;
    rtc_cedge c{0, 0, 0};
    uint32_t na = 0, nb = 0, q = 0;
    bool merge = false;
    if (e < m) {
      c = cand[e];
      q = c.i - row0;
      merge = q < nq && c.j < n_db;
      if (merge) { na = len[c.i]; nb = len[c.j]; }
    }
    uint32_t common = 0, denom = 0;
    const uint64_t todo = __ballot(merge);
    for (uint64_t t = todo; t; t &= t - 1) {  // uniform
      const uint32_t k = (uint32_t)__builtin_ctzll(t);
      const uint32_t ki = __shfl(c.i, k), kj = __shfl(c.j, k);
      uint32_t kc, kd;
      mash_merge_wave(hashes + start[ki], __shfl(na, k), hashes + start[kj], __shfl(nb, k), sketch_size, sb, lane, &kc, &kd);
      if (lane == k) { common = kc; denom = kd; }
    }
    if (lane == 0 && todo) atomicAdd(&cnt[0], (unsigned long long)__popcll(todo));
    if (merge) {
      const uint32_t d = denom < D ? denom : D;  // denom <= D by construction
      TkRec r;
      r.slot = c.j; r.common = common; r.denom = denom; r.pad = common >= cmin[d] ? 1u : 0u;
      const uint32_t p = atomicAdd(&cursor[q], 1u);
      if (off[q] + p < off[q + 1]) out[off[q] + p] = r;
    }
  }
}

// What a lane, a wave and then the workgroup hold of a query's segment (tk_fold_segment's F)
struct AsFold {
  uint32_t nn, nc;     // |N(q)|, the core points among them
  int32_t lmin, lmax;  // over the core points of N(q)
  TkRec best;          // over every candidate
  __device__ __forceinline__ void take(const TkRec& x, const int32_t* __restrict__ labels, const uint8_t* __restrict__ core) {
    if (x.pad & 1u) {
      nn++;
      if (core[x.slot]) {
        const int32_t l = labels[x.slot];
        nc++;
        lmin = l < lmin ? l : lmin;
        lmax = l > lmax ? l : lmax;
      }
    }
    if (tk_beats(x, best)) best = x;
  }
  __device__ __forceinline__ void merge(const AsFold& b) {
    nn += b.nn; nc += b.nc;
    lmin = b.lmin < lmin ? b.lmin : lmin;
    lmax = b.lmax > lmax ? b.lmax : lmax;
    if (tk_beats(b.best, best)) best = b.best;
  }
};

// a workgroup of B lanes per query whose segment length lies in [lo, hi].  need: q would be a core point with that many neighbours.
template <int B>
__global__ __launch_bounds__(B) void as_fold_kernel(const TkRec* __restrict__ seg, const uint64_t* __restrict__ off, uint32_t nq,
                                                    uint32_t lo, uint32_t hi, const int32_t* __restrict__ labels,
                                                    const uint8_t* __restrict__ core, long long need, rtc_dbscan_place* __restrict__ out) {
  __shared__ AsFold part[B > 64 ? B / 64 : 1];  // the waves' partials of the 256-lane workgroup (one unused slot at B = 64)
  const uint32_t q = blockIdx.x;
  if (q >= nq) return;
  const uint64_t s0 = off[q], s1 = off[q + 1];
  if (s1 - s0 < lo || s1 - s0 > hi) return;  // uniform across the workgroup
  // no candidate: denom 1 keeps the key 0 / 1 below every real record's.  A MinHash candidate whose truncated common is 0 has
  // that key too and must still win: equal keys go to the lower index, and every real slot is below AS_NONE because
  // rtc_dbscan_assign refuses n_db + n_queries >= 2^31 - 1.
  const AsFold f = tk_fold_segment<B>(seg, s0, s1, AsFold{0, 0, 0x7fffffff, -1, TkRec{AS_NONE, 0, 1, 0}}, part, labels, core);
  if (threadIdx.x == 0) {
    rtc_dbscan_place r;
    const bool none = f.best.slot == AS_NONE;
    r.label = f.nc ? f.lmin : -1;
    r.label_max = f.nc ? f.lmax : -1;
    r.n_neighbours = f.nn; r.n_core = f.nc;
    r.nearest = f.best.slot; r.common = none ? 0u : f.best.common; r.denom = none ? 0u : f.best.denom;
    r.flags = (long long)f.nn >= need ? 1u : 0u;
    out[q] = r;
  }
}

struct AsArgs {
  const void* d_hashes; int width; const uint64_t* d_start; const uint32_t* d_len; uint32_t n, n_db;
  const int32_t* d_labels; const uint8_t* d_core;
  bool minhash; uint32_t sketch_size; EpsLevels lv; uint32_t sat; const uint32_t* d_cmin; uint32_t D;
  long long need; uint64_t budget;
  unsigned long long* d_fc;  // [0] merged, [1..3] eps_level_mask's
};
struct AsStats { uint64_t candidates = 0, merged = 0, asym = 0, first_asym = ~0ull, join_ns = 0, bucket_ns = 0, fold_ns = 0, n_wave = 0, n_wg = 0; };

// queries [q0, q1): rows [n_db + q0, n_db + q1) against the columns [0, n_db); h_out[0 .. q1 - q0) holds the defaults and keeps
// them where nothing can share a hash.  RTC_ERR_NOMEM: the candidates are past the budget or the join's scratch did not fit.
int assign_chunk(rtc_ctx* ctx, const AsArgs& A, const std::vector<uint32_t>& h_len, uint32_t q0, uint32_t q1, rtc_dbscan_place* h_out,
                 AsStats* st) {
  const uint32_t R = A.n_db, row0 = R + q0, row1 = R + q1, nq = q1 - q0;
  if (query_rows_alone(h_len, R, row0, row1)) return RTC_OK;
  hipStream_t s = ctx->stream;
  DevBuf db;
  const uint64_t t0 = now_ns();
  // ---- 1. candidates (row, p, common) from the join ----
  rtc_cedge* d_edges = nullptr;
  uint64_t m = 0;
  RTC_TRY(query_candidates(ctx, db, "rtc_dbscan_assign", A.d_hashes, A.width, A.d_start, A.d_len, A.n, row0, row1, R, A.budget, &d_edges, &m));
  const uint64_t t1 = now_ns();
  st->join_ns += t1 - t0;
  if (m == 0) return RTC_OK;
  // ---- 2. count, scan, predicate + scatter ----
  QuerySegments S;
  RTC_TRY(query_segments(ctx, db, d_edges, m, row0, nq, R, nullptr, 0u, &S));
  st->candidates += S.T;
  if (S.T == 0) return RTC_OK;
  TkRec* d_seg = nullptr;
  RTC_TRY(db.get(ctx, S.T, &d_seg));
  unsigned long long fc[4] = {0ull, 0ull, ~0ull, 0ull};
  RTC_HIP(ctx, hipMemcpyAsync(A.d_fc, fc, sizeof fc, hipMemcpyHostToDevice, s));
  if (A.minhash) {
    const dim3 g(mash_blocks(m, ctx->num_cu)), b(64);
    if (A.width == 8)
      hipLaunchKernelGGL(as_mash_scatter_kernel<uint64_t>, g, b, 0, s, (const uint64_t*)A.d_hashes, A.d_start, A.d_len, A.sketch_size,
                         (const rtc_cedge*)d_edges, m, row0, nq, R, A.d_cmin, A.D, (const uint64_t*)S.d_off, S.d_cur, d_seg, A.d_fc);
    else
      hipLaunchKernelGGL(as_mash_scatter_kernel<uint32_t>, g, b, 0, s, (const uint32_t*)A.d_hashes, A.d_start, A.d_len, A.sketch_size,
                         (const rtc_cedge*)d_edges, m, row0, nq, R, A.d_cmin, A.D, (const uint64_t*)S.d_off, S.d_cur, d_seg, A.d_fc);
  } else {
    hipLaunchKernelGGL(as_kssd_scatter_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, s, (const rtc_cedge*)d_edges, m, row0, nq, R, A.d_len, A.lv, A.sat,
                       (const uint64_t*)S.d_off, S.d_cur, d_seg, A.d_fc);
  }
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipMemcpyAsync(fc, A.d_fc, sizeof fc, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  db.release(d_edges);
  st->merged += fc[0];
  st->asym += fc[1];
  st->first_asym = std::min<uint64_t>(st->first_asym, fc[2]);
  const uint64_t t2 = now_ns();
  st->bucket_ns += t2 - t1;
  // ---- 3. fold, 4. the records ----
  uint64_t n_long = 0, n_short = 0;
  for (uint32_t q = 0; q < nq; q++) { n_long += S.h_cnt[q] > AS_WAVE_TILE; n_short += S.h_cnt[q] && S.h_cnt[q] <= AS_WAVE_TILE; }
  rtc_dbscan_place* d_out = nullptr;
  RTC_TRY(db.get(ctx, nq, &d_out));
  if (n_long < nq) {
    hipLaunchKernelGGL(as_fold_kernel<64>, dim3(nq), dim3(64), 0, s, (const TkRec*)d_seg, (const uint64_t*)S.d_off, nq, 0u, AS_WAVE_TILE, A.d_labels,
                       A.d_core, A.need, d_out);
    RTC_CHECK_LAUNCH(ctx);
  }
  if (n_long) {
    hipLaunchKernelGGL(as_fold_kernel<256>, dim3(nq), dim3(256), 0, s, (const TkRec*)d_seg, (const uint64_t*)S.d_off, nq, AS_WAVE_TILE + 1, 0xffffffffu,
                       A.d_labels, A.d_core, A.need, d_out);
    RTC_CHECK_LAUNCH(ctx);
  }
  RTC_HIP(ctx, hipMemcpyAsync(h_out, d_out, (size_t)nq * sizeof(rtc_dbscan_place), hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  st->n_wave += n_short;
  st->n_wg += n_long;
  st->fold_ns += now_ns() - t2;
  return RTC_OK;
}

}  // namespace

extern "C" int rtc_dbscan_assign(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                                 uint32_t n_db, uint32_t n_queries, const int32_t* h_labels, const uint8_t* h_core, int is_minhash,
                                 uint32_t sketch_size, double eps, int min_pts, int kmer_size, uint32_t query_chunk,
                                 rtc_dbscan_place* h_out) {
  const char* who = "rtc_dbscan_assign";
  if (!ctx) return RTC_ERR_ARG;
  if (width != 4 && width != 8) return rtc_fail(ctx, RTC_ERR_ARG, "%s: width must be 4 or 8", who);
  if (n_queries && !h_out) return rtc_fail(ctx, RTC_ERR_ARG, "%s: no room for the records", who);
  if (n_db && !h_labels) return rtc_fail(ctx, RTC_ERR_ARG, "%s: the model's labels (h_labels) are missing", who);
  if (n_db && !h_core) return rtc_fail(ctx, RTC_ERR_ARG, "%s: the model's core flags (h_core) are missing", who);
  if ((uint64_t)n_db + n_queries >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u + %u points", who, n_db, n_queries);
  const uint32_t n = n_db + n_queries;
  if (n && (!d_hashes || !d_start || !d_len)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: no sketches", who);
  AsArgs A;
  memset(&A.lv, 0, sizeof A.lv);
  if (is_minhash) {  // rtc_dbscan_mash's checks
    if (sketch_size == 0 || sketch_size >= (1u << 28)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: sketch size %u", who, sketch_size);
    if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: k-mer size %d", who, kmer_size);
    if (!(eps >= 0.0)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: eps %g is not in [0, 1)", who, eps);
    if (eps >= 1.0) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: eps %g: from 1 on, pairs without a common hash are neighbours", who, eps);
  } else if (!eps_to_t(eps, kmer_size, &A.lv.t[0], &A.lv.one_plus_t[0])) {  // rtc_dbscan's
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: eps %g with k %d gives jaccard_min %g <= 1e-12", who, eps, kmer_size, A.lv.t[0]);
  }
  for (int i = 0; i < 10; i++) ctx->dbscan_assign[i] = 0;
  ctx->dbscan_assign_path = 0;
  if (n_queries == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  uint32_t max_len = 0;
  for (uint32_t g = 0; g < n; g++) max_len = std::max(max_len, h_len[g]);
  if (width == 4 && !is_minhash && !u32_size_bound_fits(max_len, A.lv.t[0]))
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: size bound ceil(%u / %g) past INT_MAX", who, max_len, A.lv.t[0]);
  if (max_len > 0x7fffffffu)  // denom = |p| + |q| - common in 32 bits, the order's products below 2^63
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: a sketch of %u hashes, the order of `nearest` is exact up to %u", who, max_len, 0x7fffffffu);
  A.d_hashes = d_hashes; A.width = width; A.d_start = d_start; A.d_len = d_len; A.n = n; A.n_db = n_db;
  A.minhash = is_minhash != 0; A.sketch_size = sketch_size;
  A.sat = width == 4 ? 65535u : 0xffffffffu;
  A.d_cmin = nullptr; A.D = 0;
  // q would be a core point with `need` neighbours: KssdDBSCAN counts the point itself, MinHashDBSCAN the neighbours alone
  A.need = is_minhash ? (long long)std::max(min_pts, 0) : (long long)min_pts - 1;
  A.budget = ctx->opt.edge_budget ? ctx->opt.edge_budget : (uint64_t)256 << 20;
  A.budget = std::max<uint64_t>(A.budget, (uint64_t)n_db + 1024);  // one query's candidates always fit
  const rtc_dbscan_place none{-1, -1, 0, 0, AS_NONE, 0, 0, 0 >= A.need ? 1u : 0u};
  std::fill(h_out, h_out + n_queries, none);
  DevBuf db;
  int32_t* d_labels = nullptr;
  uint8_t* d_core = nullptr;
  RTC_TRY(db.get(ctx, std::max<uint32_t>(n_db, 1), &d_labels));
  RTC_TRY(db.get(ctx, std::max<uint32_t>(n_db, 1), &d_core));
  RTC_TRY(db.get(ctx, 4, &A.d_fc));
  if (n_db) {
    RTC_HIP(ctx, hipMemcpyAsync(d_labels, h_labels, (size_t)n_db * 4, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemcpyAsync(d_core, h_core, n_db, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
  }
  A.d_labels = d_labels; A.d_core = d_core;
  MashTables mt;
  if (is_minhash) {
    RTC_TRY(mash_tables(ctx, db, sketch_size, max_len, kmer_size, &eps, 1, &mt));
    A.d_cmin = mt.d_cmin; A.D = mt.D;
  }
  AsStats st;
  AsStats before;
  uint64_t chunks = 0;
  RTC_TRY(for_query_chunks(
      ctx, n_queries, query_chunk,
      [&](uint32_t q0, uint32_t q1) {
        before = st;
        return assign_chunk(ctx, A, h_len, q0, q1, h_out + q0, &st);
      },
      [&](uint32_t q0, uint32_t q1) {
        st = before;
        std::fill(h_out + q0, h_out + q1, none);
      },
      &chunks));
  if (st.asym)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: %llu pairs whose eps test depends on the orientation, e.g. (query %u, model point %u)", who,
                    (unsigned long long)st.asym, (uint32_t)(st.first_asym >> 32) - n_db, (uint32_t)st.first_asym);
  // The u64 brute force has no emptiness test (rtc_dbscan_sweep.hip): an empty query is the neighbour of every empty model
  // sketch and of nothing else.  It shares no hash with anything, so the device left its record at the default.
  if (width == 8 && !is_minhash) {
    rtc_dbscan_place e = none;
    for (uint32_t p = 0; p < n_db; p++) {
      if (h_len[p]) continue;
      e.n_neighbours++;
      if (!h_core[p]) continue;
      e.label = e.n_core ? std::min(e.label, h_labels[p]) : h_labels[p];
      e.label_max = e.n_core ? std::max(e.label_max, h_labels[p]) : h_labels[p];
      e.n_core++;
    }
    e.flags = (long long)e.n_neighbours >= A.need ? 1u : 0u;
    for (uint32_t q = 0; q < n_queries; q++)
      if (!h_len[n_db + q]) h_out[q] = e;
  }
  uint64_t neighbours = 0, placed = 0, bridging = 0;
  for (uint32_t q = 0; q < n_queries; q++) {
    neighbours += h_out[q].n_neighbours;
    placed += h_out[q].label >= 0;
    bridging += h_out[q].label != h_out[q].label_max;
  }
  // (the candidates merged are all of them for a MinHash model and none for a KSSD one: no slot)
  const uint64_t c[10] = {chunks, st.candidates, neighbours, placed, n_queries - placed, bridging, st.join_ns, st.bucket_ns, st.fold_ns,
                          now_ns() - t_begin};
  std::copy(c, c + 10, ctx->dbscan_assign);
  ctx->dbscan_assign_path = (st.n_wave ? 1 : 0) | (st.n_wg ? 2 : 0);
  return RTC_OK;
}

extern "C" int rtc_dbscan_assign_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->dbscan_assign[i];
  return RTC_OK;
}

extern "C" int rtc_dbscan_assign_last_path(const rtc_ctx* ctx) { return ctx ? ctx->dbscan_assign_path : 0; }
