// rtc_rep_topk.hip -- clust-mst --db --query / --assign: every query's best representatives (MinHashMstQueryTopK /
// KssdMstQueryTopK, src/mst_state.cpp:1211-1340), DESIGN 3.4b.
//
// The reference probes the representatives' inverted index one query at a time, measures every live representative that
// shares a hash and sorts by distance.  Here a chunk of queries (for_query_chunks, rtc_query_chunks.h) goes through five steps
// on the device, the first three through that header's query_candidates and query_segments:
//   1. join     the representatives [0, R) and the queries [R, R + Q) through the inverted join of rtc_pairs_join.hip with the
//               columns [0, R) only: (row R + q, slot, common) for every pair that shares a hash.  Queries never see each other.
//   2. count    a lane per candidate: retired slots (h_live[s] == 0) are dropped, the rest add one to their query's count
//   3. scan     one workgroup: the exclusive offsets of the candidate segments, and of the kept records (min(count, topk))
//   4. scatter  a lane per candidate: (slot, common, denom) into its query's segment -- denom by the weight mode; in mode 2
//               common and denom are recounted by Mash's union-truncated merge (rtc_mash_merge.h).  The atomic order of the
//               scatter is not fixed; nothing below depends on it.
//   5. select   a workgroup per query keeps a running top-k in LDS: 64 lanes (one wave) for segments of up to 4 096
//               candidates, 256 lanes for the longer ones.  A tile of the segment is tested against the current k-th record,
//               the survivors are compacted into LDS, and every record of (top-k u survivors) finds its new rank by counting
//               the records that rank before it -- the order is total, so the ranks are a permutation.
// The order: larger common / denom first, compared exactly by cross-multiplication in 64 bits; equal keys by slot, lower
// first.  topk == 0 (all) and topk > 256 take the full-segment path instead: steps 1-4 on the device, then every segment is
// read back and sorted on the host by the same order.  Only the kept records cross PCIe on the select path.  The device never
// forms a distance: the caller takes it from (common, denom) with libm.

#include "rtc_mash_merge.h"
#include "rtc_query_chunks.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void tk_scatter_kernel(const rtc_cedge* __restrict__ e, uint64_t m, uint32_t row0, uint32_t nq,
                                                         uint32_t n_reps, const uint8_t* __restrict__ live,
                                                         const uint64_t* __restrict__ off, uint32_t* __restrict__ cursor,
                                                         const T* __restrict__ hashes, const uint64_t* __restrict__ start,
                                                         const uint32_t* __restrict__ len, int wmode, TkRec* __restrict__ out) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const rtc_cedge c = e[a];
  const uint32_t q = c.i - row0;
  if (q >= nq || c.j >= n_reps || (live && !live[c.j])) return;
  const uint32_t sq = len[c.i], sr = len[c.j];
  TkRec r;
  r.slot = c.j; r.pad = 0;
  const int mode = wmode & 3;
  if (mode == 2) {
    rtc_mash_merge(hashes + start[c.i], sq, hashes + start[c.j], sr, (uint32_t)wmode >> 2, &r.common, &r.denom);
  } else {
    r.common = c.common;
    r.denom = mode == 1 ? (sq < sr ? sq : sr) : sq + sr - c.common;
  }
  const uint32_t p = atomicAdd(&cursor[q], 1u);
  if (off[q] + p < off[q + 1]) out[off[q] + p] = r;
}

struct TkArgs {
  const void* d_hashes; int width; const uint64_t* d_start; const uint32_t* d_len; uint32_t n, n_reps;
  const uint8_t* d_live; int wmode; uint32_t topk;
};

// queries [q0, q1): rows [R + q0, R + q1) against the columns [0, R).  Appends the kept records (query, rank order) and the
// per-query counts.  RTC_ERR_NOMEM: the join's scratch did not fit.
int rep_topk_chunk(rtc_ctx* ctx, const TkArgs& A, const std::vector<uint32_t>& h_len, uint32_t q0, uint32_t q1,
                   std::vector<rtc_rep_hit>& out, uint32_t* per_query) {
  const uint32_t R = A.n_reps, row0 = R + q0, row1 = R + q1, nq = q1 - q0;
  if (query_rows_alone(h_len, R, row0, row1)) return RTC_OK;
  hipStream_t s = ctx->stream;
  DevBuf db;
  const uint64_t t0 = now_ns();
  // ---- 1. candidates (row, slot, common) from the join; nothing bounds the list ----
  rtc_cedge* d_edges = nullptr;
  uint64_t m = 0;
  RTC_TRY(query_candidates(ctx, db, "rtc_rep_topk", A.d_hashes, A.width, A.d_start, A.d_len, A.n, row0, row1, R, QC_NO_BUDGET, &d_edges, &m));
  const uint64_t t1 = now_ns();
  ctx->rep_topk[6] += t1 - t0;
  if (m == 0) return RTC_OK;
  // ---- 2. count, 3. scan, 4. scatter ----
  const bool select = A.topk >= 1 && A.topk <= TK_KMAX;
  QuerySegments S;
  RTC_TRY(query_segments(ctx, db, d_edges, m, row0, nq, R, A.d_live, select ? A.topk : 0u, &S));
  const std::vector<uint32_t>& h_cnt = S.h_cnt;
  const uint64_t T = S.T, M = S.M;
  ctx->rep_topk[4] += T;
  ctx->rep_topk[5] += (uint64_t)nq * 4 + (select ? 16 : 8);
  if (T == 0) return RTC_OK;
  TkRec* d_seg = nullptr;
  RTC_TRY(db.get(ctx, T, &d_seg));
  const uint32_t blocks = (uint32_t)((m + 255) / 256);
  if (A.width == 8)
    hipLaunchKernelGGL(tk_scatter_kernel<uint64_t>, dim3(blocks), dim3(256), 0, s, (const rtc_cedge*)d_edges, m, row0, nq, R, A.d_live,
                       (const uint64_t*)S.d_off, S.d_cur, (const uint64_t*)A.d_hashes, A.d_start, A.d_len, A.wmode, d_seg);
  else
    hipLaunchKernelGGL(tk_scatter_kernel<uint32_t>, dim3(blocks), dim3(256), 0, s, (const rtc_cedge*)d_edges, m, row0, nq, R, A.d_live,
                       (const uint64_t*)S.d_off, S.d_cur, (const uint32_t*)A.d_hashes, A.d_start, A.d_len, A.wmode, d_seg);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint64_t t2 = now_ns();
  ctx->rep_topk[7] += t2 - t1;
  // ---- 5. select ----
  const size_t base = out.size();
  if (select) {
    uint64_t n_short = 0, n_long = 0;
    for (uint32_t q = 0; q < nq; q++) { if (h_cnt[q] > TK_LONG) n_long++; else if (h_cnt[q]) n_short++; }
    rtc_rep_hit* d_hits = nullptr;
    RTC_TRY(db.get(ctx, M, &d_hits));
    if (n_short) {
      hipLaunchKernelGGL(tk_select_kernel<64>, dim3(nq), dim3(64), 0, s, (const TkRec*)d_seg, (const uint64_t*)S.d_off, (const uint64_t*)S.d_koff,
                         nq, q0, A.topk, 1u, TK_LONG, d_hits);
      RTC_CHECK_LAUNCH(ctx);
    }
    if (n_long) {
      hipLaunchKernelGGL(tk_select_kernel<256>, dim3(nq), dim3(256), 0, s, (const TkRec*)d_seg, (const uint64_t*)S.d_off, (const uint64_t*)S.d_koff,
                         nq, q0, A.topk, TK_LONG + 1, 0xffffffffu, d_hits);
      RTC_CHECK_LAUNCH(ctx);
    }
    out.resize(base + M);
    RTC_HIP(ctx, hipMemcpyAsync(out.data() + base, d_hits, M * sizeof(rtc_rep_hit), hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    ctx->rep_topk[1] += n_short;
    ctx->rep_topk[2] += n_long;
    ctx->rep_topk[5] += M * sizeof(rtc_rep_hit);
    for (uint32_t q = 0; q < nq; q++) per_query[q] = std::min(h_cnt[q], A.topk);
  } else {  // the full-segment path: every segment to the host, sorted by the same order
    std::vector<TkRec> h_seg(T);
    RTC_HIP(ctx, hipMemcpyAsync(h_seg.data(), d_seg, T * sizeof(TkRec), hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    ctx->rep_topk[5] += T * sizeof(TkRec);
    uint64_t o = 0;
    for (uint32_t q = 0; q < nq; q++) {
      const uint32_t c = h_cnt[q];
      if (!c) continue;
      ctx->rep_topk[3]++;
      TkRec* b = h_seg.data() + o;
      const uint32_t keep = A.topk ? std::min(c, A.topk) : c;
      if (keep < c) std::partial_sort(b, b + keep, b + c, tk_beats_host);
      else std::sort(b, b + c, tk_beats_host);
      for (uint32_t r = 0; r < keep; r++) out.push_back(rtc_rep_hit{q0 + q, b[r].slot, b[r].common, b[r].denom});
      per_query[q] = keep;
      o += c;
    }
  }
  ctx->rep_topk[8] += now_ns() - t2;
  return RTC_OK;
}

}  // namespace

extern "C" int rtc_rep_topk(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                            uint32_t n_reps, uint32_t n_queries, const uint8_t* h_live, int wmode, uint32_t topk,
                            uint32_t query_chunk, rtc_rep_hit* h_hits, uint64_t cap, uint64_t* n_hits, uint32_t* h_per_query) {
  if (!ctx) return RTC_ERR_ARG;
  const int mode = wmode & 3;
  if (!n_hits || (width != 4 && width != 8) || mode == 3 || (mode != 2 && wmode != mode) || (mode == 2 && ((uint32_t)wmode >> 2) == 0) ||
      wmode < 0 || (cap && !h_hits) || (uint64_t)n_reps + n_queries > 0x7fffffffu)
    return rtc_fail(ctx, RTC_ERR_ARG, "rtc_rep_topk: bad arguments");
  *n_hits = 0;
  for (int i = 0; i < 10; i++) ctx->rep_topk[i] = 0;
  ctx->rep_topk_path = 0;
  if (h_per_query) std::fill(h_per_query, h_per_query + n_queries, 0u);
  const uint32_t n = n_reps + n_queries;
  if (n_queries == 0) return RTC_OK;
  if (!d_hashes || !d_start || !d_len) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_rep_topk: no sketches");
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  DevBuf db;
  uint8_t* d_live = nullptr;
  if (h_live && n_reps) {
    RTC_TRY(db.get(ctx, n_reps, &d_live));
    RTC_HIP(ctx, hipMemcpyAsync(d_live, h_live, n_reps, hipMemcpyHostToDevice, ctx->stream));
  }
  TkArgs A{d_hashes, width, d_start, d_len, n, n_reps, d_live, wmode, topk};
  std::vector<rtc_rep_hit> all;
  std::vector<uint32_t> per(n_queries, 0);
  size_t had = 0;
  uint64_t before[10];
  RTC_TRY(for_query_chunks(
      ctx, n_queries, query_chunk,
      [&](uint32_t q0, uint32_t q1) {
        had = all.size();
        std::copy(ctx->rep_topk, ctx->rep_topk + 10, before);
        return rep_topk_chunk(ctx, A, h_len, q0, q1, all, per.data() + q0);
      },
      [&](uint32_t q0, uint32_t q1) {
        all.resize(had);
        std::fill(per.begin() + q0, per.begin() + q1, 0u);
        std::copy(before, before + 10, ctx->rep_topk);
      },
      &ctx->rep_topk[0]));
  ctx->rep_topk_path = (ctx->rep_topk[1] ? 1 : 0) | (ctx->rep_topk[2] ? 2 : 0) | (ctx->rep_topk[3] ? 4 : 0);
  *n_hits = all.size();
  if (h_per_query) std::copy(per.begin(), per.end(), h_per_query);
  if (h_hits && cap) std::copy(all.begin(), all.begin() + std::min<uint64_t>(cap, all.size()), h_hits);
  return RTC_OK;
}

extern "C" int rtc_rep_topk_last_path(const rtc_ctx* ctx) { return ctx ? ctx->rep_topk_path : 0; }

extern "C" int rtc_rep_topk_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->rep_topk[i];
  return RTC_OK;
}
