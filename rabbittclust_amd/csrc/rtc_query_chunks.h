// rtc_query_chunks.h -- what the entry points that place new genomes ("queries") against a finished model share on the host:
// rtc_rep_match, rtc_rep_topk, rtc_dbscan_assign and rtc_graph_query.  The set on the device is the model's rows
// [0, R) followed by the queries' rows, and a chunk of queries [q0, q1) is the rows [R + q0, R + q1):
//   query_candidates  the inverted join of the chunk's rows against the columns [0, col1), into a list that is grown to the
//                     join's count when it was too short
//   query_segments    the candidates bucketed by query: tk_count_kernel, tk_scan_kernel and the sizes read back
//   for_query_chunks  the loop over the chunks, which halves a chunk that came back with RTC_ERR_NOMEM
// What is done with a candidate -- the scatter, and the fold, selection or sort behind it -- stays with each entry point.
// rtc_rep_screen takes for_query_chunks alone: its join keeps the shared hashes, which these candidates have folded away.
#pragma once
#include "rtc_dbscan_common.h"
#include "rtc_topk_select.h"

namespace {

constexpr uint64_t QC_NO_BUDGET = ~0ull;

// Nothing can share a hash (the join declines such sets): no model, or no hash among the columns [0, R) or the rows [row0, row1)
inline bool query_rows_alone(const std::vector<uint32_t>& h_len, uint32_t R, uint32_t row0, uint32_t row1) {
  uint64_t k_cols = 0, k_rows = 0;
  for (uint32_t g = 0; g < R; g++) k_cols += h_len[g];
  for (uint32_t g = row0; g < row1; g++) k_rows += h_len[g];
  return R == 0 || k_cols == 0 || k_rows == 0;
}

// Candidates (row, col, common) of the rows [row0, row1) against the columns [0, col1): *m of them in *d_edges, which db owns.
// The list starts with room for max(65 536, 64 per query) records and is grown to the join's count plus an eighth when that
// was too short, three attempts in all.  budget: the most candidates a chunk may have -- the list never grows past it, and a
// count past it is RTC_ERR_NOMEM, as is a join whose scratch does not fit: the caller halves the chunk.  With QC_NO_BUDGET
// min(budget, x) is x and max(m, min(budget, m + m / 8)) is m + m / 8, and no count is past it.
int query_candidates(rtc_ctx* ctx, DevBuf& db, const char* who, const void* d_hashes, int width, const uint64_t* d_start,
                     const uint32_t* d_len, uint32_t n, uint32_t row0, uint32_t row1, uint32_t col1, uint64_t budget, rtc_cedge** d_edges,
                     uint64_t* m) {
  hipStream_t s = ctx->stream;
  const uint32_t nq = row1 - row0;
  unsigned long long* d_m = nullptr;
  *d_edges = nullptr;
  *m = 0;
  RTC_TRY(db.get(ctx, 2, &d_m));
  uint64_t cap = std::min<uint64_t>(budget, std::max<uint64_t>(1u << 16, (uint64_t)nq * 64));
  for (int attempt = 0; attempt < 3; attempt++) {
    if (*d_edges) db.release(*d_edges);
    RTC_TRY(db.get(ctx, cap, d_edges));
    RTC_HIP(ctx, hipMemsetAsync(d_m, 0, 16, s));
    int handled = 0;
    RTC_TRY(rtc_pair_edges_join(ctx, d_hashes, width, d_start, d_len, n, row0, row1, 0, col1, -1, *d_edges, cap, (uint64_t*)d_m, -1.0, &handled));
    if (!handled) return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: the join's scratch does not fit %u queries", who, nq);
    void* hpin = nullptr;  // (asked for behind the join, which stages through the same block and may have moved it)
    RTC_TRY(rtc_pinned(ctx, 64, &hpin));
    RTC_HIP(ctx, hipMemcpyAsync(hpin, d_m, 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    const uint64_t count = *(const uint64_t*)hpin;
    if (count <= cap) {
      *m = count;
      return RTC_OK;
    }
    if (count > budget)
      return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: %llu candidates of %u queries, edge budget %llu", who, (unsigned long long)count, nq,
                      (unsigned long long)budget);
    cap = std::max<uint64_t>(count, std::min<uint64_t>(budget, count + count / 8));
  }
  return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: candidate list kept growing", who);
}

// The candidates bucketed by query: the segment of query q is [d_off[q], d_off[q + 1]) of a list of T records, h_cnt[q] long.
struct QuerySegments {
  uint32_t* d_cur = nullptr;                     // a cursor per query for the scatter, zeroed
  uint64_t *d_off = nullptr, *d_koff = nullptr;  // off[nq + 1]; koff[nq + 1]: the same over min(count, k)
  std::vector<uint32_t> h_cnt;
  uint64_t T = 0, M = 0;  // off[nq], koff[nq]
};

// live: the columns that count (NULL: all of [0, R)).  k: tk_scan_kernel's (0: koff is off, and M is T without a read-back).
int query_segments(rtc_ctx* ctx, DevBuf& db, const rtc_cedge* d_edges, uint64_t m, uint32_t row0, uint32_t nq, uint32_t R, const uint8_t* d_live,
                   uint32_t k, QuerySegments* S) {
  hipStream_t s = ctx->stream;
  uint32_t* d_cnt = nullptr;  // counts, then the scatter's cursors
  RTC_TRY(db.get(ctx, (size_t)nq * 2, &d_cnt));
  RTC_TRY(db.get(ctx, (size_t)(nq + 1) * 2, &S->d_off));
  S->d_cur = d_cnt + nq;
  S->d_koff = S->d_off + nq + 1;
  RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, (size_t)nq * 8, s));
  hipLaunchKernelGGL(tk_count_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, s, d_edges, m, row0, nq, R, d_live, d_cnt);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(tk_scan_kernel, dim3(1), dim3(TK_SCAN_THREADS), 0, s, (const uint32_t*)d_cnt, nq, k, S->d_off, S->d_koff);
  RTC_CHECK_LAUNCH(ctx);
  S->h_cnt.resize(nq);
  RTC_HIP(ctx, hipMemcpyAsync(S->h_cnt.data(), d_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(&S->T, S->d_off + nq, 8, hipMemcpyDeviceToHost, s));
  if (k) RTC_HIP(ctx, hipMemcpyAsync(&S->M, S->d_koff + nq, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  if (!k) S->M = S->T;
  return RTC_OK;
}

// run(q0, q1) for chunks of query_chunk queries (0: all at once).  A chunk of more than one query that comes back with
// RTC_ERR_NOMEM -- the join's scratch or a list did not fit, or the candidates are past the budget -- is undone (undo(q0, q1):
// the chunk's outputs and statistics as they were before run) and run again in halves; the error that is cleared is a failed
// hipMalloc's, in the context and in the runtime.  *chunks counts the chunks that ran to the end.
template <class Run, class Undo>
int for_query_chunks(rtc_ctx* ctx, uint32_t n_queries, uint32_t query_chunk, Run&& run, Undo&& undo, uint64_t* chunks) {
  uint32_t chunk = query_chunk ? std::min(query_chunk, n_queries) : n_queries;
  for (uint32_t q0 = 0; q0 < n_queries;) {
    const uint32_t q1 = std::min(n_queries, q0 + chunk);
    const int st = run(q0, q1);
    if (st == RTC_ERR_NOMEM && q1 - q0 > 1) {  // half the queries: fewer candidates, a smaller join
      undo(q0, q1);
      chunk = std::max<uint32_t>(1, (q1 - q0) / 2);
      ctx->err.clear();
      (void)hipGetLastError();
      continue;
    }
    if (st != RTC_OK) return st;
    (*chunks)++;
    q0 = q1;
  }
  return RTC_OK;
}

}  // namespace
