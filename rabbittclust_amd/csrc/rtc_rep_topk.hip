// rtc_rep_topk.hip -- clust-mst --db --query / --assign: every query's best representatives (MinHashMstQueryTopK /
// KssdMstQueryTopK, src/mst_state.cpp:1211-1340), DESIGN 3.4b.
//
// The reference probes the representatives' inverted index one query at a time, measures every live representative that
// shares a hash and sorts by distance.  Here a chunk of queries goes through five steps on the device:
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

#include <algorithm>
#include <chrono>
#include <vector>

#include "rtc_internal.h"
#include "rtc_mash_merge.h"
#include "rtc_topk_select.h"

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

struct DevBuf {  // through rtc_dev_alloc / rtc_dev_free: the context's free-memory figure stays current
  rtc_ctx* ctx = nullptr;
  void* p = nullptr;
  ~DevBuf() { if (p) (void)rtc_dev_free(ctx, p); }
  int get(rtc_ctx* c, size_t bytes) {
    ctx = c;
    if (p) { (void)rtc_dev_free(ctx, p); p = nullptr; }
    return rtc_dev_alloc(ctx, std::max<size_t>(bytes, 256), &p);  // RTC_ERR_NOMEM when it does not fit
  }
};

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct TkArgs {
  const void* d_hashes; int width; const uint64_t* d_start; const uint32_t* d_len; uint32_t n, n_reps;
  const uint8_t* d_live; int wmode; uint32_t topk;
};

// queries [q0, q1): rows [R + q0, R + q1) against the columns [0, R).  Appends the kept records (query, rank order) and the
// per-query counts.  RTC_ERR_NOMEM: the join's scratch did not fit.
int rep_topk_chunk(rtc_ctx* ctx, const TkArgs& A, const std::vector<uint32_t>& h_len, uint32_t q0, uint32_t q1,
                   std::vector<rtc_rep_hit>& out, uint32_t* per_query) {
  const uint32_t R = A.n_reps, row0 = R + q0, row1 = R + q1, nq = q1 - q0;
  uint64_t k_cols = 0, k_rows = 0;
  for (uint32_t g = 0; g < R; g++) k_cols += h_len[g];
  for (uint32_t g = row0; g < row1; g++) k_rows += h_len[g];
  if (R == 0 || k_cols == 0 || k_rows == 0) return RTC_OK;  // nothing can share a hash (the join declines such sets)
  hipStream_t s = ctx->stream;
  void* hpin = nullptr;
  double t0 = now_s();
  // ---- 1. candidates (row, slot, common) from the join; the list is grown to the count when it was too short ----
  DevBuf edges, cnt;
  RTC_TRY(cnt.get(ctx, 16));
  uint64_t cap = std::max<uint64_t>(1u << 16, (uint64_t)nq * 64), m = 0;
  for (int attempt = 0; attempt < 3; attempt++) {
    RTC_TRY(edges.get(ctx, cap * sizeof(rtc_cedge)));
    RTC_HIP(ctx, hipMemsetAsync(cnt.p, 0, 16, s));
    int handled = 0;
    RTC_TRY(rtc_pair_edges_join(ctx, A.d_hashes, A.width, A.d_start, A.d_len, A.n, row0, row1, 0, R, -1, (rtc_cedge*)edges.p, cap,
                                (uint64_t*)cnt.p, -1.0, &handled));
    if (!handled) return rtc_fail(ctx, RTC_ERR_NOMEM, "rtc_rep_topk: the join's scratch does not fit %u queries", nq);
    RTC_TRY(rtc_pinned(ctx, 64, &hpin));
    RTC_HIP(ctx, hipMemcpyAsync(hpin, cnt.p, 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    m = *(const uint64_t*)hpin;
    if (m <= cap) break;
    cap = m + m / 8;
    m = 0;
    if (attempt == 2) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "rtc_rep_topk: candidate list kept growing");
  }
  double t1 = now_s();
  ctx->rep_topk[6] += (uint64_t)((t1 - t0) * 1e9);
  if (m == 0) return RTC_OK;
  // ---- 2. count, 3. scan, 4. scatter ----
  DevBuf qcnt, offs, seg;
  RTC_TRY(qcnt.get(ctx, (size_t)nq * 8));                 // counts, then the scatter's cursors
  RTC_TRY(offs.get(ctx, (size_t)(nq + 1) * 16));          // off[nq + 1], koff[nq + 1]
  uint32_t* d_cnt = (uint32_t*)qcnt.p;
  uint32_t* d_cur = d_cnt + nq;
  uint64_t* d_off = (uint64_t*)offs.p;
  uint64_t* d_koff = d_off + nq + 1;
  RTC_HIP(ctx, hipMemsetAsync(qcnt.p, 0, (size_t)nq * 8, s));
  const uint32_t blocks = (uint32_t)((m + 255) / 256);
  hipLaunchKernelGGL(tk_count_kernel, dim3(blocks), dim3(256), 0, s, (const rtc_cedge*)edges.p, m, row0, nq, R, A.d_live, d_cnt);
  RTC_CHECK_LAUNCH(ctx);
  const bool select = A.topk >= 1 && A.topk <= TK_KMAX;
  hipLaunchKernelGGL(tk_scan_kernel, dim3(1), dim3(TK_SCAN_THREADS), 0, s, (const uint32_t*)d_cnt, nq, select ? A.topk : 0u, d_off, d_koff);
  RTC_CHECK_LAUNCH(ctx);
  std::vector<uint32_t> h_cnt(nq);
  uint64_t tot[2] = {0, 0};
  RTC_HIP(ctx, hipMemcpyAsync(h_cnt.data(), d_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(&tot[0], d_off + nq, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(&tot[1], d_koff + nq, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint64_t T = tot[0], M = tot[1];
  ctx->rep_topk[4] += T;
  ctx->rep_topk[5] += (uint64_t)nq * 4 + 16;
  if (T == 0) return RTC_OK;
  RTC_TRY(seg.get(ctx, T * sizeof(TkRec)));
  const int width = A.width;
  if (width == 8)
    hipLaunchKernelGGL(tk_scatter_kernel<uint64_t>, dim3(blocks), dim3(256), 0, s, (const rtc_cedge*)edges.p, m, row0, nq, R, A.d_live,
                       (const uint64_t*)d_off, d_cur, (const uint64_t*)A.d_hashes, A.d_start, A.d_len, A.wmode, (TkRec*)seg.p);
  else
    hipLaunchKernelGGL(tk_scatter_kernel<uint32_t>, dim3(blocks), dim3(256), 0, s, (const rtc_cedge*)edges.p, m, row0, nq, R, A.d_live,
                       (const uint64_t*)d_off, d_cur, (const uint32_t*)A.d_hashes, A.d_start, A.d_len, A.wmode, (TkRec*)seg.p);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipStreamSynchronize(s));
  double t2 = now_s();
  ctx->rep_topk[7] += (uint64_t)((t2 - t1) * 1e9);
  // ---- 5. select ----
  const size_t base = out.size();
  if (select) {
    uint64_t n_short = 0, n_long = 0;
    for (uint32_t q = 0; q < nq; q++) { if (h_cnt[q] > TK_LONG) n_long++; else if (h_cnt[q]) n_short++; }
    DevBuf hits;
    RTC_TRY(hits.get(ctx, M * sizeof(rtc_rep_hit)));
    if (n_short) {
      hipLaunchKernelGGL(tk_select_kernel<64>, dim3(nq), dim3(64), 0, s, (const TkRec*)seg.p, (const uint64_t*)d_off, (const uint64_t*)d_koff,
                         nq, q0, A.topk, 1u, TK_LONG, (rtc_rep_hit*)hits.p);
      RTC_CHECK_LAUNCH(ctx);
    }
    if (n_long) {
      hipLaunchKernelGGL(tk_select_kernel<256>, dim3(nq), dim3(256), 0, s, (const TkRec*)seg.p, (const uint64_t*)d_off, (const uint64_t*)d_koff,
                         nq, q0, A.topk, TK_LONG + 1, 0xffffffffu, (rtc_rep_hit*)hits.p);
      RTC_CHECK_LAUNCH(ctx);
    }
    out.resize(base + M);
    RTC_HIP(ctx, hipMemcpyAsync(out.data() + base, hits.p, M * sizeof(rtc_rep_hit), hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    ctx->rep_topk[1] += n_short;
    ctx->rep_topk[2] += n_long;
    ctx->rep_topk[5] += M * sizeof(rtc_rep_hit);
    for (uint32_t q = 0; q < nq; q++) per_query[q] = std::min(h_cnt[q], A.topk);
  } else {  // the full-segment path: every segment to the host, sorted by the same order
    std::vector<TkRec> h_seg(T);
    RTC_HIP(ctx, hipMemcpyAsync(h_seg.data(), seg.p, T * sizeof(TkRec), hipMemcpyDeviceToHost, s));
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
  ctx->rep_topk[8] += (uint64_t)((now_s() - t2) * 1e9);
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
  DevBuf live;
  if (h_live && n_reps) {
    RTC_TRY(live.get(ctx, n_reps));
    RTC_HIP(ctx, hipMemcpyAsync(live.p, h_live, n_reps, hipMemcpyHostToDevice, ctx->stream));
  }
  TkArgs A{d_hashes, width, d_start, d_len, n, n_reps, (const uint8_t*)live.p, wmode, topk};
  std::vector<rtc_rep_hit> all;
  std::vector<uint32_t> per(n_queries, 0);
  uint32_t chunk = query_chunk ? std::min(query_chunk, n_queries) : n_queries;
  for (uint32_t q0 = 0; q0 < n_queries;) {
    const uint32_t q1 = std::min(n_queries, q0 + chunk);
    const size_t base = all.size();
    const int st = rep_topk_chunk(ctx, A, h_len, q0, q1, all, per.data() + q0);
    if (st == RTC_ERR_NOMEM && q1 - q0 > 1) {  // half the queries: less to sort, fewer candidates
      all.resize(base);
      std::fill(per.begin() + q0, per.begin() + q1, 0u);
      chunk = std::max<uint32_t>(1, (q1 - q0) / 2);
      ctx->err.clear();
      continue;
    }
    if (st != RTC_OK) return st;
    ctx->rep_topk[0]++;
    q0 = q1;
  }
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
