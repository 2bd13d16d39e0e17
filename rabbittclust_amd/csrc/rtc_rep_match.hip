// rtc_rep_match.hip -- clust-mst --append against a --save-rep state: the pairs (query, representative slot) that pass the
// reference's filters (MinHashMstAppendCluster / KssdMstAppendCluster, src/mst_state.cpp:681-1106).
//
// The reference walks the queries one by one: probe the representatives' inverted index, count the hits of every
// representative, filter, measure, then decide.  Only the decision depends on the queries before it (a query that matches
// nothing becomes a representative the later queries are measured against); the counts and the filters do not.  So the
// whole set is measured at once here and the decisions are replayed on the host (append_mst_state, host/rtc_host.cpp):
//   1. join     the representatives [0, R) and the queries [R, R + Q) as one sketch set through the inverted join of
//               rtc_pairs_join.hip (query_candidates, rtc_query_chunks.h): (row, col, common) for every row genome R + q and
//               every col < R + q that share a hash -- old representatives and earlier queries
//   2. count    a lane per candidate applies the reference's filters (size ratio for KSSD, min_common_needed, the distance
//               against the threshold); a wave adds its survivors with one atomic
//   3. emit     the same test again into a list of exactly that size, a place per survivor from the wave's ballot
// The distance is taken again on the host with its libm (the device log may differ by an ulp); the device keeps a pair when
// it is within 1e-12 of the threshold, the host decides.  The queries go in chunks (for_query_chunks), halved where the join's
// scratch does not fit.

#include <cmath>

#include "rtc_query_chunks.h"

namespace {

struct RmParams {
  uint32_t n_reps;
  int kssd, containment;
  double radio, inv_radio, jmin, inv_k, thr_dev;
};

// the reference's filters and distance for the pair (query = row genome i, reference = col genome j)
__device__ __forceinline__ bool rm_keep(uint32_t i, uint32_t j, uint32_t common, const uint32_t* __restrict__ len,
                                        const RmParams& p, double& d) {
  const int sizeQry = (int)len[i], sizeRef = (int)len[j];
  if (sizeRef == 0 || common == 0) return false;  // no hit: the reference never sees the representative
  if (p.kssd) {
    const double ratio = (double)sizeQry / (double)sizeRef;
    if (ratio > p.radio || ratio < p.inv_radio) return false;
  }
  const int minSz = sizeQry < sizeRef ? sizeQry : sizeRef;
  const int min_common_needed = p.containment ? (int)(p.jmin * minSz) : (int)(p.jmin * (sizeQry + sizeRef) / (1.0 + p.jmin));
  if ((int)common < min_common_needed) return false;
  double jac;
  if (p.containment) jac = (double)common / (double)minSz;
  else {
    const int denom = sizeQry + sizeRef - (int)common;
    if (denom <= 0) return false;
    jac = (double)common / (double)denom;
  }
  if (jac >= 1.0) d = 0.0;
  else if (jac <= 0.0) d = 1.0;
  else {
    d = -log(2.0 * jac / (1.0 + jac)) * p.inv_k;
    if (d > 1.0) d = 1.0;
  }
  return d <= p.thr_dev && !isnan(d) && !isinf(d);
}

__global__ __launch_bounds__(256) void rep_match_count_kernel(const rtc_cedge* __restrict__ e, uint64_t m, const uint32_t* __restrict__ len,
                                                              RmParams p, unsigned long long* __restrict__ total) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double d = 0.0;
  const bool keep = a < m && rm_keep(e[a].i, e[a].j, e[a].common, len, p, d);
  const uint64_t mask = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(total, (unsigned long long)__popcll(mask));
}

__global__ __launch_bounds__(256) void rep_match_emit_kernel(const rtc_cedge* __restrict__ e, uint64_t m, const uint32_t* __restrict__ len,
                                                             RmParams p, rtc_rep_pair* __restrict__ out, unsigned long long cap,
                                                             unsigned long long* __restrict__ count) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double d = 0.0;
  rtc_cedge c = {0, 0, 0};
  if (a < m) c = e[a];
  const bool keep = a < m && rm_keep(c.i, c.j, c.common, len, p, d);
  const uint64_t mask = __ballot(keep);
  if (!mask) return;
  unsigned long long base = 0;
  if ((threadIdx.x & 63) == 0) base = atomicAdd(count, (unsigned long long)__popcll(mask));
  base = __shfl(base, 0, 64);
  if (!keep) return;
  const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
  const unsigned long long pos = base + below;
  if (pos < cap) {
    rtc_rep_pair r;
    r.query = c.i - p.n_reps; r.slot = c.j; r.common = c.common; r.pad = 0; r.dist = d;
    out[pos] = r;
  }
}

// the same distance with the host's libm (src/mst_state.cpp:785-802, :1025-1039): the value the replay compares
double host_distance(int sizeQry, int sizeRef, int common, bool containment, double inv_k, bool& ok) {
  double jac;
  ok = true;
  if (containment) jac = (double)common / (double)std::min(sizeQry, sizeRef);
  else {
    const int denom = sizeQry + sizeRef - common;
    if (denom <= 0) { ok = false; return 0.0; }
    jac = (double)common / (double)denom;
  }
  double d;
  if (jac >= 1.0) d = 0.0;
  else if (jac <= 0.0) d = 1.0;
  else { d = -std::log(2.0 * jac / (1.0 + jac)) * inv_k; if (d > 1.0) d = 1.0; }
  return d;
}

// queries [q0, q1): rows [R + q0, R + q1) against the columns [0, R + q1); the pairs that pass are appended to out.
// RTC_ERR_NOMEM: the join's scratch did not fit.
int rep_match_chunk(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                    const std::vector<uint32_t>& h_len, const RmParams& p, uint32_t q0, uint32_t q1, double threshold,
                    std::vector<rtc_rep_pair>& out) {
  const uint32_t row0 = p.n_reps + q0, row1 = p.n_reps + q1;
  uint64_t k_all = 0, k_rows = 0;
  for (uint32_t g = 0; g < row1; g++) { k_all += h_len[g]; if (g >= row0) k_rows += h_len[g]; }
  if (row1 < 2 || k_all < 2 || k_rows == 0) return RTC_OK;  // nothing can share a hash (the join declines such sets)
  hipStream_t s = ctx->stream;
  // ---- 1. candidates (row, col, common) from the join: the earlier queries are columns too, and nothing bounds the list ----
  DevBuf db;
  rtc_cedge* d_edges = nullptr;
  uint64_t m = 0;
  RTC_TRY(query_candidates(ctx, db, "rtc_rep_match", d_hashes, width, d_start, d_len, n, row0, row1, row1, QC_NO_BUDGET, &d_edges, &m));
  if (m == 0) return RTC_OK;
  // ---- 2. count the survivors, 3. emit them into a list of that size ----
  const uint32_t blocks = (uint32_t)((m + 255) / 256);
  unsigned long long* d_cnt = nullptr;  // [0] the survivors counted, [1] emitted
  void* hpin = nullptr;
  RTC_TRY(db.get(ctx, 2, &d_cnt));
  RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 16, s));
  hipLaunchKernelGGL(rep_match_count_kernel, dim3(blocks), dim3(256), 0, s, (const rtc_cedge*)d_edges, m, d_len, p, d_cnt);
  RTC_CHECK_LAUNCH(ctx);
  RTC_TRY(rtc_pinned(ctx, 64, &hpin));
  RTC_HIP(ctx, hipMemcpyAsync(hpin, d_cnt, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint64_t keep = *(const uint64_t*)hpin;
  if (keep == 0) return RTC_OK;
  rtc_rep_pair* d_out = nullptr;
  RTC_TRY(db.get(ctx, keep, &d_out));
  hipLaunchKernelGGL(rep_match_emit_kernel, dim3(blocks), dim3(256), 0, s, (const rtc_cedge*)d_edges, m, d_len, p, d_out,
                     (unsigned long long)keep, d_cnt + 1);
  RTC_CHECK_LAUNCH(ctx);
  std::vector<rtc_rep_pair> h(keep);
  RTC_HIP(ctx, hipMemcpyAsync(h.data(), d_out, keep * sizeof(rtc_rep_pair), hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  for (rtc_rep_pair& r : h) {
    bool ok = true;
    const double d = host_distance((int)h_len[p.n_reps + r.query], (int)h_len[r.slot], (int)r.common, p.containment != 0, p.inv_k, ok);
    if (!ok || !(d <= threshold) || std::isnan(d) || std::isinf(d)) continue;
    r.dist = d;
    out.push_back(r);
  }
  return RTC_OK;
}

}  // namespace

extern "C" int rtc_rep_match(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                             uint32_t n_reps, uint32_t n_queries, int kmer_size, int is_kssd, int is_containment, double threshold,
                             uint32_t query_chunk, rtc_rep_pair* h_pairs, uint64_t cap, uint64_t* n_pairs) {
  if (!ctx) return RTC_ERR_ARG;
  if (!n_pairs || (width != 4 && width != 8) || kmer_size <= 0 || (cap && !h_pairs) || (uint64_t)n_reps + n_queries > 0x7fffffffu)
    return rtc_fail(ctx, RTC_ERR_ARG, "rtc_rep_match: bad arguments");
  *n_pairs = 0;
  const uint32_t n = n_reps + n_queries;
  if (n_queries == 0) return RTC_OK;
  if (!d_hashes || !d_start || !d_len) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_rep_match: no sketches");
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // the constants as the reference forms them (src/mst_state.cpp:696-698, :892-897)
  const double exp_dk = std::exp(-threshold * (double)kmer_size);
  RmParams p;
  p.n_reps = n_reps;
  p.kssd = is_kssd ? 1 : 0;
  p.containment = (!is_kssd && is_containment) ? 1 : 0;
  p.jmin = exp_dk / (2.0 - exp_dk);
  p.radio = std::pow(exp_dk, -1.0);
  p.inv_radio = 1.0 / p.radio;
  p.inv_k = 1.0 / (double)kmer_size;
  p.thr_dev = threshold + std::fabs(threshold) * 1e-12;
  std::vector<rtc_rep_pair> all;
  size_t had = 0;
  RTC_TRY(for_query_chunks(
      ctx, n_queries, query_chunk,
      [&](uint32_t q0, uint32_t q1) {
        had = all.size();
        return rep_match_chunk(ctx, d_hashes, width, d_start, d_len, n, h_len, p, q0, q1, threshold, all);
      },
      [&](uint32_t, uint32_t) { all.resize(had); }, &ctx->diag[7]));
  std::sort(all.begin(), all.end(), [](const rtc_rep_pair& a, const rtc_rep_pair& b) {
    return a.query != b.query ? a.query < b.query : a.slot < b.slot;
  });
  *n_pairs = all.size();
  if (h_pairs && cap) std::copy(all.begin(), all.begin() + std::min<uint64_t>(cap, all.size()), h_pairs);
  return RTC_OK;
}
