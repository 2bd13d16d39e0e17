// rtc_postprocess.hip -- the tree medoid of clust-mst --dedup-dist (build_dedup_candidates_per_cluster_core,
// src/cluster_postprocess.cpp:60-156) on the GPU.
//
// The reference runs one traversal over all N vertices per member of every dedup group: O(N * group size), 10^9-10^10 steps
// on sets of 10^5 genomes with large near-identical families.  Here the host builds the groups and a CSR of each
// (rtc_tree_medoid.h), small groups are done on the host threads (O(g^2) per group) and the large ones here: one wave per
// candidate c, a level-synchronous traversal from c over its group (the parent of a vertex is the neighbour it was reached
// from), dist(c, .) in a scratch row of the wave, then the serial left-to-right sum over the members in ascending id.  Both
// the per-edge adds and the sum are single rounded fp64 adds in the reference's order (__dadd_rn; the build also passes
// -ffp-contract=off), so the totals carry the reference's bits and the host's choice among them its ties.
#include <algorithm>

#include "rtc_internal.h"
#include "rtc_tree_medoid.h"

namespace {

// Groups of at least this many members go to the GPU under RTC_DEDUP_GPU=1.  tools/run_dedup.py on MI355X against 16 host
// threads (ms host / GPU): random trees 1.03 / 0.71 at 2 048, 3.07 / 1.74 at 4 096, 16.9 / 11.9 at 10 000; chains 1.64 / 2.72,
// 6.51 / 6.75, 42.6 / 44.1; stars 0.86 / 1.17, 2.09 / 2.65, 11.2 / 15.2.  From 4 096 on the GPU is ahead on random trees and
// about even over the three shapes (geometric mean 1.10x at 4 096, 1.01x at 10 000; 0.86x at 2 048).  The kernel is bound by
// the latency of its scratch rows (one lane walks a high-degree vertex's list alone, a chain is one vertex per level).
constexpr uint32_t kDedupGpuMinGroup = 4096;
// scratch of the candidates in flight: dist (8 B) + parent (4 B) + queue (4 B) per member of the candidate's group
constexpr uint64_t kScratchPerMember = 16;
constexpr uint64_t kScratchBudget = 1ull << 30;

struct TmCand {
  uint64_t base;  // the group's first member in the CSR row table
  uint64_t soff;  // the wave's scratch row, in doubles from the chunk's scratch
  uint32_t g, c;  // group size, candidate (position in the group)
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(256) void tree_medoid_totals_kernel(const TmCand* __restrict__ cand, uint32_t ncand,
                                                                 const uint64_t* __restrict__ aoff, const uint32_t* __restrict__ anbr,
                                                                 const double* __restrict__ aw, double* __restrict__ scratch,
                                                                 double* __restrict__ tot) {
  __shared__ uint32_t tail_s[4];
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t w = blockIdx.x * 4 + wv;
  if (w >= ncand) return;  // the whole wave: no workgroup barrier below
  const TmCand cd = cand[w];
  const uint32_t g = cd.g, c = cd.c;
  double* dist = scratch + cd.soff;
  uint32_t* parent = reinterpret_cast<uint32_t*>(dist + g);
  uint32_t* queue = parent + g;
  const uint64_t* off = aoff + cd.base;
  for (uint32_t j = lane; j < g; j += 64) dist[j] = -1.0;  // never reached: skipped by the sum, as the reference's -1
  wave_sync();
  if (lane == 0) { dist[c] = 0.0; parent[c] = c; queue[0] = c; tail_s[wv] = 1; }
  wave_sync();
  uint32_t head = 0, tail = 1;
  while (head < tail) {  // one level per pass: queue[head, tail) is the frontier
    for (uint32_t i = head + lane; i < tail; i += 64) {
      const uint32_t u = queue[i];
      const double du = dist[u];
      const uint32_t pu = parent[u];
      for (uint64_t e = off[u], e1 = off[u + 1]; e < e1; e++) {
        const uint32_t v = anbr[e];
        if (v == pu) continue;
        const uint32_t pos = atomicAdd(&tail_s[wv], 1u);
        if (pos >= g || v >= g) continue;  // only a cycle could get here (the host refuses those): keeps the writes in the row
        dist[v] = __dadd_rn(du, aw[e]);
        parent[v] = u;
        queue[pos] = v;
      }
    }
    wave_sync();
    head = tail;
    tail = min(tail_s[wv], g);
  }
  // total(c): members in ascending id, c skipped, dist >= 0 only, one rounded add after the other.  The wave reads 64
  // values at a time and every lane runs the same serial chain over them.
  double t = 0.0;
  for (uint32_t j0 = 0; j0 < g; j0 += 64) {
    const uint32_t j = j0 + lane;
    const double x = j < g ? dist[j] : -1.0;
    const uint32_t cnt = min(64u, g - j0);
    for (uint32_t k = 0; k < cnt; k++) {
      const double y = __shfl(x, (int)k, 64);
      if (j0 + k != c && y >= 0.0) t = __dadd_rn(t, y);
    }
  }
  if (lane == 0) tot[w] = t;
}

template <class T>
int upload(rtc_ctx* ctx, const std::vector<T>& h, T** d, std::vector<void*>& owned) {
  *d = nullptr;
  const size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
  RTC_HIP(ctx, hipMalloc(reinterpret_cast<void**>(d), bytes));
  owned.push_back(*d);
  if (!h.empty()) RTC_HIP(ctx, hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  return RTC_OK;
}

// totals of every member of the groups in `which`, written to tot (one per member, mem order); enqueued on the context stream,
// *d_tot: the device totals (cands order), read back after rtc_tree_medoids' host work
int totals_gpu(rtc_ctx* ctx, const rtc_tm::Groups& G, const std::vector<uint32_t>& which, std::vector<void*>& owned,
               std::vector<TmCand>& cands, double** d_tot) {
  cands.clear();
  uint64_t max_row = 0;
  for (uint32_t g : which) {
    const uint32_t sz = G.size(g);
    max_row = std::max<uint64_t>(max_row, sz * kScratchPerMember);
    for (uint32_t c = 0; c < sz; c++) cands.push_back({G.goff[g], 0, sz, c});
  }
  ctx->free_hbm_at = -1.0;
  const uint64_t budget = std::max<uint64_t>(std::min<uint64_t>(kScratchBudget, rtc_free_hbm(ctx) / 4), max_row);
  uint64_t *d_aoff; uint32_t* d_anbr; double* d_aw; TmCand* d_cand;
  // chunks of consecutive candidates whose scratch rows fit the budget (rows 16-byte aligned: sizes padded to even)
  std::vector<uint32_t> chunk_at{0};
  uint64_t used = 0;
  for (size_t i = 0; i < cands.size(); i++) {
    const uint64_t row = ((cands[i].g + 1ull) & ~1ull) * (kScratchPerMember / 8);  // in doubles
    if (used + row * 8 > budget && i > chunk_at.back()) { chunk_at.push_back((uint32_t)i); used = 0; }
    cands[i].soff = used / 8;
    used += row * 8;
  }
  chunk_at.push_back((uint32_t)cands.size());
  uint64_t scratch_bytes = 0;
  for (size_t k = 0; k + 1 < chunk_at.size(); k++) {
    const TmCand& last = cands[chunk_at[k + 1] - 1];
    scratch_bytes = std::max<uint64_t>(scratch_bytes, (last.soff + ((last.g + 1ull) & ~1ull) * 2) * 8);
  }
  RTC_TRY(upload(ctx, G.aoff, &d_aoff, owned));
  RTC_TRY(upload(ctx, G.anbr, &d_anbr, owned));
  RTC_TRY(upload(ctx, G.aw, &d_aw, owned));
  RTC_TRY(upload(ctx, cands, &d_cand, owned));
  double* d_scratch = nullptr;
  RTC_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&d_scratch), std::max<uint64_t>(scratch_bytes, 16)));
  owned.push_back(d_scratch);
  RTC_HIP(ctx, hipMalloc(reinterpret_cast<void**>(d_tot), std::max<size_t>(cands.size(), 1) * sizeof(double)));
  owned.push_back(*d_tot);
  for (size_t k = 0; k + 1 < chunk_at.size(); k++) {
    const uint32_t a = chunk_at[k], nc = chunk_at[k + 1] - a;
    hipLaunchKernelGGL(tree_medoid_totals_kernel, dim3((nc + 3) / 4), dim3(256), 0, ctx->stream, d_cand + a, nc, d_aoff, d_anbr, d_aw,
                       d_scratch, *d_tot + a);
    RTC_CHECK_LAUNCH(ctx);
  }
  return RTC_OK;
}

}  // namespace

extern "C" {

int rtc_ctx_set_host_threads(rtc_ctx* ctx, int threads) {
  if (!ctx || threads < 1) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_ctx_set_host_threads: %d threads", threads);
  ctx->host_threads = threads;
  return RTC_OK;
}

int rtc_dedup_last_path(const rtc_ctx* ctx) { return ctx ? ctx->dedup_last_path : 0; }

int rtc_tree_medoids(rtc_ctx* ctx, uint32_t n, const rtc_edge* h_edges, uint64_t m, double dedup_dist, const uint64_t* h_seq_len,
                     int32_t* h_node_to_rep) {
  if (!ctx) return rtc_fail(nullptr, RTC_ERR_ARG, "rtc_tree_medoids: no context");
  if ((m && !h_edges) || (n && !h_node_to_rep) || n > 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_tree_medoids: bad arguments");
  ctx->dedup_last_path = 0;
  if (!(dedup_dist > 0)) {  // the reference's no-op (:69-73): every node its own representative
    for (uint32_t i = 0; i < n; i++) h_node_to_rep[i] = (int32_t)i;
    return RTC_OK;
  }
  rtc_tm::Groups G;
  if (!rtc_tm::build_groups((int)n, h_edges, m, dedup_dist, G))
    return rtc_fail(ctx, RTC_ERR_ARG, "rtc_tree_medoids: the edges with dist <= %g are not a forest over %u nodes", dedup_dist, n);
  const int mode = ctx->opt.dedup_gpu;
  std::vector<uint32_t> on_gpu, on_host;
  for (uint32_t g = 0; g < G.count(); g++) {
    const bool gpu = mode == 2 || (mode == 1 && G.size(g) >= kDedupGpuMinGroup);
    (gpu ? on_gpu : on_host).push_back(g);
  }
  std::vector<double> tot(G.mem.size());
  std::vector<void*> owned;
  std::vector<TmCand> cands;
  double* d_tot = nullptr;
  int st = RTC_OK;
  if (!on_gpu.empty()) {
    RTC_HIP(ctx, hipSetDevice(ctx->device));
    st = totals_gpu(ctx, G, on_gpu, owned, cands, &d_tot);
  }
  if (st == RTC_OK) {
    rtc_tm::totals_host(G, on_host, tot.data(), ctx->host_threads);  // beside the kernels
    if (!on_gpu.empty()) {
      std::vector<double> got(cands.size());
      hipError_t e = hipMemcpyAsync(got.data(), d_tot, got.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) st = rtc_fail(ctx, RTC_ERR_HIP, "rtc_tree_medoids: %s", hipGetErrorString(e));
      for (size_t i = 0; st == RTC_OK && i < cands.size(); i++) tot[cands[i].base + cands[i].c] = got[i];
    }
  }
  (void)hipStreamSynchronize(ctx->stream);
  for (void* p : owned) (void)hipFree(p);
  if (!owned.empty()) ctx->free_hbm_at = -1.0;
  if (st != RTC_OK) return st;
  rtc_tm::assign(G, (int)n, tot.data(), h_seq_len, h_node_to_rep);
  ctx->dedup_last_path = (on_host.empty() ? 0 : 1) | (on_gpu.empty() ? 0 : 2);
  return RTC_OK;
}

}  // extern "C"
