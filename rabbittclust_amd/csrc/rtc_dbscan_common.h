// rtc_dbscan_common.h -- the parts of the one DBSCAN implementation (rtc_dbscan_sweep.hip, with rtc_dbscan_hier.h) that do not
// depend on what a call asks for: the neighbour predicate and its refusals, the filter kernels' predicate block and wave
// append, the growing device list a filter appends to, the --max-posting pruning and the row-chunk loop of the pair
// phase (the scratch holder, DevBuf, is rtc_internal.h's).  Every unit that evaluates eps_pred is built with -ffp-contract=off.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "rtc_internal.h"

namespace {

inline uint64_t now_ns() {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline uint32_t blocks_for(uint64_t work, int num_cu) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((work + 255) / 256, (uint64_t)num_cu * 16));
}

// The neighbour test of findNeighborsKSSDWithIndex for reference point p (size a) and candidate q (size b): the size
// filter floor(t a) <= b <= ceil(a / t), then  !(common (1 + t) + 1e-12 < t a + t b)  in double, in that form
// (:531-533, :573-585; the u64 brute force :393-397, :426-431).  The unit is built with -ffp-contract=off: no FMA.
__host__ __device__ __forceinline__ bool eps_pred(uint32_t a, uint32_t b, uint32_t common, double t, double one_plus_t) {
  if (a == 0 || b == 0) return false;
  const double da = (double)a, db = (double)b;
  const double t_times_a = t * da;
  if (db < floor(t_times_a) || db > ceil(da / t)) return false;
  const double lhs = (double)common * one_plus_t;
  const double rhs = t_times_a + t * db;
  return !(lhs + 1e-12 < rhs);
}

// x and t of an eps on the host with libm (:751-752).  Outside t > 1e-12 (false) the reference's relation is not the one the
// closed form needs: pairs without a common hash pass the test (the u64 brute force lists them, the u32 index never sees them).
inline bool eps_to_t(double eps, int kmer_size, double* t, double* one_plus_t) {
  const double x = exp(-eps * kmer_size);
  *t = x / (2.0 - x);
  *one_plus_t = 1.0 + *t;
  return *t > 1e-12;
}
// u32 sketches: a size bound ceil(a / t) past INT_MAX is an undefined int conversion in the reference (:514)
inline bool u32_size_bound_fits(uint32_t max_len, double t) { return !(ceil((double)max_len / t) > 2147483647.0); }

// ---- what the filter kernels share ----
constexpr uint32_t DB_MAX_LEVELS = 32;
struct EpsLevels { double t[DB_MAX_LEVELS], one_plus_t[DB_MAX_LEVELS]; };

// The predicate block: the levels (one bit each) at which candidate c passes in both orientations, the levels not assumed to
// be nested; *common is the count the predicate sees, MarkCnt's u16 count for u32 sketches (:75-80, :496-506; sat = ~0u for u64).
// cnt[1]: pairs whose orientations disagree at some level, cnt[2]: the smallest such pair (i << 32 | j), cnt[3]: those levels.
__device__ __forceinline__ uint32_t eps_level_mask(const rtc_cedge& c, const uint32_t* __restrict__ len, const EpsLevels& lv, uint32_t n_lv,
                                                   uint32_t sat, uint32_t* common, unsigned long long* __restrict__ cnt) {
  *common = c.common < sat ? c.common : sat;
  const uint32_t a = len[c.i], b = len[c.j];
  uint32_t mask = 0, asym = 0;
  for (uint32_t l = 0; l < n_lv; l++) {
    const bool fwd = eps_pred(a, b, *common, lv.t[l], lv.one_plus_t[l]), bwd = eps_pred(b, a, *common, lv.t[l], lv.one_plus_t[l]);
    if (fwd != bwd) asym |= 1u << l;
    if (fwd && bwd) mask |= 1u << l;
  }
  if (asym) {
    atomicAdd(&cnt[1], 1ull);
    atomicMin(&cnt[2], ((unsigned long long)c.i << 32) | c.j);
    atomicOr(&cnt[3], (unsigned long long)asym);
  }
  return mask;
}
// The wave append: the lanes with `keep` take consecutive slots of a list behind *counter (one ballot, one atomic per wave, a
// prefix popcount per lane) and store their record where the slot lies below cap; the counter runs on past it, which the
// host sees.  Every lane of the wave calls it.
template <class T>
__device__ __forceinline__ void wave_append(bool keep, const T& rec, T* __restrict__ list, uint64_t cap, unsigned long long* __restrict__ counter) {
  const uint64_t bal = __ballot(keep);
  if (!bal) return;
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long at = 0;
  if (lane == 0) at = atomicAdd(counter, (unsigned long long)__popcll(bal));
  at = __shfl(at, 0);
  const uint64_t idx = at + (uint64_t)__popcll(bal & ((1ULL << lane) - 1ULL));
  if (keep && idx < cap) list[idx] = rec;
}

// ---- --max-posting ----
__global__ __launch_bounds__(256) void gather_hashes_kernel(const uint32_t* __restrict__ h, const uint64_t* __restrict__ start,
                                                            const uint32_t* __restrict__ len, const uint64_t* __restrict__ pstart,
                                                            uint32_t n, uint32_t* __restrict__ out, uint32_t* __restrict__ at) {
  // one wave per sketch; at[x] = x, the position each hash carries through the sort
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t g = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; g < n; g += waves) {
    const uint64_t s = start[g], d = pstart[g];
    for (uint32_t e = lane; e < len[g]; e += 64) { out[d + e] = h[s + e]; at[d + e] = (uint32_t)(d + e); }
  }
}
// head[i] = i where a run of equal hashes starts in the sorted copy, 0 elsewhere (a max-scan then gives every element its run's start)
__global__ __launch_bounds__(256) void run_heads_kernel(const uint32_t* __restrict__ sorted, uint64_t total, uint32_t* __restrict__ head) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x)
    head[i] = (i == 0 || sorted[i - 1] != sorted[i]) ? (uint32_t)i : 0u;
}
// keep[at[i]] = 1 when the run of sorted[i] (starting at start[i]) holds at most M hashes, i.e. its (M + 1)-th element is another hash
__global__ __launch_bounds__(256) void posting_keep_kernel(const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ at,
                                                           const uint32_t* __restrict__ start, uint64_t total, uint64_t max_posting,
                                                           uint32_t* __restrict__ keep) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t past = (uint64_t)start[i] + max_posting;  // the run's (M + 1)-th element
    keep[at[i]] = (past < total && sorted[past] == sorted[i]) ? 0u : 1u;
  }
}
__global__ __launch_bounds__(256) void posting_scatter_kernel(const uint32_t* __restrict__ flat, const uint32_t* __restrict__ keep,
                                                              const uint64_t* __restrict__ pos, uint64_t total, uint32_t* __restrict__ out) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x)
    if (keep[x]) out[pos[x]] = flat[x];
}
// pruned sketch g: [pos[pstart[g]], pos[pstart[g] + len[g]]) of the compacted array (pos has total + 1 entries)
__global__ __launch_bounds__(256) void posting_rows_kernel(const uint64_t* __restrict__ pos, const uint64_t* __restrict__ pstart,
                                                           const uint32_t* __restrict__ len, uint32_t n, uint64_t* __restrict__ nstart,
                                                           uint32_t* __restrict__ nlen) {
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += gridDim.x * blockDim.x) {
    const uint64_t a = pos[pstart[g]], b = pos[pstart[g] + len[g]];
    nstart[g] = a;
    nlen[g] = (uint32_t)(b - a);
  }
}

// A device list of pairs that a filter kernel appends to chunk by chunk, and what the filter has found so far.  R: the record
// (rtc_cedge everywhere but in rtc_graph_build_mash, whose 16-byte record carries the truncated denom beside the common).
template <class R>
struct KeptListOf {
  R* d = nullptr;
  uint64_t cap = 0, used = 0, asym = 0, first_asym = ~0ull, asym_levels = 0, ns = 0;
};
using KeptList = KeptListOf<rtc_cedge>;
using FilterKernel = void (*)(const rtc_cedge*, uint64_t, const uint32_t*, EpsLevels, uint32_t, uint32_t, rtc_cedge*, uint64_t, unsigned long long*);

// Room for `need` pairs in the list before a filter runs, so the kernel never runs past it and runs once: doubled while that
// covers the need, so many row chunks move the list a few times, and the exact size where the doubled list is too small or
// does not fit.
template <class R>
int kept_reserve(rtc_ctx* ctx, DevBuf& db, KeptListOf<R>* L, uint64_t need) {
  if (need <= L->cap) return RTC_OK;
  auto regrow = [&](uint64_t want) -> int {
    R* nd = nullptr;
    RTC_TRY(db.get(ctx, want, &nd));
    if (L->used) RTC_HIP(ctx, hipMemcpyAsync(nd, L->d, L->used * sizeof(R), hipMemcpyDeviceToDevice, ctx->stream));
    RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    db.release(L->d);
    L->d = nd; L->cap = want;
    return RTC_OK;
  };
  if (2 * L->cap <= need || regrow(2 * L->cap) != RTC_OK) {
    (void)hipGetLastError();  // a doubled list that did not fit is no failure yet: the exact size may
    RTC_TRY(regrow(need));
  }
  return RTC_OK;
}

// One chunk of candidates through `filter` into the list, grown first to hold used + the whole chunk (at most every candidate
// is kept: kept_reserve).  d_fc: the four device counters of eps_level_mask and wave_append.
int filter_chunk(rtc_ctx* ctx, DevBuf& db, const char* who, FilterKernel filter, const rtc_cedge* d_cand, uint64_t m,
                 const uint32_t* d_len, const EpsLevels& lv, uint32_t n_lv, uint32_t sat, unsigned long long* d_fc, KeptList* L) {
  hipStream_t s = ctx->stream;
  const uint64_t t0 = now_ns();
  RTC_TRY(kept_reserve(ctx, db, L, L->used + m));
  unsigned long long fc[4] = {(unsigned long long)L->used, 0ull, ~0ull, 0ull};
  RTC_HIP(ctx, hipMemcpyAsync(d_fc, fc, sizeof fc, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(filter, dim3(blocks_for(m, ctx->num_cu)), dim3(256), 0, s, d_cand, m, d_len, lv, n_lv, sat, L->d, L->cap, d_fc);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipMemcpyAsync(fc, d_fc, sizeof fc, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  if (fc[0] > L->cap) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu pairs kept, room for %llu", who, fc[0], (unsigned long long)L->cap);
  L->used = fc[0];
  L->asym += fc[1];
  L->first_asym = std::min<uint64_t>(L->first_asym, fc[2]);
  L->asym_levels |= fc[3];
  L->ns += now_ns() - t0;
  return RTC_OK;
}

// The pruned copy of a u32 sketch set (buildInvertedIndexCSR32 with max_posting > 0): all hashes gathered with their positions,
// sorted (rtc_sort_u32_pairs), every run of one hash measured against M, the kept hashes compacted in their original order.
int prune_postings(rtc_ctx* ctx, DevBuf& db, const uint32_t* d_h, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                   const std::vector<uint32_t>& h_len, uint64_t max_posting, uint32_t** d_ph, uint64_t** d_pstart, uint32_t** d_plen) {
  hipStream_t s = ctx->stream;
  std::vector<uint64_t> pst(n + 1, 0);
  for (uint32_t g = 0; g < n; g++) pst[g + 1] = pst[g] + h_len[g];
  const uint64_t total = pst[n];
  if (total >= 0xffffffffull) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "rtc_dbscan --max-posting: %llu hashes", (unsigned long long)total);
  uint64_t *d_pst = nullptr, *d_pos = nullptr;
  uint32_t *d_flat = nullptr, *d_sorted = nullptr, *d_at = nullptr, *d_at_sorted = nullptr, *d_head = nullptr, *d_keep = nullptr;
  RTC_TRY(db.get(ctx, n + 1, &d_pst));
  RTC_TRY(db.get(ctx, total, &d_flat));
  RTC_TRY(db.get(ctx, total, &d_sorted));
  RTC_TRY(db.get(ctx, total, &d_at));
  RTC_TRY(db.get(ctx, total, &d_at_sorted));
  RTC_TRY(db.get(ctx, total, &d_head));
  RTC_TRY(db.get(ctx, total + 1, &d_keep));
  RTC_TRY(db.get(ctx, total + 1, &d_pos));
  RTC_TRY(db.get(ctx, total, d_ph));
  RTC_TRY(db.get(ctx, n, d_pstart));
  RTC_TRY(db.get(ctx, n, d_plen));
  RTC_HIP(ctx, hipMemcpyAsync(d_pst, pst.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(gather_hashes_kernel, dim3(blocks_for((uint64_t)n * 64, ctx->num_cu)), dim3(256), 0, s, d_h, d_start, d_len,
                     (const uint64_t*)d_pst, n, d_flat, d_at);
  RTC_CHECK_LAUNCH(ctx);
  RTC_TRY(rtc_sort_u32_pairs(ctx, d_flat, d_sorted, d_at, d_at_sorted, (size_t)total));
  hipLaunchKernelGGL(run_heads_kernel, dim3(blocks_for(total, ctx->num_cu)), dim3(256), 0, s, (const uint32_t*)d_sorted, total, d_flat);
  RTC_CHECK_LAUNCH(ctx);
  size_t tb = 0, tb2 = 0;
  RTC_HIP(ctx, rocprim::inclusive_scan(nullptr, tb, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)total, rocprim::maximum<uint32_t>(), s));
  RTC_HIP(ctx, rocprim::exclusive_scan(nullptr, tb2, (const uint32_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)total + 1,
                                       rocprim::plus<uint64_t>(), s));
  tb = std::max(tb, tb2);
  void* tmp = nullptr;
  RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
  RTC_HIP(ctx, rocprim::inclusive_scan(tmp, tb, (const uint32_t*)d_flat, d_head, (size_t)total, rocprim::maximum<uint32_t>(), s));
  hipLaunchKernelGGL(posting_keep_kernel, dim3(blocks_for(total, ctx->num_cu)), dim3(256), 0, s, (const uint32_t*)d_sorted,
                     (const uint32_t*)d_at_sorted, (const uint32_t*)d_head, total, max_posting, d_keep);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipMemsetAsync(d_keep + total, 0, 4, s));
  // the gathered hashes again, in sketch order, for the scatter (d_flat held the run heads)
  hipLaunchKernelGGL(gather_hashes_kernel, dim3(blocks_for((uint64_t)n * 64, ctx->num_cu)), dim3(256), 0, s, d_h, d_start, d_len,
                     (const uint64_t*)d_pst, n, d_flat, d_at);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, rocprim::exclusive_scan(tmp, tb, (const uint32_t*)d_keep, d_pos, (uint64_t)0, (size_t)total + 1, rocprim::plus<uint64_t>(), s));
  hipLaunchKernelGGL(posting_scatter_kernel, dim3(blocks_for(total, ctx->num_cu)), dim3(256), 0, s, (const uint32_t*)d_flat,
                     (const uint32_t*)d_keep, (const uint64_t*)d_pos, total, *d_ph);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(posting_rows_kernel, dim3(blocks_for(n, ctx->num_cu)), dim3(256), 0, s, (const uint64_t*)d_pos,
                     (const uint64_t*)d_pst, d_len, n, *d_pstart, *d_plen);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipStreamSynchronize(s));
  for (void* q : {(void*)d_flat, (void*)d_sorted, (void*)d_at, (void*)d_at_sorted, (void*)d_head, (void*)d_keep, (void*)d_pos, (void*)d_pst})
    db.release(q);
  return RTC_OK;
}

// Leaves the tiled pair kernel's plan hold off on every way out of the chunk loop (the plan is only valid while the caller holds it)
struct PlanHold {
  rtc_ctx* ctx;
  bool on = false;
  void take(uint32_t tc1_hint) { on = true; ctx->pair_plan_hold = 1; ctx->pair_plan_valid = 0; ctx->pair_plan_tc1_hint = tc1_hint; }
  ~PlanHold() { if (on) { ctx->pair_plan_hold = 0; ctx->pair_plan_valid = 0; } }
};


// The pair phase of a DBSCAN call: every pair sharing a hash (rtc_pair_edges_dev, radio < 0) over row chunks, the overflow
// protocol of rtc_candidate_edges_device.  on_chunk(d_cand, count) sees every chunk once, before the next one is produced;
// the candidate list is released on the way out.  budget: the candidate edges of one chunk.  first_row: the rows below it are
// columns only (1: every pair of the set; rtc_dbscan_update joins its row ranges alone).  radio: rtc_pair_edges_dev's size-ratio
// bound, below 0 for none (rtc_cluster_support passes the MST's).
struct PairPhase { uint64_t chunks = 0, cand_total = 0, pair_ns = 0; };
template <class F>
int dbscan_pair_chunks(rtc_ctx* ctx, DevBuf& db, const void* ph, int width, const uint64_t* pstart, const uint32_t* plen, uint32_t n,
                       uint32_t first_row, unsigned long long* d_cnt, PairPhase* pp, F&& on_chunk, int radio = -1) {
  hipStream_t s = ctx->stream;
  uint64_t budget = (uint64_t)256 << 20;  // candidate edges of one chunk (3 GiB)
  if (ctx->opt.edge_budget) budget = ctx->opt.edge_budget;
  budget = std::max<uint64_t>(budget, 64ull * n + 1024);  // a 64-row block always fits
  rtc_cedge* d_cand = nullptr;
  uint64_t cand_cap = std::min<uint64_t>(budget, std::max<uint64_t>((uint64_t)1 << 20, (uint64_t)n * 160));
  RTC_TRY(db.get(ctx, cand_cap, &d_cand));
  const uint32_t row_end = n;
  uint32_t r0 = std::max<uint32_t>(first_row, 1), rows_per = n;
  int redo = 0;
  PlanHold hold{ctx};
  while (r0 < row_end) {
    const uint32_t r1 = (uint32_t)std::min<uint64_t>(row_end, (uint64_t)r0 + rows_per);
    const uint64_t tp = now_ns();
    unsigned long long cnt = 0;
    RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 8, s));
    const int st = rtc_pair_edges_dev(ctx, ph, width, pstart, plen, n, r0, r1, 0, r1 - 1, radio, d_cand, cand_cap, (uint64_t*)d_cnt);
    if (st != RTC_OK) { (void)hipStreamSynchronize(s); return st; }
    RTC_HIP(ctx, hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    pp->pair_ns += now_ns() - tp;
    if (cnt > cand_cap) {
      // past the list: exact, or the join's estimate (rtc_pair_edges_dev's overflow protocol) -- grow and run the rows again
      // while the count fits the budget, otherwise cut the rows
      if (cnt <= budget && redo < 3) {
        redo++;
        db.release(d_cand);
        cand_cap = std::min<uint64_t>(budget, cnt + cnt / 16);
        RTC_TRY(db.get(ctx, cand_cap, &d_cand));
        continue;
      }
      if (cand_cap < budget) {
        db.release(d_cand);
        cand_cap = budget;
        RTC_TRY(db.get(ctx, cand_cap, &d_cand));
      }
      if (r1 - r0 <= 64) {
        (void)hipStreamSynchronize(s);
        return rtc_fail(ctx, RTC_ERR_NOMEM, "rtc_dbscan: edge budget %llu too small for a 64-row block", (unsigned long long)budget);
      }
      if (!hold.on) hold.take(row_end - 1);  // the sketches do not change between the chunk launches: the tiled kernel builds its plan once
      rows_per = std::max<uint32_t>(64, (uint32_t)std::min<uint64_t>((uint64_t)(r1 - r0) / 2, (budget / 2) / std::max<uint32_t>(r1, 1)) / 64 * 64);
      redo = 0;
      continue;
    }
    redo = 0;
    pp->chunks++;
    pp->cand_total += cnt;
    RTC_TRY(on_chunk(d_cand, (uint64_t)cnt));
    r0 = r1;
  }
  db.release(d_cand);
  return RTC_OK;
}

}  // namespace
