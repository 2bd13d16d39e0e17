// rtc_rep_screen.hip -- clust-mst --db --screen: which representatives a sample contains (include/rtclust.h has the
// definition, DESIGN 3.4t the reasoning).  The inverted join of rtc_pairs_join.hip folds a pair to a count and forgets which
// hashes were shared; the winner-takes-all rounds need exactly those, so this unit has a join of its own that keeps them.
//
//   index       once per call: the (hash, slot) pairs of the live, non-empty representatives, sorted by hash on all 64 bits
//               (rtc_sort_u64_pairs; hashes of width 4 are widened).
// and per chunk of samples (for_query_chunks, rtc_query_chunks.h), a "position" being one hash of one sample of the chunk:
//   count       a lane per position: the run of its hash in the index by two binary searches
//   scan        the exclusive 64-bit offsets of the runs (rocPRIM)
//   fill        the match records ((sample, slot) as one 64-bit key, position): a lane writes a run of up to SCREEN_SHORT_RUN
//               entries itself, the wave writes a longer one together, 64 records a step -- a hub hash that sits in thousands of
//               representatives is ordinary
//   sort        the records by (sample, slot): a run of equal keys is a candidate and its length is `common`; the sorted
//               positions are the view candidate -> positions as they stand
//   candidates  run heads, run numbers (scan), the eligibility test in integers, the eligible runs numbered (scan) and
//               compacted; a count per sample is read back and gives the segments
//   view        position -> the eligible candidates that hold it, written into the position's own run of the fill layout
//               through a cursor per position (the cursor that stays 0 marks a hash that is not matched)
//   gather      one workgroup per sample runs all of its rounds in one launch: an argmax over the remaining counts u on the key
//               (u, lower slot), then the lanes stride over the winner's positions, retire those still alive and decrement u
//               of every candidate that holds them -- the winner's own too, so that a picked candidate ends at 0 and is never
//               picked again.  u lives in LDS for one wave (up to SCREEN_WAVE_CANDS candidates) or 256 lanes (up to
//               SCREEN_BLOCK_CANDS), in global memory beyond.  The round loop is counted by the sample's candidates; the
//               min_unique test is an early way out of it, never the only one.
// The picks are ordered by rank and the others by containment on the host, as rtc_rep_topk orders with topk == 0.

#include "rtc_query_chunks.h"
#include "rtc_screen.h"

namespace {

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

// one wave per representative: its hashes with its slot, at ioff[g] (live, non-empty representatives only)
template <typename T>
__global__ __launch_bounds__(256) void screen_index_kernel(const T* __restrict__ h, const uint64_t* __restrict__ start,
                                                           const uint32_t* __restrict__ len, const uint8_t* __restrict__ live,
                                                           const uint64_t* __restrict__ ioff, uint32_t n_reps, uint64_t* __restrict__ key,
                                                           uint32_t* __restrict__ slot) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t g = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; g < n_reps; g += waves) {
    if (live && !live[g]) continue;
    const uint64_t s = start[g], d = ioff[g];
    const uint32_t l = len[g];
    for (uint32_t e = lane; e < l; e += 64) { key[d + e] = (uint64_t)h[s + e]; slot[d + e] = g; }
  }
}

// position p of the chunk: the sample it belongs to (qoff[nq + 1]: the samples' first positions), the run [lo, lo + cnt) of its
// hash in the index of K entries
template <typename T>
__global__ __launch_bounds__(256) void screen_count_kernel(const T* __restrict__ h, const uint64_t* __restrict__ start, uint32_t row0,
                                                           const uint64_t* __restrict__ qoff, uint32_t nq, uint64_t P,
                                                           const uint64_t* __restrict__ ikey, uint64_t K, uint64_t* __restrict__ lo,
                                                           uint64_t* __restrict__ cnt, uint32_t* __restrict__ pq) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  uint32_t a = 0, b = nq;  // the last q with qoff[q] <= p
  while (b - a > 1) { const uint32_t m = a + (b - a) / 2; if (qoff[m] <= p) a = m; else b = m; }
  const uint64_t x = (uint64_t)h[start[row0 + a] + (p - qoff[a])];
  uint64_t l0 = 0, l1 = K;  // first entry >= x
  while (l0 < l1) { const uint64_t m = l0 + (l1 - l0) / 2; if (ikey[m] < x) l0 = m + 1; else l1 = m; }
  uint64_t u0 = l0, u1 = K;  // first entry > x
  while (u0 < u1) { const uint64_t m = u0 + (u1 - u0) / 2; if (ikey[m] <= x) u0 = m + 1; else u1 = m; }
  lo[p] = l0;
  cnt[p] = u0 - l0;
  pq[p] = a;
}

// the match records of position p at moff[p] .. moff[p + 1): key = sample << 32 | slot, value = p
__global__ __launch_bounds__(256) void screen_fill_kernel(const uint64_t* __restrict__ lo, const uint64_t* __restrict__ moff,
                                                          const uint32_t* __restrict__ pq, const uint32_t* __restrict__ islot, uint64_t P,
                                                          uint64_t* __restrict__ mkey, uint32_t* __restrict__ mpos) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const bool valid = p < P;
  const uint64_t at = valid ? moff[p] : 0, l0 = valid ? lo[p] : 0;
  const uint64_t c = valid ? moff[p + 1] - at : 0;
  const uint64_t qhi = valid ? (uint64_t)pq[p] << 32 : 0;
  if (c && c <= SCREEN_SHORT_RUN)
    for (uint32_t j = 0; j < (uint32_t)c; j++) { mkey[at + j] = qhi | islot[l0 + j]; mpos[at + j] = (uint32_t)p; }
  uint64_t todo = __ballot(c > SCREEN_SHORT_RUN);  // every lane of the wave is here
  while (todo) {
    const int src = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const uint64_t w_at = shfl_u64(at, src), w_lo = shfl_u64(l0, src), w_c = shfl_u64(c, src), w_q = shfl_u64(qhi, src);
    const uint32_t w_p = __shfl((uint32_t)p, src);
    for (uint64_t j = lane; j < w_c; j += 64) { mkey[w_at + j] = w_q | islot[w_lo + j]; mpos[w_at + j] = w_p; }
  }
}

__global__ __launch_bounds__(256) void screen_heads_kernel(const uint64_t* __restrict__ skey, uint32_t M, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) head[i] = (i == 0 || skey[i - 1] != skey[i]) ? 1u : 0u;
}

// rstart[c]: the first record of run c (cid1: the inclusive scan of the heads, so run numbers plus one); rstart[C] = M
__global__ __launch_bounds__(256) void screen_runs_kernel(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ cid1, uint32_t M,
                                                          uint32_t C, uint32_t* __restrict__ rstart) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  if (i == 0 || skey[i - 1] != skey[i]) { const uint32_t c = cid1[i] - 1; if (c < C) rstart[c] = i; }
  if (i == M - 1) rstart[C] = M;
}

// the eligibility test of run c, in integers; elig[C] = 0 closes the scan
__global__ __launch_bounds__(256) void screen_elig_kernel(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ rstart, uint32_t C,
                                                          const uint32_t* __restrict__ len, uint32_t n_reps, uint32_t nq, uint32_t min_common,
                                                          uint32_t min_cont_q20, uint32_t* __restrict__ elig, uint32_t* __restrict__ qcnt) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > C) return;
  if (c == C) { elig[c] = 0; return; }
  const uint64_t key = skey[rstart[c]];
  const uint32_t q = (uint32_t)(key >> 32), slot = (uint32_t)key;
  const uint32_t common = rstart[c + 1] - rstart[c];
  bool ok = q < nq && slot < n_reps && common >= (min_common ? min_common : 1u);
  if (ok) ok = ((uint64_t)common << 20) >= (uint64_t)min_cont_q20 * (uint64_t)len[slot];
  elig[c] = ok ? 1u : 0u;
  if (ok) atomicAdd(&qcnt[q], 1u);
}

// the eligible runs, in (sample, slot) order: slot, common, first record, and u = common (every shared hash is matched)
__global__ __launch_bounds__(256) void screen_compact_kernel(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ rstart,
                                                             const uint32_t* __restrict__ elig, const uint32_t* __restrict__ eid, uint32_t C,
                                                             uint32_t E, uint32_t* __restrict__ cslot, uint32_t* __restrict__ ccommon,
                                                             uint32_t* __restrict__ cms, uint32_t* __restrict__ u) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C || !elig[c]) return;
  const uint32_t e = eid[c];
  if (e >= E) return;
  const uint32_t s = rstart[c], common = rstart[c + 1] - s;
  cslot[e] = (uint32_t)skey[s];
  ccommon[e] = common;
  cms[e] = s;
  u[e] = common;
}

// position -> its eligible candidates, in the position's run of the fill layout; pcur[p] ends as their number
__global__ __launch_bounds__(256) void screen_view_kernel(const uint32_t* __restrict__ cid1, const uint32_t* __restrict__ elig,
                                                          const uint32_t* __restrict__ eid, const uint32_t* __restrict__ spos, uint32_t M,
                                                          uint32_t C, uint64_t P, const uint64_t* __restrict__ moff, uint32_t* __restrict__ pcur,
                                                          uint32_t* __restrict__ pcand) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const uint32_t c = cid1[i] - 1;
  if (c >= C || !elig[c]) return;
  const uint32_t p = spos[i];
  if (p >= P) return;
  const uint32_t k = atomicAdd(&pcur[p], 1u);
  const uint64_t at = moff[p] + k;
  if (at < moff[p + 1]) pcand[at] = eid[c];
}

struct GatherArgs {
  const uint64_t* qeoff;    // [nq + 1] the samples' candidate segments
  const uint64_t* qoff;     // [nq + 1] the samples' positions
  const uint32_t* cms;      // candidate -> its first sorted record
  const uint32_t* ccommon;  // candidate -> common
  const uint32_t* spos;     // sorted records: candidate -> positions
  const uint64_t* moff;     // position -> its run of pcand
  const uint32_t* pcur;     // position -> the number of its eligible candidates
  const uint32_t* pcand;    // position -> eligible candidates
  uint8_t* alive;           // position still in R (all ones at the start; only matched positions are ever read)
  uint32_t* u;              // candidate -> remaining count (the global path works on it, the LDS paths copy it)
  uint32_t* rank;           // candidate -> rank, zeroed
  uint32_t* unique;         // candidate -> unique
  rtc_screen_sum* sum;      // [nq]; n_hashes is the host's
  uint32_t* rounds;         // [nq]
  uint32_t nq, lo, hi, min_unique, max_picks;
};

template <int B>
__device__ __forceinline__ uint64_t block_max(uint64_t v, uint64_t* part) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const uint64_t o = shfl_u64(v, (int)((threadIdx.x & 63) ^ d)); v = o > v ? o : v; }
  if (B == 64) return v;
  if ((threadIdx.x & 63) == 0) part[threadIdx.x / 64] = v;
  __syncthreads();
  uint64_t r = part[0];
#pragma unroll
  for (int w = 1; w < B / 64; w++) r = part[w] > r ? part[w] : r;
  return r;
}

// One workgroup of B lanes, one sample.  LDS_U: the counts in LDS (up to CAP of them).
template <int B, bool LDS_U, uint32_t CAP>
__global__ __launch_bounds__(B) void screen_gather_kernel(GatherArgs A) {
  __shared__ uint32_t s_u[LDS_U ? CAP : 1];
  __shared__ uint64_t s_part[B / 64];
  __shared__ uint32_t s_cnt[B / 64];
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  if (q >= A.nq) return;
  const uint64_t e0 = A.qeoff[q];
  const uint64_t ne64 = A.qeoff[q + 1] - e0;
  if (ne64 < A.lo || ne64 > A.hi) return;  // another launch's sample, or none (lo >= 1)
  const uint32_t ne = (uint32_t)ne64;
  if (LDS_U && ne > CAP) return;
  uint32_t* gu = A.u + e0;
  if (LDS_U) for (uint32_t i = tid; i < ne; i += B) s_u[i] = A.ccommon[e0 + i];
  // matched: the positions of the sample that some eligible candidate holds
  uint32_t mine = 0;
  for (uint64_t p = A.qoff[q] + tid; p < A.qoff[q + 1]; p += B) mine += A.pcur[p] ? 1u : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
  if ((tid & 63) == 0) s_cnt[tid / 64] = mine;
  __syncthreads();
  uint32_t matched = 0;
#pragma unroll
  for (int w = 0; w < B / 64; w++) matched += s_cnt[w];
  const uint32_t limit = A.max_picks ? (A.max_picks < ne ? A.max_picks : ne) : ne;
  uint32_t picks = 0, explained = 0;
  for (uint32_t t = 1; t <= limit; t++) {
    __syncthreads();  // the last round's decrements are done (and s_part is read)
    uint64_t best = 0;
    for (uint32_t i = tid; i < ne; i += B) {
      const uint32_t v = LDS_U ? s_u[i] : __hip_atomic_load(&gu[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint64_t key = ((uint64_t)v << 32) | (0xffffffffu - i);  // candidates are in slot order: the lower index is the lower slot
      best = key > best ? key : best;
    }
    best = block_max<B>(best, s_part);
    const uint32_t bu = (uint32_t)(best >> 32);
    if (bu < A.min_unique) break;  // the same value in every lane
    const uint32_t w = 0xffffffffu - (uint32_t)best;
    if (w >= ne) break;
    if (tid == 0) { A.rank[e0 + w] = t; A.unique[e0 + w] = bu; }
    picks++;
    explained += bu;
    const uint32_t ms = A.cms[e0 + w], cw = A.ccommon[e0 + w];
    for (uint32_t j = tid; j < cw; j += B) {
      const uint32_t p = A.spos[ms + j];
      if (!A.alive[p]) continue;
      A.alive[p] = 0;
      const uint64_t at = A.moff[p];
      const uint32_t n = A.pcur[p];
      for (uint32_t k = 0; k < n; k++) {
        const uint64_t c = (uint64_t)A.pcand[at + k] - e0;
        if (c >= ne) continue;
        if (LDS_U) atomicSub(&s_u[(uint32_t)c], 1u);
        else atomicSub(&gu[c], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < ne; i += B)
    if (A.rank[e0 + i] == 0)
      A.unique[e0 + i] = LDS_U ? s_u[i] : __hip_atomic_load(&gu[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) {
    rtc_screen_sum s;
    s.n_hashes = (uint32_t)(A.qoff[q + 1] - A.qoff[q]);
    s.n_matched = matched; s.n_explained = explained; s.n_hits = ne; s.n_picks = picks; s.pad = 0;
    A.sum[q] = s;
    A.rounds[q] = picks;
  }
}

struct ScreenArgs {
  const void* d_hashes; int width; const uint64_t* d_start; const uint32_t* d_len; uint32_t n_reps;
  uint32_t min_common, min_cont_q20, min_unique, max_picks;
  const uint64_t* d_ikey; const uint32_t* d_islot; uint64_t K;
};

int scan_u64(rtc_ctx* ctx, const uint64_t* in, uint64_t* out, size_t n) {
  size_t tb = 0;
  RTC_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), ctx->stream));
  void* tmp = nullptr;
  RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
  RTC_HIP(ctx, rocprim::exclusive_scan(tmp, tb, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), ctx->stream));
  return RTC_OK;
}
int scan_u32(rtc_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n, bool inclusive) {
  size_t tb = 0;
  if (inclusive) RTC_HIP(ctx, rocprim::inclusive_scan(nullptr, tb, in, out, n, rocprim::plus<uint32_t>(), ctx->stream));
  else RTC_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, in, out, 0u, n, rocprim::plus<uint32_t>(), ctx->stream));
  void* tmp = nullptr;
  RTC_TRY(rtc_ws(ctx, 5, tb + 256, &tmp));
  if (inclusive) RTC_HIP(ctx, rocprim::inclusive_scan(tmp, tb, in, out, n, rocprim::plus<uint32_t>(), ctx->stream));
  else RTC_HIP(ctx, rocprim::exclusive_scan(tmp, tb, in, out, 0u, n, rocprim::plus<uint32_t>(), ctx->stream));
  return RTC_OK;
}

bool hit_order(const rtc_screen_hit& a, const rtc_screen_hit& b) {
  if ((a.rank != 0) != (b.rank != 0)) return a.rank != 0;
  if (a.rank) return a.rank < b.rank;
  const uint64_t l = (uint64_t)a.common * b.size, r = (uint64_t)b.common * a.size;
  return l != r ? l > r : a.slot < b.slot;
}

// samples [q0, q1): appends their hits in order, fills their sums.  RTC_ERR_NOMEM: the chunk does not fit the budget.
int rep_screen_chunk(rtc_ctx* ctx, const ScreenArgs& A, const std::vector<uint32_t>& h_len, uint32_t q0, uint32_t q1,
                     std::vector<rtc_screen_hit>& out, rtc_screen_sum* sum) {
  const uint32_t R = A.n_reps, row0 = R + q0, nq = q1 - q0;
  hipStream_t s = ctx->stream;
  const uint64_t t0 = now_ns();
  std::vector<uint64_t> h_qoff(nq + 1, 0);
  for (uint32_t q = 0; q < nq; q++) {
    h_qoff[q + 1] = h_qoff[q] + h_len[row0 + q];
    sum[q] = rtc_screen_sum{h_len[row0 + q], 0, 0, 0, 0, 0};
  }
  const uint64_t P = h_qoff[nq];
  if (P == 0 || A.K == 0) return RTC_OK;
  const uint64_t budget = ctx->opt.screen_bytes ? ctx->opt.screen_bytes : rtc_free_hbm(ctx) / 2;
  if (P >= 0xffffffffull || P * SCREEN_POS_BYTES > budget)
    return rtc_fail(ctx, RTC_ERR_NOMEM, "rtc_rep_screen: %llu hashes of %u samples need %llu bytes, the budget is %llu (RTC_SCREEN_BYTES)",
                    (unsigned long long)P, nq, (unsigned long long)(P * SCREEN_POS_BYTES), (unsigned long long)budget);
  DevBuf db;
  // ---- count, scan ----
  uint64_t *d_qoff = nullptr, *d_lo = nullptr, *d_cnt = nullptr, *d_moff = nullptr;
  uint32_t *d_pq = nullptr, *d_pcur = nullptr;
  uint8_t* d_alive = nullptr;
  RTC_TRY(db.get(ctx, (size_t)nq + 1, &d_qoff));
  RTC_TRY(db.get(ctx, P, &d_lo));
  RTC_TRY(db.get(ctx, P + 1, &d_cnt));
  RTC_TRY(db.get(ctx, P + 1, &d_moff));
  RTC_TRY(db.get(ctx, P, &d_pq));
  RTC_TRY(db.get(ctx, P, &d_pcur));
  RTC_TRY(db.get(ctx, P, &d_alive));
  RTC_HIP(ctx, hipMemcpyAsync(d_qoff, h_qoff.data(), ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, s));
  RTC_HIP(ctx, hipMemsetAsync(d_cnt + P, 0, 8, s));
  RTC_HIP(ctx, hipMemsetAsync(d_pcur, 0, P * 4, s));
  RTC_HIP(ctx, hipMemsetAsync(d_alive, 1, P, s));
  const dim3 gp((uint32_t)((P + 255) / 256)), b256(256);
  if (A.width == 8)
    hipLaunchKernelGGL(screen_count_kernel<uint64_t>, gp, b256, 0, s, (const uint64_t*)A.d_hashes, A.d_start, row0, (const uint64_t*)d_qoff, nq, P,
                       A.d_ikey, A.K, d_lo, d_cnt, d_pq);
  else
    hipLaunchKernelGGL(screen_count_kernel<uint32_t>, gp, b256, 0, s, (const uint32_t*)A.d_hashes, A.d_start, row0, (const uint64_t*)d_qoff, nq, P,
                       A.d_ikey, A.K, d_lo, d_cnt, d_pq);
  RTC_CHECK_LAUNCH(ctx);
  RTC_TRY(scan_u64(ctx, d_cnt, d_moff, P + 1));
  uint64_t M = 0;
  RTC_HIP(ctx, hipMemcpyAsync(&M, d_moff + P, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  db.release(d_cnt);
  if (M == 0) { ctx->rep_screen[9] += now_ns() - t0; return RTC_OK; }
  const uint64_t need = P * SCREEN_POS_BYTES + M * SCREEN_MATCH_BYTES;
  if (M >= 0xffffffffull || need > budget)
    return rtc_fail(ctx, RTC_ERR_NOMEM, "rtc_rep_screen: %llu match records of %u samples need %llu bytes, the budget is %llu (RTC_SCREEN_BYTES)",
                    (unsigned long long)M, nq, (unsigned long long)need, (unsigned long long)budget);
  const uint32_t M32 = (uint32_t)M;
  // ---- fill, sort ----
  uint64_t *d_mkey = nullptr, *d_skey = nullptr;
  uint32_t *d_mpos = nullptr, *d_spos = nullptr;
  RTC_TRY(db.get(ctx, M, &d_mkey));
  RTC_TRY(db.get(ctx, M, &d_mpos));
  RTC_TRY(db.get(ctx, M, &d_skey));
  RTC_TRY(db.get(ctx, M, &d_spos));
  hipLaunchKernelGGL(screen_fill_kernel, gp, b256, 0, s, (const uint64_t*)d_lo, (const uint64_t*)d_moff, (const uint32_t*)d_pq, A.d_islot, P, d_mkey,
                     d_mpos);
  RTC_CHECK_LAUNCH(ctx);
  RTC_TRY(rtc_sort_u64_pairs(ctx, d_mkey, d_skey, d_mpos, d_spos, M));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  db.release(d_mkey); db.release(d_mpos); db.release(d_lo); db.release(d_pq);
  // ---- candidates ----
  uint32_t *d_cid1 = nullptr, *d_head = nullptr;
  RTC_TRY(db.get(ctx, M, &d_head));
  RTC_TRY(db.get(ctx, M, &d_cid1));
  const dim3 gm((M32 + 255) / 256);
  hipLaunchKernelGGL(screen_heads_kernel, gm, b256, 0, s, (const uint64_t*)d_skey, M32, d_head);
  RTC_CHECK_LAUNCH(ctx);
  RTC_TRY(scan_u32(ctx, d_head, d_cid1, M, true));
  uint32_t C = 0;
  RTC_HIP(ctx, hipMemcpyAsync(&C, d_cid1 + (M - 1), 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  db.release(d_head);
  uint32_t *d_rstart = nullptr, *d_elig = nullptr, *d_eid = nullptr, *d_qcnt = nullptr;
  RTC_TRY(db.get(ctx, (size_t)C + 1, &d_rstart));
  RTC_TRY(db.get(ctx, (size_t)C + 1, &d_elig));
  RTC_TRY(db.get(ctx, (size_t)C + 1, &d_eid));
  RTC_TRY(db.get(ctx, nq, &d_qcnt));
  RTC_HIP(ctx, hipMemsetAsync(d_qcnt, 0, (size_t)nq * 4, s));
  hipLaunchKernelGGL(screen_runs_kernel, gm, b256, 0, s, (const uint64_t*)d_skey, (const uint32_t*)d_cid1, M32, C, d_rstart);
  RTC_CHECK_LAUNCH(ctx);
  const dim3 gc(C / 256 + 1);  // C + 1 lanes
  hipLaunchKernelGGL(screen_elig_kernel, gc, b256, 0, s, (const uint64_t*)d_skey, (const uint32_t*)d_rstart, C, A.d_len, R, nq, A.min_common,
                     A.min_cont_q20, d_elig, d_qcnt);
  RTC_CHECK_LAUNCH(ctx);
  RTC_TRY(scan_u32(ctx, d_elig, d_eid, (size_t)C + 1, false));
  std::vector<uint32_t> h_qcnt(nq);
  RTC_HIP(ctx, hipMemcpyAsync(h_qcnt.data(), d_qcnt, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  std::vector<uint64_t> h_qeoff(nq + 1, 0);
  for (uint32_t q = 0; q < nq; q++) h_qeoff[q + 1] = h_qeoff[q] + h_qcnt[q];
  const uint32_t E = (uint32_t)h_qeoff[nq];
  ctx->rep_screen[1] += M;
  ctx->rep_screen[2] += C;
  ctx->rep_screen[3] += E;
  if (E == 0) { ctx->rep_screen[9] += now_ns() - t0; return RTC_OK; }
  // ---- the candidates compacted, the position view ----
  uint32_t *d_cslot = nullptr, *d_ccommon = nullptr, *d_cms = nullptr, *d_u = nullptr, *d_rank = nullptr, *d_unique = nullptr, *d_pcand = nullptr,
           *d_rounds = nullptr;
  uint64_t* d_qeoff = nullptr;
  rtc_screen_sum* d_sum = nullptr;
  RTC_TRY(db.get(ctx, E, &d_cslot));
  RTC_TRY(db.get(ctx, E, &d_ccommon));
  RTC_TRY(db.get(ctx, E, &d_cms));
  RTC_TRY(db.get(ctx, E, &d_u));
  RTC_TRY(db.get(ctx, E, &d_rank));
  RTC_TRY(db.get(ctx, E, &d_unique));
  RTC_TRY(db.get(ctx, M, &d_pcand));
  RTC_TRY(db.get(ctx, nq, &d_rounds));
  RTC_TRY(db.get(ctx, (size_t)nq + 1, &d_qeoff));
  RTC_TRY(db.get(ctx, nq, &d_sum));
  RTC_HIP(ctx, hipMemsetAsync(d_rank, 0, (size_t)E * 4, s));
  RTC_HIP(ctx, hipMemsetAsync(d_unique, 0, (size_t)E * 4, s));
  RTC_HIP(ctx, hipMemsetAsync(d_rounds, 0, (size_t)nq * 4, s));
  RTC_HIP(ctx, hipMemcpyAsync(d_qeoff, h_qeoff.data(), ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(screen_compact_kernel, dim3((C + 255) / 256), b256, 0, s, (const uint64_t*)d_skey, (const uint32_t*)d_rstart,
                     (const uint32_t*)d_elig, (const uint32_t*)d_eid, C, E, d_cslot, d_ccommon, d_cms, d_u);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(screen_view_kernel, gm, b256, 0, s, (const uint32_t*)d_cid1, (const uint32_t*)d_elig, (const uint32_t*)d_eid,
                     (const uint32_t*)d_spos, M32, C, P, (const uint64_t*)d_moff, d_pcur, d_pcand);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint64_t t1 = now_ns();
  ctx->rep_screen[9] += t1 - t0;
  // ---- gather: a launch per path that has a sample ----
  uint64_t n_path[3] = {0, 0, 0};
  const bool all_global = ctx->opt.screen_global != 0;
  for (uint32_t q = 0; q < nq; q++) {
    if (!h_qcnt[q]) continue;
    n_path[all_global || h_qcnt[q] > SCREEN_BLOCK_CANDS ? 2 : h_qcnt[q] > SCREEN_WAVE_CANDS ? 1 : 0]++;
  }
  GatherArgs G{d_qeoff, d_qoff, d_cms, d_ccommon, d_spos, d_moff, d_pcur, d_pcand, d_alive, d_u, d_rank, d_unique, d_sum, d_rounds,
               nq, 0, 0, A.min_unique, A.max_picks};
  if (n_path[0]) {
    G.lo = 1; G.hi = SCREEN_WAVE_CANDS;
    hipLaunchKernelGGL((screen_gather_kernel<64, true, SCREEN_WAVE_CANDS>), dim3(nq), dim3(64), 0, s, G);
    RTC_CHECK_LAUNCH(ctx);
  }
  if (n_path[1]) {
    G.lo = SCREEN_WAVE_CANDS + 1; G.hi = SCREEN_BLOCK_CANDS;
    hipLaunchKernelGGL((screen_gather_kernel<256, true, SCREEN_BLOCK_CANDS>), dim3(nq), dim3(256), 0, s, G);
    RTC_CHECK_LAUNCH(ctx);
  }
  if (n_path[2]) {
    G.lo = all_global ? 1 : SCREEN_BLOCK_CANDS + 1; G.hi = 0xffffffffu;
    hipLaunchKernelGGL((screen_gather_kernel<256, false, 1>), dim3(nq), dim3(256), 0, s, G);
    RTC_CHECK_LAUNCH(ctx);
  }
  std::vector<uint32_t> h_cslot(E), h_ccommon(E), h_rank(E), h_unique(E), h_rounds(nq);
  std::vector<rtc_screen_sum> h_sum(nq);
  RTC_HIP(ctx, hipMemcpyAsync(h_cslot.data(), d_cslot, (size_t)E * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(h_ccommon.data(), d_ccommon, (size_t)E * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(h_rank.data(), d_rank, (size_t)E * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(h_unique.data(), d_unique, (size_t)E * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(h_rounds.data(), d_rounds, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(h_sum.data(), d_sum, (size_t)nq * sizeof(rtc_screen_sum), hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  for (uint32_t q = 0; q < nq; q++) {
    if (!h_qcnt[q]) continue;
    sum[q] = h_sum[q];
    sum[q].n_hashes = h_len[row0 + q];
    ctx->rep_screen[4] += h_sum[q].n_picks;
    ctx->rep_screen[5] = std::max<uint64_t>(ctx->rep_screen[5], h_rounds[q]);
    const size_t base = out.size();
    for (uint64_t e = h_qeoff[q]; e < h_qeoff[q + 1]; e++)
      out.push_back(rtc_screen_hit{q0 + q, h_cslot[e], h_ccommon[e], h_len[h_cslot[e]], h_unique[e], h_rank[e]});
    std::sort(out.begin() + base, out.end(), hit_order);
  }
  for (int i = 0; i < 3; i++) ctx->rep_screen[6 + i] += n_path[i];
  ctx->rep_screen[10] += now_ns() - t1;
  return RTC_OK;
}

}  // namespace

extern "C" int rtc_rep_screen(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                              uint32_t n_reps, uint32_t n_queries, const uint8_t* h_live, uint32_t min_common, uint32_t min_cont_q20,
                              uint32_t min_unique, uint32_t max_picks, uint32_t query_chunk, rtc_screen_hit* h_hits, uint64_t cap,
                              uint64_t* n_hits, rtc_screen_sum* h_sum) {
  if (!ctx) return RTC_ERR_ARG;
  if (!n_hits || (width != 4 && width != 8) || min_unique == 0 || min_cont_q20 > (1u << 20) || (cap && !h_hits) ||
      (uint64_t)n_reps + n_queries >= 0x7fffffffull || (n_queries && !h_sum))
    return rtc_fail(ctx, RTC_ERR_ARG, "rtc_rep_screen: bad arguments");
  const uint64_t t_call = now_ns();
  *n_hits = 0;
  for (int i = 0; i < 12; i++) ctx->rep_screen[i] = 0;
  ctx->rep_screen_path = 0;
  if (n_queries == 0) return RTC_OK;
  if (!d_hashes || !d_start || !d_len) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_rep_screen: no sketches");
  const uint32_t n = n_reps + n_queries;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  for (uint32_t g = 0; g < n; g++)
    if (h_len[g] >= 0x80000000u) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "rtc_rep_screen: sketch %u has %u hashes, 2^31 or more", g, h_len[g]);
  // ---- the model index ----
  DevBuf db;
  std::vector<uint64_t> h_ioff(std::max<uint32_t>(n_reps, 1), 0);
  uint64_t K = 0;
  for (uint32_t g = 0; g < n_reps; g++) {
    h_ioff[g] = K;
    if (!h_live || h_live[g]) K += h_len[g];
  }
  uint64_t* d_ikey = nullptr;
  uint32_t* d_islot = nullptr;
  if (K) {
    uint8_t* d_live = nullptr;
    uint64_t *d_ioff = nullptr, *d_key0 = nullptr;
    uint32_t* d_slot0 = nullptr;
    if (h_live) {
      RTC_TRY(db.get(ctx, n_reps, &d_live));
      RTC_HIP(ctx, hipMemcpyAsync(d_live, h_live, n_reps, hipMemcpyHostToDevice, s));
    }
    RTC_TRY(db.get(ctx, n_reps, &d_ioff));
    RTC_TRY(db.get(ctx, K, &d_key0));
    RTC_TRY(db.get(ctx, K, &d_slot0));
    RTC_TRY(db.get(ctx, K, &d_ikey));
    RTC_TRY(db.get(ctx, K, &d_islot));
    RTC_HIP(ctx, hipMemcpyAsync(d_ioff, h_ioff.data(), (size_t)n_reps * 8, hipMemcpyHostToDevice, s));
    const dim3 g(std::max<uint32_t>(1, std::min<uint32_t>((n_reps + 3) / 4, (uint32_t)ctx->num_cu * 16))), b(256);
    if (width == 8)
      hipLaunchKernelGGL(screen_index_kernel<uint64_t>, g, b, 0, s, (const uint64_t*)d_hashes, d_start, d_len, (const uint8_t*)d_live,
                         (const uint64_t*)d_ioff, n_reps, d_key0, d_slot0);
    else
      hipLaunchKernelGGL(screen_index_kernel<uint32_t>, g, b, 0, s, (const uint32_t*)d_hashes, d_start, d_len, (const uint8_t*)d_live,
                         (const uint64_t*)d_ioff, n_reps, d_key0, d_slot0);
    RTC_CHECK_LAUNCH(ctx);
    RTC_TRY(rtc_sort_u64_pairs(ctx, d_key0, d_ikey, d_slot0, d_islot, K));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    db.release(d_key0); db.release(d_slot0);
  }
  ctx->rep_screen[9] += now_ns() - t_call;
  ScreenArgs A{d_hashes, width, d_start, d_len, n_reps, min_common, min_cont_q20, min_unique, max_picks, d_ikey, d_islot, K};
  std::vector<rtc_screen_hit> all;
  std::vector<rtc_screen_sum> sums(n_queries);
  size_t had = 0;
  uint64_t before[12];
  const int st = for_query_chunks(
      ctx, n_queries, query_chunk,
      [&](uint32_t q0, uint32_t q1) {
        had = all.size();
        std::copy(ctx->rep_screen, ctx->rep_screen + 12, before);
        return rep_screen_chunk(ctx, A, h_len, q0, q1, all, sums.data() + q0);
      },
      [&](uint32_t, uint32_t) {
        all.resize(had);
        std::copy(before, before + 12, ctx->rep_screen);
      },
      &ctx->rep_screen[0]);
  if (st != RTC_OK) return st;
  ctx->rep_screen_path = (ctx->rep_screen[6] ? 1 : 0) | (ctx->rep_screen[7] ? 2 : 0) | (ctx->rep_screen[8] ? 4 : 0);
  *n_hits = all.size();
  std::copy(sums.begin(), sums.end(), h_sum);
  if (h_hits && cap) std::copy(all.begin(), all.begin() + std::min<uint64_t>(cap, all.size()), h_hits);
  ctx->rep_screen[11] = now_ns() - t_call;
  return RTC_OK;
}

extern "C" int rtc_rep_screen_counters(const rtc_ctx* ctx, uint64_t out[12]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 12; i++) out[i] = ctx->rep_screen[i];
  return RTC_OK;
}

extern "C" int rtc_rep_screen_last_path(const rtc_ctx* ctx) { return ctx ? ctx->rep_screen_path : 0; }

extern "C" double rtc_screen_identity(uint32_t common, uint32_t size, int kmer_size) {
  if (common == size) return 1.0;
  if (common == 0) return 0.0;
  return pow((double)common / (double)size, 1.0 / (double)kmer_size);
}
