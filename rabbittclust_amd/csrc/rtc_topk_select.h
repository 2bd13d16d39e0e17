// rtc_topk_select.h -- a query's candidates as a segment of records under an exact rational key: the record, its total order, the
// per-query count of the join's candidates and the one-workgroup scan of the segment offsets (both run from rtc_query_chunks.h
// for the placement entry points, the scan also by rtc_dbscan_sweep.hip for the k-th nearest candidate of a point), the running
// top-k selection in LDS of rtc_rep_topk.hip and rtc_dbscan_sweep.hip (one wave for segments of up to TK_LONG records, 256 lanes
// for the longer ones) and the segment fold of rtc_dbscan_assign.hip and rtc_leiden_assign.hip.
#pragma once
#include <type_traits>

#include "rtc_internal.h"

namespace {

constexpr uint32_t TK_KMAX = 256;        // largest topk of the select path
constexpr uint32_t TK_LONG = 4096;       // segments longer than this take the 256-lane workgroup
constexpr uint32_t TK_SCAN_THREADS = 1024;

struct TkRec { uint32_t slot, common, denom, pad; };

// a ranks before b
__device__ __forceinline__ bool tk_beats(const TkRec& a, const TkRec& b) {
  const uint64_t l = (uint64_t)a.common * b.denom, r = (uint64_t)b.common * a.denom;
  return l != r ? l > r : a.slot < b.slot;
}
static bool tk_beats_host(const TkRec& a, const TkRec& b) {
  const uint64_t l = (uint64_t)a.common * b.denom, r = (uint64_t)b.common * a.denom;
  return l != r ? l > r : a.slot < b.slot;
}

// a lane per candidate (row0 + q, slot, common) of the join: cnt[q] += 1 for the live slots below n_reps (live == NULL: all)
__global__ __launch_bounds__(256) void tk_count_kernel(const rtc_cedge* __restrict__ e, uint64_t m, uint32_t row0, uint32_t nq,
                                                       uint32_t n_reps, const uint8_t* __restrict__ live, uint32_t* __restrict__ cnt) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const rtc_cedge c = e[a];
  const uint32_t q = c.i - row0;
  if (q >= nq || c.j >= n_reps || (live && !live[c.j])) return;
  atomicAdd(&cnt[q], 1u);
}

// one workgroup of TK_SCAN_THREADS: off[q] = sum of cnt[0 .. q), koff[q] = sum of min(cnt, k) (k == 0: cnt); off[nq], koff[nq]: totals
__global__ __launch_bounds__(TK_SCAN_THREADS) void tk_scan_kernel(const uint32_t* __restrict__ cnt, uint32_t nq, uint32_t k,
                                                                  uint64_t* __restrict__ off, uint64_t* __restrict__ koff) {
  __shared__ uint64_t sa[TK_SCAN_THREADS], sb[TK_SCAN_THREADS];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nq + TK_SCAN_THREADS - 1) / TK_SCAN_THREADS;
  const uint32_t b0 = (uint32_t)min((uint64_t)nq, (uint64_t)t * per), b1 = (uint32_t)min((uint64_t)nq, (uint64_t)b0 + per);
  uint64_t a = 0, b = 0;
  for (uint32_t i = b0; i < b1; i++) { const uint32_t c = cnt[i]; a += c; b += (k && c > k) ? k : c; }
  sa[t] = a; sb[t] = b;
  __syncthreads();
  for (uint32_t d = 1; d < TK_SCAN_THREADS; d <<= 1) {
    const uint64_t va = t >= d ? sa[t - d] : 0, vb = t >= d ? sb[t - d] : 0;
    __syncthreads();
    sa[t] += va; sb[t] += vb;
    __syncthreads();
  }
  uint64_t xa = sa[t] - a, xb = sb[t] - b;
  for (uint32_t i = b0; i < b1; i++) {
    const uint32_t c = cnt[i];
    off[i] = xa; koff[i] = xb;
    xa += c; xb += (k && c > k) ? k : c;
  }
  if (t == TK_SCAN_THREADS - 1) { off[nq] = sa[t]; koff[nq] = sb[t]; }
}

// A workgroup of B lanes folds the segment [s0, s1) into one F: every lane strides over the segment and takes its records
// (f.take(record, args...)), __shfl_xor steps merge the lanes of a wave word by word (f.merge(other)), and the waves of a
// 256-lane workgroup meet through lds_part (B / 64 entries) behind one barrier.  The result is thread 0's.  merge must not
// depend on the order of its operands -- sums, min, max, the best record under tk_beats, which is a total order -- so the result
// is the same for every order the scatter left the records in.  Every lane of the workgroup calls it.
template <int B, class F, class... A>
__device__ __forceinline__ F tk_fold_segment(const TkRec* __restrict__ seg, uint64_t s0, uint64_t s1, F f, F* lds_part, A... args) {
  static_assert(sizeof(F) % 4 == 0 && std::is_trivially_copyable<F>::value, "the lanes exchange F as 32-bit words");
  constexpr int W = sizeof(F) / 4;
  for (uint64_t idx = s0 + threadIdx.x; idx < s1; idx += B) f.take(seg[idx], args...);
  for (int d = 32; d; d >>= 1) {
    uint32_t w[W];
    __builtin_memcpy(w, &f, sizeof(F));
#pragma unroll
    for (int i = 0; i < W; i++) w[i] = __shfl_xor(w[i], d);
    F o;
    __builtin_memcpy(&o, w, sizeof(F));
    f.merge(o);
  }
  if (B > 64) {
    if ((threadIdx.x & 63) == 0) lds_part[threadIdx.x >> 6] = f;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < B / 64; w++) f.merge(lds_part[w]);
  }
  return f;
}

// a workgroup of B lanes per query whose segment length lies in [lo, hi]; k in [1, TK_KMAX]
template <int B>
__global__ __launch_bounds__(B) void tk_select_kernel(const TkRec* __restrict__ seg, const uint64_t* __restrict__ off,
                                                      const uint64_t* __restrict__ koff, uint32_t nq, uint32_t q0, uint32_t k,
                                                      uint32_t lo, uint32_t hi, rtc_rep_hit* __restrict__ out) {
  __shared__ TkRec top[2][TK_KMAX];
  __shared__ TkRec cand[B];
  __shared__ uint32_t ncand;
  const uint32_t q = blockIdx.x;
  if (q >= nq) return;
  const uint64_t s0 = off[q], s1 = off[q + 1];
  if (s1 - s0 < lo || s1 - s0 > hi) return;  // uniform across the workgroup
  uint32_t cnt = 0, cur = 0;
  for (uint64_t base = s0; base < s1; base += B) {
    const uint64_t idx = base + threadIdx.x;
    TkRec x = {0, 0, 1, 0};
    bool keep = false;
    if (idx < s1) { x = seg[idx]; keep = cnt < k || tk_beats(x, top[cur][cnt - 1]); }
    if (threadIdx.x == 0) ncand = 0;
    __syncthreads();
    if (keep) cand[atomicAdd(&ncand, 1u)] = x;
    __syncthreads();
    const uint32_t mm = ncand;
    if (mm == 0) continue;  // uniform; ncand stays 0 until every lane has read it
    const uint32_t nxt = cur ^ 1u;
    for (uint32_t t = threadIdx.x; t < cnt; t += B) {  // a record of the top-k: its rank there plus the survivors before it
      const TkRec y = top[cur][t];
      uint32_t r = t;
      for (uint32_t j = 0; j < mm; j++) r += tk_beats(cand[j], y) ? 1u : 0u;
      if (r < k) top[nxt][r] = y;
    }
    for (uint32_t t = threadIdx.x; t < mm; t += B) {  // a survivor: the top-k records before it (a prefix) plus the survivors
      const TkRec y = cand[t];
      uint32_t a = 0, b = cnt;
      while (a < b) { const uint32_t mid = (a + b) >> 1; if (tk_beats(top[cur][mid], y)) a = mid + 1; else b = mid; }
      uint32_t r = a;
      for (uint32_t j = 0; j < mm; j++) r += tk_beats(cand[j], y) ? 1u : 0u;
      if (r < k) top[nxt][r] = y;
    }
    __syncthreads();
    cnt = cnt + mm < k ? cnt + mm : k;
    cur = nxt;
  }
  const uint64_t o = koff[q];
  for (uint32_t t = threadIdx.x; t < cnt; t += B) {
    const TkRec y = top[cur][t];
    rtc_rep_hit h;
    h.query = q0 + q; h.slot = y.slot; h.common = y.common; h.denom = y.denom;
    out[o + t] = h;
  }
}

}  // namespace
