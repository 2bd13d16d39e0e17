// rtc_dbscan_mash.h -- clust-dbscan --minhash: the neighbour predicate of MinHashDBSCAN (findNeighborsMinHash, src/dbscan.cpp:685-720
// in the reference tree: dist <= eps with MinHash::distance()) for rtc_dbscan_sweep.hip, whose pair phase and level engine
// (dbscan_run) it shares.  The distance is Mash's union-truncated estimator as this project restates it
// (rtc_mash_merge.h; parity-unpinned against RabbitSketch like rtc_mst_mash).  The device forms no distance:
//   * mash_tables: for every level e and every denom d the host finds cmin[e][d], the least common whose distance -- by the very
//     function that defines it, rtc_mash_distance_host -- is <= eps_e (d + 1 where none is).  On the device the predicate is
//     common >= cmin[e][denom], one mask bit per level.
//   * the prefilter: the pair phase's full-set common bounds the truncated one from above and the truncated denom is at least
//     d0 = min(sketch_size, max(|a|, |b|)); a candidate whose full common is below min over d >= d0 of cmin[e][d] at every
//     level is dropped without a merge (smin, the suffix minima of cmin over the d where some common passes).
//   * mash_edges_kernel: the truncated (common, denom) of 64 candidates per wave.  Cooperative: the wave takes one candidate at
//     a time, stages the second list into LDS with coalesced loads and walks the first in coalesced chunks of 64,
//     every lane ranking its element in the second list by binary search; a ballot's prefix count gives every element its place
//     in the union, which decides whether it lies among the first sketch_size.  Serial (RTC_DBSCAN_MASH_SERIAL=1): every lane
//     merges its own candidate with rtc_mash_merge, the baseline.  Either way lane k then holds candidate k's counts and the
//     epilogue is lane-parallel: the counts go to the caller (rtc_pair_mash_edges_dev) or through the tables into the kept list.
// rtc_graph_build_mash (rtc_graph.hip) runs the same candidates through the same merge with one strict table
// (mash_tables<true>) and an epilogue of its own: the kept record is a rtc_medge, which carries both counts.
#pragma once
#include <type_traits>

#include "rtc_dbscan_common.h"
#include "rtc_mash_merge.h"

// rtc_mst.hip: host_mst_distance in mode 2 for a given (common, denom), denom <= sketch_size
double rtc_mash_distance_host(uint32_t common, uint32_t denom, uint32_t sketch_size, int kmer_size);

namespace {

constexpr uint32_t MASH_LDS_ELEMS = 1024;  // the second list is staged in LDS up to this length (8 KiB of u64 per wave)

// What rtc_graph_build_mash keeps of a passing pair (i > j): the truncated counts, both of them -- the rank and the weight need
// the denom, and rtc_cedge has no room for it
struct rtc_medge { uint32_t i, j, common, denom; };

// cmin[0 .. D] for one eps: least common with distance(common, d) <= eps, d + 1 where there is none.  For a fixed d the
// distance does not increase with common: j = common / d grows by a relative step of at least 1 / common, far above the
// rounding of 2j / (1 + j), and the C library's log is monotone.  pass(0) is false (distance 1 > eps) and pass(d) true
// (distance 0), so the bisection keeps lo failing and hi passing: both sides of the boundary have been evaluated when it ends.
// STRICT: distance < eps, the edge rule of rtc_graph_build_mash, for 0 < eps <= 1: pass(0) is false (1 < eps never) and pass(d)
// true (0 < eps), and the argument is the same.
template <bool STRICT = false>
inline void mash_cmin_row(uint32_t D, uint32_t sketch_size, int kmer_size, double eps, uint32_t* row) {
  row[0] = 1;  // denom 0: two empty lists, j = 0, distance 1
  for (uint32_t d = 1; d <= D; d++) {
    uint32_t lo = 0, hi = d;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      const double dist = rtc_mash_distance_host(mid, d, sketch_size, kmer_size);
      if (STRICT ? dist < eps : dist <= eps) hi = mid; else lo = mid;
    }
    row[d] = hi;
  }
}

// What dbscan_run needs of a MinHash call: the tables on the device and the switches
struct MashTables {
  uint32_t D = 0;            // the largest denom the call can meet: min(sketch_size, 2 * the longest list)
  uint32_t* d_cmin = nullptr;  // [L][D + 1]
  uint32_t* d_smin = nullptr;  // [L][D + 1]: min of cmin[e][d'] over d' >= d with cmin[e][d'] <= d', 0xffffffff where none
};

struct MashParams {
  const uint32_t* cmin;  // null: no predicate, the counts go to common_out / denom_out
  const uint32_t* smin;  // null: no prefilter
  uint32_t D, n_lv;
};

// the cooperative truncated merge of one pair by one wave; every lane returns the pair's (common, denom).  sb: this wave's
// MASH_LDS_ELEMS elements of LDS.  Only a[0 .. min(na, s)) and b[0 .. min(nb, s)) can lie among the first s of the union.
template <typename T>
__device__ __forceinline__ void mash_merge_wave(const T* __restrict__ a, uint32_t na, const T* __restrict__ b, uint32_t nb, uint32_t s,
                                                T* sb, uint32_t lane, uint32_t* common, uint32_t* denom) {
  const uint32_t nap = na < s ? na : s, nbp = nb < s ? nb : s;
  const bool staged = nbp <= MASH_LDS_ELEMS;
  __syncthreads();  // the candidate before is done with sb (one wave per block)
  if (staged)
    for (uint32_t x = lane; x < nbp; x += 64) sb[x] = b[x];
  __syncthreads();
  uint32_t c = 0, matched = 0, lo0 = 0;
  for (uint32_t base = 0; base < nap; base += 64) {  // uniform
    const uint32_t i = base + lane;
    const bool valid = i < nap;
    T va = 0;
    if (valid) va = a[i];
    // r = the elements of b below va; the chunk before left lo0 of them below its last element
    uint32_t lo = valid ? lo0 : nbp, hi = nbp;
    bool m = false;
    if (staged) {
      while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (sb[mid] < va) lo = mid + 1; else hi = mid; }
      m = valid && lo < nbp && sb[lo] == va;
    } else {
      while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (b[mid] < va) lo = mid + 1; else hi = mid; }
      m = valid && lo < nbp && b[lo] == va;
    }
    const uint64_t bal = __ballot(m);
    const uint32_t before = matched + (uint32_t)__popcll(bal & ((1ULL << lane) - 1ULL));
    const uint64_t at = (uint64_t)i + lo - before;  // va's place in the union, from 0
    c += (uint32_t)__popcll(__ballot(m && at < s));
    matched += (uint32_t)__popcll(bal);
    const uint32_t last = nap - base < 64 ? nap - base - 1 : 63;
    lo0 = __shfl(lo, last);
    if (__shfl((uint32_t)(at >= s), last)) break;  // the places only grow: nothing further lies among the first s
  }
  // the union holds nap + nbp - (all matches) elements; a walk that stopped early has passed place s, and then so has the sum
  const uint64_t u = (uint64_t)nap + nbp - matched;
  *common = c;
  *denom = u < s ? (uint32_t)u : s;
}

// One wave per block, 64 candidates per wave and round.  cnt[0]: pairs kept (wave_append), cnt[1]: candidates merged.  R: the
// kept record -- rtc_cedge with the levels' mask in `common` (rtc_dbscan_mash), or rtc_medge with the counts themselves
// (rtc_graph_build_mash: one level).
template <typename T, bool SERIAL, class R>
__global__ __launch_bounds__(64) void mash_edges_kernel(const T* __restrict__ hashes, const uint64_t* __restrict__ start,
                                                        const uint32_t* __restrict__ len, uint32_t sketch_size,
                                                        const rtc_cedge* __restrict__ cand, uint64_t m, MashParams P,
                                                        uint32_t* __restrict__ common_out, uint32_t* __restrict__ denom_out,
                                                        R* __restrict__ kept, uint64_t cap, unsigned long long* __restrict__ cnt) {
  __shared__ T sb[MASH_LDS_ELEMS];
  const uint32_t lane = threadIdx.x;
  for (uint64_t base = (uint64_t)blockIdx.x * 64; base < m; base += (uint64_t)gridDim.x * 64) {  // uniform
    const uint64_t e = base + lane;
    rtc_cedge c{0, 0, 0};
    uint32_t na = 0, nb = 0;
    bool merge = false;
    if (e < m) {
      c = cand[e];
      na = len[c.i]; nb = len[c.j];
      merge = true;
      if (P.smin) {  // the prefilter: at some level the full common reaches the least cmin of any denom this pair can have
        const uint32_t big = na > nb ? na : nb, d0 = big < P.D ? big : P.D;
        merge = false;
        for (uint32_t l = 0; l < P.n_lv; l++) merge |= c.common >= P.smin[(uint64_t)l * (P.D + 1) + d0];
      }
    }
    uint32_t common = 0, denom = 0;
    const uint64_t todo = __ballot(merge);
    if constexpr (SERIAL) {
      if (merge) rtc_mash_merge(hashes + start[c.i], na, hashes + start[c.j], nb, sketch_size, &common, &denom);
    } else {
      for (uint64_t t = todo; t; t &= t - 1) {  // uniform
        const uint32_t k = (uint32_t)__builtin_ctzll(t);
        const uint32_t ki = __shfl(c.i, k), kj = __shfl(c.j, k);
        uint32_t kc, kd;
        mash_merge_wave(hashes + start[ki], __shfl(na, k), hashes + start[kj], __shfl(nb, k), sketch_size, sb, lane, &kc, &kd);
        if (lane == k) { common = kc; denom = kd; }
      }
    }
    if (!P.cmin) {
      if (e < m) { common_out[e] = common; denom_out[e] = denom; }
      continue;
    }
    if (lane == 0 && todo) atomicAdd(&cnt[1], (unsigned long long)__popcll(todo));
    if constexpr (std::is_same<R, rtc_medge>::value) {
      bool keep = false;
      if (merge) keep = common >= P.cmin[denom < P.D ? denom : P.D];  // denom <= D by construction; cmin >= 1: a shared hash among the first s
      wave_append(keep, rtc_medge{c.i, c.j, common, denom}, kept, cap, &cnt[0]);
    } else {
      uint32_t mask = 0;
      if (merge) {
        const uint32_t d = denom < P.D ? denom : P.D;  // denom <= D by construction
        for (uint32_t l = 0; l < P.n_lv; l++)
          if (common >= P.cmin[(uint64_t)l * (P.D + 1) + d]) mask |= 1u << l;
      }
      c.common = mask;
      wave_append(mask != 0, c, kept, cap, &cnt[0]);
    }
  }
}

inline uint32_t mash_blocks(uint64_t m, int num_cu) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((m + 63) / 64, (uint64_t)num_cu * 64));
}

template <bool SERIAL, class R>
void mash_edges_launch(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t sketch_size,
                       const rtc_cedge* d_cand, uint64_t m, const MashParams& P, uint32_t* d_common, uint32_t* d_denom, R* d_kept,
                       uint64_t cap, unsigned long long* d_cnt) {
  const dim3 g(mash_blocks(m, ctx->num_cu)), b(64);
  if (width == 8)
    hipLaunchKernelGGL((mash_edges_kernel<uint64_t, SERIAL, R>), g, b, 0, ctx->stream, (const uint64_t*)d_hashes, d_start, d_len, sketch_size, d_cand, m, P,
                       d_common, d_denom, d_kept, cap, d_cnt);
  else
    hipLaunchKernelGGL((mash_edges_kernel<uint32_t, SERIAL, R>), g, b, 0, ctx->stream, (const uint32_t*)d_hashes, d_start, d_len, sketch_size, d_cand, m, P,
                       d_common, d_denom, d_kept, cap, d_cnt);
}

// cmin and smin for the levels of a call, on the device (STRICT: mash_cmin_row's)
template <bool STRICT = false>
int mash_tables(rtc_ctx* ctx, DevBuf& db, uint32_t sketch_size, uint32_t max_len, int kmer_size, const double* h_eps, uint32_t n_eps,
                MashTables* T) {
  T->D = (uint32_t)std::min<uint64_t>(sketch_size, 2ull * max_len);
  const size_t W = (size_t)T->D + 1;
  std::vector<uint32_t> cmin(W * n_eps), smin(W * n_eps);
  for (uint32_t e = 0; e < n_eps; e++) {
    uint32_t* row = cmin.data() + W * e;
    mash_cmin_row<STRICT>(T->D, sketch_size, kmer_size, h_eps[e], row);
    uint32_t best = 0xffffffffu;
    for (size_t d = W; d-- > 0;) {
      if (row[d] <= d) best = std::min(best, row[d]);
      smin[W * e + d] = best;
    }
  }
  RTC_TRY(db.get(ctx, cmin.size(), &T->d_cmin));
  RTC_TRY(db.get(ctx, smin.size(), &T->d_smin));
  RTC_HIP(ctx, hipMemcpyAsync(T->d_cmin, cmin.data(), cmin.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  RTC_HIP(ctx, hipMemcpyAsync(T->d_smin, smin.data(), smin.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the host vectors go away
  return RTC_OK;
}

// One chunk of candidates through the predicate into the kept list: filter_chunk's protocol (the list grown first to hold the
// whole chunk, one launch) with the recount in the filter's place.  d_fc: cnt[0..1] of mash_edges_kernel.
template <class R>
int mash_filter_chunk(rtc_ctx* ctx, DevBuf& db, const char* who, const void* d_hashes, int width, const uint64_t* d_start,
                      const uint32_t* d_len, uint32_t sketch_size, const rtc_cedge* d_cand, uint64_t m, const MashTables& T, uint32_t n_lv,
                      unsigned long long* d_fc, KeptListOf<R>* L, uint64_t* merged) {
  hipStream_t s = ctx->stream;
  const uint64_t t0 = now_ns();
  RTC_TRY(kept_reserve(ctx, db, L, L->used + m));
  unsigned long long fc[2] = {(unsigned long long)L->used, 0ull};
  RTC_HIP(ctx, hipMemcpyAsync(d_fc, fc, sizeof fc, hipMemcpyHostToDevice, s));
  const MashParams P{T.d_cmin, ctx->opt.dbscan_mash_noprefilter ? nullptr : T.d_smin, T.D, n_lv};
  if (ctx->opt.dbscan_mash_serial)
    mash_edges_launch<true>(ctx, d_hashes, width, d_start, d_len, sketch_size, d_cand, m, P, nullptr, nullptr, L->d, L->cap, d_fc);
  else
    mash_edges_launch<false>(ctx, d_hashes, width, d_start, d_len, sketch_size, d_cand, m, P, nullptr, nullptr, L->d, L->cap, d_fc);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipMemcpyAsync(fc, d_fc, sizeof fc, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  if (fc[0] > L->cap) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu pairs kept, room for %llu", who, fc[0], (unsigned long long)L->cap);
  L->used = fc[0];
  *merged += fc[1];
  L->ns += now_ns() - t0;
  return RTC_OK;
}

}  // namespace
