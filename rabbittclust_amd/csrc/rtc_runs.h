// rtc_runs.h -- lookups in the run list of the 2-bit staging format, shared by the units that sketch from packed bases
// (rtc_sketch_minhash_packed.hip, rtc_sketch_kssd.hip).  The list holds (start, length) pairs of everything outside
// ACGT, ascending and disjoint (include/rtclust.h), so the runs' ends ascend with their starts.
#pragma once
#include "rtc_internal.h"

namespace {

// the first run of [lo, hi) that ends behind x (start + length > x); hi if there is none
__device__ __forceinline__ uint32_t first_run_ending_after(const uint64_t* __restrict__ runs, uint32_t lo, uint32_t hi, int64_t x) {
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((int64_t)(runs[2 * (uint64_t)mid] + runs[2 * (uint64_t)mid + 1]) <= x) lo = mid + 1; else hi = mid; }
  return lo;
}
// the first run of [lo, hi) that starts at or behind x; hi if there is none
__device__ __forceinline__ uint32_t first_run_starting_from(const uint64_t* __restrict__ runs, uint32_t lo, uint32_t hi, int64_t x) {
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((int64_t)runs[2 * (uint64_t)mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}

// per segment (any type with s_begin / s_end: the k-mer END positions it owns), the runs [x, y) that can touch a k-mer
// it owns: the first run that ends behind s_begin - (k - 1) and the first that starts at or behind s_end -- none for
// most segments of a finished genome
template <class Seg>
__global__ __launch_bounds__(256) void seg_runs_kernel(const Seg* __restrict__ segs, uint32_t nseg, const uint64_t* __restrict__ runs,
                                                       uint32_t n_runs, int k, uint2* __restrict__ seg_runs) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t x = first_run_ending_after(runs, 0, n_runs, (int64_t)segs[s].s_begin - (k - 1));
  seg_runs[s] = make_uint2(x, first_run_starting_from(runs, x, n_runs, (int64_t)segs[s].s_end));
}

}  // namespace
