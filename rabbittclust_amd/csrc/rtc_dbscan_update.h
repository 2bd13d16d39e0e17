// rtc_dbscan_update.h -- what rtc_dbscan_update adds to dbscan_run (rtc_dbscan_sweep.hip; include/rtclust.h defines the rule,
// DESIGN 3.4g-update has the argument): the flags of the old rows that stage 2 measures again, the view that places those rows last
// among the old ones without copying a hash, the way back from the view's pairs to the original numbering, and the seeds that
// stand for every old core-core edge.  All of it is a few words per point; the cost of an update is its two joins.
#pragma once
#include "rtc_dbscan_common.h"

namespace {

// T: an old noise point (label < 0, so no core point) at the old end of a pair that stage 1 kept gains a neighbour.  Every pair
// of stage 1 has its new point in i; the old border points (B) are flagged by the host before.
__global__ __launch_bounds__(256) void upd_touch_kernel(const rtc_cedge* __restrict__ kept, uint64_t m, uint32_t n_old,
                                                        const int32_t* __restrict__ label_old, uint32_t* __restrict__ flag) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_cedge c = kept[e];
    if (c.common == 0) continue;
    if (c.j < n_old && c.i >= n_old && label_old[c.j] < 0) flag[c.j] = 1u;
    if (c.i < n_old && c.j >= n_old && label_old[c.i] < 0) flag[c.i] = 1u;
  }
}
// u64 KSSD sketches: the empty sketches are neighbours of each other without a candidate pair, so a new empty sketch touches
// every old empty one that is noise
__global__ __launch_bounds__(256) void upd_touch_empty_kernel(const uint32_t* __restrict__ len, uint32_t n_old,
                                                              const int32_t* __restrict__ label_old, uint32_t* __restrict__ flag) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n_old; v += gridDim.x * blockDim.x)
    if (len[v] == 0 && label_old[v] < 0) flag[v] = 1u;
}
// The view: the old rows in their order, the flagged ones (pos: the exclusive scan of the flags, k of them) after the others.
// perm[row of the view] = original row; vstart / vlen address the same hash buffer.
__global__ __launch_bounds__(256) void upd_view_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint32_t n_old,
                                                       uint32_t k, const uint64_t* __restrict__ start, const uint32_t* __restrict__ len,
                                                       uint64_t* __restrict__ vstart, uint32_t* __restrict__ vlen, uint32_t* __restrict__ perm) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n_old; v += gridDim.x * blockDim.x) {
    const uint32_t p = pos[v];                                   // flagged rows below v: p <= v, p <= k
    const uint32_t at = flag[v] ? (n_old - k) + p : v - p;       // < n_old either way
    vstart[at] = start[v];
    vlen[at] = len[v];
    perm[at] = v;
  }
}
// a chunk's pairs of the view in the original numbering, the larger index in i as the pair phase leaves them
__global__ __launch_bounds__(256) void upd_unview_kernel(rtc_cedge* __restrict__ cand, uint64_t m, uint32_t n_view,
                                                         const uint32_t* __restrict__ perm) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    rtc_cedge c = cand[e];
    if (c.i >= n_view || c.j >= n_view) continue;  // (the pair phase emits rows and columns of the view only)
    const uint32_t a = perm[c.i], b = perm[c.j];
    c.i = a > b ? a : b;
    c.j = a > b ? b : a;
    cand[e] = c;
  }
}
// tab[c] = the smallest core index of old cluster c (tab starts at ~0u)
__global__ __launch_bounds__(256) void upd_seed_min_kernel(const int32_t* __restrict__ label_old, const uint8_t* __restrict__ core_old,
                                                           uint32_t n_old, uint32_t n_clusters, uint32_t* __restrict__ tab) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n_old; v += gridDim.x * blockDim.x) {
    const int32_t l = label_old[v];
    if (core_old[v] && l >= 0 && (uint32_t)l < n_clusters) atomicMin(&tab[l], v);
  }
}
// the seeds, after core_init_kernel: every old core point hangs under its old cluster's smallest core index (<= its own, so
// parent[v] <= v still holds) and is a core point whatever its count over the measured rows says
__global__ __launch_bounds__(256) void upd_seed_kernel(const int32_t* __restrict__ label_old, const uint8_t* __restrict__ core_old,
                                                       uint32_t n_old, uint32_t n_clusters, const uint32_t* __restrict__ tab,
                                                       uint32_t* __restrict__ coremask, uint32_t* __restrict__ parent) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n_old; v += gridDim.x * blockDim.x) {
    const int32_t l = label_old[v];
    if (!core_old[v] || l < 0 || (uint32_t)l >= n_clusters) continue;
    const uint32_t r = tab[l];
    coremask[v] = 1u;
    parent[v] = r <= v ? r : v;
  }
}

}  // namespace
