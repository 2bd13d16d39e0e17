// rtc_pangenome.hip -- clust-mst --pangenome: core and accessory hashes of the clusters (include/rtclust.h holds the definition,
// tests/refpangenome.py restates it, DESIGN 3.4u has the choices and the figures).
//
// One open-addressing table of (hash, count) slots per cluster, never more than half full (rtc_pan.h), and three steps over it:
// count every (member, hash) record in, sweep the slots into the cluster's histogram, look every member's hashes up again for
// the genomes' records.  The members are reached through the clustered genomes ordered by cluster: perm and, per cluster, the
// segment [m0, m1) of it; moff[x] is the number of records before member x.
//   pan_lds_kernel      a cluster a workgroup (one wave, or 256 lanes), table and histogram in LDS, the three steps in one turn:
//                       the count runs flat over the cluster's records, a lane finding its member by a search of moff, so a
//                       cluster of many short sketches keeps its lanes busy as one long sketch does; the look-up takes a
//                       member a wave
//   pan_count_kernel    the arena: device-wide, a member a wave over all arena clusters of the group at once
//   pan_sweep_kernel    the arena: device-wide over tiles of 256 slots, a workgroup a contiguous run of tiles; occ == 1 and
//                       occ == m -- the two counts almost every slot has -- stay in registers and the other counts up to 1 025
//                       in bins in LDS until the workgroup leaves the cluster; larger ones leave in one add per distinct value
//                       and wave
//   pan_genome_kernel   the arena: a member a wave, shuffle reduction
// Integer atomics only (compare-and-swap on the key, add on the count and the histogram): nothing depends on the order.  The
// class counts of a cluster are sums over its histogram and are formed on the host.
#include <thread>

#include "rtc_dbscan_common.h"
#include "rtc_pan.h"

namespace {

constexpr uint32_t PAN_NONE = 0xFFFFFFFFu;

struct PanDesc {     // a cluster of the group
  uint64_t tab_off;  // its table's first slot in the arena (arena path)
  uint32_t m0, m1;   // its members in the group's permutation
  uint32_t log2;     // its table has 1 << log2 slots (arena path)
  uint32_t pad;
};

__device__ __forceinline__ uint64_t pan_load(const void* __restrict__ hashes, int width, uint64_t at) {
  return width == 4 ? (uint64_t)((const uint32_t*)hashes)[at] : ((const uint64_t*)hashes)[at];
}
__device__ __forceinline__ uint64_t pan_slot(uint64_t h, uint32_t log2_slots) { return (h * PAN_MULT) >> (64 - log2_slots); }

// One more member holds h (never PAN_EMPTY).  The table is at most half full, so the probe meets h or an empty slot.
template <bool GLOBAL>
__device__ __forceinline__ void pan_insert(unsigned long long* keys, uint32_t* cnt, uint64_t h, uint32_t log2_slots) {
  const uint64_t mask = (1ull << log2_slots) - 1;
  for (uint64_t s = pan_slot(h, log2_slots);; s = (s + 1) & mask) {
    unsigned long long k = GLOBAL ? __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : keys[s];
    if (k == PAN_EMPTY) {
      k = atomicCAS(&keys[s], (unsigned long long)PAN_EMPTY, (unsigned long long)h);
      if (k == PAN_EMPTY) k = h;
    }
    if (k == h) { atomicAdd(&cnt[s], 1u); return; }
  }
}

// occ of h in a finished table; 0 if it is not there (it always is: the member counted it in)
__device__ __forceinline__ uint32_t pan_find(const unsigned long long* keys, const uint32_t* cnt, uint64_t h, uint32_t log2_slots) {
  const uint64_t mask = (1ull << log2_slots) - 1;
  for (uint64_t s = pan_slot(h, log2_slots);; s = (s + 1) & mask) {
    const unsigned long long k = keys[s];
    if (k == h) return cnt[s];
    if (k == PAN_EMPTY) return 0;
  }
}

// One wave: the record of member g of a cluster of m, over the cluster's finished table.  Lane 0 writes it.
__device__ __forceinline__ void pan_member(const unsigned long long* keys, const uint32_t* cnt, uint32_t ones, uint32_t log2_slots, uint32_t m,
                                           uint32_t soft_pct, uint32_t cloud_pct, const void* __restrict__ hashes, int width, uint64_t s0, uint32_t L,
                                           uint32_t lane, rtc_pan_genome* __restrict__ out) {
  uint32_t uq = 0, co = 0, so = 0, sh = 0, cl = 0;
  unsigned long long os = 0;
  for (uint32_t i = lane; i < L; i += 64) {
    const uint64_t h = pan_load(hashes, width, s0 + i);
    const uint32_t f = h == PAN_EMPTY ? ones : pan_find(keys, cnt, h, log2_slots);
    if (f == 0) continue;
    uq += f == 1;
    os += f;
    if (f == m) co++;
    else if (100ull * f >= (uint64_t)soft_pct * m) so++;
    else if (100ull * f < (uint64_t)cloud_pct * m) cl++;
    else sh++;
  }
  for (int o = 32; o > 0; o >>= 1) {
    uq += __shfl_xor(uq, o); co += __shfl_xor(co, o); so += __shfl_xor(so, o); sh += __shfl_xor(sh, o); cl += __shfl_xor(cl, o);
    os += __shfl_xor(os, o);
  }
  if (lane == 0) {
    rtc_pan_genome r;
    r.occ_sum = os; r.unique = uq; r.core = co; r.soft = so; r.shell = sh; r.cloud = cl; r.pad = 0;
    *out = r;
  }
}

// Cluster desc[list[it]] a turn: at most SLOTS / 2 records.  hist (zeroed before the launch) gets the cluster's m entries: from
// the LDS copy when m <= HIST, by adds otherwise.  A count above m can only come from a sketch that holds a hash twice, which
// the contract excludes; such a slot is left out of the histogram, never written past it.
template <int BLOCK, uint32_t SLOTS, uint32_t HIST>
__global__ __launch_bounds__(BLOCK) void pan_lds_kernel(const uint32_t* __restrict__ list, uint32_t n_list, const PanDesc* __restrict__ desc,
                                                        const uint32_t* __restrict__ perm, const uint64_t* __restrict__ moff,
                                                        const void* __restrict__ hashes, int width, const uint64_t* __restrict__ start,
                                                        const uint32_t* __restrict__ len, uint32_t soft_pct, uint32_t cloud_pct,
                                                        unsigned long long* hist, rtc_pan_genome* __restrict__ gen) {
  __shared__ unsigned long long s_keys[SLOTS];
  __shared__ uint32_t s_cnt[SLOTS];
  __shared__ uint32_t s_hist[HIST];
  __shared__ uint32_t s_ones;
  constexpr uint32_t LOG2 = 31 - __builtin_clz(SLOTS);
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  for (uint32_t it = blockIdx.x; it < n_list; it += gridDim.x) {  // uniform over the workgroup: the barriers below are reached by all
    const PanDesc d = desc[list[it]];
    const uint32_t m = d.m1 - d.m0;
    const bool lh = m <= HIST;
    for (uint32_t s = tid; s < SLOTS; s += BLOCK) { s_keys[s] = PAN_EMPTY; s_cnt[s] = 0u; }
    if (lh) for (uint32_t f = tid; f < m; f += BLOCK) s_hist[f] = 0u;
    if (tid == 0) s_ones = 0u;
    __syncthreads();
    // ---- count: flat over the records; record R belongs to the last member x with moff[x] <= R ----
    const uint64_t R0 = moff[d.m0];
    uint64_t K = moff[d.m1] - R0;
    K = K < SLOTS / 2 ? K : SLOTS / 2;  // the host sends nothing larger
    for (uint64_t r = tid; r < K; r += BLOCK) {
      const uint64_t R = R0 + r;
      uint32_t lo = d.m0, hi = d.m1;  // moff[lo] <= R < moff[hi]
      while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (moff[mid] <= R) lo = mid; else hi = mid;
      }
      const uint64_t h = pan_load(hashes, width, start[perm[lo]] + (R - moff[lo]));
      if (h == PAN_EMPTY) atomicAdd(&s_ones, 1u);
      else pan_insert<false>(s_keys, s_cnt, h, LOG2);
    }
    __syncthreads();
    // ---- sweep: the slots and the all-ones word ----
    for (uint32_t s = tid; s < SLOTS + 1; s += BLOCK) {
      const uint32_t f = s < SLOTS ? s_cnt[s] : s_ones;
      if (f == 0 || f > m) continue;
      if (lh) atomicAdd(&s_hist[f - 1], 1u);
      else atomicAdd(&hist[d.m0 + f - 1], 1ull);
    }
    // ---- look-up: a member a wave; the table is only read from here on ----
    const uint32_t ones = s_ones;
    for (uint32_t x = d.m0 + tid / 64; x < d.m1; x += BLOCK / 64) {  // uniform per wave
      const uint32_t g = perm[x];
      pan_member(s_keys, s_cnt, ones, LOG2, m, soft_pct, cloud_pct, hashes, width, start[g], len[g], lane, &gen[x]);
    }
    __syncthreads();
    if (lh) for (uint32_t f = tid; f < m; f += BLOCK) hist[d.m0 + f] = (unsigned long long)s_hist[f];
    __syncthreads();  // the table and the histogram are written again in the next turn
  }
}

// mcl[x]: the place of member x's cluster in the arena list, PAN_NONE for a member of an LDS cluster.  A member a wave.
__global__ __launch_bounds__(256) void pan_count_kernel(const uint32_t* __restrict__ mcl, uint32_t M, const uint32_t* __restrict__ alist,
                                                        const PanDesc* __restrict__ desc, const uint32_t* __restrict__ perm,
                                                        const void* __restrict__ hashes, int width, const uint64_t* __restrict__ start,
                                                        const uint32_t* __restrict__ len, unsigned long long* keys, uint32_t* cnt, uint32_t* ones) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t x = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; x < M; x += waves) {  // uniform per wave
    const uint32_t a = mcl[x];
    if (a == PAN_NONE) continue;
    const PanDesc d = desc[alist[a]];
    const uint32_t g = perm[x];
    const uint64_t s0 = start[g];
    const uint32_t L = len[g];
    // Sketches ascend, so the members of a cluster hold a core hash at about the same place: waves that all started at their
    // sketch's head would meet on 64 addresses at a time.  Every wave starts at a place of its own and wraps.
    const uint32_t rot = L ? (uint32_t)(((uint64_t)x * 2654435761u) % L) : 0;
    for (uint32_t k = lane; k < L; k += 64) {
      const uint32_t i = k + rot < L ? k + rot : k + rot - L;
      const uint64_t h = pan_load(hashes, width, s0 + i);
      if (h == PAN_EMPTY) atomicAdd(&ones[a], 1u);
      else pan_insert<true>(keys + d.tab_off, cnt + d.tab_off, h, d.log2);
    }
  }
}

// One add per distinct value of f among the wave's lanes with `pend` (f >= 2): into the workgroup's bins while f - 2 fits them,
// into the histogram otherwise.  Every lane of the wave calls it.
__device__ __forceinline__ void pan_hist_add(uint32_t* bins, unsigned long long* hist, uint32_t f, bool pend, uint32_t lane) {
  uint64_t todo = __ballot(pend);
  while (todo) {  // uniform
    const uint32_t lead = (uint32_t)__ffsll((unsigned long long)todo) - 1;
    const uint32_t fl = __shfl(f, lead);
    const uint64_t same = __ballot(pend && f == fl);
    if (lane == lead) {
      if (fl - 2 < PAN_SWEEP_BINS) atomicAdd(&bins[fl - 2], (uint32_t)__popcll(same));
      else atomicAdd(&hist[fl - 1], (unsigned long long)__popcll(same));
    }
    todo &= ~same;
  }
}

// aoff[a]: the first slot of the a-th arena table, aoff[n_arena] the slots of all; every one a multiple of 256.  Workgroup b takes
// the tiles [tiles b / B, tiles (b + 1) / B).  The table's first tile also sweeps the cluster's all-ones word.  occ == 1 and
// occ == m are counted in registers and 2 <= occ < 2 + PAN_SWEEP_BINS in the workgroup's bins in LDS; both reach the histogram
// when the workgroup leaves the cluster.  (Straight to the histogram, one cluster of everything swept in 1.8 ms where 200 families
// of the same records took 0.04: a cluster's few common counts are few addresses.)
__global__ __launch_bounds__(256) void pan_sweep_kernel(const uint64_t* __restrict__ aoff, uint32_t n_arena, const uint32_t* __restrict__ alist,
                                                        const PanDesc* __restrict__ desc, const uint32_t* __restrict__ cnt,
                                                        const uint32_t* __restrict__ ones, unsigned long long* hist) {
  __shared__ uint32_t s_bins[PAN_SWEEP_BINS];
  __shared__ uint32_t s_acc[2];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  for (uint32_t b = tid; b < PAN_SWEEP_BINS; b += 256) s_bins[b] = 0u;
  if (tid < 2) s_acc[tid] = 0u;
  __syncthreads();
  const uint64_t tiles = aoff[n_arena] >> 8;
  const uint64_t t0 = tiles * blockIdx.x / gridDim.x, t1 = tiles * (blockIdx.x + 1) / gridDim.x;
  if (t0 >= t1) return;  // uniform
  uint32_t a = 0;
  {  // the table of tile t0: the last a with aoff[a] <= t0 << 8
    uint32_t lo = 0, hi = n_arena;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (aoff[mid] <= (t0 << 8)) lo = mid; else hi = mid;
    }
    a = lo;
  }
  PanDesc d = desc[alist[a]];
  uint32_t m = d.m1 - d.m0;
  uint32_t acc1 = 0, accm = 0;
  auto flush = [&]() {  // every lane of the workgroup
    for (int o = 32; o > 0; o >>= 1) { acc1 += __shfl_xor(acc1, o); accm += __shfl_xor(accm, o); }
    if (lane == 0) {
      if (acc1) atomicAdd(&s_acc[0], acc1);
      if (accm) atomicAdd(&s_acc[1], accm);
    }
    acc1 = accm = 0;
    __syncthreads();  // the bins and the two sums are complete
    if (tid < 2 && s_acc[tid]) {
      atomicAdd(&hist[tid == 0 ? d.m0 : d.m0 + m - 1], (unsigned long long)s_acc[tid]);
      s_acc[tid] = 0u;
    }
    for (uint32_t b = tid; b < PAN_SWEEP_BINS && b + 2 < m; b += 256) {  // a bin of f = b + 2 < m
      const uint32_t k = s_bins[b];
      if (k) { atomicAdd(&hist[d.m0 + b + 1], (unsigned long long)k); s_bins[b] = 0u; }
    }
    __syncthreads();
  };
  for (uint64_t t = t0; t < t1; t++) {  // uniform
    const uint64_t base = t << 8;
    while (a + 1 < n_arena && base >= aoff[a + 1]) {  // uniform
      flush();
      a++;
      d = desc[alist[a]];
      m = d.m1 - d.m0;
    }
    uint32_t f = cnt[base + tid];
    for (int turn = 0; turn < 2; turn++) {  // the slot, then (thread 0 of the table's first tile) the all-ones word
      if (f > m) f = 0;                     // rtc_pan.h: a contract breach is left out
      if (f == m) accm += 1;                // m == 1: f == 1 lands here
      else if (f == 1) acc1 += 1;
      pan_hist_add(s_bins, hist + d.m0, f, f > 1 && f != m, lane);
      if (base != aoff[a]) break;  // uniform
      f = tid == 0 ? ones[a] : 0u;
    }
  }
  flush();
}

__global__ __launch_bounds__(256) void pan_genome_kernel(const uint32_t* __restrict__ mcl, uint32_t M, const uint32_t* __restrict__ alist,
                                                         const PanDesc* __restrict__ desc, const uint32_t* __restrict__ perm,
                                                         const void* __restrict__ hashes, int width, const uint64_t* __restrict__ start,
                                                         const uint32_t* __restrict__ len, const unsigned long long* __restrict__ keys,
                                                         const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ ones, uint32_t soft_pct,
                                                         uint32_t cloud_pct, rtc_pan_genome* __restrict__ gen) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t x = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; x < M; x += waves) {  // uniform per wave
    const uint32_t a = mcl[x];
    if (a == PAN_NONE) continue;
    const PanDesc d = desc[alist[a]];
    const uint32_t g = perm[x];
    pan_member(keys + d.tab_off, cnt + d.tab_off, ones[a], d.log2, d.m1 - d.m0, soft_pct, cloud_pct, hashes, width, start[g], len[g], lane, &gen[x]);
  }
}

struct PanGroup { uint32_t c0, c1; uint64_t slots; };  // clusters [c0, c1) and the slots of their arena tables

}  // namespace

extern "C" int rtc_pangenome(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                             const int32_t* h_label, uint32_t soft_pct, uint32_t cloud_pct, rtc_pan* h_clusters, uint64_t* h_hist,
                             rtc_pan_genome* h_genomes, uint32_t* h_n_clusters) {
  const char* who = "rtc_pangenome";
  if (!ctx || !h_n_clusters || !h_clusters || (n && (!d_hashes || !d_start || !d_len || !h_label || !h_hist || !h_genomes)) || (width != 4 && width != 8))
    return RTC_ERR_ARG;
  memset(ctx->pan, 0, sizeof ctx->pan);
  memset(ctx->pan_phase, 0, sizeof ctx->pan_phase);
  ctx->pan_path = 0;
  *h_n_clusters = 0;
  if (!(1 <= cloud_pct && cloud_pct <= soft_pct && soft_pct <= 100))
    return rtc_fail(ctx, RTC_ERR_ARG, "%s: soft %u and cloud %u: 1 <= cloud <= soft <= 100 is needed", who, soft_pct, cloud_pct);
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u sketches", who, n);
  uint64_t* S = ctx->pan;
  const uint64_t t_begin = now_ns();
  if (n == 0) return RTC_OK;
  for (uint32_t g = 0; g < n; g++)
    if (h_label[g] >= 0 && (uint32_t)h_label[g] >= n) return rtc_fail(ctx, RTC_ERR_ARG, "%s: label %d of sketch %u with %u sketches", who, h_label[g], g, n);
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  for (uint32_t g = 0; g < n; g++)
    if (h_len[g] >= 0x80000000u) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: sketch %u has %u hashes, 2^31 or more", who, g, h_len[g]);

  // ---- clusters in order of their smallest member, members ascending; unclustered genomes are in none ----
  std::vector<uint32_t> cl(n, PAN_NONE), csize;
  {
    std::vector<uint32_t> number(n, PAN_NONE);
    for (uint32_t g = 0; g < n; g++) {
      if (h_label[g] < 0) continue;
      uint32_t& c = number[h_label[g]];
      if (c == PAN_NONE) { c = (uint32_t)csize.size(); csize.push_back(0); }
      cl[g] = c;
      csize[c]++;
    }
  }
  const uint32_t n_cl = (uint32_t)csize.size();
  std::vector<uint32_t> cfirst((size_t)n_cl + 1, 0);
  for (uint32_t c = 0; c < n_cl; c++) cfirst[c + 1] = cfirst[c] + csize[c];
  const uint32_t n_in = cfirst[n_cl];
  std::vector<uint32_t> perm(n_in);
  {
    std::vector<uint32_t> at(cfirst.begin(), cfirst.end() - 1);
    for (uint32_t g = 0; g < n; g++) if (cl[g] != PAN_NONE) perm[at[cl[g]]++] = g;
  }
  std::vector<uint64_t> moff((size_t)n_in + 1, 0);
  for (uint32_t x = 0; x < n_in; x++) moff[x + 1] = moff[x] + h_len[perm[x]];
  memset(h_hist, 0, (size_t)n * 8);
  memset(h_genomes, 0, (size_t)n * sizeof(rtc_pan_genome));
  *h_n_clusters = n_cl;
  S[0] = n_cl; S[1] = n_in; S[2] = moff[n_in];
  if (n_cl == 0) { S[9] = now_ns() - t_begin; return RTC_OK; }

  // ---- the path and the table of every cluster; groups in cluster order under the byte budget ----
  const bool all_global = ctx->opt.pan_global != 0;
  std::vector<uint8_t> path(n_cl), lg2(n_cl, 0);
  const uint64_t budget = ctx->opt.pan_bytes ? ctx->opt.pan_bytes : rtc_free_hbm(ctx) / 2;
  std::vector<PanGroup> groups;
  uint64_t group_bytes = 0, max_slots = 0;
  uint32_t max_members = 0, max_clusters = 0;
  for (uint32_t c = 0; c < n_cl; c++) {
    const uint64_t K = moff[cfirst[c + 1]] - moff[cfirst[c]];
    uint64_t slots = 0;
    if (!all_global && K <= PAN_WAVE_RECORDS) path[c] = 0;
    else if (!all_global && K <= PAN_BLOCK_RECORDS) path[c] = 1;
    else {
      uint32_t lg = PAN_GLOBAL_LOG2_MIN;
      while ((1ull << lg) < 2 * K) lg++;
      path[c] = 2;
      lg2[c] = (uint8_t)lg;
      slots = 1ull << lg;
    }
    S[4 + path[c]]++;
    ctx->pan_path |= 1 << path[c];
    const uint64_t bytes = PAN_SLOT_BYTES * slots + PAN_MEMBER_BYTES * csize[c] + PAN_CLUSTER_BYTES;
    if (bytes > budget)
      return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: %llu bytes for cluster %u alone (%u members, %llu records, %llu slots), the budget is %llu", who,
                      (unsigned long long)bytes, c, csize[c], (unsigned long long)K, (unsigned long long)slots, (unsigned long long)budget);
    if (groups.empty() || group_bytes + bytes > budget) { groups.push_back(PanGroup{c, c, 0}); group_bytes = 0; }
    PanGroup& G = groups.back();
    G.c1 = c + 1;
    G.slots += slots;
    group_bytes += bytes;
    max_slots = std::max(max_slots, G.slots);
    max_members = std::max(max_members, cfirst[G.c1] - cfirst[G.c0]);
    max_clusters = std::max(max_clusters, G.c1 - G.c0);
  }
  S[7] = groups.size();

  // ---- device state, sized for the largest group ----
  const uint64_t all_bytes = PAN_SLOT_BYTES * max_slots + PAN_MEMBER_BYTES * (uint64_t)max_members + PAN_CLUSTER_BYTES * (uint64_t)max_clusters + 4096;
  DevBuf db;
  auto nomem = [&](int st) -> int {
    if (st != RTC_ERR_NOMEM) return st;
    const std::string why = ctx->err;
    return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: %llu bytes (%llu slots, %u members and %u clusters of the largest of %zu group(s)): %s", who,
                    (unsigned long long)all_bytes, (unsigned long long)max_slots, max_members, max_clusters, groups.size(), why.c_str());
  };
  uint32_t *d_perm = nullptr, *d_mcl = nullptr, *d_list = nullptr, *d_cnt = nullptr, *d_ones = nullptr;
  uint64_t *d_moff = nullptr, *d_aoff = nullptr;
  unsigned long long *d_hist = nullptr, *d_keys = nullptr;
  rtc_pan_genome* d_gen = nullptr;
  PanDesc* d_desc = nullptr;
#define PAN_GET(count, ptr) do { const int st__ = db.get(ctx, (size_t)(count), ptr); if (st__ != RTC_OK) return nomem(st__); } while (0)
  PAN_GET(max_members, &d_perm);
  PAN_GET(max_members, &d_mcl);
  PAN_GET((uint64_t)max_members + 1, &d_moff);
  PAN_GET(max_members, &d_hist);
  PAN_GET(max_members, &d_gen);
  PAN_GET(max_clusters, &d_desc);
  PAN_GET(max_clusters, &d_list);
  PAN_GET((uint64_t)max_clusters + 1, &d_aoff);
  PAN_GET(max_clusters, &d_ones);
  if (max_slots) {
    PAN_GET(max_slots, &d_keys);
    PAN_GET(max_slots, &d_cnt);
  }
#undef PAN_GET

  std::vector<PanDesc> desc;
  std::vector<uint32_t> list, mcl;
  std::vector<uint64_t> aoff;
  std::vector<rtc_pan_genome> gen;
  for (const PanGroup& G : groups) {
    const uint32_t C = G.c1 - G.c0, mb0 = cfirst[G.c0], M = cfirst[G.c1] - mb0;
    desc.assign(C, PanDesc{0, 0, 0, 0, 0});
    list.clear();
    mcl.assign(M, PAN_NONE);
    aoff.assign(1, 0);
    uint32_t n_path[3] = {0, 0, 0};
    for (int p = 0; p < 3; p++)  // the list: the wave clusters, the workgroup clusters, the arena clusters
      for (uint32_t c = G.c0; c < G.c1; c++) {
        if (path[c] != p) continue;
        PanDesc& d = desc[c - G.c0];
        d.m0 = cfirst[c] - mb0;
        d.m1 = cfirst[c + 1] - mb0;
        if (p == 2) {
          d.tab_off = aoff.back();
          d.log2 = lg2[c];
          for (uint32_t x = d.m0; x < d.m1; x++) mcl[x] = n_path[2];
          aoff.push_back(d.tab_off + (1ull << d.log2));
        }
        list.push_back(c - G.c0);
        n_path[p]++;
      }
    const uint32_t na = n_path[2];
    const uint64_t slots = aoff.back();  // == G.slots
    RTC_HIP(ctx, hipMemcpyAsync(d_perm, perm.data() + mb0, (size_t)M * 4, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemcpyAsync(d_mcl, mcl.data(), (size_t)M * 4, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemcpyAsync(d_moff, moff.data() + mb0, ((size_t)M + 1) * 8, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemcpyAsync(d_desc, desc.data(), (size_t)C * sizeof(PanDesc), hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemcpyAsync(d_list, list.data(), (size_t)C * 4, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemcpyAsync(d_aoff, aoff.data(), aoff.size() * 8, hipMemcpyHostToDevice, s));
    RTC_HIP(ctx, hipMemsetAsync(d_hist, 0, (size_t)M * 8, s));
    RTC_HIP(ctx, hipMemsetAsync(d_gen, 0, (size_t)M * sizeof(rtc_pan_genome), s));
    if (na) {
      RTC_HIP(ctx, hipMemsetAsync(d_keys, 0xFF, slots * 8, s));
      RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, slots * 4, s));
      RTC_HIP(ctx, hipMemsetAsync(d_ones, 0, (size_t)na * 4, s));
    }
    RTC_HIP(ctx, hipStreamSynchronize(s));
    const uint64_t k0 = now_ns();
    if (n_path[0]) {
      const uint32_t nb = (uint32_t)std::min<uint64_t>(n_path[0], (uint64_t)ctx->num_cu * PAN_WAVE_WGS_PER_CU);
      hipLaunchKernelGGL((pan_lds_kernel<64, PAN_WAVE_SLOTS, PAN_WAVE_HIST>), dim3(nb), dim3(64), 0, s, (const uint32_t*)d_list, n_path[0],
                         (const PanDesc*)d_desc, (const uint32_t*)d_perm, (const uint64_t*)d_moff, d_hashes, width, d_start, d_len, soft_pct, cloud_pct,
                         d_hist, d_gen);
      RTC_CHECK_LAUNCH(ctx);
    }
    if (n_path[1]) {
      const uint32_t nb = (uint32_t)std::min<uint64_t>(n_path[1], (uint64_t)ctx->num_cu * PAN_BLOCK_WGS_PER_CU);
      hipLaunchKernelGGL((pan_lds_kernel<256, PAN_BLOCK_SLOTS, PAN_BLOCK_HIST>), dim3(nb), dim3(256), 0, s, (const uint32_t*)d_list + n_path[0], n_path[1],
                         (const PanDesc*)d_desc, (const uint32_t*)d_perm, (const uint64_t*)d_moff, d_hashes, width, d_start, d_len, soft_pct, cloud_pct,
                         d_hist, d_gen);
      RTC_CHECK_LAUNCH(ctx);
    }
    const uint32_t* d_alist = d_list + n_path[0] + n_path[1];
    const uint32_t member_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)M + 3) / 4, (uint64_t)ctx->num_cu * PAN_GLOBAL_WGS_PER_CU));
    if (na) {
      hipLaunchKernelGGL(pan_count_kernel, dim3(member_grid), dim3(256), 0, s, (const uint32_t*)d_mcl, M, d_alist, (const PanDesc*)d_desc,
                         (const uint32_t*)d_perm, d_hashes, width, d_start, d_len, d_keys, d_cnt, d_ones);
      RTC_CHECK_LAUNCH(ctx);
    }
    RTC_HIP(ctx, hipStreamSynchronize(s));
    const uint64_t k1 = now_ns();
    uint64_t k2 = k1, k3 = k1;
    if (na) {
      const uint32_t sweep_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(slots >> 8, (uint64_t)ctx->num_cu * PAN_GLOBAL_WGS_PER_CU));
      hipLaunchKernelGGL(pan_sweep_kernel, dim3(sweep_grid), dim3(256), 0, s, (const uint64_t*)d_aoff, na, d_alist, (const PanDesc*)d_desc,
                         (const uint32_t*)d_cnt, (const uint32_t*)d_ones, d_hist);
      RTC_CHECK_LAUNCH(ctx);
      RTC_HIP(ctx, hipStreamSynchronize(s));
      k2 = now_ns();
      hipLaunchKernelGGL(pan_genome_kernel, dim3(member_grid), dim3(256), 0, s, (const uint32_t*)d_mcl, M, d_alist, (const PanDesc*)d_desc,
                         (const uint32_t*)d_perm, d_hashes, width, d_start, d_len, (const unsigned long long*)d_keys, (const uint32_t*)d_cnt,
                         (const uint32_t*)d_ones, soft_pct, cloud_pct, d_gen);
      RTC_CHECK_LAUNCH(ctx);
      RTC_HIP(ctx, hipStreamSynchronize(s));
      k3 = now_ns();
    }
    ctx->pan_phase[0] += k1 - k0;
    ctx->pan_phase[1] += k2 - k1;
    ctx->pan_phase[2] += k3 - k2;
    S[8] += k3 - k0;
    gen.resize(M);
    RTC_HIP(ctx, hipMemcpyAsync(h_hist + mb0, d_hist, (size_t)M * 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipMemcpyAsync(gen.data(), d_gen, (size_t)M * sizeof(rtc_pan_genome), hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    for (uint32_t x = 0; x < M; x++) h_genomes[perm[mb0 + x]] = gen[x];
  }

  // ---- the clusters' records: sums over their histograms ----
  for (uint32_t c = 0; c < n_cl; c++) {
    const uint64_t m = csize[c];
    const uint64_t* hist = h_hist + cfirst[c];
    rtc_pan r;
    memset(&r, 0, sizeof r);
    r.size = (uint32_t)m;
    r.total = moff[cfirst[c + 1]] - moff[cfirst[c]];
    for (uint64_t f = 1; f <= m; f++) {
      const uint64_t k = hist[f - 1];
      r.pan += k;
      if (f == m) r.core += k;
      else if (100 * f >= (uint64_t)soft_pct * m) r.soft += k;
      else if (100 * f < (uint64_t)cloud_pct * m) r.cloud += k;
      else r.shell += k;
    }
    r.single = hist[0];
    h_clusters[c] = r;
    S[3] += r.pan;
  }
  S[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_pangenome_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->pan[i];
  return RTC_OK;
}

extern "C" int rtc_pangenome_phases(const rtc_ctx* ctx, uint64_t out[3]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 3; i++) out[i] = ctx->pan_phase[i];
  return RTC_OK;
}

extern "C" int rtc_pangenome_last_path(const rtc_ctx* ctx) { return ctx ? ctx->pan_path : 0; }

// The unit is built with -ffp-contract=off: every line below is the one IEEE-754 operation it names.
extern "C" int rtc_pan_growth(const uint64_t* h_hist, uint32_t m, int threads, uint32_t* h_j, double* h_pan, double* h_core, uint32_t* h_points) {
  if (!h_points || (m && (!h_hist || !h_j || !h_pan || !h_core))) return RTC_ERR_ARG;
  const uint32_t P = m <= PAN_GROWTH_POINTS ? m : PAN_GROWTH_POINTS;
  *h_points = P;
  if (m == 0) return RTC_OK;
  for (uint32_t i = 0; i < P; i++) {
    h_j[i] = m <= PAN_GROWTH_POINTS ? i + 1 : 1 + (uint32_t)((uint64_t)i * (m - 1) / (PAN_GROWTH_POINTS - 1));
    h_pan[i] = 0.0;
    h_core[i] = 0.0;
  }
  std::vector<uint32_t> fs;
  for (uint32_t f = 1; f <= m; f++) if (h_hist[f - 1] > 0) fs.push_back(f);
  // u_f and v_f at the points, a block of f at a time; the sums then take the block in ascending f
  const size_t block = 1024;
  std::vector<double> U(std::min(block, fs.size()) * P), V(U.size());
  for (size_t b0 = 0; b0 < fs.size(); b0 += block) {
    const size_t nb = std::min(block, fs.size() - b0);
    auto work = [&](size_t q0, size_t q1) {
      for (size_t q = q0; q < q1; q++) {
        const uint32_t f = fs[b0 + q];
        double u = 1.0, v = 1.0;
        uint32_t p = 0;
        for (uint32_t i = 0; i < m && p < P; i++) {
          if (i >= m - f) u = 0.0;
          else u = u * (double)(m - f - i) / (double)(m - i);
          v = v * (double)((int64_t)f - (int64_t)i) / (double)(m - i);
          while (p < P && h_j[p] == i + 1) { U[q * P + p] = u; V[q * P + p] = v; p++; }
        }
      }
    };
    const size_t T = std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), nb));
    if (T == 1) work(0, nb);
    else {
      std::vector<std::thread> pool;
      for (size_t t = 0; t < T; t++) pool.emplace_back(work, nb * t / T, nb * (t + 1) / T);
      for (std::thread& th : pool) th.join();
    }
    for (size_t q = 0; q < nb; q++) {
      const double k = (double)h_hist[fs[b0 + q] - 1];
      for (uint32_t p = 0; p < P; p++) {
        h_pan[p] = h_pan[p] + k * (1.0 - U[q * P + p]);
        h_core[p] = h_core[p] + k * V[q * P + p];
      }
    }
  }
  return RTC_OK;
}
