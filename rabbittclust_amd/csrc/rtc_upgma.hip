// rtc_upgma.hip -- clust-mst --upgma: average linkage (UPGMA) of the clusters on the device, in exact integers.
//
// The definition is in include/rtclust.h (tests/refupgma.py restates it).  A candidate is (S, n_a n_b, a, b); two candidates are
// ordered by the mean S / (n_a n_b), compared as 128-bit cross products, then by a, then by b.  That order is total, so neither
// the path nor the way the search is split over lanes, waves or workgroups changes a record.  Every step scans all active pairs:
// there is no cached best partner to keep right under ties, and nothing to rescan.
//
// The three paths -- wave, workgroup, grid -- their kernels, the launch chain and the batch loop are rtc_agglom.h's; this unit is
// the rule they run for average linkage, the argument checks and the entry points.  The cells are the sums S, a cluster's state
// is its size, the loop runs down to one cluster and nothing closes it; the grid path's first m is RTC_UPGMA_GRID_MIN.  Both
// triangles of S are kept in step.  No sums from different lanes meet: every cell has one writer a step, so there is no atomic.
#include "rtc_agglom.h"
#include "rtc_upgma.h"

namespace {

typedef unsigned __int128 u128;
constexpr uint32_t UP_NONE = AGG_NONE;

struct up_cand { uint64_t s, p; uint32_t a, b; };  // sum, n_a n_b, the pair

struct up_rule {
  using cell = uint64_t;
  using state = uint32_t;  // the size
  using held = uint64_t;   // a size in a scan: the factors of n_a n_b
  using cand = up_cand;
  using record = rtc_umerge;
  static constexpr uint32_t END = 1;
  static constexpr bool CLOSING = false;

  // the order of a step's choice: mean ascending (s_x p_y against s_y p_x; s < 2^62, p < 2^44), then a ascending, then b ascending
  static __device__ __forceinline__ bool better(const up_cand& x, const up_cand& y) {
    const u128 l = (u128)x.s * y.p, r = (u128)y.s * x.p;
    return l < r || (l == r && (x.a < y.a || (x.a == y.a && x.b < y.b)));
  }
  // behind every real candidate: a real s is below 2^62
  static __device__ __forceinline__ up_cand none() { return up_cand{~0ull, 1ull, UP_NONE, UP_NONE}; }
  static __device__ __forceinline__ up_cand shfl(const up_cand& v, int off) {
    up_cand o;
    o.s = (uint64_t)__shfl_xor((unsigned long long)v.s, off); o.p = (uint64_t)__shfl_xor((unsigned long long)v.p, off);
    o.a = __shfl_xor(v.a, off); o.b = __shfl_xor(v.b, off);
    return o;
  }
  template <class I>
  static __device__ __forceinline__ void init(const uint64_t*, I, uint32_t, uint32_t x, uint32_t* N, const uint32_t* w) { N[x] = w ? w[x] : 1u; }
  static __device__ __forceinline__ int step(uint32_t) { return 0; }
  static __device__ __forceinline__ void consider(up_cand& v, int, uint64_t na, uint64_t s, uint64_t nb, uint32_t a, uint32_t b) {
    const up_cand c{s, na * nb, a, b};
    if (better(c, v)) v = c;
  }
  template <class I>
  static __device__ __forceinline__ uint64_t pivot(const uint64_t*, I, const up_cand& v) { return v.s; }
  // step 3 for the cluster k
  template <class I>
  static __device__ __forceinline__ void update(uint64_t* S, I ld, uint32_t*, uint32_t k, const up_cand& v, uint64_t) {
    const uint64_t s = S[(I)v.a * ld + k] + S[(I)v.b * ld + k];
    S[(I)v.a * ld + k] = s;
    S[(I)k * ld + v.a] = s;
  }
  // steps 2 and 4; N[v.a] and N[v.b] are read by nobody else between the scan and the next barrier
  static __device__ __forceinline__ void emit(uint32_t* N, const up_cand& v, uint64_t, uint32_t, rtc_umerge* out) {
    const uint32_t na = N[v.a], nb = N[v.b];
    *out = rtc_umerge{v.a, v.b, na, nb, v.s};
    N[v.a] = na + nb;
  }

  static constexpr uint32_t WAVE_MAX = UPGMA_WAVE_MAX;
  static constexpr uint32_t SCAN_BLOCKS = UPGMA_SCAN_BLOCKS;
  static uint64_t records_of(uint32_t m) { return m - 1; }
  static uint32_t grid_min(const rtc_ctx* ctx) { return ctx->opt.upgma_grid_min ? std::max<uint32_t>(ctx->opt.upgma_grid_min, 4) : UPGMA_GRID_MIN; }
  // RTC_UPGMA_SCAN_BLOCKS below the ceiling the scratch reserves (tests reach a second row per workgroup with it)
  static uint32_t scan_blocks(const rtc_ctx* ctx) { return ctx->opt.upgma_scan_blocks ? std::min<uint32_t>(ctx->opt.upgma_scan_blocks, SCAN_BLOCKS) : SCAN_BLOCKS; }
  static uint64_t* counters(rtc_ctx* ctx) { return ctx->upgma; }
  static int* path(rtc_ctx* ctx) { return &ctx->upgma_path; }
  static uint64_t budget(const rtc_ctx* ctx) { return ctx->opt.upgma_bytes; }
  // all sizes are 1: W is m.  8 m^2 bytes run out long before, so this does not happen
  static int batch(rtc_ctx* ctx, const std::vector<rtc_kb_comp>& comps) {
    for (const rtc_kb_comp& c : comps)
      if (c.m >= UPGMA_W_MAX) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_clusters: a component of %u members, must be below 2^22", c.m);
    return RTC_OK;
  }
};

}  // namespace

extern "C" int rtc_upgma_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->upgma[i];
  return RTC_OK;
}

extern "C" int rtc_upgma_last_path(const rtc_ctx* ctx) { return ctx ? ctx->upgma_path : 0; }

extern "C" int rtc_upgma_scan_blocks(const rtc_ctx* ctx) { return ctx ? (int)up_rule::scan_blocks(ctx) : 0; }

extern "C" double rtc_upgma_distance(uint64_t sum, uint32_t size_a, uint32_t size_b) {
  const double pairs = (double)size_a * (double)size_b;
  const double scale = pairs * 1048576.0;
  return (double)sum / scale;
}

extern "C" int rtc_upgma_dev(rtc_ctx* ctx, uint32_t m, uint64_t* d_sum, uint64_t ld, const uint32_t* h_size, rtc_umerge* h_merges) {
  if (!ctx) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) ctx->upgma[i] = 0;
  ctx->upgma_path = 0;
  if (!d_sum || !h_merges) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_dev: d_sum and h_merges must not be NULL");
  if (((uintptr_t)d_sum & 7) != 0) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_dev: d_sum must be 8-byte aligned");
  if (ld < m) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_dev: ld smaller than m");
  uint64_t W = m;
  if (h_size) {
    W = 0;
    for (uint32_t i = 0; i < m; i++) {
      if (h_size[i] == 0) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_dev: h_size[%u] is 0", i);
      W += h_size[i];
    }
  }
  if (W >= UPGMA_W_MAX) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_dev: the sizes sum to %llu, must be below 2^22", (unsigned long long)W);
  if (m < 2) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t t0 = rtc_now_ns();
  DevBuf B;
  uint32_t* d_w = nullptr;
  if (h_size) {
    RTC_TRY(B.get(ctx, m, &d_w));
    RTC_HIP(ctx, hipMemcpyAsync(d_w, h_size, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  std::vector<rtc_kb_comp> comps(1);
  comps[0] = rtc_kb_comp{0, ld, 0, 0, m, 0};
  std::vector<rtc_umerge> out;
  uint64_t n_path[3];
  RTC_TRY(agg_run<up_rule>(ctx, d_sum, comps, d_w, out, n_path));
  memcpy(h_merges, out.data(), out.size() * sizeof(rtc_umerge));
  agg_count_one<up_rule>(ctx, n_path, out.size(), rtc_now_ns() - t0);
  return RTC_OK;
}

extern "C" int rtc_upgma_clusters(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                  const uint32_t* h_comp, int kmer_size, rtc_umerge* h_merges, uint64_t cap, uint64_t* h_n_merges, uint64_t* h_first) {
  // a key becomes its q; the diagonal 0
  return agg_clusters<up_rule>(ctx, "rtc_upgma_clusters", d_hashes, width, d_start, d_len, n, h_comp, kmer_size, h_merges, cap, h_n_merges, h_first, 0, nullptr,
                               [kmer_size](bool diagonal, uint32_t common, uint32_t denom) {
                                 if (diagonal) return (uint64_t)0;
                                 long long q = (common == 0 || denom == 0) ? (long long)UPGMA_Q1 : llround(rtc_linkage_distance(common, denom, kmer_size) * 1048576.0);
                                 q = std::min<long long>((long long)UPGMA_Q1, std::max<long long>(q, 0));
                                 return (uint64_t)q;
                               });
}
