// rtc_nj.hip -- clust-mst --nj-tree / --nj-all: neighbour joining of the clusters on the device.
//
// The definition is in include/rtclust.h (tests/refnj.py restates it).  Every value a join forms is one double operation in the
// written order (the unit is built with -ffp-contract=off), and the only sum whose order matters -- the initial R -- is one
// thread's loop over ascending j.  The least Q is found on the triple (Q, i, j) with exact comparisons, so neither the path nor
// the way the search is split over lanes, waves or workgroups changes a record.
//
// The three paths -- wave, workgroup, grid -- their kernels, the launch chain and the batch loop are rtc_agglom.h's; this unit is
// the rule they run for neighbour joining, the argument checks and the entry points.  The cells are the distances, a node's
// state is its R, the loop ends at three live nodes and a closing record follows; the grid path's first m is RTC_NJ_GRID_MIN.
#include "rtc_agglom.h"

namespace {

constexpr uint32_t NJ_NONE = AGG_NONE;
constexpr uint32_t NJ_GRID_MIN = 256;      // the grid path's default first m (RTC_NJ_GRID_MIN; measured)
constexpr uint32_t NJ_SCAN_BLOCKS = 1024;  // the most workgroups of a scan launch: their minima are read again by every step workgroup

struct nj_cand { double q; uint32_t a, b; };

struct nj_rule {
  using cell = double;
  using state = double;  // R
  using held = double;
  using cand = nj_cand;
  using record = rtc_njoin;
  static constexpr uint32_t END = 3;
  static constexpr bool CLOSING = true;

  // the order of a step's choice: Q ascending, then i ascending, then j ascending
  static __device__ __forceinline__ bool better(const nj_cand& x, const nj_cand& y) {
    return x.q < y.q || (x.q == y.q && (x.a < y.a || (x.a == y.a && x.b < y.b)));
  }
  static __device__ __forceinline__ nj_cand none() { return nj_cand{__longlong_as_double(0x7FF0000000000000ll), NJ_NONE, NJ_NONE}; }
  static __device__ __forceinline__ nj_cand shfl(const nj_cand& v, int off) {
    nj_cand o;
    o.q = __shfl_xor(v.q, off); o.a = __shfl_xor(v.a, off); o.b = __shfl_xor(v.b, off);
    return o;
  }
  // R[x] in ascending y
  template <class I>
  static __device__ __forceinline__ void init(const double* col, I stride, uint32_t m, uint32_t x, double* R, const uint32_t*) {
    double s = 0.0;
    for (uint32_t y = 0; y < m; y++) {
      const double d = col[(I)y * stride];
      if (y != x) s = s + d;
    }
    R[x] = s;
  }
  static __device__ __forceinline__ double step(uint32_t r) { return (double)(r - 2); }
  // a lane meets its pairs in ascending (i, j), so the first of equal Q stays
  static __device__ __forceinline__ void consider(nj_cand& v, double rm2, double ra, double d, double rb, uint32_t a, uint32_t b) {
    const double q = (rm2 * d - ra) - rb;
    if (q < v.q) v = nj_cand{q, a, b};
  }
  template <class I>
  static __device__ __forceinline__ double pivot(const double* D, I ld, const nj_cand& v) { return D[(I)v.a * ld + v.b]; }
  // step 5 for the node k
  template <class I>
  static __device__ __forceinline__ void update(double* D, I ld, double* R, uint32_t k, const nj_cand& v, double dij) {
    const double dik = D[(I)v.a * ld + k], djk = D[(I)v.b * ld + k];
    const double duk = 0.5 * ((dik + djk) - dij);
    R[k] = ((R[k] - dik) - djk) + duk;
    D[(I)v.a * ld + k] = duk;
    D[(I)k * ld + v.a] = duk;
  }
  // what a join does to its two nodes (steps 4 and 6)
  static __device__ __forceinline__ void emit(double* R, const nj_cand& v, double dij, uint32_t r, rtc_njoin* out) {
    const uint32_t i = v.a, j = v.b;
    const double ri = R[i], rj = R[j];
    const double delta = (ri - rj) / (double)(2 * (uint64_t)(r - 2));
    const double len_i = 0.5 * dij + delta;
    const double len_j = dij - len_i;
    R[i] = 0.5 * ((ri + rj) - (double)r * dij);
    *out = rtc_njoin{i, j, NJ_NONE, 0u, len_i, len_j, 0.0};
  }
  template <class I>
  static __device__ __forceinline__ void close(const double* D, I ld, uint32_t i, uint32_t j, uint32_t k, uint32_t m, rtc_njoin* out) {
    const double dij = D[(I)i * ld + j];
    if (m == 2) { const double la = 0.5 * dij; *out = rtc_njoin{i, j, NJ_NONE, 0u, la, dij - la, 0.0}; return; }
    const double dik = D[(I)i * ld + k], djk = D[(I)j * ld + k];
    *out = rtc_njoin{i, j, k, 0u, 0.5 * ((dij + dik) - djk), 0.5 * ((dij + djk) - dik), 0.5 * ((dik + djk) - dij)};
  }

  static constexpr uint32_t WAVE_MAX = 64;  // the wave path's largest m
  static constexpr uint32_t SCAN_BLOCKS = NJ_SCAN_BLOCKS;
  static uint64_t records_of(uint32_t m) { return rtc_nj_records_of(m); }
  static uint32_t grid_min(const rtc_ctx* ctx) { return ctx->opt.nj_grid_min ? std::max<uint32_t>(ctx->opt.nj_grid_min, 4) : NJ_GRID_MIN; }
  // RTC_NJ_SCAN_BLOCKS below the ceiling the scratch reserves (tests reach a second row per workgroup with it)
  static uint32_t scan_blocks(const rtc_ctx* ctx) { return ctx->opt.nj_scan_blocks ? std::min<uint32_t>(ctx->opt.nj_scan_blocks, SCAN_BLOCKS) : SCAN_BLOCKS; }
  static uint64_t* counters(rtc_ctx* ctx) { return ctx->nj; }
  static int* path(rtc_ctx* ctx) { return &ctx->nj_path; }
  static uint64_t budget(const rtc_ctx* ctx) { return ctx->opt.nj_bytes; }
  static int batch(rtc_ctx* ctx, const std::vector<rtc_kb_comp>&) { ctx->nj[5]++; return RTC_OK; }
};

}  // namespace

extern "C" int rtc_nj_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->nj[i];
  return RTC_OK;
}

extern "C" int rtc_nj_last_path(const rtc_ctx* ctx) { return ctx ? ctx->nj_path : 0; }

extern "C" int rtc_nj_scan_blocks(const rtc_ctx* ctx) { return ctx ? (int)nj_rule::scan_blocks(ctx) : 0; }

extern "C" int rtc_nj_dev(rtc_ctx* ctx, uint32_t m, double* d_dist, uint64_t ld, rtc_njoin* h_joins, uint32_t* h_n_joins) {
  if (!ctx || !h_n_joins) return RTC_ERR_ARG;
  *h_n_joins = 0;
  if (m >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_nj_dev: m must be below 2^31 - 1");
  for (int i = 0; i < 10; i++) ctx->nj[i] = 0;
  ctx->nj_path = 0;
  if (!d_dist || !h_joins) return RTC_ERR_ARG;
  if (((uintptr_t)d_dist & 7) != 0) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_nj_dev: d_dist must be 8-byte aligned");
  if (ld < m) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_nj_dev: ld smaller than m");
  if (m < 2) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t t0 = rtc_now_ns();
  std::vector<rtc_kb_comp> comps(1);
  comps[0] = rtc_kb_comp{0, ld, 0, 0, m, 0};
  std::vector<rtc_njoin> out;
  uint64_t n_path[3];
  RTC_TRY(agg_run<nj_rule>(ctx, d_dist, comps, nullptr, out, n_path));
  memcpy(h_joins, out.data(), out.size() * sizeof(rtc_njoin));
  *h_n_joins = (uint32_t)out.size();
  agg_count_one<nj_rule>(ctx, n_path, out.size(), rtc_now_ns() - t0);
  ctx->nj[5] = 1;
  return RTC_OK;
}

int rtc_nj_join(rtc_ctx* ctx, double* d_dist, std::vector<rtc_kb_comp>& comps, std::vector<rtc_njoin>& h_out, uint64_t n_path[3]) {
  return agg_run<nj_rule>(ctx, d_dist, comps, nullptr, h_out, n_path);
}

extern "C" int rtc_nj_clusters(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                               const uint32_t* h_comp, int kmer_size, rtc_njoin* h_joins, uint64_t cap, uint64_t* h_n_joins, uint64_t* h_first) {
  return rtc_nj_clusters_impl(ctx, "rtc_nj_clusters", d_hashes, width, d_start, d_len, n, h_comp, kmer_size, h_joins, cap, h_n_joins, h_first, 0, nullptr);
}

int rtc_nj_clusters_impl(rtc_ctx* ctx, const char* who, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                         uint32_t n, const uint32_t* h_comp, int kmer_size, rtc_njoin* h_joins, uint64_t cap, uint64_t* h_n_joins,
                         uint64_t* h_first, uint32_t spare_copies, const rtc_nj_hook* hook) {
  // a key becomes its distance; the diagonal 0
  return agg_clusters<nj_rule>(ctx, who, d_hashes, width, d_start, d_len, n, h_comp, kmer_size, h_joins, cap, h_n_joins, h_first, spare_copies, hook,
                               [kmer_size](bool diagonal, uint32_t common, uint32_t denom) {
                                 const double d = diagonal ? 0.0 : (common == 0 || denom == 0) ? 1.0 : rtc_linkage_distance(common, denom, kmer_size);
                                 uint64_t bits;
                                 memcpy(&bits, &d, 8);
                                 return bits;
                               });
}
