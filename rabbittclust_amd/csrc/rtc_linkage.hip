// rtc_linkage.hip -- clust-mst --linkage complete: complete-linkage agglomeration inside the single-linkage clusters.
//
// The definition is in include/rtclust.h (tests/reflinkage.py restates it).  Everything the device does is a comparison of exact
// rationals common / denom by 64-bit cross-multiplication and a minimum or maximum of them: no distance is formed here, nothing
// is summed, so the merge list depends neither on scheduling nor on the kernel path.
//
//   wave path       m <= 64: one wave per component, the key matrix in LDS, lane x owns cluster x and walks column x
//   workgroup path  m >  64: one 256-lane workgroup per component, the matrix (both halves) in global memory, the row-bests
//                            (partner, key) in a global scratch of 12 m bytes
// Both run a component's whole dendrogram in one launch.  A retired cluster's entries are overwritten with the key 0 / 0, whose
// kappa is 0 and which no row-best ever takes, so a scan needs no list of the live clusters; the workgroup path keeps the member
// count of cluster x in the diagonal entry (x, x) as {size, 0} -- kappa 0 as well.
#include <algorithm>
#include <numeric>
#include <vector>

#include "rtc_internal.h"

namespace {

constexpr uint32_t LK_NONE = 0xFFFFFFFEu;     // a live row without a key above 0
constexpr uint32_t LK_RETIRED = 0xFFFFFFFFu;  // a row merged into another
constexpr uint32_t LK_WAVE_MAX = 64;          // the wave path's largest m
constexpr uint32_t LK_BAND_SPAN = 4096;       // components of up to this many sketches share a band of the fill (RTC_LINKAGE_SPAN)
constexpr uint64_t LK_BAND_BYTES = (uint64_t)64 << 20;  // the u32 temporary of one band

using lk_comp = rtc_kb_comp;  // key_off, ld and m come from the fill; merge_off and scratch_off (workgroup path: first u32 of the row-bests) are set here

struct lk_cand { uint32_t c, d, a, b; };

// sign of kappa(c0 / d0) - kappa(c1 / d1); denom 0 counts as kappa 0
__device__ __forceinline__ int lk_cmp(uint32_t c0, uint32_t d0, uint32_t c1, uint32_t d1) {
  if (d0 == 0) { c0 = 0; d0 = 1; }
  if (d1 == 0) { c1 = 0; d1 = 1; }
  const uint64_t l = (uint64_t)c0 * d1, r = (uint64_t)c1 * d0;
  return (l > r) - (l < r);
}
// the order of K(X, Y): kappa ascending, then denom ascending
__device__ __forceinline__ uint2 lk_min(uint2 x, uint2 y) {
  const int s = lk_cmp(x.x, x.y, y.x, y.y);
  return (s < 0 || (s == 0 && x.y <= y.y)) ? x : y;
}
// the order of a step's choice: kappa descending, then a ascending, then b ascending
__device__ __forceinline__ bool lk_better(const lk_cand& x, const lk_cand& y) {
  const int s = lk_cmp(x.c, x.d, y.c, y.d);
  return s > 0 || (s == 0 && (x.a < y.a || (x.a == y.a && x.b < y.b)));
}
__device__ __forceinline__ lk_cand lk_wave_best(lk_cand v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    lk_cand o;
    o.c = __shfl_xor(v.c, off); o.d = __shfl_xor(v.d, off); o.a = __shfl_xor(v.a, off); o.b = __shfl_xor(v.b, off);
    if (lk_better(o, v)) v = o;
  }
  return v;
}
__device__ __forceinline__ bool lk_stops(const lk_cand& v, uint32_t knum, uint32_t kden) {
  return v.c == 0 || v.d == 0 || (uint64_t)v.c * kden < (uint64_t)knum * v.d;
}

// ---- wave path --------------------------------------------------------------------------------------------------------------
// LDS: K[y * lds + x], lds = m | 1 (an odd stride spreads the one strided store of a step, K[x][a], over the banks).  Lane x reads
// only column x, K[y][x]: consecutive lanes on consecutive addresses.
__global__ __launch_bounds__(64) void lk_wave_kernel(const rtc_lkey* __restrict__ keys, const lk_comp* __restrict__ comps, uint32_t knum,
                                                     uint32_t kden, rtc_lmerge* __restrict__ merges, uint32_t* __restrict__ n_merges,
                                                     uint32_t* __restrict__ n_rescans) {
  extern __shared__ uint2 lk_K[];
  const lk_comp cp = comps[blockIdx.x];
  const uint32_t m = cp.m, x = threadIdx.x, lds = m | 1;
  const uint2* g = (const uint2*)(keys + cp.key_off);
  if (x < m)
    for (uint32_t y = 0; y < m; y++) lk_K[y * lds + x] = x == y ? make_uint2(0, 0) : g[(uint64_t)y * cp.ld + x];
  __syncthreads();
  bool active = x < m;
  uint32_t size = 1, bp = LK_NONE, bc = 0, bd = 1;
  auto scan = [&]() {
    bp = LK_NONE; bc = 0; bd = 1;
    for (uint32_t y = 0; y < m; y++) {
      const uint2 k = lk_K[y * lds + x];
      if (lk_cmp(k.x, k.y, bc, bd) > 0) { bc = k.x; bd = k.y; bp = y; }  // strictly above: the smallest y of a tie stays
    }
  };
  if (active) scan();
  uint32_t nm = 0, nres = 0;
  while (nm + 1 < m) {  // at most m - 1 merges: the room of the component's list
    lk_cand v = {0u, 1u, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (active && bp != LK_NONE) v = lk_cand{bc, bd, min(x, bp), max(x, bp)};
    v = lk_wave_best(v);
    if (lk_stops(v, knum, kden)) break;
    const uint32_t a = v.a, b = v.b;
    const uint32_t sab = __shfl(size, (int)a) + __shfl(size, (int)b);
    if (x == 0) merges[cp.merge_off + nm] = rtc_lmerge{a, b, v.c, v.d, sab};
    nm++;
    if (x < m) {
      if (active && x != a && x != b) {  // a retired lane's column is dead: it must not write its stale keys into column a
        const uint2 kn = lk_min(lk_K[a * lds + x], lk_K[b * lds + x]);
        lk_K[a * lds + x] = kn;
        lk_K[x * lds + a] = kn;
      }
      lk_K[b * lds + x] = make_uint2(0, 0);  // b is retired: every column loses its entry
    }
    if (x == a) size = sab;
    if (x == b) active = false;
    __syncthreads();
    const bool rs = active && (x == a || bp == a || bp == b);
    nres += (uint32_t)__popcll(__ballot(rs));
    if (rs) scan();
  }
  if (x == 0) { n_merges[blockIdx.x] = nm; n_rescans[blockIdx.x] = nres; }
}

// ---- workgroup path ---------------------------------------------------------------------------------------------------------
// One wave rescans one row: lanes stride the row (coalesced), then a cross-lane maximum with ties to the smallest partner.
__device__ __forceinline__ void lk_wg_rescan_row(const uint2* K, uint64_t ld, uint32_t m, uint32_t r, uint32_t lane,
                                                 uint32_t* part, uint2* bkey) {
  lk_cand v = {0u, 1u, LK_NONE, 0u};  // a: the partner
  const uint2* row = K + (uint64_t)r * ld;
  for (uint32_t y0 = lane; y0 < m; y0 += 256) {  // four loads in flight a lane: a row scan is a chain of L2 latencies otherwise
    uint2 k[4];
#pragma unroll
    for (int u = 0; u < 4; u++) k[u] = y0 + 64 * u < m ? row[y0 + 64 * u] : make_uint2(0, 0);
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (lk_cmp(k[u].x, k[u].y, v.c, v.d) > 0) { v.c = k[u].x; v.d = k[u].y; v.a = y0 + 64 * u; }  // ascending y: the smallest of a tie stays
  }
  v = lk_wave_best(v);
  if (lane == 0) { part[r] = v.a; bkey[r] = make_uint2(v.c, v.d); }
}

__global__ __launch_bounds__(256) void lk_wg_kernel(rtc_lkey* __restrict__ keys, const lk_comp* __restrict__ comps, uint32_t knum, uint32_t kden,
                                                    rtc_lmerge* __restrict__ merges, uint32_t* __restrict__ n_merges,
                                                    uint32_t* __restrict__ n_rescans, uint32_t* __restrict__ scratch) {
  __shared__ lk_cand s_best[4];
  __shared__ uint32_t s_res;
  const lk_comp cp = comps[blockIdx.x];
  const uint32_t m = cp.m, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t ld = cp.ld;
  uint2* K = (uint2*)(keys + cp.key_off);
  uint32_t* part = scratch + cp.scratch_off;           // partner of row x, LK_NONE or LK_RETIRED
  uint2* bkey = (uint2*)(part + m + (m & 1));          // its key
  if (tid == 0) s_res = 0;
  for (uint32_t x = tid; x < m; x += 256) K[(uint64_t)x * ld + x] = make_uint2(1, 0);  // member counts live in the diagonal
  __syncthreads();
  for (uint32_t r = wave; r < m; r += 4) lk_wg_rescan_row(K, ld, m, r, lane, part, bkey);
  __syncthreads();
  uint32_t nm = 0, nres = 0;
  while (nm + 1 < m) {  // at most m - 1 merges: the room of the component's list
    // 1. the step's pair from the row-bests
    lk_cand v = {0u, 1u, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t x0 = tid; x0 < m; x0 += 1024) {
      uint32_t p[4];
      uint2 k[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t x = x0 + 256 * u;
        p[u] = x < m ? part[x] : LK_RETIRED;
        k[u] = x < m ? bkey[x] : make_uint2(0, 0);
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (p[u] < LK_NONE) {
          const uint32_t x = x0 + 256 * u;
          const lk_cand c = {k[u].x, k[u].y, min(x, p[u]), max(x, p[u])};
          if (lk_better(c, v)) v = c;
        }
    }
    v = lk_wave_best(v);
    if (lane == 0) s_best[wave] = v;
    __syncthreads();
    v = s_best[0];
    for (int w = 1; w < 4; w++) { const lk_cand o = s_best[w]; if (lk_better(o, v)) v = o; }
    if (lk_stops(v, knum, kden)) break;  // from LDS words written before the barrier: the same answer in every lane
    const uint32_t a = v.a, b = v.b;
    if (tid == 0) {
      const uint32_t sab = K[(uint64_t)a * ld + a].x + K[(uint64_t)b * ld + b].x;
      merges[cp.merge_off + nm] = rtc_lmerge{a, b, v.c, v.d, sab};
      K[(uint64_t)a * ld + a] = make_uint2(sab, 0);
      part[b] = LK_RETIRED;
    }
    nm++;
    // 2. row and column a take the minimum with b's, column b is retired
    for (uint32_t x0 = tid; x0 < m; x0 += 1024) {
      uint2 ka[4], kb[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t x = x0 + 256 * u;
        ka[u] = x < m ? K[(uint64_t)a * ld + x] : make_uint2(0, 0);
        kb[u] = x < m ? K[(uint64_t)b * ld + x] : make_uint2(0, 0);
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t x = x0 + 256 * u;
        if (x >= m) break;
        if (x != a && x != b) {
          const uint2 kn = lk_min(ka[u], kb[u]);
          K[(uint64_t)a * ld + x] = kn;
          K[(uint64_t)x * ld + a] = kn;
        }
        if (x != b) K[(uint64_t)x * ld + b] = make_uint2(0, 0);
      }
    }
    __syncthreads();
    // 3. exactly the rows whose best partner was a or b, and row a: keys only shrink, and only towards a
    for (uint32_t base = wave * 64; base < m; base += 256) {
      const uint32_t x = base + lane;
      const uint32_t p = x < m ? part[x] : LK_RETIRED;
      unsigned long long need = __ballot(p != LK_RETIRED && (x == a || p == a || p == b));
      nres += (uint32_t)__popcll(need);
      while (need) {
        const uint32_t r = base + (uint32_t)__ffsll((long long)need) - 1;
        need &= need - 1;
        lk_wg_rescan_row(K, ld, m, r, lane, part, bkey);
      }
    }
    __syncthreads();
  }
  if (lane == 0 && nres) atomicAdd(&s_res, nres);
  __syncthreads();
  if (tid == 0) { n_merges[blockIdx.x] = nm; n_rescans[blockIdx.x] = s_res; }
}

// ---- key blocks -------------------------------------------------------------------------------------------------------------
// One band of the permuted set: common[(r - r0) * ldc + (c - c0)] holds |r ∩ c| for c < r.  A pair of one component goes into
// its block, both halves; every other entry of the band is dropped.
struct lk_row { uint64_t off; uint32_t first, m; };  // per permuted row: its component's block, first row and size
__global__ __launch_bounds__(256) void lk_fill_kernel(const uint32_t* __restrict__ common, uint64_t ldc, uint32_t r0, uint32_t r1, uint32_t c0,
                                                      const uint32_t* __restrict__ len, const lk_row* __restrict__ rows,
                                                      rtc_lkey* __restrict__ keys) {
  const uint32_t c = c0 + blockIdx.x * 64 + (threadIdx.x & 63);
  const uint32_t r = r0 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (r >= r1 || c >= r) return;
  const lk_row R = rows[r];
  if (c < R.first) return;
  const uint32_t cm = common[(uint64_t)(r - r0) * ldc + (c - c0)];
  const rtc_lkey k = {cm, len[r] + len[c] - cm};
  const uint64_t i = r - R.first, j = c - R.first;
  keys[R.off + i * R.m + j] = k;
  keys[R.off + j * R.m + i] = k;
}

__global__ __launch_bounds__(256) void lk_gather_kernel(const uint64_t* __restrict__ start, const uint32_t* __restrict__ len,
                                                        const uint32_t* __restrict__ perm, uint32_t np, uint64_t* __restrict__ p_start,
                                                        uint32_t* __restrict__ p_len) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  const uint32_t g = perm[i];
  p_start[i] = start[g];
  p_len[i] = len[g];
}

// Agglomerates comps[0 .. nc) over the blocks in d_keys: one launch per path, then the merge lists and counts come back.
// h_merges_out: sum(m - 1) records, laid out by merge_off; h_nm / h_nres: per component.
int lk_agglomerate(rtc_ctx* ctx, rtc_lkey* d_keys, std::vector<lk_comp>& comps, uint32_t knum, uint32_t kden, std::vector<rtc_lmerge>& h_merges_out,
                   std::vector<uint32_t>& h_nm, std::vector<uint32_t>& h_nres) {
  const size_t nc = comps.size();
  h_nm.assign(nc, 0);
  h_nres.assign(nc, 0);
  h_merges_out.clear();
  if (!nc) return RTC_OK;
  // wave-path components first, workgroup-path ones behind them: two contiguous descriptor ranges
  std::vector<uint32_t> order(nc);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_partition(order.begin(), order.end(), [&](uint32_t i) { return comps[i].m <= LK_WAVE_MAX; });
  uint64_t n_rec = 0, n_scratch = 0;
  uint32_t n_wave = 0, m_wave = 0;
  std::vector<lk_comp> sorted(nc);
  for (size_t s = 0; s < nc; s++) {
    lk_comp& c = comps[order[s]];
    c.merge_off = n_rec;
    n_rec += c.m - 1;
    if (c.m <= LK_WAVE_MAX) { n_wave++; m_wave = std::max(m_wave, c.m); }
    else { c.scratch_off = n_scratch; n_scratch += (uint64_t)3 * c.m + (c.m & 1); }
    sorted[s] = c;
  }
  DevBuf B;
  lk_comp* d_comps = nullptr;
  rtc_lmerge* d_merges = nullptr;
  uint32_t *d_cnt = nullptr, *d_scratch = nullptr;
  RTC_TRY(B.get(ctx, nc, &d_comps));
  RTC_TRY(B.get(ctx, n_rec, &d_merges));
  RTC_TRY(B.get(ctx, 2 * nc, &d_cnt));
  RTC_TRY(B.get(ctx, n_scratch, &d_scratch));
  RTC_HIP(ctx, hipMemcpyAsync(d_comps, sorted.data(), nc * sizeof(lk_comp), hipMemcpyHostToDevice, ctx->stream));
  RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, nc * 8, ctx->stream));
  uint32_t* d_nm = d_cnt;
  uint32_t* d_nres = d_cnt + nc;
  if (n_wave) {
    const uint32_t lds = m_wave | 1;
    hipLaunchKernelGGL(lk_wave_kernel, dim3(n_wave), dim3(64), (size_t)m_wave * lds * 8, ctx->stream, (const rtc_lkey*)d_keys,
                       (const lk_comp*)d_comps, knum, kden, d_merges, d_nm, d_nres);
    RTC_CHECK_LAUNCH(ctx);
  }
  if (nc > n_wave) {
    hipLaunchKernelGGL(lk_wg_kernel, dim3((uint32_t)(nc - n_wave)), dim3(256), 0, ctx->stream, d_keys, (const lk_comp*)(d_comps + n_wave), knum,
                       kden, d_merges, d_nm + n_wave, d_nres + n_wave, d_scratch);
    RTC_CHECK_LAUNCH(ctx);
  }
  std::vector<uint32_t> cnt(2 * nc);
  h_merges_out.resize(n_rec);
  RTC_HIP(ctx, hipMemcpyAsync(cnt.data(), d_cnt, nc * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (n_rec) RTC_HIP(ctx, hipMemcpyAsync(h_merges_out.data(), d_merges, n_rec * sizeof(rtc_lmerge), hipMemcpyDeviceToHost, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t s = 0; s < nc; s++) {
    h_nm[order[s]] = cnt[s];
    h_nres[order[s]] = cnt[nc + s];
    if (cnt[s] > comps[order[s]].m - 1) return rtc_fail(ctx, RTC_ERR_HIP, "rtc_linkage: a component of %u reported %u merges", comps[order[s]].m, cnt[s]);
  }
  return RTC_OK;
}

int lk_check_bound(rtc_ctx* ctx, uint32_t kmin_num, uint32_t kmin_den) {
  if (kmin_den == 0) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_linkage: kmin_den must not be 0 (0 / 1 means no bound)");
  (void)kmin_num;
  return RTC_OK;
}

}  // namespace

extern "C" int rtc_linkage_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->linkage[i];
  return RTC_OK;
}

extern "C" int rtc_linkage_dev(rtc_ctx* ctx, uint32_t m, rtc_lkey* d_key, uint64_t ld, uint32_t kmin_num, uint32_t kmin_den,
                               rtc_lmerge* h_merges, uint32_t* h_n_merges) {
  if (!ctx || !h_n_merges) return RTC_ERR_ARG;
  *h_n_merges = 0;
  RTC_TRY(lk_check_bound(ctx, kmin_num, kmin_den));
  if (m >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_linkage_dev: m must be below 2^31 - 1");
  for (int i = 0; i < 10; i++) ctx->linkage[i] = 0;
  if (m < 2) return RTC_OK;
  if (!d_key || !h_merges) return RTC_ERR_ARG;
  if (((uintptr_t)d_key & 7) != 0) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_linkage_dev: d_key must be 8-byte aligned");
  if (ld < m) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_linkage_dev: ld smaller than m");
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t t0 = rtc_now_ns();
  std::vector<lk_comp> comps(1);
  comps[0] = lk_comp{0, ld, 0, 0, m, 0};
  std::vector<rtc_lmerge> mg;
  std::vector<uint32_t> nm, nres;
  RTC_TRY(lk_agglomerate(ctx, d_key, comps, kmin_num, kmin_den, mg, nm, nres));
  if (nm[0]) memcpy(h_merges, mg.data(), (size_t)nm[0] * sizeof(rtc_lmerge));
  *h_n_merges = nm[0];
  const uint64_t t1 = rtc_now_ns();
  uint64_t* C = ctx->linkage;
  C[0] = 1; C[1] = m <= LK_WAVE_MAX; C[2] = m > LK_WAVE_MAX; C[3] = nm[0]; C[4] = nres[0]; C[5] = 1; C[7] = t1 - t0; C[8] = m; C[9] = t1 - t0;
  return RTC_OK;
}

// The key blocks of every component, batch after batch (rtc_internal.h): what rtc_linkage_complete agglomerates and
// rtc_nj_clusters joins.
int rtc_key_blocks(rtc_ctx* ctx, const char* who, uint64_t budget_opt, const void* d_hashes, int width, const uint64_t* d_start,
                   const uint32_t* d_len, uint32_t n, const uint32_t* h_comp, uint64_t* h_first,
                   const std::function<int(const rtc_kb_batch&)>& on_batch, uint32_t spare_copies) {
  // ---- components in order of their smallest member; members in ascending genome order ----
  std::vector<uint32_t> by_label(n);
  std::iota(by_label.begin(), by_label.end(), 0u);
  std::stable_sort(by_label.begin(), by_label.end(), [&](uint32_t x, uint32_t y) { return h_comp[x] < h_comp[y]; });
  std::vector<uint32_t> rank(n);  // component of genome g, numbered by smallest member
  std::vector<uint32_t> csize;
  {
    std::vector<std::pair<uint32_t, uint32_t>> groups;  // (smallest member, position in by_label)
    for (uint32_t i = 0; i < n; i++)
      if (i == 0 || h_comp[by_label[i]] != h_comp[by_label[i - 1]]) groups.emplace_back(by_label[i], i);
    std::sort(groups.begin(), groups.end());
    csize.resize(groups.size());
    for (size_t c = 0; c < groups.size(); c++) {
      uint32_t i = groups[c].second;
      const uint32_t lab = h_comp[by_label[i]];
      for (; i < n && h_comp[by_label[i]] == lab; i++) { rank[by_label[i]] = (uint32_t)c; csize[c]++; }
    }
  }
  const size_t n_comp = csize.size();
  // the permuted set: the members of the components of two or more, component after component
  std::vector<uint32_t> cfirst(n_comp, 0), perm;
  {
    uint32_t np = 0;
    for (size_t c = 0; c < n_comp; c++) { cfirst[c] = np; if (csize[c] >= 2) np += csize[c]; }
    perm.resize(np);
    std::vector<uint32_t> fill(cfirst);
    for (uint32_t g = 0; g < n; g++) if (csize[rank[g]] >= 2) perm[fill[rank[g]]++] = g;
  }
  const uint32_t np = (uint32_t)perm.size();
  for (size_t c = 0; c <= n_comp; c++) h_first[c] = 0;
  if (np == 0) return RTC_OK;
  if (!d_hashes) return RTC_ERR_ARG;

  DevBuf B;
  uint32_t *d_perm = nullptr, *p_len = nullptr;
  uint64_t* p_start = nullptr;
  lk_row* d_rows = nullptr;
  RTC_TRY(B.get(ctx, np, &d_perm));
  RTC_TRY(B.get(ctx, np, &p_start));
  RTC_TRY(B.get(ctx, np, &p_len));
  RTC_TRY(B.get(ctx, np, &d_rows));
  RTC_HIP(ctx, hipMemcpyAsync(d_perm, perm.data(), (size_t)np * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(lk_gather_kernel, dim3((np + 255) / 256), dim3(256), 0, ctx->stream, d_start, d_len, (const uint32_t*)d_perm, np, p_start, p_len);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));

  // ---- batches under the byte budget: the blocks of a batch and one band of the fill ----
  const uint64_t budget = std::min<uint64_t>(budget_opt ? budget_opt : std::max<uint64_t>(rtc_free_hbm(ctx) / 2, 1), (uint64_t)1 << 61);
  auto block_bytes = [](uint64_t m) { return m > ((uint64_t)1 << 28) ? (uint64_t)1 << 62 : 8 * m * m; };  // past any budget, and no overflow
  auto min_band = [](uint64_t m) { return 4 * m * std::min<uint64_t>(m, 64); };
  std::vector<lk_row> rows(np);
  std::vector<lk_comp> comps;
  rtc_kb_batch batch = {nullptr, 0, &comps, 0, 0, 0, &csize, &cfirst, &perm, budget};
  const uint64_t copies = 1 + (uint64_t)spare_copies;  // block_bytes is at most 2^62 / 8 per copy below the cut, and the cut itself ends the sum
  size_t c = 0;
  while (c < n_comp) {
    comps.clear();
    if (csize[c] < 2) {
      batch.d_keys = nullptr; batch.n_keys = 0; batch.c = c; batch.ce = c + 1; batch.fill_ns = 0;
      RTC_TRY(on_batch(batch));
      c++;
      continue;
    }
    // the batch [c, ce)
    uint64_t kb = 0, band = 0;
    size_t ce = c;
    while (ce < n_comp) {
      const uint64_t m = csize[ce];
      if (m >= 2) {
        const uint64_t nb = std::max(band, min_band(m));
        if (block_bytes(m) > budget || copies * (kb + block_bytes(m)) + nb > budget) {
          if (kb == 0 && spare_copies)
            return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: a component of m = %llu needs %llu bytes (8 m^2, %u replicate block(s) of 8 m^2 and one band), the budget is %llu",
                            who, (unsigned long long)m, (unsigned long long)(block_bytes(m) > budget ? block_bytes(m) : copies * block_bytes(m) + min_band(m)),
                            spare_copies, (unsigned long long)budget);
          if (kb == 0)
            return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: a component of m = %llu needs %llu bytes (8 m^2 and one band), the budget is %llu", who,
                            (unsigned long long)m, (unsigned long long)(block_bytes(m) + min_band(m)), (unsigned long long)budget);
          break;
        }
        kb += block_bytes(m);
        band = nb;
      }
      ce++;
    }
    const uint64_t temp_cap = std::max(band, std::min<uint64_t>(LK_BAND_BYTES, budget - kb));
    const uint64_t tf0 = rtc_now_ns();
    rtc_lkey* d_keys = nullptr;
    uint32_t* d_tmp = nullptr;
    RTC_TRY(B.get(ctx, kb / sizeof(rtc_lkey), &d_keys));
    std::vector<size_t> comp_of;  // comps[i] is component comp_of[i]
    {
      uint64_t off = 0;
      for (size_t q = c; q < ce; q++) {
        const uint32_t m = csize[q];
        if (m < 2) continue;
        comps.push_back(lk_comp{off, m, 0, 0, m, 0});
        comp_of.push_back(q);
        for (uint32_t i = 0; i < m; i++) rows[cfirst[q] + i] = lk_row{off, cfirst[q], m};
        off += (uint64_t)m * m;
      }
    }
    const uint32_t b_r0 = cfirst[comp_of.front()], b_r1 = cfirst[comp_of.back()] + csize[comp_of.back()];
    RTC_HIP(ctx, hipMemcpyAsync(d_rows + b_r0, rows.data() + b_r0, (size_t)(b_r1 - b_r0) * sizeof(lk_row), hipMemcpyHostToDevice, ctx->stream));
    // bands: runs of whole small components, or row chunks of one large component
    uint64_t span_max = std::min<uint64_t>(ctx->opt.linkage_span ? ctx->opt.linkage_span : LK_BAND_SPAN, (uint64_t)sqrt((double)(temp_cap / 4)));
    while (4 * span_max * span_max > temp_cap) span_max--;
    uint64_t tmp_bytes = 0;
    struct band_t { uint32_t r0, r1, c0; };
    std::vector<band_t> bands;
    for (size_t i = 0; i < comps.size();) {
      const uint32_t m = comps[i].m, first = cfirst[comp_of[i]];
      if (m <= span_max) {
        size_t j = i + 1;
        while (j < comps.size() && comps[j].m <= span_max && cfirst[comp_of[j]] + comps[j].m - first <= span_max) j++;
        const uint32_t r1 = cfirst[comp_of[j - 1]] + comps[j - 1].m;
        bands.push_back(band_t{first, r1, first});
        i = j;
      } else {
        const uint32_t rows_per = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(temp_cap / (4ull * m), std::min<uint32_t>(m, 64)), 262140);
        for (uint32_t r = 0; r < m; r += rows_per) bands.push_back(band_t{first + r, first + std::min(m, r + rows_per), first});
        i++;
      }
    }
    for (const band_t& b : bands) tmp_bytes = std::max<uint64_t>(tmp_bytes, 4ull * (b.r1 - b.r0) * (b.r1 - b.c0));
    RTC_TRY(B.get(ctx, tmp_bytes / 4, &d_tmp));
    for (const band_t& b : bands) {
      const uint32_t ldc = b.r1 - b.c0;
      // the band is handed over as a set of its own, so the tiled kernel's plan covers its sketches only; RTC_PAIR_FORCE_MERGE:
      // the per-pair merge kernel instead (the A/B of DESIGN 3.4k and the tests)
      RTC_TRY(rtc_pair_common_dev(ctx, d_hashes, width, p_start + b.c0, p_len + b.c0, b.r1 - b.c0, b.r0 - b.c0, b.r1 - b.c0, 0, b.r1 - b.c0, d_tmp, ldc, 1,
                                  ctx->opt.pair_force_merge ? 1 : 0));
      hipLaunchKernelGGL(lk_fill_kernel, dim3((ldc + 63) / 64, (b.r1 - b.r0 + 3) / 4), dim3(256), 0, ctx->stream, (const uint32_t*)d_tmp, (uint64_t)ldc,
                         b.r0, b.r1, b.c0, (const uint32_t*)p_len, (const lk_row*)d_rows, d_keys);
      RTC_CHECK_LAUNCH(ctx);
    }
    RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    batch.d_keys = d_keys; batch.n_keys = kb / 8; batch.c = c; batch.ce = ce; batch.fill_ns = rtc_now_ns() - tf0;
    RTC_TRY(on_batch(batch));
    B.release(d_tmp);
    B.release(d_keys);
    c = ce;
  }
  return RTC_OK;
}

extern "C" int rtc_linkage_complete(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                    const uint32_t* h_comp, uint32_t kmin_num, uint32_t kmin_den, rtc_lmerge* h_merges, uint64_t cap,
                                    uint64_t* h_n_merges, uint64_t* h_first) {
  if (!ctx || !h_n_merges || !h_first) return RTC_ERR_ARG;
  *h_n_merges = 0;
  h_first[0] = 0;
  if (width != 4 && width != 8) return rtc_fail(ctx, RTC_ERR_ARG, "width must be 4 or 8");
  RTC_TRY(lk_check_bound(ctx, kmin_num, kmin_den));
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_linkage_complete: n must be below 2^31 - 1");
  if (cap && !h_merges) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) ctx->linkage[i] = 0;
  if (n == 0) return RTC_OK;
  if (!d_start || !d_len || !h_comp) return RTC_ERR_ARG;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t t0 = rtc_now_ns();
  uint64_t* C = ctx->linkage;
  uint64_t total = 0;
  bool overflow = false;
  RTC_TRY(rtc_key_blocks(ctx, "rtc_linkage_complete", ctx->opt.linkage_bytes, d_hashes, width, d_start, d_len, n, h_comp, h_first, [&](const rtc_kb_batch& b) -> int {
    std::vector<lk_comp>& comps = *b.comps;
    std::vector<rtc_lmerge> mg;
    std::vector<uint32_t> nm, nres;
    if (b.d_keys) {
      C[5]++;
      C[6] += b.fill_ns;
      const uint64_t tf1 = rtc_now_ns();
      RTC_TRY(lk_agglomerate(ctx, b.d_keys, comps, kmin_num, kmin_den, mg, nm, nres));
      C[7] += rtc_now_ns() - tf1;
    }
    // the merge lists in component order, local indices turned into genome indices
    rtc_kb_remap(b, mg, [&](size_t i, const lk_comp& cp) -> uint64_t {
      C[0]++; C[cp.m <= LK_WAVE_MAX ? 1 : 2]++; C[3] += nm[i]; C[4] += nres[i]; C[8] = std::max<uint64_t>(C[8], cp.m);
      return nm[i];
    }, h_merges, cap, h_first, &total, &overflow);
    return RTC_OK;
  }));
  *h_n_merges = total;
  C[9] = rtc_now_ns() - t0;
  if (overflow) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "rtc_linkage_complete: %llu merges, room for %llu", (unsigned long long)total, (unsigned long long)cap);
  return RTC_OK;
}
