// rtc_quality.hip -- rtc_silhouette and rtc_cluster_quality: clust-mst --quality (include/rtclust.h holds the definition,
// tests/refquality.py restates it, DESIGN 3.4n has the choices and the figures).
//   - The records become a CSR as rtc_louvain's level 0 does (rtc_community.h: one sort, one reduce_by_key); a pair given twice
//     leaves fewer than 2 m entries, which is how it is found.
//   - sil_fill_kernel writes every vertex's record as if it had no listed neighbour: all its distances are Q1.
//   - sil_row_kernel, one row a workgroup, rewrites the record of a clustered vertex with a row: an open-addressing table keyed by
//     the neighbours' cluster holds the count and the sum of q (integer atomics: order-free), far_q and near_q / near_cluster are
//     register reductions beside the gather, then every occupied slot is scored and the workgroup reduces the total order
//     (mean ascending, cluster ascending) with the means compared as 128-bit cross products.  Three paths by row length
//     (rtc_quality.h), as louvain_move_kernel's; RTC_SIL_GLOBAL=1 sends every row through the global table.
//   - rtc_cluster_quality: every pair sharing a hash from the pair phase's row chunks (rtc_dbscan_common.h), copied to the host
//     chunk by chunk, each one's distance through rtc_linkage_distance on the context's host threads, then the above.
#include <thread>

#include "rtc_community.h"
#include "rtc_quality.h"

namespace {

constexpr uint32_t SIL_Q1 = 1u << 20;
typedef unsigned __int128 u128;

// (S1 / N1, d1) before (S2 / N2, d2) in the order mean ascending, cluster ascending; d == LV_NONE: no candidate, after all
__device__ __forceinline__ bool sil_before(uint64_t S1, uint32_t N1, uint32_t d1, uint64_t S2, uint32_t N2, uint32_t d2) {
  if (d1 == LV_NONE) return false;
  if (d2 == LV_NONE) return true;
  const u128 l = (u128)S1 * N2, r = (u128)S2 * N1;  // S < 2^51, N < 2^31: past 64 bits
  return l < r || (l == r && d1 < d2);
}

// A slot read after the gather.  The global table was written by this workgroup's atomics, which act in L2: the read goes there
// too (device scope) and never takes a line the CU's vector cache kept from the fill.
template <bool GLOBAL, class T>
__device__ __forceinline__ T sil_slot(const T* p) {
  return GLOBAL ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}

// the record of a vertex none of whose listed neighbours is clustered
__device__ __forceinline__ rtc_sil sil_bare(int32_t c, const uint32_t* __restrict__ csize, uint32_t n_clustered) {
  rtc_sil r;
  r.a_num = r.b_num = 0;
  r.a_den = r.b_den = r.far_q = r.near_q = 0;
  r.b_cluster = r.near_cluster = LV_NONE;
  if (c < 0) return r;
  const uint32_t nc = csize[c];
  r.a_num = (uint64_t)(nc - 1) * SIL_Q1;
  r.a_den = nc - 1;
  if (n_clustered > nc) { r.b_num = SIL_Q1; r.b_den = 1; }
  r.far_q = nc > 1 ? SIL_Q1 : 0;
  r.near_q = SIL_Q1;
  return r;
}

__global__ __launch_bounds__(256) void sil_fill_kernel(const int32_t* __restrict__ label, const uint32_t* __restrict__ csize, uint32_t n,
                                                       uint32_t n_clustered, rtc_sil* __restrict__ out) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) out[x] = sil_bare(label[x], csize, n_clustered);
}

// Row list[it], a clustered vertex with at least one entry.  SLOTS > 0: the table lies in LDS; SLOTS == 0: in global memory,
// 1 << tab_log2[it] slots from tab_off[it] on.  Lane 0 writes the vertex's record; nothing else touches it.
template <int BLOCK, uint32_t SLOTS>
__global__ __launch_bounds__(BLOCK) void sil_row_kernel(const uint32_t* __restrict__ list, uint32_t n_list, const uint64_t* __restrict__ row_off,
                                                        const uint64_t* __restrict__ key, const uint64_t* __restrict__ w,
                                                        const int32_t* __restrict__ label, const uint32_t* __restrict__ csize, uint32_t n_clustered,
                                                        const uint64_t* __restrict__ tab_off, const uint32_t* __restrict__ tab_log2, uint32_t* gkeys,
                                                        uint32_t* gcnt, unsigned long long* gsum, rtc_sil* __restrict__ out) {
  __shared__ uint32_t s_keys[SLOTS ? SLOTS : 1];
  __shared__ uint32_t s_cnt[SLOTS ? SLOTS : 1];
  __shared__ unsigned long long s_sum[SLOTS ? SLOTS : 1];
  __shared__ unsigned long long s_near[4], s_S[4];
  __shared__ uint32_t s_far[4], s_N[4], s_d[4];
  for (uint32_t it = blockIdx.x; it < n_list; it += gridDim.x) {  // uniform over the workgroup: the barriers below are reached by all
    const uint32_t x = list[it];
    uint32_t* keys = s_keys;
    uint32_t* cnts = s_cnt;
    unsigned long long* sums = s_sum;
    uint32_t log2_slots = 31 - __builtin_clz(SLOTS ? SLOTS : 1u);
    if (!SLOTS) {
      keys = gkeys + tab_off[it];
      cnts = gcnt + tab_off[it];
      sums = gsum + tab_off[it];
      log2_slots = tab_log2[it];
    }
    const uint32_t slots = 1u << log2_slots, mask = slots - 1, shift = 32 - log2_slots;
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) { keys[s] = LV_NONE; cnts[s] = 0u; sums[s] = 0ull; }
    __syncthreads();
    const uint32_t c = (uint32_t)label[x];
    const uint64_t r0 = row_off[x], r1 = row_off[x + 1];
    uint32_t far = 0;
    unsigned long long near = ((unsigned long long)SIL_Q1 << 32) | LV_NONE;  // (q, cluster): the least, q first
    for (uint64_t e = r0 + threadIdx.x; e < r1; e += BLOCK) {
      const int32_t dl = label[(uint32_t)key[e]];
      if (dl < 0) continue;  // an unclustered neighbour is no member of anything
      const uint32_t d = (uint32_t)dl, q = (uint32_t)w[e];
      const uint32_t h = lv_table_slot(keys, d, shift, mask);
      atomicAdd(&sums[h], (unsigned long long)q);
      atomicAdd(&cnts[h], 1u);
      if (d == c) far = q > far ? q : far;
      else {
        const unsigned long long cand = ((unsigned long long)q << 32) | d;
        near = cand < near ? cand : near;
      }
    }
    for (int off = 32; off; off >>= 1) {
      const uint32_t of = __shfl_xor(far, off);
      const unsigned long long on = __shfl_xor(near, off);
      far = of > far ? of : far;
      near = on < near ? on : near;
    }
    if (BLOCK > 64) {
      if ((threadIdx.x & 63) == 0) { s_far[threadIdx.x / 64] = far; s_near[threadIdx.x / 64] = near; }
    }
    __syncthreads();  // the table is complete, and so are the waves' far and near
    if (BLOCK > 64)
      for (uint32_t wv = 0; wv < BLOCK / 64; wv++) {
        far = s_far[wv] > far ? s_far[wv] : far;
        near = s_near[wv] < near ? s_near[wv] : near;
      }
    // (mean, cluster) of the best other cluster that holds a listed neighbour
    uint64_t bS = 0;
    uint32_t bN = 0, bd = LV_NONE;
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) {
      const uint32_t d = sil_slot<SLOTS == 0>(&keys[s]);
      if (d == LV_NONE || d == c) continue;
      const uint32_t N = csize[d];
      const uint64_t S = sil_slot<SLOTS == 0>(&sums[s]) + (uint64_t)(N - sil_slot<SLOTS == 0>(&cnts[s])) * SIL_Q1;
      if (sil_before(S, N, d, bS, bN, bd)) { bS = S; bN = N; bd = d; }
    }
    for (int off = 32; off; off >>= 1) {
      const uint64_t oS = __shfl_xor((unsigned long long)bS, off);
      const uint32_t oN = __shfl_xor(bN, off), od = __shfl_xor(bd, off);
      if (sil_before(oS, oN, od, bS, bN, bd)) { bS = oS; bN = oN; bd = od; }
    }
    if (BLOCK > 64) {
      if ((threadIdx.x & 63) == 0) { s_S[threadIdx.x / 64] = bS; s_N[threadIdx.x / 64] = bN; s_d[threadIdx.x / 64] = bd; }
      __syncthreads();
      if (threadIdx.x == 0)
        for (uint32_t wv = 1; wv < BLOCK / 64; wv++)
          if (sil_before(s_S[wv], s_N[wv], s_d[wv], bS, bN, bd)) { bS = s_S[wv]; bN = s_N[wv]; bd = s_d[wv]; }
    }
    if (threadIdx.x == 0) {
      uint32_t cnt_c = 0;
      uint64_t sum_c = 0;
      for (uint32_t h = (c * 2654435761u) >> shift;; h = (h + 1) & mask) {
        const uint32_t k = sil_slot<SLOTS == 0>(&keys[h]);
        if (k == c) { cnt_c = sil_slot<SLOTS == 0>(&cnts[h]); sum_c = sil_slot<SLOTS == 0>(&sums[h]); }
        if (k == c || k == LV_NONE) break;
      }
      rtc_sil r = sil_bare((int32_t)c, csize, n_clustered);
      const uint32_t nc = csize[c];
      r.a_num = sum_c + (uint64_t)(nc - 1 - cnt_c) * SIL_Q1;
      r.far_q = cnt_c < nc - 1 ? SIL_Q1 : far;
      if (bd != LV_NONE && bS < (uint64_t)bN * SIL_Q1) { r.b_num = bS; r.b_den = bN; r.b_cluster = bd; }
      r.near_q = (uint32_t)(near >> 32);
      r.near_cluster = (uint32_t)near;
      out[x] = r;
    }
    __syncthreads();  // the table and the wave slots are written again in the next turn
  }
}

// The score of n vertices under h_label from m records that are already known to be in range.  C[0 .. 9]: rtc_silhouette's
// counters, C[9] left to the caller.  A label out of range and a pair given twice are found here.
int sil_score(rtc_ctx* ctx, const char* who, uint32_t n, const rtc_wedge* rec, uint64_t m, const int32_t* h_label, rtc_sil* h_out, uint64_t* C,
              int* path) {
  std::vector<uint32_t> csize(n, 0);
  uint32_t n_clustered = 0, n_clusters = 0;
  for (uint32_t x = 0; x < n; x++) {
    if (h_label[x] < 0) continue;
    if ((uint32_t)h_label[x] >= n) return rtc_fail(ctx, RTC_ERR_ARG, "%s: label %d of vertex %u with %u vertices", who, h_label[x], x, n);
    n_clusters += csize[h_label[x]]++ == 0;
    n_clustered++;
  }
  C[0] = m; C[2] = n_clustered; C[3] = n_clusters;
  if (n == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // 2 m directed entries: five arrays of 8 bytes (rtc_community.h's Louvain) and the sort's second buffer of 16, the records
  // themselves, and per vertex the level's arrays, the label, the size and the record (100 bytes).  The path lists and the global
  // tables are known only once the CSR stands: they are checked then.
  const uint64_t need = 2 * m * (40 + 16) + m * sizeof(rtc_wedge) + (uint64_t)n * (8 * 3 + 4 * 7 + 4 + 4 + sizeof(rtc_sil)) + (1 << 20);
  const uint64_t free_bytes = rtc_free_hbm(ctx);
  if (need > free_bytes)
    return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: %llu bytes for %llu records over %u vertices, %llu free", who, (unsigned long long)need,
                    (unsigned long long)m, n, (unsigned long long)free_bytes);
  Louvain L{ctx};
  int32_t* d_label = nullptr;
  uint32_t* d_csize = nullptr;
  rtc_sil* d_out = nullptr;
  RTC_TRY(L.db.get(ctx, n, &d_label));
  RTC_TRY(L.db.get(ctx, n, &d_csize));
  RTC_TRY(L.db.get(ctx, n, &d_out));
  RTC_HIP(ctx, hipMemcpyAsync(d_label, h_label, (size_t)n * 4, hipMemcpyHostToDevice, s));
  RTC_HIP(ctx, hipMemcpyAsync(d_csize, csize.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(sil_fill_kernel, dim3(blocks_for(n, ctx->num_cu)), dim3(256), 0, s, (const int32_t*)d_label, (const uint32_t*)d_csize, n,
                     n_clustered, d_out);
  RTC_CHECK_LAUNCH(ctx);
  if (m) {
    const uint64_t t_csr = now_ns();
    const uint64_t E0 = 2 * m;
    uint64_t E = 0;
    RTC_TRY(L.alloc(n, E0));
    rtc_wedge* d_edges = nullptr;
    RTC_TRY(L.db.get(ctx, m, &d_edges));
    RTC_HIP(ctx, hipMemcpyAsync(d_edges, rec, m * sizeof(rtc_wedge), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(louvain_entries_kernel, dim3(blocks_for(m, ctx->num_cu)), dim3(256), 0, s, (const rtc_wedge*)d_edges, m, L.key_in, L.w);
    RTC_CHECK_LAUNCH(ctx);
    RTC_TRY(L.build(n, E0, &E));
    C[1] = E;
    if (E < E0) {  // which pair: the host looks only now
      std::vector<std::pair<uint64_t, uint64_t>> keyed(m);
      for (uint64_t e = 0; e < m; e++)
        keyed[e] = {((uint64_t)std::min(rec[e].u, rec[e].v) << 32) | std::max(rec[e].u, rec[e].v), e};
      std::sort(keyed.begin(), keyed.end());
      uint64_t at = 0;
      for (uint64_t e = 1; e < m; e++)
        if (keyed[e].first == keyed[e - 1].first) { at = keyed[e].second; break; }
      (void)hipStreamSynchronize(s);
      return rtc_fail(ctx, RTC_ERR_ARG, "%s: record %llu gives the pair (%u, %u) a second time", who, (unsigned long long)at, rec[at].u, rec[at].v);
    }
    // the rows by kernel path, and the tables of the long ones
    std::vector<uint64_t> h_row((size_t)n + 1), h_off;
    RTC_HIP(ctx, hipMemcpyAsync(h_row.data(), L.row_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    C[7] = now_ns() - t_csr;
    const uint64_t t_rows = now_ns();
    std::vector<uint32_t> lists[3], h_log2;
    uint64_t table_slots = 0;
    const int all_global = ctx->opt.sil_global;
    for (uint32_t x = 0; x < n; x++) {
      const uint64_t len = h_row[x + 1] - h_row[x];
      if (len == 0 || h_label[x] < 0) continue;  // the fill kernel's record stands
      if (!all_global && len <= SIL_WAVE_ROW) lists[0].push_back(x);
      else if (!all_global && len <= SIL_BLOCK_ROW) lists[1].push_back(x);
      else {
        uint32_t lg = SIL_GLOBAL_LOG2_MIN;
        while ((1ull << lg) < 2 * len) lg++;
        if (lg > 31) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: a row of %llu entries", who, (unsigned long long)len);
        lists[2].push_back(x);
        h_log2.push_back(lg);
        h_off.push_back(table_slots);
        table_slots += 1ull << lg;
      }
    }
    // the lists (4 bytes a row), and 16 bytes a slot and 12 a row for the tables
    const uint64_t need_tab = 4ull * (lists[0].size() + lists[1].size() + lists[2].size()) + 16 * table_slots + 12ull * lists[2].size() + 4096;
    const uint64_t free_tab = rtc_free_hbm(ctx);
    if (need_tab > free_tab)
      return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: %llu bytes for the row lists and %llu slots of global tables (%llu rows), %llu free", who,
                      (unsigned long long)need_tab, (unsigned long long)table_slots, (unsigned long long)lists[2].size(),
                      (unsigned long long)free_tab);
    uint32_t *d_list[3] = {nullptr, nullptr, nullptr}, *d_log2 = nullptr, *d_gkeys = nullptr, *d_gcnt = nullptr;
    uint64_t* d_off = nullptr;
    unsigned long long* d_gsum = nullptr;
    for (int p = 0; p < 3; p++)
      if (!lists[p].empty()) {
        RTC_TRY(L.db.get(ctx, lists[p].size(), &d_list[p]));
        RTC_HIP(ctx, hipMemcpyAsync(d_list[p], lists[p].data(), lists[p].size() * 4, hipMemcpyHostToDevice, s));
        C[4 + p] = lists[p].size();
        *path |= 1 << p;
      }
    if (!lists[2].empty()) {
      RTC_TRY(L.db.get(ctx, h_log2.size(), &d_log2));
      RTC_TRY(L.db.get(ctx, h_off.size(), &d_off));
      RTC_TRY(L.db.get(ctx, table_slots, &d_gkeys));
      RTC_TRY(L.db.get(ctx, table_slots, &d_gcnt));
      RTC_TRY(L.db.get(ctx, table_slots, &d_gsum));
      RTC_HIP(ctx, hipMemcpyAsync(d_log2, h_log2.data(), h_log2.size() * 4, hipMemcpyHostToDevice, s));
      RTC_HIP(ctx, hipMemcpyAsync(d_off, h_off.data(), h_off.size() * 8, hipMemcpyHostToDevice, s));
    }
    // one launch a path; the table arguments are NULL unless a row takes the global path
    auto launch = [&](auto kernel, uint32_t block, int p, uint32_t wgs_per_cu) -> int {
      if (lists[p].empty()) return RTC_OK;
      const uint32_t nb = (uint32_t)std::min<uint64_t>(lists[p].size(), (uint64_t)ctx->num_cu * wgs_per_cu);
      hipLaunchKernelGGL(kernel, dim3(nb), dim3(block), 0, s, (const uint32_t*)d_list[p], (uint32_t)lists[p].size(), (const uint64_t*)L.row_off,
                         (const uint64_t*)L.key, (const uint64_t*)L.w, (const int32_t*)d_label, (const uint32_t*)d_csize, n_clustered,
                         (const uint64_t*)d_off, (const uint32_t*)d_log2, d_gkeys, d_gcnt, d_gsum, d_out);
      RTC_CHECK_LAUNCH(ctx);
      return RTC_OK;
    };
    RTC_TRY(launch(sil_row_kernel<64, SIL_WAVE_SLOTS>, 64, 0, SIL_WAVE_WGS_PER_CU));
    RTC_TRY(launch(sil_row_kernel<256, SIL_BLOCK_SLOTS>, 256, 1, SIL_BLOCK_WGS_PER_CU));
    RTC_TRY(launch(sil_row_kernel<256, 0>, 256, 2, SIL_GLOBAL_WGS_PER_CU));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    C[8] = now_ns() - t_rows;
  }
  RTC_HIP(ctx, hipMemcpyAsync(h_out, d_out, (size_t)n * sizeof(rtc_sil), hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  return RTC_OK;
}

}  // namespace

extern "C" int rtc_silhouette(rtc_ctx* ctx, uint32_t n, const rtc_wedge* h_edges, uint64_t m, const int32_t* h_label, rtc_sil* h_out) {
  const char* who = "rtc_silhouette";
  if (!ctx || (n && (!h_label || !h_out)) || (m && !h_edges)) return RTC_ERR_ARG;
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u vertices", who, n);
  for (uint64_t e = 0; e < m; e++)
    if (h_edges[e].u >= n || h_edges[e].v >= n || h_edges[e].u == h_edges[e].v || h_edges[e].q > SIL_Q1)
      return rtc_fail(ctx, RTC_ERR_ARG, "%s: record %llu is (%u, %u, %u) with %u vertices", who, (unsigned long long)e, h_edges[e].u, h_edges[e].v,
                      h_edges[e].q, n);
  memset(ctx->sil, 0, sizeof ctx->sil);
  ctx->sil_path = 0;
  const uint64_t t_begin = now_ns();
  RTC_TRY(sil_score(ctx, who, n, h_edges, m, h_label, h_out, ctx->sil, &ctx->sil_path));
  ctx->sil[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_silhouette_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->sil[i];
  return RTC_OK;
}

extern "C" int rtc_silhouette_last_path(const rtc_ctx* ctx) { return ctx ? ctx->sil_path : 0; }

extern "C" double rtc_silhouette_value(const rtc_sil* r) {
  if (!r || r->a_den == 0 || r->b_den == 0) return 0.0;
  const double a = (double)r->a_num / ((double)r->a_den * 1048576.0);
  const double b = (double)r->b_num / ((double)r->b_den * 1048576.0);
  const double hi = a > b ? a : b;
  if (hi == 0.0) return 0.0;
  return (b - a) / hi;
}

extern "C" int rtc_cluster_quality(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                   const int32_t* h_label, int kmer_size, rtc_sil* h_out) {
  const char* who = "rtc_cluster_quality";
  if (!ctx || (n && (!d_hashes || !d_start || !d_len || !h_label || !h_out)) || (width != 4 && width != 8)) return RTC_ERR_ARG;
  if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: k-mer size %d", who, kmer_size);
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u sketches", who, n);
  memset(ctx->quality, 0, sizeof ctx->quality);
  memset(ctx->sil, 0, sizeof ctx->sil);
  ctx->sil_path = 0;
  uint64_t* Q = ctx->quality;
  const uint64_t t_begin = now_ns();
  std::vector<rtc_wedge> rec;
  if (n >= 2) {
    RTC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> h_len(n);
    RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    const uint32_t max_len = *std::max_element(h_len.begin(), h_len.end());
    if (max_len >= 0x80000000u)  // rtc_linkage_distance's denominators end at 2^31 - 1
      return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: a sketch of %u hashes, the distance is defined below 2^31", who, max_len);
    std::vector<rtc_cedge> cand;
    uint64_t copy_ns = 0;
    {
      DevBuf db;
      unsigned long long* d_cnt = nullptr;
      RTC_TRY(db.get(ctx, 8, &d_cnt));
      PairPhase pp;
      auto on_chunk = [&](const rtc_cedge* d_cand, uint64_t cnt) -> int {
        if (!cnt) return RTC_OK;
        const uint64_t t0 = now_ns();
        const size_t at = cand.size();
        cand.resize(at + cnt);
        RTC_HIP(ctx, hipMemcpyAsync(cand.data() + at, d_cand, cnt * sizeof(rtc_cedge), hipMemcpyDeviceToHost, s));
        RTC_HIP(ctx, hipStreamSynchronize(s));
        copy_ns += now_ns() - t0;
        return RTC_OK;
      };
      const int st = dbscan_pair_chunks(ctx, db, d_hashes, width, d_start, d_len, n, 1, d_cnt, &pp, on_chunk);
      if (st != RTC_OK) {  // the chunk loop names rtc_dbscan, whose loop it is
        const std::string why = ctx->err;
        return rtc_fail(ctx, st, "%s: in the pair phase: %s", who, why.c_str());
      }
      Q[0] = pp.chunks; Q[1] = pp.cand_total; Q[5] = pp.pair_ns;
    }
    // the distances, on the host's libm
    const uint64_t t_dist = now_ns();
    const uint64_t m = cand.size();
    rec.resize(m);
    auto work = [&](uint64_t e0, uint64_t e1) {
      for (uint64_t e = e0; e < e1; e++) {
        const rtc_cedge& c = cand[e];
        const uint32_t denom = h_len[c.i] + h_len[c.j] - c.common;  // below 2^32: both sizes are below 2^31
        const long long q = llround(rtc_linkage_distance(c.common, denom, kmer_size) * 1048576.0);
        rec[e] = rtc_wedge{c.i, c.j, (uint32_t)std::min<long long>((long long)SIL_Q1, std::max<long long>(q, 0))};
      }
    };
    const uint64_t T = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(ctx->host_threads, 1), m / 4096 + 1));
    if (T == 1) work(0, m);
    else {
      std::vector<std::thread> pool;
      for (uint64_t t = 0; t < T; t++) pool.emplace_back(work, m * t / T, m * (t + 1) / T);
      for (std::thread& th : pool) th.join();
    }
    Q[6] = now_ns() - t_dist + copy_ns;
    std::vector<rtc_cedge>().swap(cand);
  }
  const uint64_t t_score = now_ns();
  RTC_TRY(sil_score(ctx, who, n, rec.data(), rec.size(), h_label, h_out, ctx->sil, &ctx->sil_path));
  Q[7] = now_ns() - t_score;
  ctx->sil[9] = Q[7];
  Q[2] = ctx->sil[4]; Q[3] = ctx->sil[5]; Q[4] = ctx->sil[6];
  Q[8] = ctx->sil[3];
  Q[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_cluster_quality_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->quality[i];
  return RTC_OK;
}
