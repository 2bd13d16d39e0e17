// rtc_quality.hip -- rtc_silhouette and rtc_cluster_quality: clust-mst --quality (include/rtclust.h holds the definition,
// tests/refquality.py restates it, DESIGN 3.4n has the choices and the figures).
//   - The records become a CSR as rtc_louvain's level 0 does (rtc_community.h: one sort, one reduce_by_key); a pair given twice
//     leaves fewer than 2 m entries, which is how it is found.
//   - sil_fill_kernel writes every vertex's record as if it had no listed neighbour: all its distances are Q1.
//   - row_kernel (rtc_rowtable.h) under sil_rule, one row a workgroup, rewrites the record of a clustered vertex with a row: an
//     open-addressing table keyed by the neighbours' cluster holds the count and the sum of q (integer atomics: order-free), far_q
//     and near_q / near_cluster are register reductions beside the gather, then every occupied slot is scored and the workgroup
//     reduces the total order (mean ascending, cluster ascending) with the means compared as 128-bit cross products.  Three paths
//     by row length (rtc_quality.h), as Louvain's rows; RTC_SIL_GLOBAL=1 sends every row through the global table.
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

// 16-byte slots (rtc_quality.h): the cluster, the listed neighbours in it, the sum of their q
struct sil_shape {
  static constexpr uint32_t WAVE_ROW = SIL_WAVE_ROW, WAVE_SLOTS = SIL_WAVE_SLOTS, BLOCK_ROW = SIL_BLOCK_ROW, BLOCK_SLOTS = SIL_BLOCK_SLOTS;
  static constexpr uint32_t GLOBAL_LOG2_MIN = SIL_GLOBAL_LOG2_MIN;
  static constexpr uint32_t WGS_PER_CU[3] = {SIL_WAVE_WGS_PER_CU, SIL_BLOCK_WGS_PER_CU, SIL_GLOBAL_WGS_PER_CU};
  static constexpr bool CNT = true;
};
struct SilArgs { const uint64_t *row_off, *key, *w; const int32_t* label; const uint32_t* csize; uint32_t n_clustered; rtc_sil* out; };
struct SilBest { uint64_t S; uint32_t N, d; };  // (mean S / N, cluster) under sil_before
struct __attribute__((packed, aligned(4))) SilEnds {
  unsigned long long near;  // (q, cluster) of the nearest listed neighbour in another cluster: the least, q first
  uint32_t far;             // the largest q of a listed neighbour in the vertex's own cluster
};
// row_kernel's rule (rtc_rowtable.h) for row x, a clustered vertex with at least one entry.  Lane 0 writes the vertex's
// record; nothing else touches it.  A slot of a global table is read at device scope (RowTable: AGENT_READS).
struct sil_rule {
  typedef sil_shape shape;
  typedef RowTable<sil_shape::CNT, /* AGENT_READS */ true> Table;
  typedef SilArgs Args;
  typedef SilBest Best;
  struct Lds { Best best[4]; SilEnds ends[4]; };
  uint32_t c;
  SilEnds ends;

  static __device__ __forceinline__ void widen(SilEnds& m, const SilEnds& o) {
    m.far = o.far > m.far ? o.far : m.far;
    m.near = o.near < m.near ? o.near : m.near;
  }
  __device__ __forceinline__ bool enter(const Args& a, uint32_t x) {
    c = (uint32_t)a.label[x];
    ends = SilEnds{((unsigned long long)SIL_Q1 << 32) | LV_NONE, 0};
    return true;
  }
  __device__ __forceinline__ void gather(const Args& a, const Table& tab, uint32_t, uint64_t e) {
    const int32_t dl = a.label[(uint32_t)a.key[e]];
    if (dl < 0) return;  // an unclustered neighbour is no member of anything
    const uint32_t d = (uint32_t)dl, q = (uint32_t)a.w[e];
    const uint32_t h = tab.claim(d);
    atomicAdd(&tab.sum[h], (unsigned long long)q);
    atomicAdd(&tab.cnt[h], 1u);
    if (d == c) ends.far = q > ends.far ? q : ends.far;
    else {
      const unsigned long long cand = ((unsigned long long)q << 32) | d;
      ends.near = cand < ends.near ? cand : ends.near;
    }
  }
  template <int BLOCK>
  __device__ __forceinline__ void gathered(Lds& lds) { ends = row_reduce_wave<BLOCK>(ends, widen, lds.ends); }
  // (mean, cluster) of the best other cluster that holds a listed neighbour: none yet
  template <int BLOCK>
  __device__ __forceinline__ Best begin(const Args&, const Table&, uint32_t, const Lds& lds) {
    ends = row_reduce_all<BLOCK>(ends, widen, lds.ends);
    return Best{0, 0, LV_NONE};
  }
  __device__ __forceinline__ void sweep(const Args& a, const Table& tab, uint32_t s, Best& b) {
    const uint32_t d = tab.read(&tab.keys[s]);
    if (d == LV_NONE || d == c) return;
    const uint32_t N = a.csize[d];
    const uint64_t S = tab.read(&tab.sum[s]) + (uint64_t)(N - tab.read(&tab.cnt[s])) * SIL_Q1;
    if (sil_before(S, N, d, b.S, b.N, b.d)) b = Best{S, N, d};
  }
  static __device__ __forceinline__ void fold(Best& b, const Best& o) {
    if (sil_before(o.S, o.N, o.d, b.S, b.N, b.d)) b = o;
  }
  __device__ __forceinline__ void finish(const Args& a, const Table& tab, uint32_t x, uint64_t, const Best& b) {
    uint32_t cnt_c = 0;
    uint64_t sum_c = 0;
    const uint32_t h = tab.find(c);
    if (h != RT_NONE) { cnt_c = tab.read(&tab.cnt[h]); sum_c = tab.read(&tab.sum[h]); }
    rtc_sil r = sil_bare((int32_t)c, a.csize, a.n_clustered);
    const uint32_t nc = a.csize[c];
    r.a_num = sum_c + (uint64_t)(nc - 1 - cnt_c) * SIL_Q1;
    r.far_q = cnt_c < nc - 1 ? SIL_Q1 : ends.far;
    if (b.d != LV_NONE && b.S < (uint64_t)b.N * SIL_Q1) { r.b_num = b.S; r.b_den = b.N; r.b_cluster = b.d; }
    r.near_q = (uint32_t)(ends.near >> 32);
    r.near_cluster = (uint32_t)ends.near;
    a.out[x] = r;
  }
};

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
    // the rows by kernel path, and the tables of the long ones: the fill kernel's record of an unclustered vertex stands
    RowPaths<sil_shape> P;
    RTC_TRY(P.fetch(ctx, L.row_off, n));
    C[7] = now_ns() - t_csr;
    const uint64_t t_rows = now_ns();
    RTC_TRY(P.plan(ctx, who, ctx->opt.sil_global != 0, [&](uint32_t x) { return h_label[x] >= 0; }));
    const uint64_t need_tab = P.bytes() + 4096;
    const uint64_t free_tab = rtc_free_hbm(ctx);
    if (need_tab > free_tab)
      return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: %llu bytes for the row lists and %llu slots of global tables (%llu rows), %llu free", who,
                      (unsigned long long)need_tab, (unsigned long long)P.table_slots, (unsigned long long)P.lists[2].size(),
                      (unsigned long long)free_tab);
    for (int p = 0; p < 3; p++) C[4 + p] = P.lists[p].size();
    *path |= P.path_mask();
    RTC_TRY(P.alloc(ctx, L.db));
    RTC_TRY(P.launch<sil_rule>(ctx, SilArgs{L.row_off, L.key, L.w, d_label, d_csize, n_clustered, d_out}));
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
