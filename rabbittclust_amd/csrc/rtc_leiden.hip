// rtc_leiden.hip -- rtc_leiden: the deterministic Leiden of clust-leiden --leiden, in exact integers (include/rtclust.h holds the
// definition, tests/refleiden.py restates it).  The levels' graphs, the row kernel and its three row-length paths are
// rtc_louvain's (rtc_community.h); here are what Leiden adds:
//   * the move phase starts from a given partition and scores with the objective's (A, B, nu);
//   * the refinement: leiden_inner_kernel and leiden_cut_kernel sum, entry by entry with integer atomics, a vertex's weight into
//     its coarse community and a refined community's weight to the rest of its coarse community; the row kernel in its PROPOSE
//     form finds every lone eligible vertex's best eligible target; leiden_accept_kernel applies the proposals whose target
//     does not propose itself (a community that has members holds the vertex it is named after, and that vertex is its only
//     member that can propose, so prop[d] answers for community d);
//   * the aggregation on the refined partition, the coarse community of the members carried up under the name of its smallest
//     member at the new level;
//   * the iterations from the level-0 graph, which is kept beside the working level.
#include "rtc_community.h"

namespace {

constexpr uint32_t LD_MAX_ITERATIONS = 100;

__global__ __launch_bounds__(256) void leiden_fill_kernel(uint32_t n, uint64_t value, uint64_t* __restrict__ out) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) out[x] = value;
}
// inner (zeroed) [x] = the weight from x to the members of its coarse community other than x
__global__ __launch_bounds__(256) void leiden_inner_kernel(const uint64_t* __restrict__ key, const uint64_t* __restrict__ w, uint64_t E,
                                                           const uint32_t* __restrict__ coarse, unsigned long long* __restrict__ inner) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t x = (uint32_t)(key[e] >> 32), y = (uint32_t)key[e];
    if (x != y && coarse[x] == coarse[y]) atomicAdd(&inner[x], (unsigned long long)w[e]);
  }
}
// elig[x] = inner_x A >= gB nu_x (N_C - nu_x), C the coarse community of x
__global__ __launch_bounds__(256) void leiden_eligible_kernel(const uint64_t* __restrict__ inner, const uint64_t* __restrict__ nu,
                                                              const uint64_t* __restrict__ tot_coarse, const uint32_t* __restrict__ coarse, uint32_t n,
                                                              uint64_t A, uint64_t gB, uint32_t* __restrict__ elig) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x)
    elig[x] = (i128)inner[x] * (i128)A >= (i128)gB * (i128)nu[x] * (i128)(tot_coarse[coarse[x]] - nu[x]) ? 1u : 0u;
}
// tot and members (both zeroed) of the refined communities
__global__ __launch_bounds__(256) void leiden_refined_totals_kernel(const uint32_t* __restrict__ R, const uint64_t* __restrict__ nu, uint32_t n,
                                                                    unsigned long long* __restrict__ tot, uint32_t* __restrict__ members) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
    atomicAdd(&tot[R[x]], (unsigned long long)nu[x]);
    atomicAdd(&members[R[x]], 1u);
  }
}
// cut (zeroed) [r] = the weight between refined community r and the rest of its coarse community
__global__ __launch_bounds__(256) void leiden_cut_kernel(const uint64_t* __restrict__ key, const uint64_t* __restrict__ w, uint64_t E,
                                                         const uint32_t* __restrict__ coarse, const uint32_t* __restrict__ R,
                                                         unsigned long long* __restrict__ cut) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t x = (uint32_t)(key[e] >> 32), y = (uint32_t)key[e];
    if (x != y && coarse[x] == coarse[y] && R[x] != R[y]) atomicAdd(&cut[R[x]], (unsigned long long)w[e]);
  }
}
// target[r] = r has members and cut_r A >= gB N_r (N_C - N_r); vertex r is a member of r, so coarse[r] names C
__global__ __launch_bounds__(256) void leiden_target_kernel(const uint64_t* __restrict__ cut, const uint64_t* __restrict__ tot_refined,
                                                            const uint32_t* __restrict__ members, const uint64_t* __restrict__ tot_coarse,
                                                            const uint32_t* __restrict__ coarse, uint32_t n, uint64_t A, uint64_t gB,
                                                            uint32_t* __restrict__ target) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
    target[r] = members[r] && (i128)cut[r] * (i128)A >= (i128)gB * (i128)tot_refined[r] * (i128)(tot_coarse[coarse[r]] - tot_refined[r]) ? 1u : 0u;
}
// cnt[0] accepted, cnt[1] rejected
__global__ __launch_bounds__(256) void leiden_accept_kernel(const uint32_t* __restrict__ prop, uint32_t n, uint32_t* __restrict__ R,
                                                            unsigned long long* __restrict__ cnt) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
    const uint32_t d = prop[x];
    if (d == LV_NONE) continue;
    if (prop[d] == LV_NONE) {
      R[x] = d;
      atomicAdd(&cnt[0], 1ull);
    } else {
      atomicAdd(&cnt[1], 1ull);
    }
  }
}
// smallest (all ones on entry) [C] = the smallest new number among the members of coarse community C
__global__ __launch_bounds__(256) void leiden_coarse_min_kernel(const uint32_t* __restrict__ coarse, const uint32_t* __restrict__ newc, uint32_t n,
                                                                uint32_t* __restrict__ smallest) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) atomicMin(&smallest[coarse[x]], newc[x]);
}
// the next level's coarse communities (every member of a new vertex writes the same value) and, nu_next not null, its node
// weights (zeroed on entry)
__global__ __launch_bounds__(256) void leiden_carry_kernel(const uint32_t* __restrict__ coarse, const uint32_t* __restrict__ newc,
                                                           const uint32_t* __restrict__ smallest, const uint64_t* __restrict__ nu, uint32_t n,
                                                           uint32_t* __restrict__ coarse_next, unsigned long long* __restrict__ nu_next) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
    coarse_next[newc[x]] = smallest[coarse[x]];
    if (nu_next) atomicAdd(&nu_next[newc[x]], (unsigned long long)nu[x]);
  }
}
// out[v] = map[label[v]]
__global__ __launch_bounds__(256) void leiden_gather_kernel(const uint32_t* __restrict__ map, const uint32_t* __restrict__ label, uint32_t n0,
                                                            uint32_t* __restrict__ out) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n0; v += gridDim.x * blockDim.x) out[v] = map[label[v]];
}

#define LD_LAUNCH(kernel, work, ...)                                                                         \
  do {                                                                                                       \
    hipLaunchKernelGGL(kernel, dim3(blocks_for((work), ctx->num_cu)), dim3(256), 0, s, __VA_ARGS__);        \
    RTC_CHECK_LAUNCH(ctx);                                                                                   \
  } while (0)

}  // namespace

extern "C" int rtc_leiden(rtc_ctx* ctx, uint32_t n, const rtc_wedge* h_edges, uint64_t m, double resolution, int objective, int32_t* h_labels,
                          uint32_t* h_n_clusters, double* h_quality) {
  const char* who = "rtc_leiden";
  if (!ctx || !h_n_clusters || (n && !h_labels) || (m && !h_edges)) return RTC_ERR_ARG;
  if (objective != RTC_LEIDEN_CPM && objective != RTC_LEIDEN_MODULARITY) return rtc_fail(ctx, RTC_ERR_ARG, "%s: objective %d", who, objective);
  if (!(resolution > 0.0) || !(resolution * 65536.0 < 4294967295.5)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: resolution %g", who, resolution);
  const uint64_t g = (uint64_t)llround(resolution * 65536.0);
  if (g == 0 || g >= (1ull << 32)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: resolution %g", who, resolution);
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u vertices", who, n);
  uint64_t M2 = 0;
  for (uint64_t e = 0; e < m; e++) {
    if (h_edges[e].u >= n || h_edges[e].v >= n || h_edges[e].q == 0)
      return rtc_fail(ctx, RTC_ERR_ARG, "%s: record %llu is (%u, %u, %u) with %u vertices", who, (unsigned long long)e, h_edges[e].u, h_edges[e].v,
                      h_edges[e].q, n);
    M2 += 2ull * h_edges[e].q;
    if (M2 >= (1ull << 46)) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: total weight past 2^46 units", who);
  }
  memset(ctx->leiden, 0, sizeof ctx->leiden);
  *h_n_clusters = n;
  if (h_quality) *h_quality = 0.0;
  for (uint32_t x = 0; x < n; x++) h_labels[x] = (int32_t)x;
  if (m == 0 || n == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  uint64_t* C = ctx->leiden;
  const bool cpm = objective == RTC_LEIDEN_CPM;
  const uint64_t A = cpm ? 65536ull : M2 << 16, gB = cpm ? g << 20 : g;

  Louvain L{ctx};
  const uint64_t E0 = 2 * m;
  RTC_TRY(L.alloc(n, E0));
  uint64_t *key0 = nullptr, *w0 = nullptr, *row0 = nullptr, *k0 = nullptr;  // the level-0 graph, kept for the next iteration
  uint64_t *nu_a = nullptr, *nu_b = nullptr, *tot_refined = nullptr, *acc = nullptr;
  uint32_t *R = nullptr, *prop = nullptr, *elig = nullptr, *members = nullptr, *target = nullptr, *coarse_next = nullptr, *start = nullptr, *fin = nullptr;
  unsigned long long* d_cnt = nullptr;  // [0] moves or proposals, [1] accepted, [2] rejected
  RTC_TRY(L.db.get(ctx, E0, &key0));
  RTC_TRY(L.db.get(ctx, E0, &w0));
  RTC_TRY(L.db.get(ctx, (size_t)n + 1, &row0));
  for (uint64_t** p : {&k0, &nu_a, &nu_b, &tot_refined, &acc}) RTC_TRY(L.db.get(ctx, n, p));
  for (uint32_t** p : {&R, &prop, &elig, &members, &target, &coarse_next, &start, &fin}) RTC_TRY(L.db.get(ctx, n, p));
  RTC_TRY(L.db.get(ctx, 4, &d_cnt));
  {
    rtc_wedge* d_edges = nullptr;
    RTC_TRY(L.db.get(ctx, m, &d_edges));
    RTC_HIP(ctx, hipMemcpyAsync(d_edges, h_edges, m * sizeof(rtc_wedge), hipMemcpyHostToDevice, s));
    LD_LAUNCH(louvain_entries_kernel, m, (const rtc_wedge*)d_edges, m, L.key_in, L.w);
    RTC_HIP(ctx, hipStreamSynchronize(s));
    L.db.release(d_edges);
  }
  uint64_t E_level0 = 0;
  RTC_TRY(L.build(n, E0, &E_level0));
  RTC_HIP(ctx, hipMemcpyAsync(key0, L.key, E_level0 * 8, hipMemcpyDeviceToDevice, s));
  RTC_HIP(ctx, hipMemcpyAsync(w0, L.w, E_level0 * 8, hipMemcpyDeviceToDevice, s));
  RTC_HIP(ctx, hipMemcpyAsync(row0, L.row_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToDevice, s));
  RTC_HIP(ctx, hipMemcpyAsync(k0, L.k, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
  LD_LAUNCH(louvain_iota_kernel, n, n, start);

  std::vector<int32_t> h_new(n);
  RowPaths<lv_shape> P;
  uint32_t ncl = n;
  for (uint32_t iteration = 0; iteration < LD_MAX_ITERATIONS; iteration++) {
    uint32_t nl = n;
    uint64_t E = E_level0;
    if (iteration) {
      RTC_HIP(ctx, hipMemcpyAsync(L.key, key0, E * 8, hipMemcpyDeviceToDevice, s));
      RTC_HIP(ctx, hipMemcpyAsync(L.w, w0, E * 8, hipMemcpyDeviceToDevice, s));
      RTC_HIP(ctx, hipMemcpyAsync(L.row_off, row0, ((size_t)n + 1) * 8, hipMemcpyDeviceToDevice, s));
      RTC_HIP(ctx, hipMemcpyAsync(L.k, k0, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    }
    LD_LAUNCH(louvain_iota_kernel, n, n, L.label);
    RTC_HIP(ctx, hipMemcpyAsync(L.comm, start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    uint64_t *nu = cpm ? nu_a : L.k, *nu_next = cpm ? nu_b : nullptr;
    if (cpm) LD_LAUNCH(leiden_fill_kernel, n, n, (uint64_t)1, nu);

    uint32_t levels = 0;
    for (;;) {
      RTC_TRY(P.prepare(ctx, L.db, L.row_off, nl, who));
      // ---- (a) the move phase, from the partition in L.comm ----
      uint64_t t0 = now_ns();
      RTC_HIP(ctx, hipMemsetAsync(L.tot, 0, (size_t)nl * 8, s));
      LD_LAUNCH(louvain_totals_kernel, nl, (const uint32_t*)L.comm, (const uint64_t*)nu, nl, (unsigned long long*)L.tot);
      uint32_t rounds = 0, idle = 0;
      while (rounds < LV_MAX_ROUNDS && idle < 2) {
        const LevelView G{L.row_off, L.key, L.w, nu, L.tot, L.comm, nullptr, nullptr, nullptr, nullptr};
        RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 8, s));
        RTC_HIP(ctx, hipMemcpyAsync(L.comm_new, L.comm, (size_t)nl * 4, hipMemcpyDeviceToDevice, s));
        RTC_TRY(P.launch<move_rule<false>>(ctx, MoveArgs{G, A, gB, (int)(rounds & 1), L.comm_new, d_cnt}));
        std::swap(L.comm, L.comm_new);
        RTC_HIP(ctx, hipMemsetAsync(L.tot, 0, (size_t)nl * 8, s));
        LD_LAUNCH(louvain_totals_kernel, nl, (const uint32_t*)L.comm, (const uint64_t*)nu, nl, (unsigned long long*)L.tot);
        unsigned long long moved = 0;
        RTC_HIP(ctx, hipMemcpyAsync(&moved, d_cnt, 8, hipMemcpyDeviceToHost, s));
        RTC_HIP(ctx, hipStreamSynchronize(s));
        rounds++;
        C[3] += moved;
        idle = moved ? 0 : idle + 1;
      }
      C[2] += rounds;
      C[7] += now_ns() - t0;

      // ---- (b) the refinement inside the coarse communities L.comm, whose totals L.tot holds ----
      t0 = now_ns();
      const uint32_t* coarse = L.comm;
      LD_LAUNCH(louvain_iota_kernel, nl, nl, R);
      RTC_HIP(ctx, hipMemsetAsync(acc, 0, (size_t)nl * 8, s));
      LD_LAUNCH(leiden_inner_kernel, E, (const uint64_t*)L.key, (const uint64_t*)L.w, E, coarse, (unsigned long long*)acc);
      LD_LAUNCH(leiden_eligible_kernel, nl, (const uint64_t*)acc, (const uint64_t*)nu, (const uint64_t*)L.tot, coarse, nl, A, gB, elig);
      uint64_t merges = 0;
      rounds = idle = 0;
      while (rounds < LV_MAX_ROUNDS && idle < 2) {
        RTC_HIP(ctx, hipMemsetAsync(tot_refined, 0, (size_t)nl * 8, s));
        RTC_HIP(ctx, hipMemsetAsync(members, 0, (size_t)nl * 4, s));
        LD_LAUNCH(leiden_refined_totals_kernel, nl, (const uint32_t*)R, (const uint64_t*)nu, nl, (unsigned long long*)tot_refined, members);
        RTC_HIP(ctx, hipMemsetAsync(acc, 0, (size_t)nl * 8, s));
        LD_LAUNCH(leiden_cut_kernel, E, (const uint64_t*)L.key, (const uint64_t*)L.w, E, coarse, (const uint32_t*)R, (unsigned long long*)acc);
        LD_LAUNCH(leiden_target_kernel, nl, (const uint64_t*)acc, (const uint64_t*)tot_refined, (const uint32_t*)members, (const uint64_t*)L.tot,
                  coarse, nl, A, gB, target);
        RTC_HIP(ctx, hipMemsetAsync(prop, 0xff, (size_t)nl * 4, s));
        RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, 3 * 8, s));
        const LevelView G{L.row_off, L.key, L.w, nu, tot_refined, R, coarse, elig, members, target};
        RTC_TRY(P.launch<move_rule<true>>(ctx, MoveArgs{G, A, gB, (int)(rounds & 1), prop, d_cnt}));
        LD_LAUNCH(leiden_accept_kernel, nl, (const uint32_t*)prop, nl, R, d_cnt + 1);
        unsigned long long cnt[3] = {0, 0, 0};
        RTC_HIP(ctx, hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, s));
        RTC_HIP(ctx, hipStreamSynchronize(s));
        rounds++;
        merges += cnt[1];
        C[6] += cnt[2];
        idle = cnt[1] ? 0 : idle + 1;
      }
      C[4] += rounds;
      C[5] += merges;
      C[8] += now_ns() - t0;
      P.release(L.db);
      levels++;
      C[1]++;
      if (!merges || levels == LV_MAX_LEVELS) break;

      // ---- (c) the refined communities, numbered by their smallest member, become the vertices ----
      RTC_HIP(ctx, hipMemsetAsync(L.smallest, 0xff, (size_t)nl * 4, s));
      LD_LAUNCH(louvain_smallest_kernel, nl, (const uint32_t*)R, nl, L.smallest);
      LD_LAUNCH(louvain_heads_kernel, nl, (const uint32_t*)R, (const uint32_t*)L.smallest, nl, L.head);
      size_t tb = L.tmp_bytes;
      RTC_HIP(ctx, rocprim::exclusive_scan(L.tmp, tb, (const uint32_t*)L.head, L.rank, 0u, (size_t)nl, rocprim::plus<uint32_t>(), s));
      LD_LAUNCH(louvain_newc_kernel, nl, (const uint32_t*)R, (const uint32_t*)L.smallest, (const uint32_t*)L.rank, nl, L.newc);
      LD_LAUNCH(louvain_compose_kernel, n, (const uint32_t*)L.newc, n, L.label);
      uint32_t last[2] = {0, 0};  // the number of refined communities: the last vertex's rank, and one more if it heads one
      RTC_HIP(ctx, hipMemcpyAsync(&last[0], L.rank + (nl - 1), 4, hipMemcpyDeviceToHost, s));
      RTC_HIP(ctx, hipMemcpyAsync(&last[1], L.head + (nl - 1), 4, hipMemcpyDeviceToHost, s));
      RTC_HIP(ctx, hipMemsetAsync(L.smallest, 0xff, (size_t)nl * 4, s));  // now by coarse community, in the new numbers
      LD_LAUNCH(leiden_coarse_min_kernel, nl, coarse, (const uint32_t*)L.newc, nl, L.smallest);
      if (nu_next) RTC_HIP(ctx, hipMemsetAsync(nu_next, 0, (size_t)nl * 8, s));
      LD_LAUNCH(leiden_carry_kernel, nl, coarse, (const uint32_t*)L.newc, (const uint32_t*)L.smallest, (const uint64_t*)nu, nl, coarse_next,
                (unsigned long long*)nu_next);
      LD_LAUNCH(louvain_rekey_kernel, E, (const uint64_t*)L.key, E, (const uint32_t*)L.newc, L.key_in);
      RTC_HIP(ctx, hipStreamSynchronize(s));
      nl = last[0] + last[1];
      RTC_TRY(L.build(nl, E, &E));
      std::swap(L.comm, coarse_next);
      if (cpm) std::swap(nu, nu_next);
      else nu = L.k;
    }

    // ---- the iteration's result: the coarse communities down at the original vertices, numbered by their smallest one ----
    LD_LAUNCH(leiden_gather_kernel, n, (const uint32_t*)L.comm, (const uint32_t*)L.label, n, fin);
    RTC_HIP(ctx, hipMemsetAsync(L.smallest, 0xff, (size_t)n * 4, s));
    LD_LAUNCH(louvain_smallest_kernel, n, (const uint32_t*)fin, n, L.smallest);
    LD_LAUNCH(louvain_heads_kernel, n, (const uint32_t*)fin, (const uint32_t*)L.smallest, n, L.head);
    size_t tb = L.tmp_bytes;
    RTC_HIP(ctx, rocprim::exclusive_scan(L.tmp, tb, (const uint32_t*)L.head, L.rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), s));
    LD_LAUNCH(louvain_newc_kernel, n, (const uint32_t*)fin, (const uint32_t*)L.smallest, (const uint32_t*)L.rank, n, L.newc);
    LD_LAUNCH(leiden_gather_kernel, n, (const uint32_t*)L.smallest, (const uint32_t*)fin, n, start);  // named by the smallest member
    uint32_t last[2] = {0, 0};
    RTC_HIP(ctx, hipMemcpyAsync(&last[0], L.rank + (n - 1), 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipMemcpyAsync(&last[1], L.head + (n - 1), 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipMemcpyAsync(h_new.data(), L.newc, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    ncl = last[0] + last[1];
    C[0]++;
    const bool same = memcmp(h_new.data(), h_labels, (size_t)n * 4) == 0;
    memcpy(h_labels, h_new.data(), (size_t)n * 4);
    if (same) break;
  }

  *h_n_clusters = ncl;
  if (h_quality) {  // on the host, from the labels
    std::vector<uint64_t> in(ncl, 0), tot(ncl, 0), size(ncl, 0);
    for (uint32_t x = 0; x < n; x++) size[(uint32_t)h_labels[x]]++;
    for (uint64_t e = 0; e < m; e++) {
      const uint32_t cu = (uint32_t)h_labels[h_edges[e].u], cv = (uint32_t)h_labels[h_edges[e].v];
      tot[cu] += h_edges[e].q;
      tot[cv] += h_edges[e].q;
      if (cu == cv) in[cu] += 2ull * h_edges[e].q;
    }
    i128 num = 0;
    for (uint32_t c = 0; c < ncl; c++)
      num += cpm ? (i128)in[c] * 65536 - (i128)(g << 20) * (i128)size[c] * (i128)size[c]
                 : (i128)in[c] * ((i128)M2 << 16) - (i128)g * (i128)tot[c] * (i128)tot[c];
    *h_quality = cpm ? (double)num / ((double)M2 * 65536.0) : (double)num / ((double)M2 * (double)M2 * 65536.0);
  }
  C[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_leiden_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->leiden[i];
  return RTC_OK;
}
