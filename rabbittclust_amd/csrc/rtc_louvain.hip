// rtc_louvain.hip -- rtc_louvain: the deterministic Louvain of clust-leiden --louvain, in exact integers (include/rtclust.h holds
// the definition, tests/reflouvain.py restates it).
//   * A level's graph is a CSR of (row << 32 | column) keys in ascending order with u64 weights, built by one rocPRIM radix sort
//     and one reduce_by_key over the directed entries: the input's at level 0, the relabelled entries of the level below after.
//   * row_kernel (rtc_rowtable.h) under move_rule (rtc_community.h, shared with rtc_leiden.hip) is the hot path: one row per
//     workgroup, the weights to the neighbouring communities summed in a hash table over community ids (integer atomics: the sums do not depend on the order), every occupied slot scored in 128-bit
//     integers, the best (score, then smaller id) reduced over the workgroup.  Three launches share the code:
//       - rows of up to LV_WAVE_ROW entries: a workgroup of ONE wave, its table of LV_WAVE_SLOTS slots in LDS (3 KiB);
//       - rows of up to LV_BLOCK_ROW entries: 256 lanes, LV_BLOCK_SLOTS slots in LDS (48 KiB, three workgroups on a CU's 160 KiB);
//       - longer rows: 256 lanes, a table of at least twice the row's entries in global memory.
//     A table always has at least two slots per entry of its row, so a probe ends.  The outcome of a row is the maximum of a
//     total order over exact integers and so the same on every path.
//   * After a round tot is rebuilt from the memberships (integer atomics).  After a level the communities are numbered by
//     their smallest member: an atomic minimum per community, a scan over the vertices that are such a minimum.
#include "rtc_community.h"

extern "C" int rtc_louvain(rtc_ctx* ctx, uint32_t n, const rtc_wedge* h_edges, uint64_t m, double resolution, int32_t* h_labels,
                           uint32_t* h_n_clusters, double* h_modularity) {
  const char* who = "rtc_louvain";
  if (!ctx || !h_n_clusters || (n && !h_labels) || (m && !h_edges)) return RTC_ERR_ARG;
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
  memset(ctx->louvain, 0, sizeof ctx->louvain);
  *h_n_clusters = n;
  if (h_modularity) *h_modularity = 0.0;
  for (uint32_t x = 0; x < n; x++) h_labels[x] = (int32_t)x;
  if (m == 0 || n == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  uint64_t* C = ctx->louvain;

  Louvain L{ctx};
  const uint64_t E0 = 2 * m;
  RTC_TRY(L.alloc(n, E0));
  {
    rtc_wedge* d_edges = nullptr;
    RTC_TRY(L.db.get(ctx, m, &d_edges));
    RTC_HIP(ctx, hipMemcpyAsync(d_edges, h_edges, m * sizeof(rtc_wedge), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(louvain_entries_kernel, dim3(blocks_for(m, ctx->num_cu)), dim3(256), 0, s, (const rtc_wedge*)d_edges, m, L.key_in, L.w);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipStreamSynchronize(s));
    L.db.release(d_edges);
  }
  uint32_t nl = n;
  uint64_t E = 0;
  uint64_t t0 = now_ns();
  RTC_TRY(L.build(nl, E0, &E));
  hipLaunchKernelGGL(louvain_iota_kernel, dim3(blocks_for(n, ctx->num_cu)), dim3(256), 0, s, n, L.label);
  RTC_CHECK_LAUNCH(ctx);
  C[7] += now_ns() - t0;

  RowPaths<lv_shape> P;
  uint32_t levels = 0;
  while (levels < LV_MAX_LEVELS) {
    RTC_TRY(P.prepare(ctx, L.db, L.row_off, nl, who));
    hipLaunchKernelGGL(louvain_iota_kernel, dim3(blocks_for(nl, ctx->num_cu)), dim3(256), 0, s, nl, L.comm);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemcpyAsync(L.tot, L.k, (size_t)nl * 8, hipMemcpyDeviceToDevice, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));  // the host lists are rewritten at the next level

    t0 = now_ns();
    uint32_t rounds = 0, idle = 0;
    uint64_t level_moves = 0;
    while (rounds < LV_MAX_ROUNDS && idle < 2) {
      const LevelView G{L.row_off, L.key, L.w, L.k, L.tot, L.comm, nullptr, nullptr, nullptr, nullptr};
      const int odd = (int)(rounds & 1);
      RTC_HIP(ctx, hipMemsetAsync(L.d_cnt + 1, 0, 8, s));
      RTC_HIP(ctx, hipMemcpyAsync(L.comm_new, L.comm, (size_t)nl * 4, hipMemcpyDeviceToDevice, s));
      RTC_TRY(P.launch<move_rule<false>>(ctx, MoveArgs{G, M2 << 16, g, odd, L.comm_new, L.d_cnt + 1}));
      std::swap(L.comm, L.comm_new);
      RTC_HIP(ctx, hipMemsetAsync(L.tot, 0, (size_t)nl * 8, s));
      hipLaunchKernelGGL(louvain_totals_kernel, dim3(blocks_for(nl, ctx->num_cu)), dim3(256), 0, s, (const uint32_t*)L.comm, (const uint64_t*)L.k, nl,
                         (unsigned long long*)L.tot);
      RTC_CHECK_LAUNCH(ctx);
      unsigned long long moved = 0;
      RTC_HIP(ctx, hipMemcpyAsync(&moved, L.d_cnt + 1, 8, hipMemcpyDeviceToHost, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
      rounds++;
      level_moves += moved;
      idle = moved ? 0 : idle + 1;
      C[5] += P.lists[1].size() + P.lists[2].size();
      C[8] += P.lists[2].size();
    }
    C[6] += now_ns() - t0;
    P.release(L.db);
    levels++;
    C[0] = levels; C[1] += rounds; C[2] += level_moves; C[3] = nl; C[4] = E;
    if (!level_moves) break;

    // ---- the next level: communities numbered by their smallest member, the entries renamed and summed ----
    t0 = now_ns();
    RTC_HIP(ctx, hipMemsetAsync(L.smallest, 0xff, (size_t)nl * 4, s));
    hipLaunchKernelGGL(louvain_smallest_kernel, dim3(blocks_for(nl, ctx->num_cu)), dim3(256), 0, s, (const uint32_t*)L.comm, nl, L.smallest);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(louvain_heads_kernel, dim3(blocks_for(nl, ctx->num_cu)), dim3(256), 0, s, (const uint32_t*)L.comm, (const uint32_t*)L.smallest,
                       nl, L.head);
    RTC_CHECK_LAUNCH(ctx);
    size_t tb = L.tmp_bytes;
    RTC_HIP(ctx, rocprim::exclusive_scan(L.tmp, tb, (const uint32_t*)L.head, L.rank, 0u, (size_t)nl, rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(louvain_newc_kernel, dim3(blocks_for(nl, ctx->num_cu)), dim3(256), 0, s, (const uint32_t*)L.comm, (const uint32_t*)L.smallest,
                       (const uint32_t*)L.rank, nl, L.newc);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(louvain_compose_kernel, dim3(blocks_for(n, ctx->num_cu)), dim3(256), 0, s, (const uint32_t*)L.newc, n, L.label);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(louvain_rekey_kernel, dim3(blocks_for(E, ctx->num_cu)), dim3(256), 0, s, (const uint64_t*)L.key, E, (const uint32_t*)L.newc,
                       L.key_in);
    RTC_CHECK_LAUNCH(ctx);
    uint32_t last[2] = {0, 0};  // the number of communities: the last vertex's rank, and one more if it heads one
    RTC_HIP(ctx, hipMemcpyAsync(&last[0], L.rank + (nl - 1), 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipMemcpyAsync(&last[1], L.head + (nl - 1), 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    nl = last[0] + last[1];
    RTC_TRY(L.build(nl, E, &E));
    C[7] += now_ns() - t0;
    C[3] = nl; C[4] = E;
  }

  RTC_HIP(ctx, hipMemcpyAsync(h_labels, L.label, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  *h_n_clusters = nl;
  if (h_modularity) {  // on the host, from the labels: in_c and tot_c as the definition's last level holds them
    std::vector<uint64_t> in(nl, 0), tot(nl, 0);
    for (uint64_t e = 0; e < m; e++) {
      const uint32_t cu = (uint32_t)h_labels[h_edges[e].u], cv = (uint32_t)h_labels[h_edges[e].v];
      tot[cu] += h_edges[e].q;
      tot[cv] += h_edges[e].q;
      if (cu == cv) in[cu] += 2ull * h_edges[e].q;
    }
    i128 num = 0;
    for (uint32_t c = 0; c < nl; c++) num += (i128)in[c] * ((i128)M2 << 16) - (i128)g * (i128)tot[c] * (i128)tot[c];
    *h_modularity = (double)num / ((double)M2 * (double)M2 * 65536.0);
  }
  C[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_louvain_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->louvain[i];
  return RTC_OK;
}
