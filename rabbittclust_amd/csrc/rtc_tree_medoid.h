// rtc_tree_medoid.h -- the host half of the --dedup-dist tree medoid (build_dedup_candidates_per_cluster_core,
// src/cluster_postprocess.cpp:60-156): the dedup groups, their CSR, the O(g^2) totals of one group and the reference's choice
// among the totals.  Plain C++17 without HIP, included by the HIP library (rtc_tree_medoids: host path, the groups it hands to
// the GPU, the final choice) and by the host library (the CPU test export), so both run the same code.
//
// The arithmetic the reference's result depends on, tie for tie:
//  - dist(c, v) is the fp64 sum accumulated from c outward along the unique tree path, one rounded add per edge
//    (distances_from, :33-54); any traversal order gives the same bits;
//  - total(c) adds dist(c, v) for the group's members v != c with dist >= 0, left to right in ascending id (:112-118);
//  - the choice: smaller total, then the longer sequence, then the smaller id (:121-127).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <limits>
#include <thread>
#include <vector>

#include "../../include/rtclust.h"

namespace rtc_tm {

// Union-find components of the edges with dist <= D that have two or more members; singletons stay out.
struct Groups {
  std::vector<int32_t> group;   // per node: its group, or -1 (a group of one)
  std::vector<uint64_t> goff;   // groups + 1 offsets into mem
  std::vector<int32_t> mem;     // every group's members, ascending by id
  std::vector<uint64_t> aoff;   // mem.size() + 1: CSR rows of the dedup subgraph, one per member (mem order)
  std::vector<uint32_t> anbr;   // neighbour, as its position in the group
  std::vector<double> aw;       // edge distance
  size_t count() const { return goff.empty() ? 0 : goff.size() - 1; }
  uint32_t size(size_t g) const { return (uint32_t)(goff[g + 1] - goff[g]); }
};

// false when an edge names a node outside [0, n) or the edges with dist <= D close a cycle (they must be a forest)
inline bool build_groups(int n, const rtc_edge* e, uint64_t m, double D, Groups& G) {
  std::vector<int32_t> up(n);
  for (int i = 0; i < n; i++) up[i] = i;
  auto find = [&](int32_t x) { while (up[x] != x) { up[x] = up[up[x]]; x = up[x]; } return x; };
  std::vector<uint32_t> deg(n, 0);
  for (uint64_t k = 0; k < m; k++) {
    if (!(e[k].dist <= D)) continue;
    const int32_t a = e[k].preNode, b = e[k].sufNode;
    if (a < 0 || a >= n || b < 0 || b >= n) return false;
    const int32_t ra = find(a), rb = find(b);
    if (ra == rb) return false;
    up[ra] = rb;
    deg[a]++; deg[b]++;
  }
  std::vector<uint32_t> gsize(n, 0);
  for (int i = 0; i < n; i++) gsize[find(i)]++;
  std::vector<int32_t> gid_of_root(n, -1);
  G.group.assign(n, -1);
  G.goff.assign(1, 0);
  std::vector<uint64_t> fill;  // next free slot of every group
  for (int i = 0; i < n; i++) {
    const int32_t r = find(i);
    if (gsize[r] < 2) continue;
    if (gid_of_root[r] < 0) { gid_of_root[r] = (int32_t)G.goff.size() - 1; fill.push_back(G.goff.back()); G.goff.push_back(G.goff.back() + gsize[r]); }
    G.group[i] = gid_of_root[r];
  }
  G.mem.assign(G.goff.back(), 0);
  std::vector<uint32_t> local(n, 0);
  for (int i = 0; i < n; i++) {  // ascending i: members ascending by id
    const int32_t g = G.group[i];
    if (g < 0) continue;
    local[i] = (uint32_t)(fill[g] - G.goff[g]);
    G.mem[fill[g]++] = i;
  }
  G.aoff.assign(G.mem.size() + 1, 0);
  for (size_t p = 0; p < G.mem.size(); p++) G.aoff[p + 1] = G.aoff[p] + deg[G.mem[p]];
  G.anbr.assign(G.aoff.back(), 0);
  G.aw.assign(G.aoff.back(), 0.0);
  std::vector<uint64_t> at(G.aoff.begin(), G.aoff.end() - 1);
  for (uint64_t k = 0; k < m; k++) {
    if (!(e[k].dist <= D)) continue;
    const int32_t a = e[k].preNode, b = e[k].sufNode;
    const uint64_t pa = G.goff[G.group[a]] + local[a], pb = G.goff[G.group[b]] + local[b];
    G.anbr[at[pa]] = local[b]; G.aw[at[pa]++] = e[k].dist;
    G.anbr[at[pb]] = local[a]; G.aw[at[pb]++] = e[k].dist;
  }
  return true;
}

// total(c) for the candidates c in [c0, c1) of group g: tot[c - c0].  dist / stack: scratch of the group's size.
inline void group_totals(const Groups& G, size_t g, uint32_t c0, uint32_t c1, double* tot, std::vector<double>& dist,
                         std::vector<uint32_t>& parent, std::vector<uint32_t>& stack) {
  const uint32_t sz = G.size(g);
  const uint64_t* off = G.aoff.data() + G.goff[g];
  dist.resize(sz); parent.resize(sz); stack.resize(sz);
  for (uint32_t c = c0; c < c1; c++) {
    std::fill(dist.begin(), dist.end(), -1.0);
    dist[c] = 0.0; parent[c] = c;
    uint32_t top = 0;
    stack[top++] = c;
    while (top > 0) {
      const uint32_t u = stack[--top];
      for (uint64_t k = off[u]; k < off[u + 1]; k++) {
        const uint32_t v = G.anbr[k];
        if (v == parent[u]) continue;
        parent[v] = u;
        dist[v] = dist[u] + G.aw[k];
        stack[top++] = v;
      }
    }
    double t = 0.0;
    for (uint32_t j = 0; j < sz; j++)
      if (j != c && dist[j] >= 0) t += dist[j];
    tot[c - c0] = t;
  }
}

// the reference's choice among the totals of group g (tot: one per member, mem order); seq_len may be NULL (all 0)
inline int32_t choose(const Groups& G, size_t g, const double* tot, const uint64_t* seq_len) {
  const int32_t* mem = G.mem.data() + G.goff[g];
  int32_t chosen = mem[0];
  double best = std::numeric_limits<double>::infinity();
  uint64_t chosen_len = 0;
  for (uint32_t j = 0; j < G.size(g); j++) {
    const int32_t cand = mem[j];
    const uint64_t len = seq_len ? seq_len[cand] : 0;
    if (tot[j] < best || (tot[j] == best && (len > chosen_len || (len == chosen_len && cand < chosen)))) {
      best = tot[j]; chosen = cand; chosen_len = len;
    }
  }
  return chosen;
}

// totals of every member of the groups listed in `which` (tot: one per member, mem order) on `threads` threads: whole groups
// when they are small, single candidates of the large ones
inline void totals_host(const Groups& G, const std::vector<uint32_t>& which, double* tot, int threads) {
  struct Unit { uint32_t g, c0, c1; };
  std::vector<Unit> units;
  for (uint32_t g : which) {
    const uint32_t sz = G.size(g);
    const uint32_t step = sz >= 256 ? 1 : sz;
    for (uint32_t c = 0; c < sz; c += step) units.push_back({g, c, std::min(sz, c + step)});
  }
  std::atomic<size_t> next{0};
  auto work = [&]() {
    std::vector<double> dist; std::vector<uint32_t> parent, stack;
    for (size_t u; (u = next.fetch_add(1, std::memory_order_relaxed)) < units.size();)
      group_totals(G, units[u].g, units[u].c0, units[u].c1, tot + G.goff[units[u].g] + units[u].c0, dist, parent, stack);
  };
  const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), units.size()));
  std::vector<std::thread> pool;
  for (int t = 1; t < T; t++) pool.emplace_back(work);
  work();
  for (std::thread& th : pool) th.join();
}

// node_to_rep from the groups and the totals of all their members
inline void assign(const Groups& G, int n, const double* tot, const uint64_t* seq_len, int32_t* node_to_rep) {
  std::vector<int32_t> rep(G.count());
  for (size_t g = 0; g < G.count(); g++) rep[g] = choose(G, g, tot + G.goff[g], seq_len);
  for (int i = 0; i < n; i++) node_to_rep[i] = G.group[i] < 0 ? i : rep[G.group[i]];
}

}  // namespace rtc_tm
