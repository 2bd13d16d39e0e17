// rtc_hierarchy_host.hip -- what a caller does with rtc_dbscan_hierarchy's forest, on the host alone (no context, no device):
// rtc_hierarchy_cut, DBSCAN*'s clusters at any eps up to eps_max, and rtc_hierarchy_flat, the condensed tree selected by excess
// of mass.  include/rtclust.h defines both to the last tie; this file follows it line by line.  Built with -ffp-contract=off
// like the DBSCAN units, so the predicate gives the bits rtc_dbscan's gives.
#include <limits>

#include "rtc_dbscan_common.h"

namespace {

constexpr uint32_t H_NONE = 0xffffffffu;
constexpr double HIER_MIN_DIST = 1e-12;

inline bool triple_passes(uint32_t common, uint32_t a, uint32_t b, double t, double one_plus_t) {
  if (a == 0 && b == 0) return true;  // two empty u64 sketches: the brute force accepts them at every eps
  return eps_pred(a, b, common, t, one_plus_t) && eps_pred(b, a, common, t, one_plus_t);
}

inline double triple_distance(uint32_t common, uint32_t a, uint32_t b, int kmer_size) {
  const uint64_t denom = (uint64_t)a + b - common;
  if (denom == common) return 0.0;
  const double j = (double)common / (double)denom;
  return -log(2.0 * j / (1.0 + j)) / kmer_size;
}

struct Dsu {
  std::vector<uint32_t> p;
  explicit Dsu(uint32_t n) : p(n) { for (uint32_t i = 0; i < n; i++) p[i] = i; }
  uint32_t find(uint32_t x) {
    while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; }
    return x;
  }
};

}  // namespace

extern "C" int rtc_hierarchy_cut(uint32_t n, const rtc_hedge* h_forest, uint64_t n_forest, const rtc_kdist* h_core, double eps_max, double eps,
                                 int kmer_size, int32_t* h_labels, uint8_t* h_is_core, uint32_t* n_clusters) {
  if ((n && (!h_core || !h_labels)) || (n_forest && !h_forest) || n_forest >= (n ? n : 1)) return RTC_ERR_ARG;
  if (!(eps > 0.0) || !(eps <= eps_max)) return RTC_ERR_ARG;
  const double x = exp(-eps * kmer_size);
  const double t = x / (2.0 - x), one_plus_t = 1.0 + t;
  if (!(t > 1e-12)) return RTC_ERR_UNSUPPORTED;
  std::vector<uint8_t> core(n);
  for (uint32_t p = 0; p < n; p++) {
    const rtc_kdist& c = h_core[p];
    core[p] = c.neighbour != H_NONE && triple_passes(c.common, c.size_p, c.size_q, t, one_plus_t);
    if (h_is_core) h_is_core[p] = core[p];
  }
  Dsu d(n);
  for (uint64_t e = 0; e < n_forest; e++) {
    const rtc_hedge& h = h_forest[e];
    if (h.p >= n || h.q >= n) return RTC_ERR_ARG;
    if (!core[h.p] || !core[h.q] || !triple_passes(h.common, h.size_p, h.size_q, t, one_plus_t)) continue;
    const uint32_t a = d.find(h.p), b = d.find(h.q);
    if (a != b) d.p[std::max(a, b)] = std::min(a, b);  // the root is the smallest index
  }
  uint32_t ncl = 0;
  std::vector<int32_t> id(n, -1);
  for (uint32_t p = 0; p < n; p++) {
    if (!core[p]) { h_labels[p] = -1; continue; }
    const uint32_t r = d.find(p);
    if (id[r] < 0) id[r] = (int32_t)ncl++;  // first met at its smallest core index
    h_labels[p] = id[r];
  }
  if (n_clusters) *n_clusters = ncl;
  return RTC_OK;
}

extern "C" int rtc_hierarchy_flat(uint32_t n, const rtc_hedge* h_forest, uint64_t n_forest, const rtc_kdist* h_core, int kmer_size,
                                  int min_cluster_size, int32_t* h_labels, double* h_stability, uint32_t* n_clusters) {
  if ((n && (!h_core || !h_labels)) || (n_forest && !h_forest) || n_forest >= (n ? n : 1) || min_cluster_size < 2 || kmer_size < 1)
    return RTC_ERR_ARG;
  const uint64_t F = n_forest, mcs = (uint64_t)min_cluster_size;
  constexpr int32_t NO = -1;
  // the dendrogram: leaf v < n, the merge of forest edge e is node n + e
  std::vector<uint32_t> left(F), right(F), top(n);  // top[root of a component] = its dendrogram node
  std::vector<uint64_t> size((size_t)n + F, 1);
  std::vector<double> lambda(F);
  Dsu d(n);
  for (uint32_t v = 0; v < n; v++) top[v] = v;
  for (uint64_t e = 0; e < F; e++) {
    const rtc_hedge& h = h_forest[e];
    if (h.p >= n || h.q >= n || h_core[h.p].neighbour == H_NONE || h_core[h.q].neighbour == H_NONE) return RTC_ERR_ARG;
    const uint32_t a = d.find(h.p), b = d.find(h.q);
    if (a == b) return RTC_ERR_ARG;  // not a forest
    left[e] = top[a]; right[e] = top[b];
    size[n + e] = size[left[e]] + size[right[e]];
    lambda[e] = 1.0 / std::max(triple_distance(h.common, h.size_p, h.size_q, kmer_size), HIER_MIN_DIST);
    d.p[b] = a;
    top[a] = (uint32_t)(n + e);
  }
  // top down: the cluster every node sits in (NO: none), whether it has already fallen out of it, the clusters' tree
  std::vector<int32_t> node_cluster((size_t)n + F, NO);
  std::vector<uint8_t> fallen((size_t)n + F, 0);
  std::vector<int32_t> parent, child_l, child_r;
  std::vector<double> birth, stab;
  auto new_cluster = [&](int32_t par, double b) {
    parent.push_back(par); child_l.push_back(NO); child_r.push_back(NO); birth.push_back(b); stab.push_back(0.0);
    return (int32_t)parent.size() - 1;
  };
  uint32_t n_top = 0;
  for (uint32_t v = 0; v < n; v++)  // the trees' roots, in index order of their first points
    if (d.find(v) == v && h_core[v].neighbour != H_NONE && size[top[v]] >= mcs) { node_cluster[top[v]] = new_cluster(NO, 0.0); n_top++; }
  std::vector<int32_t> term_cluster(F, NO);
  std::vector<double> term(F, 0.0);
  for (uint64_t e = F; e-- > 0;) {
    const size_t node = (size_t)n + e;
    const int32_t c = node_cluster[node];
    const uint32_t l = left[e], r = right[e];
    if (c == NO) continue;  // a tree below min_cluster_size: its points stay -1
    if (fallen[node]) { node_cluster[l] = node_cluster[r] = c; fallen[l] = fallen[r] = 1; continue; }
    const bool bl = size[l] >= mcs, br = size[r] >= mcs;
    uint64_t leaving = 0;
    if (bl && br) {
      leaving = size[l] + size[r];
      const int32_t cl = new_cluster(c, lambda[e]), cr = new_cluster(c, lambda[e]);
      child_l[c] = cl; child_r[c] = cr;
      node_cluster[l] = cl; node_cluster[r] = cr;
    } else {
      node_cluster[l] = node_cluster[r] = c;
      if (!bl) { leaving += size[l]; fallen[l] = 1; }
      if (!br) { leaving += size[r]; fallen[r] = 1; }
    }
    term_cluster[e] = c;
    term[e] = (double)leaving * (lambda[e] - birth[c]);
  }
  for (uint64_t e = 0; e < F; e++)  // the sums in forest order
    if (term_cluster[e] != NO) stab[term_cluster[e]] += term[e];
  // excess of mass, leaves first (children carry larger numbers than their parents)
  const int32_t C = (int32_t)parent.size();
  std::vector<uint8_t> selected(C, 0);
  std::vector<double> best(C, 0.0);
  for (int32_t c = C; c-- > 0;) {
    if (child_l[c] == NO) { selected[c] = 1; best[c] = stab[c]; continue; }
    const double below = best[child_l[c]] + best[child_r[c]];
    const bool root = parent[c] == NO && n_top == 1;
    if (!root && stab[c] > below) { selected[c] = 1; best[c] = stab[c]; }
    else best[c] = below;
  }
  // the selected cluster nearest the top covers everything below it
  std::vector<int32_t> shown(C, NO);
  for (int32_t c = 0; c < C; c++) {
    const int32_t up = parent[c] == NO ? NO : shown[parent[c]];
    shown[c] = up != NO ? up : selected[c] ? c : NO;
  }
  std::vector<int32_t> number(C, NO);
  uint32_t ncl = 0;
  for (uint32_t v = 0; v < n; v++) {
    const int32_t c = node_cluster[v] == NO ? NO : shown[node_cluster[v]];
    if (c == NO) { h_labels[v] = -1; continue; }
    if (number[c] == NO) {
      if (h_stability) h_stability[ncl] = stab[c];
      number[c] = (int32_t)ncl++;
    }
    h_labels[v] = number[c];
  }
  if (n_clusters) *n_clusters = ncl;
  return RTC_OK;
}
