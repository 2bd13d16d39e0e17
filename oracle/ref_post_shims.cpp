// extern "C" wrappers over the reference's --dedup-dist / --reps-per-cluster functions (build_dedup_candidates_per_cluster,
// KSSD overload, and select_k_reps_per_cluster_tree of its src/cluster_postprocess.cpp).  oracle/Makefile names that source
// and this file on one compiler line; the result is oracle/_ref/libref_post.so, which tests/reflib.py loads.
// TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "cluster_postprocess.h"

namespace {

std::vector<std::vector<int>> lists_of(int n_lists, const int64_t* off, const int32_t* flat) {
  std::vector<std::vector<int>> out((size_t)n_lists);
  for (int c = 0; c < n_lists; c++) out[c].assign(flat + off[c], flat + off[c + 1]);
  return out;
}

// lists into off[n_lists + 1] / flat (capacity cap).  Returns the total length, or -1 when it does not fit.
int64_t lists_out(const std::vector<std::vector<int>>& lists, int64_t* off, int32_t* flat, int64_t cap) {
  int64_t at = 0;
  for (size_t c = 0; c < lists.size(); c++) {
    off[c] = at;
    for (int v : lists[c]) {
      if (at >= cap) return -1;
      flat[at++] = v;
    }
  }
  off[lists.size()] = at;
  return at;
}

}  // namespace

extern "C" {

// clusters: n_clusters lists in cl_off / cl_flat.  lengths reach get_seq_len as totalSeqLength (by_file) or seqInfo.length.
// node_to_rep_out[n]; the candidate lists into cand_off[n_clusters + 1] / cand_flat[cap].
int64_t ref_dedup_candidates(int n, int n_clusters, const int64_t* cl_off, const int32_t* cl_flat, const EdgeInfo* forest,
                             int64_t m, const uint64_t* lengths, int by_file, double dedup_dist, int32_t* node_to_rep_out,
                             int64_t* cand_off, int32_t* cand_flat, int64_t cap) {
  std::vector<KssdSketchInfo> sk((size_t)n);
  for (int i = 0; i < n; i++) {
    sk[i].id = i;
    sk[i].use64 = false;
    sk[i].sketchsize = 0;
    sk[i].totalSeqLength = by_file ? lengths[i] : 0;
    sk[i].seqInfo.strand = 0;
    sk[i].seqInfo.length = by_file ? 0 : (int)lengths[i];
  }
  std::vector<EdgeInfo> f(forest, forest + m);
  std::vector<int> rep;
  std::vector<std::vector<int>> cand =
      build_dedup_candidates_per_cluster(lists_of(n_clusters, cl_off, cl_flat), f, sk, by_file != 0, dedup_dist, rep);
  for (int i = 0; i < n; i++) node_to_rep_out[i] = rep[i];
  return lists_out(cand, cand_off, cand_flat, cap);
}

int64_t ref_select_k_reps(int n, int n_clusters, const int64_t* cl_off, const int32_t* cl_flat, const int64_t* cand_off,
                          const int32_t* cand_flat, const EdgeInfo* forest, int64_t m, const int32_t* node_to_rep, int k,
                          int64_t* reps_off, int32_t* reps_flat, int64_t cap) {
  std::vector<EdgeInfo> f(forest, forest + m);
  std::vector<int> rep(node_to_rep, node_to_rep + n);
  std::vector<std::vector<int>> reps = select_k_reps_per_cluster_tree(
      lists_of(n_clusters, cl_off, cl_flat), lists_of(n_clusters, cand_off, cand_flat), f, n, rep, k);
  if ((int)reps.size() != n_clusters) return -2;
  return lists_out(reps, reps_off, reps_flat, cap);
}

}  // extern "C"
