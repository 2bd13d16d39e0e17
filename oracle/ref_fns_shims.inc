// extern "C" wrappers over the reference's self-contained distance-half functions.  oracle/Makefile streams their
// definitions (calr, calculateMaxSizeRatio, calculate_mash_distance_fast, EdgeInfo, kruskalAlgorithm, generateForest,
// shuffle / shuffleN / generate_shuffle_dim) from the reference sources into the compiler and puts this file after them;
// the result is oracle/_ref/libref_fns.so, which tests/golden/make_golden.py turns into tests/golden/ref_distance_half.npz.
#include <cstring>

extern "C" {

// calr (src/MST.cpp) and calculateMaxSizeRatio (src/greedy.cpp): NaN where the reference throws (D < 0 or k <= 0).
double ref_calr(double D, int k) {
  try { return calr(D, k); } catch (const std::exception&) { return NAN; }
}
double ref_calculate_max_size_ratio(double D, int k) {
  try { return calculateMaxSizeRatio(D, k); } catch (const std::exception&) { return NAN; }
}

double ref_mash_distance_fast(int common, int size0, int size1, int kmer_size) {
  return calculate_mash_distance_fast(common, size0, size1, kmer_size);
}

// kruskalAlgorithm over m edges already sorted by distance, then generateForest at `threshold`.  tree: up to
// vertices - 1 records, *tree_m of them written; forest: the same capacity.  Returns the forest's size.
uint64_t ref_kruskal_forest(const EdgeInfo* sorted, uint64_t m, int vertices, double threshold, EdgeInfo* tree,
                            uint64_t* tree_m, EdgeInfo* forest) {
  vector<EdgeInfo> g(sorted, sorted + m);
  vector<EdgeInfo> t = kruskalAlgorithm(g, vertices);
  vector<EdgeInfo> f = generateForest(t, threshold);
  if (!t.empty()) memcpy(tree, t.data(), t.size() * sizeof(EdgeInfo));
  if (!f.empty()) memcpy(forest, f.data(), f.size() * sizeof(EdgeInfo));
  *tree_m = t.size();
  return f.size();
}

// generate_shuffle_dim (src/SketchInfo.cpp): the table of 1 << 4 * half_subk entries into out.  Returns its length.
int ref_generate_shuffle_dim(int half_subk, int* out) {
  int* t = generate_shuffle_dim(half_subk);
  const int n = 1 << 4 * half_subk;
  memcpy(out, t, (size_t)n * sizeof(int));
  free(t);
  return n;
}

}  // extern "C"
