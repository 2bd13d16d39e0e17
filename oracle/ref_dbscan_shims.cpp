// extern "C" wrappers over the reference's KSSD DBSCAN (KssdDBSCAN, printKssdDBSCANResult of its src/dbscan.cpp).
// oracle/Makefile names that source and this file on one compiler line; the result is oracle/_ref/libref_dbscan.so, which
// tests/reflib.py loads.  TEST INFRASTRUCTURE ONLY.  The reference reports its progress on stderr; it is left alone.
#include <cstdint>
#include <string>
#include <vector>

#include "dbscan.h"

namespace {

// KssdSketchInfo records from a CSR array of sorted hashes (u32 or u64 by use64); names / lengths / comments may be null
std::vector<KssdSketchInfo> fill(int n, const uint64_t* start, const void* hashes, int use64, const char* const* files,
                                 const char* const* names, const char* const* comments, const uint64_t* lengths) {
  std::vector<KssdSketchInfo> sk((size_t)n);
  for (int i = 0; i < n; i++) {
    KssdSketchInfo& s = sk[i];
    s.id = i;
    s.use64 = use64 != 0;
    const uint64_t a = start[i], b = start[i + 1];
    if (use64) s.hash64_arr.assign((const uint64_t*)hashes + a, (const uint64_t*)hashes + b);
    else s.hash32_arr.assign((const uint32_t*)hashes + a, (const uint32_t*)hashes + b);
    s.sketchsize = (uint32_t)(b - a);
    s.totalSeqLength = lengths ? lengths[i] : 0;
    s.fileName = files ? files[i] : "";
    s.seqInfo.name = names ? names[i] : "";
    s.seqInfo.comment = comments ? comments[i] : "";
    s.seqInfo.strand = 0;
    s.seqInfo.length = lengths ? (int)lengths[i] : 0;
    if (names) s.fileSeqs.push_back(s.seqInfo);  // the -l layout prints the file's first record
  }
  return sk;
}

// labels from DBSCANResult: cluster index per member, -1 for noise.  Returns 0, or -1 when a point is missing or listed twice.
int labels_of(const DBSCANResult& r, int n, int32_t* labels, int* n_clusters, int* n_noise) {
  std::vector<int> seen((size_t)n, 0);
  for (size_t c = 0; c < r.clusters.size(); c++)
    for (int v : r.clusters[c]) {
      if (v < 0 || v >= n || seen[v]++) return -1;
      labels[v] = (int32_t)c;
    }
  for (int v : r.noise) {
    if (v < 0 || v >= n || seen[v]++) return -1;
    labels[v] = -1;
  }
  for (int i = 0; i < n; i++)
    if (!seen[i]) return -1;
  *n_clusters = r.num_clusters;
  *n_noise = r.num_noise;
  return 0;
}

}  // namespace

extern "C" {

int ref_kssd_dbscan(int n, const uint64_t* start, const void* hashes, int use64, double eps, int min_pts, int kmer_size,
                    int threads, int max_posting, int32_t* labels_out, int* n_clusters_out, int* n_noise_out) {
  std::vector<KssdSketchInfo> sk = fill(n, start, hashes, use64, nullptr, nullptr, nullptr, nullptr);
  DBSCANResult r = KssdDBSCAN(sk, eps, min_pts, kmer_size, threads, 0, max_posting);
  if (n == 0) { *n_clusters_out = r.num_clusters; *n_noise_out = r.num_noise; return 0; }
  return labels_of(r, n, labels_out, n_clusters_out, n_noise_out);
}

// KssdDBSCAN, then printKssdDBSCANResult into out_path.  by_file: the -l layout (files, lengths as totalSeqLength and the
// first record's name / comment); otherwise the sequence layout (names, lengths as seqInfo.length, comments).
int ref_kssd_dbscan_print(int n, const uint64_t* start, const void* hashes, int use64, double eps, int min_pts, int kmer_size,
                          int threads, int max_posting, int by_file, const char* const* files, const char* const* names,
                          const char* const* comments, const uint64_t* lengths, const char* out_path, int32_t* labels_out,
                          int* n_clusters_out, int* n_noise_out) {
  std::vector<KssdSketchInfo> sk = fill(n, start, hashes, use64, files, names, comments, lengths);
  DBSCANResult r = KssdDBSCAN(sk, eps, min_pts, kmer_size, threads, 0, max_posting);
  printKssdDBSCANResult(r, sk, by_file != 0, out_path, eps, min_pts);
  if (n == 0) { *n_clusters_out = r.num_clusters; *n_noise_out = r.num_noise; return 0; }
  return labels_of(r, n, labels_out, n_clusters_out, n_noise_out);
}

}  // extern "C"
