// rtc_host.h -- host side of the drop-in: FASTA reading, parameter tuning, on-disk formats,
// cluster extraction and text output, mirroring the reference's interface for this path
// (names, argument meaning, error behaviour).  The compute goes through include/rtclust.h.
#pragma once
#include <stdint.h>

#include <functional>
#include <ostream>
#include <string>
#include <vector>

#include "../../include/rtclust.h"

namespace rtc {

// == SequenceInfo / SketchInfo metadata, src/SketchInfo.h:14-39 (reference tree) ==
struct SequenceInfo {
  std::string name, comment;
  int strand = 0;
  int length = 0;
};

struct GenomeInfo {
  int id = 0;
  std::string fileName;          // list mode
  uint64_t totalSeqLength = 0;   // list mode: sum of record lengths
  SequenceInfo seq0;             // list mode: first record; sequence mode: the record
  bool use64 = false;            // KSSD only (kssd.info.* trailing byte)
};

// ---- FASTA / FASTQ reading with the semantics of klib kseq as used at src/SketchInfo.cpp:880-948 ----
struct FastaRecord {
  std::string name, comment;
  bool has_comment = false;  // false -> the reference substitutes "noName"
  std::string seq;
};
// Reads every record of `path` (plain or gzip).  Returns false if the file cannot be opened.
bool read_fasta(const std::string& path, std::vector<FastaRecord>& out);
// Streaming variant used by the sketch driver: appends the records' bases to `bases`, separated by
// '\n' (a non-ACGT byte, so k-mers never span records), and reports first-record metadata.
bool read_genome_file(const std::string& path, std::string& bases, SequenceInfo& first, uint64_t& total_len,
                      uint64_t& n_records);
// Zero-copy variant: writes the same byte stream into dst[0..cap) (e.g. a pinned staging slot).
// Returns 0 ok, 1 cannot open, 2 capacity too small (`used` then holds a capacity that suffices).
int read_genome_file_flat(const std::string& path, char* dst, uint64_t cap, uint64_t& used, SequenceInfo& first,
                          uint64_t& total_len, uint64_t& n_records);
// The same into the 2-bit packed staging format (a quarter of the bytes over PCIe): base i of the stream at bits
// 2 (i & 3) of dst[i >> 2], A/C/G/T (either case) = 0..3; every other character (N, IUPAC codes, the record
// separators) is stored as 0 and listed in `runs` as (start, length) pairs, ascending.  cap_bases: capacity of dst in
// bases (dst holds cap_bases / 4 bytes, cap_bases a multiple of 4).  rtc_unpack_bases_dev restores the ASCII stream
// ('N' over the runs) on the GPU.  Same return values as read_genome_file_flat.
int read_genome_file_packed(const std::string& path, uint8_t* dst, uint64_t cap_bases, uint64_t& used, std::vector<uint64_t>& runs,
                            SequenceInfo& first, uint64_t& total_len, uint64_t& n_records);
size_t pack_bases(const char* seq, size_t n, uint8_t* dst, std::vector<uint64_t>& runs);  // one buffer, for tests
void pack_force_portable(int on);  // tests: 1 = the portable loops only, 2 = at most AVX2, 0 = the best tier the CPU has (AVX-512 BW + VBMI2, AVX2, portable)
// Upper bound of the bytes read_genome_file_flat writes for `path` (exact bound for plain files, the
// ISIZE-based guess for gzip); 0 if the file cannot be opened.
uint64_t genome_slot_bytes(const std::string& path);

// ---- calSize / tune_parameters / tune_kssd_parameters, src/SketchInfo.cpp:438-552, src/sub_command.cpp:2317-2467 ----
bool cal_size(const std::string& list_file, uint64_t minLen, uint64_t& maxSize, uint64_t& minSize, uint64_t& averageSize);
bool tune_parameters(bool greedy, bool isSetKmer, uint64_t maxSize, uint64_t minSize, uint64_t averageSize,
                     bool& isContainment, bool isJaccard, int& kmerSize, double threshold, int& containCompress,
                     int sketchSize);
bool tune_kssd_parameters(bool isSetKmer, uint64_t maxSize, uint64_t minSize, uint64_t averageSize, bool isContainment,
                          int& kmerSize, double threshold, int drlevel);
// file size the reference uses for containment sketch sizes (gz: ISIZE trailer), src/SketchInfo.cpp:892-915
int file_length_for_containment(const std::string& path);

// ---- generate_shuffle_dim, src/SketchInfo.cpp:60-102 (glibc srand/rand) ----
std::vector<int32_t> generate_shuffle_dim(int half_subk);

// ---- on-disk formats (src/Sketch_IO.cpp, src/MST_IO.cpp, src/SketchInfo.h:115-160) ----
struct KssdParameters { int id, half_k, half_subk, drlevel, genomeNumber; };  // src/SketchInfo.h:50-56

void save_genome_info(const std::vector<GenomeInfo>& g, const std::string& folder, const std::string& type,
                      bool sketchByFile, bool kssd);
bool load_genome_info(const std::string& folder, const std::string& type, std::vector<GenomeInfo>& g, bool kssd,
                      bool& sketchByFile);

struct MinHashSketchFile {
  int kmerSize = 21;
  bool isContainment = false;
  int containCompress = 1000, sketchSize = 1000;
  std::vector<std::vector<uint64_t>> hashes;
};
void save_minhash_sketches(const std::vector<GenomeInfo>& g, const MinHashSketchFile& f, const std::string& folder,
                           bool sketchByFile);
bool load_minhash_sketches(const std::string& folder, std::vector<GenomeInfo>& g, MinHashSketchFile& f, bool& sketchByFile);
void save_minhash_index(const MinHashSketchFile& f, const std::string& folder);  // minhash.sketch.index (MHIDX001)

struct KssdSketchFile {
  KssdParameters info{};
  bool use64 = false;
  std::vector<std::vector<uint32_t>> h32;
  std::vector<std::vector<uint64_t>> h64;
};
void save_kssd_sketches(const std::vector<GenomeInfo>& g, const KssdSketchFile& f, const std::string& folder, bool sketchByFile);
bool load_kssd_sketches(const std::string& folder, std::vector<GenomeInfo>& g, KssdSketchFile& f, bool& sketchByFile);
void save_kssd_index(const KssdSketchFile& f, const std::string& folder);  // kssd.sketch.index + .dict

// cluster_state.bin of clust-greedy --fast --save-rep (KssdClusterState::save / ::load, src/greedy.cpp:1545-1734):
// threshold, k, KSSD parameters, representative ids, every sketch in clustering order (id, length, hashes,
// file name), the clusters, and the representatives' inverted index (hash -> positions in rep_ids; written from
// the sketches, skipped when read -- it is rebuilt from them wherever it is needed).
struct KssdClusterState {
  double threshold = 0.05;
  int kmer_size = 0;
  KssdParameters info{};
  std::vector<int> rep_ids;
  std::vector<GenomeInfo> genomes;   // state order: genome i has id i (RepDB: file name and length only)
  KssdSketchFile sk;                 // hashes in the same order (cluster_state.bin; empty in a RepDB)
  std::vector<GenomeInfo> rep_genomes;  // representative r: id, length, file name ...
  KssdSketchFile reps;                  // ... and hashes, r = position in rep_ids
  std::vector<std::vector<int>> clusters;  // clusters[r] belongs to representative r
  // MinHash RepDB (MinHashClusterState, src/greedy.h): u64 hashes in reps.h64, these instead of the KSSD parameters
  bool minhash = false;
  int sketch_size = 0;
  bool is_containment = false;
};
bool save_kssd_cluster_state(const std::string& path, const KssdClusterState& st);
bool load_kssd_cluster_state(const std::string& path, KssdClusterState& st);
// cluster_state.bin of clust-greedy --save-rep on MinHash sketches (MinHashClusterState::save / ::load,
// src/greedy.cpp:2134-2302): "MINHASH", parameters, representative ids, every sketch, clusters (representative first),
// index.  load keeps parameters, representative ids and clusters only -- the reference skips the sketches too and
// re-reads them from the folder.
bool save_minhash_cluster_state(const std::string& path, const KssdClusterState& st);
bool load_minhash_cluster_state(const std::string& path, KssdClusterState& st);
// RepDB of clust-greedy --fast --db (KssdClusterState::save_repdb / ::load_repdb / ::print_stats,
// src/greedy.cpp:2351-2537, :2656-2765): "REPDB002", parameters, the representatives with their sketches, the
// clusters, every genome's file name and length, the representatives' inverted index (64-bit keys; "REPDB001"
// files with 32-bit keys are read too).  The index is written from the sketches and not kept when read.
bool save_kssd_repdb(const std::string& path, const KssdClusterState& st);
bool load_kssd_repdb(const std::string& path, KssdClusterState& st);
void print_kssd_repdb_stats(const KssdClusterState& st, std::ostream& out);
// MinHash twin (MinHashClusterState::save_repdb / ::load_repdb / ::print_stats, src/greedy.cpp:2789-3147): "MHREPDB1"
bool save_minhash_repdb(const std::string& path, const KssdClusterState& st);
bool load_minhash_repdb(const std::string& path, KssdClusterState& st);

void save_mst(const std::vector<rtc_edge>& mst, const std::string& folder);   // edge.mst
bool load_mst(const std::string& folder, std::vector<rtc_edge>& mst);

// ---- --dense by-products: mst.dense / mst.ani (src/MST_IO.cpp:12-45, :219-250) and the noise-removal
// pass of compute_clusters (src/sub_command.cpp:3071-3103; getNoiseNode / modifyForest, src/MST.cpp:86-107,189-211) ----
constexpr int DENSE_SPAN = 100;  // src/common.hpp
void save_dense(const std::string& folder, const std::vector<int32_t>& dense, int span, int genome_number);  // dense: span x n row-major
bool load_dense(const std::string& folder, std::vector<int32_t>& dense, int& span, int& genome_number);
void save_ani(const std::string& folder, const uint64_t ani[101]);
bool load_ani(const std::string& folder, uint64_t ani[101]);
// nodes of every multi-member cluster whose density at the threshold's bucket is <= min(Q1 - 1, alpha = 2)
std::vector<int> noise_nodes(const std::vector<std::vector<int>>& cluster, const std::vector<int32_t>& dense, int span,
                             int genome_number, double threshold);
std::vector<rtc_edge> modify_forest(const std::vector<rtc_edge>& forest, const std::vector<int>& noise);

// ---- forest cut, BFS clusters, result text (src/MST.cpp:77-85,109-142; src/MST_IO.cpp:72-179) ----
// kruskalAlgorithm over a list already sorted by distance (src/MST.cpp:59-75, UnionFind.h:5-90): used to
// merge a stored MST with the forest of the appended rows (append_clust_mst, src/sub_command.cpp:1693-1700)
std::vector<rtc_edge> kruskal_algorithm(const std::vector<rtc_edge>& sorted_graph, int vertices);
std::vector<rtc_edge> generate_forest(const std::vector<rtc_edge>& mst, double threshold);
std::vector<std::vector<int>> generate_cluster_with_bfs(const std::vector<rtc_edge>& forest, int vertices);
void print_result(const std::vector<std::vector<int>>& cluster, const std::vector<GenomeInfo>& g, bool sketchByFile,
                  const std::string& outputFile, double threshold = -1.0);

// ---- tree / linkage writers of clust-mst (src/MST.cpp:1044-1287, src/MST_IO.cpp:252-380): the single-linkage
// dendrogram of the MST (edges by ascending distance, heights = merge distances).  As in the reference only
// the component that contains genome 0 is written when the MST is a forest. ----
std::string get_newick_tree(const std::vector<GenomeInfo>& g, const std::vector<rtc_edge>& mst, bool sketchByFile);
void print_newick_tree(const std::vector<GenomeInfo>& g, const std::vector<rtc_edge>& mst, bool sketchByFile, const std::string& output);
void print_phylip_tree(const std::vector<GenomeInfo>& g, const std::vector<rtc_edge>& mst, bool sketchByFile, const std::string& output);
void print_nexus_tree(const std::vector<GenomeInfo>& g, const std::vector<rtc_edge>& mst, bool sketchByFile, const std::string& output);
void print_linkage_matrix(int n, const std::vector<rtc_edge>& mst, const std::string& output);  // c1 \t c2 \t dist \t size

// ---- clust-mst --nj-tree / --nj-all: Newick text of the neighbour-joining records of rtc_nj_clusters (include/rtclust.h).  Leaves are
// labelled as get_newick_tree labels them, lengths printed with std::to_string, negative ones as they are. ----
std::string nj_newick_text(const std::function<std::string(uint32_t)>& label, const uint32_t* members, size_t m, const rtc_njoin* joins,
                           size_t n_joins);
std::string get_nj_newick(const std::vector<GenomeInfo>& g, const std::vector<int>& members, const rtc_njoin* joins, size_t n_joins,
                          bool sketchByFile);
void print_nj_newick(const std::vector<GenomeInfo>& g, const std::vector<std::vector<int>>& clusters, const std::vector<rtc_njoin>& joins,
                     const std::vector<uint64_t>& first, bool sketchByFile, const std::string& output);

// ---- clust-mst --nj-support: the same trees with rtc_nj_support's counts.  A node that names a split (a record with
// c == UINT32_MAX in a tree of four or more) carries nj_support_percent between ")" and ":"; the tsv has a header and a line a
// labelled node: cluster as `clusters` lists it, record index in its tree, leaves below the node, count, replicates. ----
inline uint32_t nj_support_percent(uint32_t count, uint32_t replicates) { return (200u * count + replicates) / (2u * replicates); }  // percent, half up
std::string nj_support_newick_text(const std::function<std::string(uint32_t)>& label, const uint32_t* members, size_t m, const rtc_njoin* joins,
                                   size_t n_joins, const uint32_t* support, uint32_t replicates);
std::string nj_support_tsv_lines(size_t cluster, size_t m, const rtc_njoin* joins, size_t n_joins, const uint32_t* support, uint32_t replicates);
void print_nj_support(const std::vector<GenomeInfo>& g, const std::vector<std::vector<int>>& clusters, const std::vector<rtc_njoin>& joins,
                      const std::vector<uint64_t>& first, const std::vector<uint32_t>& support, uint32_t replicates, bool sketchByFile,
                      const std::string& newick, const std::string& tsv);

// ---- clust-mst --upgma: the cut and the three writers over rtc_upgma_clusters' records (include/rtclust.h has the definition).
// upgma_height is rtc_upgma_distance (the host library does not link the device library): one double operation a step.
// upgma_keep: the integer cut rule, sum <= llround(threshold 2^20) size_a size_b in 128 bits.
// upgma_report: clusters are the run's, every genome in exactly one; first[q] .. first[q + 1] are the merges (a, b genome indices)
// of the cluster whose smallest member is the q-th smallest.  linkage_txt: ALL merges, cluster after cluster in that order,
// "c1 \t c2 \t distance (%.6f) \t size" as print_linkage_matrix writes them, leaves as genome indices, new ids n, n + 1, ... in
// file order.  refined: every cluster cut at the threshold (the prefix of its merges that upgma_keep keeps), members ascending,
// clusters by smallest member.  Returns the merges kept.
// upgma_newick_text: one ultrametric tree, node height = distance / 2, branch length = parent height - child height printed as
// nj_newick_text prints lengths; labels and the one- and two-member cases as there. ----
inline double upgma_height(uint64_t sum, uint32_t size_a, uint32_t size_b) {
  const double pairs = (double)size_a * (double)size_b;
  const double scale = pairs * 1048576.0;
  return (double)sum / scale;
}
bool upgma_keep(uint64_t sum, uint32_t size_a, uint32_t size_b, double threshold);
uint64_t upgma_report(uint32_t n, const std::vector<std::vector<int>>& clusters, const rtc_umerge* merges, const uint64_t* first, double threshold,
                      std::string* linkage_txt, std::vector<std::vector<int>>* refined);
std::string upgma_newick_text(const std::function<std::string(uint32_t)>& label, const uint32_t* members, size_t m, const rtc_umerge* merges,
                              size_t n_merges);
void print_upgma_newick(const std::vector<GenomeInfo>& g, const std::vector<std::vector<int>>& clusters, const std::vector<rtc_umerge>& merges,
                        const std::vector<uint64_t>& first, bool sketchByFile, const std::string& output);

// ---- clust-mst --quality: the two reports of rtc_cluster_quality's records (include/rtclust.h).  sil[g]: rtc_silhouette_value of
// rec[g]; clusters: the run's, numbered as <output> numbers them, every genome in exactly one.  quality_tsv: a header, a line a
// cluster -- cluster, size, mean silhouette, least silhouette, mean intra-cluster distance (the sum of a_num over the members /
// (size (size - 1) 2^20), 0 for a singleton), diameter (the largest far_q / 2^20), separation (the least near_q / 2^20), nearest
// cluster (the near_cluster of the first member in genome order that holds that least near_q, or -) -- and a last line "all"
// with the genome count and the overall mean silhouette.  silhouette_tsv: a header and a line a genome in input order -- name,
// cluster, silhouette, a, b, b_cluster or -.  Means are double sums over the members in ascending genome order; every value is
// printed %.6f.  Returns the overall mean silhouette. ----
double quality_report_text(const std::function<std::string(uint32_t)>& name, const std::vector<std::vector<int>>& clusters, const rtc_sil* rec,
                           const double* sil, uint32_t n, std::string* quality_tsv, std::string* silhouette_tsv);

// ---- clust-mst --cluster-support: the two reports of rtc_cluster_support's records (include/rtclust.h).  clusters: the run's,
// numbered as <output> numbers them, every genome in exactly one; rec: one record per cluster in the library's order, that of the
// clusters' smallest members; together[g] per genome.  support_tsv: a header, then a line a cluster in the order of `clusters` --
// cluster, size, replicates, recovered, split, merged, mixed, max_pieces, support = (200 recovered + B) / (2 B) in integer
// division: percent, half up, the rule of --nj-support's labels.  genomes_tsv: a header, then a line a genome in input order --
// name, cluster, together, fraction = together / (B (size - 1)) as %.6f, or - for a singleton.  Returns the mean of recovered over
// the clusters. ----
double support_report_text(const std::function<std::string(uint32_t)>& name, const std::vector<std::vector<int>>& clusters, const rtc_csupport* rec,
                           const uint64_t* together, uint32_t n, uint32_t replicates, std::string* support_tsv, std::string* genomes_tsv);

// ---- clust-mst --pangenome: the four reports of rtc_pangenome's records (include/rtclust.h).  clusters: the run's, numbered as
// <output> numbers them, every genome in exactly one; rec and hist in the library's order, that of the clusters' smallest members;
// gen[g] per genome.  Every real number is %.6f.
//   pan_tsv: a header, then a line a cluster in the order of `clusters` -- cluster, size, hashes (total), pan, core, soft_core,
//     shell, cloud, singletons, core_share = core / pan (- without a hash), new_per_genome = hist[1] / size (what the closed form
//     gives for pan(m) - pan(m - 1)), centre = the name of the member with the largest occ_sum, equal sums to the smaller index.
//   genomes_tsv: a header, then a line a genome in input order -- name, cluster, hashes, unique, core, soft_core, shell, cloud,
//     typicality = occ_sum / (hashes size), or - for an empty sketch.
//   hist_tsv: cluster, f, count for every count > 0.   curve_tsv: cluster, j, pan(j), core(j) at rtc_pan_growth's points, for the
//     clusters of two or more.
// growth_fn is rtc_pan_growth (this library does not link the GPU library), run on `threads` host threads.  Returns the mean of
// core_share over the clusters that have a hash. ----
typedef int (*pan_growth_fn)(const uint64_t*, uint32_t, int, uint32_t*, double*, double*, uint32_t*);
double pangenome_report_text(const std::function<std::string(uint32_t)>& name, const std::vector<std::vector<int>>& clusters, const rtc_pan* rec,
                             const uint64_t* hist, const rtc_pan_genome* gen, uint32_t n, int threads, pan_growth_fn growth_fn, std::string* pan_tsv,
                             std::string* genomes_tsv, std::string* hist_tsv, std::string* curve_tsv);

// ---- clust-mst --auto-threshold / --stability: the MST edge-length analysis (src/MST.cpp:1743-2376, structs src/MST.h:77-100) ----
struct EdgeLengthStats {
  double min_dist = 0, max_dist = 0, median_dist = 0, q1_dist = 0, q3_dist = 0, mean_dist = 0, std_dev = 0;
  std::vector<double> sorted_distances;  // the distances above 1e-10, ascending
};
struct ThresholdCandidate {
  double threshold = 0, gap_score = 0.0;
  int edge_index = -1;
  double confidence = 0;
  std::string level;
  double stability_score = 0.5, stability_split = 0.5, stability_merge = 0.5;
  int cluster_count = 0, near_edge_count = 0;
};
struct StabilityResult { double overall = 0.5, split = 0.5, merge = 0.5; int near_edge_count = 0; };
EdgeLengthStats edge_length_stats(const std::vector<rtc_edge>& mst);
StabilityResult threshold_stability(const std::vector<rtc_edge>& mst, double threshold, int num_vertices, double epsilon = 0.01,
                                    int num_samples = 5, int min_near_edges = 100);
std::vector<ThresholdCandidate> threshold_candidates(const std::vector<rtc_edge>& mst, int max_candidates, double min_gap_ratio,
                                                     bool enable_stability, int num_vertices);
ThresholdCandidate select_optimal_threshold(const std::vector<ThresholdCandidate>& candidates, const std::vector<rtc_edge>& mst);
void print_threshold_analysis(const std::vector<rtc_edge>& mst, const EdgeLengthStats& stats,
                              const std::vector<ThresholdCandidate>& candidates, const ThresholdCandidate& optimal, const std::string& file);
// The call-site blocks: --auto-threshold (<output>.threshold_analysis.txt and the stderr lines; min_gap_ratio 0.05 with
// --stability honoured in clust_from_mst / compute_kssd_clusters, 0.1 without it in the --presketched flows) and --stability
// alone (stderr only).  Neither changes the clustering threshold.
void auto_threshold_report(const std::vector<rtc_edge>& mst, int num_vertices, const std::string& outputFile, double min_gap_ratio,
                           bool stability);
void stability_report(const std::vector<rtc_edge>& mst, int num_vertices, double threshold);

// ---- clust-mst --fast --dedup-dist / --reps-per-cluster (src/cluster_postprocess.cpp) ----
// The host path of rtc_tree_medoids (the same code: csrc/rtc_tree_medoid.h) on `threads` threads; false if the edges with
// dist <= dedup_dist are not a forest.
bool tree_medoids_host(int n, const std::vector<rtc_edge>& forest, double dedup_dist, const std::vector<uint64_t>& seq_len,
                       std::vector<int>& node_to_rep, int threads);
// the candidates of every cluster: its members' representatives, unique, ascending (:143-155); dedup_dist <= 0: the clusters
std::vector<std::vector<int>> dedup_candidates(const std::vector<std::vector<int>>& clusters, const std::vector<int>& node_to_rep,
                                               double dedup_dist);
// select_k_reps_per_cluster_tree (:192-329): farthest-first over the forest's tree metric, up to k per cluster
std::vector<std::vector<int>> select_k_reps(const std::vector<std::vector<int>>& clusters, const std::vector<std::vector<int>>& candidates,
                                            const std::vector<rtc_edge>& forest, int n, const std::vector<int>& node_to_rep, int k);

// ---- clust-mst --save-rep / --append state (src/mst_state.h, src/mst_state.cpp) ----
// mst_cluster_state.bin: one tree-medoid representative per cluster, the clusters, every member's name and length, and
// the representatives' inverted index.  "MHMSTST01" (MinHashMstState::save, :129-255) or "KSMSTST01" (KssdMstState::save,
// :293-435): both share one struct here.  The index is written from the representatives' hashes, keys ascending (the
// reference writes phmap's iteration order), and skipped when read: the append measures on the GPU (rtc_rep_match).
struct MstState {
  bool kssd = false;
  double threshold = 0.0;
  int kmer_size = 0;
  int sketch_size = 0, contain_compress = 0;  // MinHash
  bool is_containment = false;                // MinHash
  int half_k = 0, half_subk = 0, drlevel = 0;  // KSSD
  bool use64 = true;                           // KSSD: h64 or h32; MinHash: always h64
  int N = 0;
  bool sketch_by_file = true;
  std::vector<int> rep_ids;
  std::vector<uint64_t> rep_lens;
  std::vector<std::string> rep_names;
  std::vector<std::vector<uint64_t>> h64;
  std::vector<std::vector<uint32_t>> h32;
  std::vector<std::vector<int>> clusters;  // clusters[r] belongs to representative r
  std::vector<std::string> member_names;
  std::vector<uint64_t> member_lens;
  size_t reps() const { return use64 ? h64.size() : h32.size(); }
};
bool save_mst_state(const std::string& path, const MstState& st);
// false (and a message) when the file is missing, has the other magic, or ends early: the caller falls back
bool load_mst_state(const std::string& path, bool kssd, MstState& st);
// MinHashInitialMstState / KssdInitialMstState (:436-560): clusters[i]'s representative is rep_of_cluster[i]
// (build_dedup_candidates_per_cluster with dedup_dist = +inf: the cluster's tree medoid); the hashes are the sketch file's.
void init_mst_state(MstState& st, const std::vector<GenomeInfo>& g, bool sketchByFile, const std::vector<std::vector<int>>& clusters,
                    const std::vector<int>& rep_of_cluster, const std::vector<std::vector<uint64_t>>* h64,
                    const std::vector<std::vector<uint32_t>>* h32);
// MinHashMstAppendCluster / KssdMstAppendCluster (:681-1106) from the pairs rtc_rep_match emitted, sorted by (query, slot):
// the queries in order, a union-find over the representatives.  A query's matches are its pairs whose slot is live (an old
// representative, or query i that became one) and still a root; the closest is the survivor (equal distances: the lowest
// slot -- DESIGN 5), the others are merged into it in ascending slot order; no match opens a cluster.  Appends the members,
// returns the live clusters and compacts the state (compact_*_state, :601-680).  Query q's hashes: qh64[q] or qh32[q].
std::vector<std::vector<int>> append_mst_state(MstState& st, const std::vector<std::string>& names, const std::vector<uint64_t>& lens,
                                               const std::vector<std::vector<uint64_t>>* qh64, const std::vector<std::vector<uint32_t>>* qh32,
                                               const std::vector<rtc_rep_pair>& pairs);
// printMstStateClusterResult (:1108-1168)
void print_mst_state_clusters(const std::vector<std::vector<int>>& clusters, const std::vector<std::string>& member_names,
                              const std::vector<uint64_t>& member_lens, bool sketch_by_file, const std::string& output_file,
                              double threshold);

// ---- clust-mst --db: the MST RepDB is the state file (src/mst_state.cpp:1150-1415) ----
// MinHashMstPrintStats / KssdMstPrintStats, byte for byte; the "unique hashes" are the distinct hashes over the representatives
void print_mst_state_stats(const MstState& st, std::ostream& os);
// build_live_index: slot -> its number among the slots with a non-empty cluster, -1 for a retired slot
std::vector<int> mst_live_index(const MstState& st);
// the search's weight mode for this state (rtc_rep_topk): 0 KSSD, 1 MinHash containment, 2 | sketch_size << 2 MinHash
int mst_query_wmode(const MstState& st);
// the reference's distance from a hit's (common, denom) with libm: mash_distance (mode 0), containDistance (1),
// MinHash::distance (2); NaN becomes +inf
double mst_query_distance(uint32_t common, uint32_t denom, int wmode, int kmer_size);
// the --query TSV (mst_repdb_query[_fast]) and the --assign TSV (mst_repdb_assign[_fast]) from rtc_rep_topk's hits, sorted by
// (query, rank), per_query[q] of them for query q; false if the file does not open
bool write_mst_query_tsv(const std::string& path, const MstState& st, const std::vector<std::string>& qnames,
                         const std::vector<rtc_rep_hit>& hits, const std::vector<uint32_t>& per_query);
bool write_mst_assign_tsv(const std::string& path, const MstState& st, const std::vector<std::string>& qnames,
                          const std::vector<rtc_rep_hit>& hits, const std::vector<uint32_t>& per_query, int* n_assigned);
// clust-mst --db --screen: the two reports from rtc_rep_screen's hits (sorted by sample, then in the library's order) and sums.
// names[q]: the sample (empty: query_<q>, as the --query TSV names it); rep_names / cluster_id / cluster_size by slot, what
// write_mst_query_tsv prints (cluster_id: mst_live_index).  *tsv: #sample rank cluster_id rep_name cluster_size shared rep_hashes
// containment identity unique unique_share, a line a hit, rank "-" for a hit that was not picked, one no_match line for a sample
// without a hit; *summary: #sample hashes matched explained hits picks unexplained_share ("-" for a sample without a hash).
// identity_fn is rtc_screen_identity; this library does not link the GPU library.
void screen_report_text(const std::vector<std::string>& names, const std::vector<std::string>& rep_names, const std::vector<int>& cluster_id,
                        const std::vector<int>& cluster_size, const rtc_screen_hit* hits, size_t n_hits, const rtc_screen_sum* sums, int kmer_size,
                        double (*identity_fn)(uint32_t, uint32_t, int), std::string* tsv, std::string* summary);
// the two files, <path> and <path>.summary.tsv; false if one does not open
bool write_mst_screen_tsv(const std::string& path, const MstState& st, const std::vector<std::string>& names,
                          const std::vector<rtc_screen_hit>& hits, const std::vector<rtc_screen_sum>& sums,
                          double (*identity_fn)(uint32_t, uint32_t, int));
bool write_mst_screen_summary_tsv(const std::string& path, const MstState& st, const std::vector<std::string>& names,
                                  const std::vector<rtc_screen_hit>& hits, const std::vector<rtc_screen_sum>& sums);

// clust-dbscan --db FILE: a clustered sketch set that new genomes can be placed into (rtc_dbscan_assign).  One binary file,
// little-endian, INTEGRATION.md section 6 lists it byte by byte.  Written to FILE.tmp and renamed.
struct DbscanModel {
  bool minhash = false;   // kind: 0 KSSD, 1 MinHash
  int width = 4;          // bytes per hash
  bool sketch_by_file = true;
  int kmer_size = 0;      // the k of the predicate (and of the MinHash sketches)
  int half_k = 0, half_subk = 0, drlevel = 0;  // KSSD
  int sketch_size = 0;    // MinHash
  int min_pts = 0, max_posting = 0, n_clusters = 0;
  uint64_t min_len = 0;
  double eps = 0.0;
  std::vector<int32_t> labels;
  std::vector<uint8_t> core;
  std::vector<GenomeInfo> genomes;
  std::vector<std::vector<uint32_t>> h32;
  std::vector<std::vector<uint64_t>> h64;
};
bool save_dbscan_model(const std::string& path, const DbscanModel& m);
// false: *why says what is wrong with the file (cannot open, foreign, version, truncated, bytes after its end)
bool load_dbscan_model(const std::string& path, DbscanModel& m, std::string* why);
// clust-dbscan --db FILE --update: the records and sketches of the new genomes appended (a32 or a64, by the model's width), the
// labels, core flags and cluster count replaced by those of rtc_dbscan_update over all genomes.  The caller saves the model
// under its own name: the same format and version.  false: the sizes do not fit together.
bool update_dbscan_model(DbscanModel& m, const std::vector<GenomeInfo>& add, const std::vector<std::vector<uint32_t>>* a32,
                         const std::vector<std::vector<uint64_t>>* a64, const std::vector<int32_t>& labels, const std::vector<uint8_t>& core,
                         int n_clusters);
void print_dbscan_model_stats(const DbscanModel& m, std::ostream& os);

std::string current_date_time();  // src/common.hpp:36-44

// clust-leiden --leiden: the weights of m edges to the q of rtc_wedge (units of 2^-20), in doubles.  objective 0 (CPM): as the
// reference prepares igraph's weights (src/leiden.cpp:343-366) -- min and max searched from 1.0 and 0.0; when max - min < 0.5
// and the range is above 1e-6, weight' = (weight - min) / range, otherwise the weights stay -- then q = llround(weight' * 2^20),
// and a record with q == 0 is dropped (the lightest edge normalises to 0 and carries no weight).  objective 1 (modularity):
// q = max(1, llround(weight * 2^20)) as the Louvain flow forms it, nothing dropped.  q is capped at 2^32 - 1.
// Returns whether max - min < 0.5 under CPM (the reference prints its "Edge weights normalized" line then); *w_min and *w_max
// (may be null) receive the two.
bool leiden_quantise(const uint32_t* u, const uint32_t* v, const double* weight, uint64_t m, int objective, std::vector<rtc_wedge>& out,
                     double* w_min, double* w_max);

// The quantisation of ONE weight, as a clust-leiden run formed its records: leiden_quantise finds (scale, lo, range) over its
// weights and calls leiden_quantise_weight for each, and clust-leiden --db --assign calls it with the model's three for the
// weights of a query, so the two cannot drift.  objective 1 (modularity; --louvain too): max(1, llround(w 2^20)), nothing
// scaled.  Returns 0 for a record that drops out (CPM, q < 1); q is capped at 2^32 - 1.
struct LeidenQuant {
  int objective = 1;
  bool scale = false;
  double lo = 0.0, range = 1.0;
};
uint32_t leiden_quantise_weight(double weight, const LeidenQuant& z);
// (scale, lo, range) of m weights under objective; returns leiden_quantise's flag; *w_min, *w_max may be null
bool leiden_quantiser(const double* weight, uint64_t m, int objective, LeidenQuant* z, double* w_min, double* w_max);

// What a model keeps of the records a run gave rtc_louvain / rtc_leiden and of its labels: k[p] the row sums as the
// rtc_louvain comment defines them (u == v adds 2q), tot[d] their sum over community d, m2 the sum of all, size[d] the members.
// false: a record's end or a label is out of range.
struct LeidenModelSums {
  std::vector<uint64_t> k, tot, size;
  uint64_t m2 = 0;
};
bool leiden_model_sums(const rtc_wedge* records, uint64_t m, const int32_t* labels, uint32_t n, uint32_t n_clusters, LeidenModelSums& out);

// clust-leiden --db FILE: the communities of one run, with everything a new genome needs to be placed into them
// (rtc_graph_query, rtc_leiden_place).  One binary file, little-endian, INTEGRATION.md section 8 lists it byte by byte; the
// genome records, sketch lengths and sketches are section 6's.  Written to FILE.tmp and renamed.
struct LeidenModel {
  int algorithm = 0;      // 0 Louvain, 1 Leiden
  int objective = 1;      // RTC_LEIDEN_CPM / RTC_LEIDEN_MODULARITY (Louvain: modularity)
  int width = 4;          // bytes per hash
  bool sketch_by_file = true;
  int kmer_size = 0, half_k = 0, half_subk = 0, drlevel = 0;
  int knn = 0;            // the effective value of the run
  int n_clusters = 0;
  uint64_t min_len = 0;
  double threshold = 0.0, resolution = 1.0;
  bool scale = false;     // the run's quantisation (CPM)
  double lo = 0.0, range = 1.0;
  uint64_t m2 = 0;        // modularity
  std::vector<int32_t> labels;
  std::vector<uint64_t> tot;  // per cluster: tot_d (modularity) or the size N_d (CPM)
  std::vector<GenomeInfo> genomes;
  std::vector<std::vector<uint32_t>> h32;
  std::vector<std::vector<uint64_t>> h64;
};
bool save_leiden_model(const std::string& path, const LeidenModel& m);
// false: *why says what is wrong with the file (cannot open, foreign, version, truncated, bytes after its end)
bool load_leiden_model(const std::string& path, LeidenModel& m, std::string* why);
void print_leiden_model_stats(const LeidenModel& m, std::ostream& os);

// clust-leiden --db --assign between its two device calls: the weight weight_fn(common, |query|, |model genome|, kmer_size) --
// weight_fn is rtc_graph_weight; this library does not link the GPU library -- of every record of rtc_graph_query on `threads`
// host threads (n_queries x knn libm calls), quantised by z.  out receives (query, model genome, q) in the records' order, the
// dropped ones left out.
void leiden_assign_weights(const rtc_qedge* edges, uint64_t m, const uint32_t* model_sizes, const uint32_t* query_sizes, int kmer_size,
                           double (*weight_fn)(uint32_t, uint32_t, uint32_t, int), const LeidenQuant& z, int threads, std::vector<rtc_wedge>& out);

// Time the parser threads spent inside gzip decompression (libdeflate or zlib), summed over threads, and the bytes it produced
// since the process started: the command lines report them (RTC_METRICS_JSON: inflate_gb_per_s_per_thread).
void rtc_host_inflate_stats(double* seconds, uint64_t* bytes_out);

}  // namespace rtc
