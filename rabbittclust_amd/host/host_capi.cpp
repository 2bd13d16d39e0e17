// host_capi.cpp -- small C ABI over the host library, for the CPU test-suite (ctypes).
#include <string.h>

#include "rtc_host.h"

using namespace rtc;

extern "C" {

// name\tcomment\tlength\n<sequence>\n per record ("noName" when the header has no comment), the
// same dump the reference harness (oracle/ref_harness.cpp over kseq.h) produces.
long rtch_fasta_dump(const char* path, char* out, long cap) {
  std::vector<FastaRecord> recs;
  if (!read_fasta(path, recs)) return -1;
  long pos = 0;
  auto put = [&](const char* s, long n) { if (out && pos + n <= cap) memcpy(out + pos, s, n); pos += n; };
  // kseq keeps its comment buffer between records: a record without a comment shows the previous
  // record's text (NULL -> "noName" only while no record has had one).  Only record 0 is ever used
  // by the reference (src/SketchInfo.cpp:944-947); the dump mimics the buffer for all records.
  std::string stale; bool have_stale = false;
  for (const FastaRecord& r : recs) {
    if (r.has_comment) { stale = r.comment; have_stale = true; }
    const std::string cm = r.has_comment ? r.comment : (have_stale ? stale : std::string("noName"));
    const std::string len = std::to_string(r.seq.size());
    put(r.name.data(), (long)r.name.size()); put("\t", 1);
    put(cm.data(), (long)cm.size()); put("\t", 1);
    put(len.data(), (long)len.size()); put("\n", 1);
    put(r.seq.data(), (long)r.seq.size()); put("\n", 1);
  }
  return pos;
}

// loads a sketch folder and writes it again (sketch files + index files): byte-level format check
int rtch_resave_folder(const char* in_dir, const char* out_dir, int kssd) {
  std::vector<GenomeInfo> g; bool byFile = true;
  if (kssd) {
    KssdSketchFile f;
    if (!load_kssd_sketches(in_dir, g, f, byFile)) return 1;
    save_kssd_sketches(g, f, out_dir, byFile);
    save_kssd_index(f, out_dir);
  } else {
    MinHashSketchFile f;
    if (!load_minhash_sketches(in_dir, g, f, byFile)) return 1;
    save_minhash_sketches(g, f, out_dir, byFile);
    save_minhash_index(f, out_dir);
  }
  return 0;
}

// --premsted flow without a GPU: info.mst + edge.mst -> cluster text; also re-saves both files
int rtch_premsted(const char* in_dir, const char* out_dir, const char* out_file, double threshold, int kssd) {
  std::vector<GenomeInfo> g; std::vector<rtc_edge> mst; bool byFile = true;
  if (!load_genome_info(in_dir, "mst", g, kssd != 0, byFile)) return 1;
  if (!load_mst(in_dir, mst)) return 1;
  if (out_dir && out_dir[0]) { save_genome_info(g, out_dir, "mst", byFile, kssd != 0); save_mst(mst, out_dir); }
  std::vector<rtc_edge> forest = generate_forest(mst, threshold);
  std::vector<std::vector<int>> cl = generate_cluster_with_bfs(forest, (int)g.size());
  print_result(cl, g, byFile, out_file, threshold);
  return 0;
}

int rtch_shuffle_dim(int half_subk, int32_t* out) {
  std::vector<int32_t> v = generate_shuffle_dim(half_subk);
  memcpy(out, v.data(), v.size() * sizeof(int32_t));
  return (int)v.size();
}

// returns 1 on success; outputs the tuned values
int rtch_tune(int greedy, int isSetKmer, int isContainment, int isJaccard, int kmerSize, double threshold,
              int containCompress, int sketchSize, uint64_t maxSize, uint64_t minSize, uint64_t avgSize, int* k_out,
              int* compress_out, int* containment_out) {
  bool ic = isContainment != 0;
  int k = kmerSize, cc = containCompress;
  bool ok = tune_parameters(greedy != 0, isSetKmer != 0, maxSize, minSize, avgSize, ic, isJaccard != 0, k, threshold, cc, sketchSize);
  *k_out = k; *compress_out = cc; *containment_out = ic ? 1 : 0;
  return ok ? 1 : 0;
}

int rtch_cal_size(const char* list_file, uint64_t minLen, uint64_t* mx, uint64_t* mn, uint64_t* avg) {
  return cal_size(list_file, minLen, *mx, *mn, *avg) ? 1 : 0;
}

int rtch_file_length(const char* path) { return file_length_for_containment(path); }

// The two genome readers of the sketch driver: mode 0 = read_genome_file (std::string), mode 1 =
// read_genome_file_flat into out[0..cap).  Writes the byte stream (records joined by '\n'), returns
// its length (the needed capacity when cap is too small for mode 1), -1 if the file cannot be opened.
long rtch_genome_bases(const char* path, int flat, char* out, long cap, uint64_t* total, uint64_t* nrec, int* first_len,
                       uint64_t* slot) {
  SequenceInfo first;
  *slot = genome_slot_bytes(path);
  if (flat) {
    uint64_t used = 0;
    const int st = read_genome_file_flat(path, out, (uint64_t)cap, used, first, *total, *nrec);
    if (st == 1) return -1;
    *first_len = first.length;
    return (long)used;
  }
  std::string bases;
  if (!read_genome_file(path, bases, first, *total, *nrec)) return -1;
  *first_len = first.length;
  if ((long)bases.size() <= cap) memcpy(out, bases.data(), bases.size());
  return (long)bases.size();
}

void rtch_pack_force_portable(int on) { pack_force_portable(on); }

// pack_bases: n characters -> ceil(n / 4) packed bytes in `out`, runs (start, length) pairs in runs_out (capacity
// runs_cap u64 values); returns the number of u64 values the runs take (the caller retries when it exceeds runs_cap)
long rtch_pack_bases(const char* seq, long n, unsigned char* out, unsigned long long* runs_out, long runs_cap) {
  std::vector<uint64_t> runs;
  pack_bases(seq, (size_t)n, out, runs);
  for (size_t i = 0; i < runs.size() && (long)i < runs_cap; i++) runs_out[i] = runs[i];
  return (long)runs.size();
}

// read_genome_file_packed: returns status (0 ok, 1 cannot open, 2 capacity); *used bases, *nruns u64 values written to runs_out
int rtch_read_genome_packed(const char* path, unsigned char* out, long cap_bases, long* used, unsigned long long* runs_out, long runs_cap,
                            long* nruns, unsigned long long* total, unsigned long long* nrec) {
  std::vector<uint64_t> runs; SequenceInfo first; uint64_t u = 0, tot = 0, nr = 0;
  const int st = read_genome_file_packed(path, out, (uint64_t)cap_bases, u, runs, first, tot, nr);
  *used = (long)u; *total = tot; *nrec = nr; *nruns = (long)runs.size();
  for (size_t i = 0; i < runs.size() && (long)i < runs_cap; i++) runs_out[i] = runs[i];
  return st;
}

// clust-mst --fast --dedup-dist / --reps-per-cluster on the host (src/sub_command.cpp:2089-2103): the clusters of the forest
// (generate_cluster_with_bfs), node_to_rep[n], the candidates and the representatives of every cluster as flat lists with
// offsets (cand_off / reps_off: clusters + 1 entries, at most n + 1; the lists at most n ids).  Returns the cluster count,
// -1 if the edges with dist <= dedup_dist are not a forest.
int rtch_dedup_reps(int n, const rtc_edge* forest, long m, const uint64_t* seq_len, double dedup_dist, int k, int threads,
                    int* node_to_rep, int* cand, int* cand_off, int* reps, int* reps_off) {
  const std::vector<rtc_edge> f(forest, forest + m);
  const std::vector<uint64_t> lens(seq_len, seq_len + n);
  std::vector<int> rep;
  if (!tree_medoids_host(n, f, dedup_dist, lens, rep, threads)) return -1;
  const std::vector<std::vector<int>> cl = generate_cluster_with_bfs(f, n);
  const std::vector<std::vector<int>> cd = dedup_candidates(cl, rep, dedup_dist);
  const std::vector<std::vector<int>> rp = select_k_reps(cl, cd, f, n, rep, k);
  for (int i = 0; i < n; i++) node_to_rep[i] = rep[i];
  auto flat = [](const std::vector<std::vector<int>>& v, int* ids, int* off) {
    off[0] = 0;
    for (size_t i = 0; i < v.size(); i++) {
      for (size_t j = 0; j < v[i].size(); j++) ids[off[i] + j] = v[i][j];
      off[i + 1] = off[i] + (int)v[i].size();
    }
  };
  flat(cd, cand, cand_off);
  flat(rp, reps, reps_off);
  return (int)cl.size();
}

// mst_cluster_state.bin: load, then save again (byte-level format check); 1 if it does not load
int rtch_mst_state_resave(const char* in_path, const char* out_path, int kssd) {
  MstState st;
  if (!load_mst_state(in_path, kssd != 0, st)) return 1;
  return save_mst_state(out_path, st) ? 0 : 2;
}

// --append against a state file without a GPU: the replay of rtc_rep_match's pairs (n_pairs records, sorted by (query, slot)).
// Query q: names[q], lens[q], hashes qhash[qoff[q] .. qoff[q + 1]) (u64, or u32 for a KSSD state without use64).  Writes the
// cluster file (out_cluster) and the compacted state (out_state, may be NULL); returns the live cluster count, -1 if the state
// does not load.
int rtch_mst_state_append(const char* in_state, int kssd, int n_queries, const char* const* names, const uint64_t* lens,
                          const void* qhash, const uint64_t* qoff, const rtc_rep_pair* pairs, long n_pairs,
                          const char* out_cluster, const char* out_state) {
  MstState st;
  if (!load_mst_state(in_state, kssd != 0, st)) return -1;
  std::vector<std::string> nm; std::vector<uint64_t> ln;
  std::vector<std::vector<uint64_t>> q64; std::vector<std::vector<uint32_t>> q32;
  for (int q = 0; q < n_queries; q++) {
    nm.push_back(names[q]); ln.push_back(lens[q]);
    if (st.use64) q64.emplace_back((const uint64_t*)qhash + qoff[q], (const uint64_t*)qhash + qoff[q + 1]);
    else q32.emplace_back((const uint32_t*)qhash + qoff[q], (const uint32_t*)qhash + qoff[q + 1]);
  }
  const std::vector<rtc_rep_pair> pv(pairs, pairs + n_pairs);
  const std::vector<std::vector<int>> live = append_mst_state(st, nm, ln, st.use64 ? &q64 : nullptr, st.use64 ? nullptr : &q32, pv);
  print_mst_state_clusters(live, st.member_names, st.member_lens, st.sketch_by_file, out_cluster, st.threshold);
  if (out_state && out_state[0] && !save_mst_state(out_state, st)) return -1;
  return (int)live.size();
}

// a clust-dbscan --db model read and written back (tests: the loader and the writer against the documented layout)
int rtch_dbscan_model_resave(const char* in_path, const char* out_path) {
  DbscanModel m;
  std::string why;
  if (!load_dbscan_model(in_path, m, &why)) return -1;
  return save_dbscan_model(out_path, m) ? 0 : -2;
}

// clust-dbscan --db --update's rewrite of the model file, in place through FILE.tmp: n_new genomes (names, lengths, the hashes
// of genome q at hashes[off[q] .. off[q + 1]) in the model's width) appended, labels / core over all genomes and the cluster
// count replaced.  labels NULL with n_new 0: the model's own.  -1: the file does not load, -2: it was not written, -3: sizes.
int rtch_dbscan_model_update(const char* path, int n_new, const char** names, const uint64_t* lens, const void* hashes, const uint64_t* off,
                             const int32_t* labels, const uint8_t* core, int n_clusters) {
  DbscanModel m;
  std::string why;
  if (!load_dbscan_model(path, m, &why)) return -1;
  std::vector<GenomeInfo> add((size_t)std::max(n_new, 0));
  std::vector<std::vector<uint64_t>> q64; std::vector<std::vector<uint32_t>> q32;
  for (int q = 0; q < n_new; q++) {
    add[q].fileName = names[q]; add[q].seq0.name = names[q]; add[q].seq0.length = (int)lens[q]; add[q].totalSeqLength = lens[q];
    add[q].use64 = m.width == 8 && !m.minhash;
    if (m.width == 8) q64.emplace_back((const uint64_t*)hashes + off[q], (const uint64_t*)hashes + off[q + 1]);
    else q32.emplace_back((const uint32_t*)hashes + off[q], (const uint32_t*)hashes + off[q + 1]);
  }
  const size_t n = m.labels.size() + add.size();
  if (!labels && n_new > 0) return -3;
  const std::vector<int32_t> lab = labels ? std::vector<int32_t>(labels, labels + n) : m.labels;
  const std::vector<uint8_t> cr = labels ? std::vector<uint8_t>(core, core + n) : m.core;
  if (!update_dbscan_model(m, add, &q32, &q64, lab, cr, labels ? n_clusters : m.n_clusters)) return -3;
  return save_dbscan_model(path, m) ? 0 : -2;
}

// leiden_quantise: out[m] receives the records kept, *n_out their number; returns 1 where the weights' range was narrow
int rtch_leiden_quantise(const uint32_t* u, const uint32_t* v, const double* weight, uint64_t m, int objective, rtc_wedge* out, uint64_t* n_out) {
  std::vector<rtc_wedge> rec;
  const bool narrow = leiden_quantise(u, v, weight, m, objective, rec, nullptr, nullptr);
  for (size_t i = 0; i < rec.size(); i++) out[i] = rec[i];
  *n_out = rec.size();
  return narrow ? 1 : 0;
}

// leiden_quantiser: (scale, lo, range) of the weights; returns leiden_quantise's flag
int rtch_leiden_quantiser(const double* weight, uint64_t m, int objective, int* scale, double* lo, double* range) {
  LeidenQuant z;
  const bool narrow = leiden_quantiser(weight, m, objective, &z, nullptr, nullptr);
  *scale = z.scale ? 1 : 0; *lo = z.lo; *range = z.range;
  return narrow ? 1 : 0;
}

// leiden_quantise_weight: q of one weight, 0 where the record drops out
uint32_t rtch_leiden_quantise_weight(double weight, int objective, int scale, double lo, double range) {
  LeidenQuant z;
  z.objective = objective; z.scale = scale != 0; z.lo = lo; z.range = range;
  return leiden_quantise_weight(weight, z);
}

// leiden_assign_weights with the caller's weight function (rtc_graph_weight): out[m], *n_out the records kept
void rtch_leiden_assign_weights(const rtc_qedge* edges, uint64_t m, const uint32_t* model_sizes, const uint32_t* query_sizes, int kmer_size,
                                double (*weight_fn)(uint32_t, uint32_t, uint32_t, int), int objective, int scale, double lo, double range,
                                int threads, rtc_wedge* out, uint64_t* n_out) {
  LeidenQuant z;
  z.objective = objective; z.scale = scale != 0; z.lo = lo; z.range = range;
  std::vector<rtc_wedge> rec;
  leiden_assign_weights(edges, m, model_sizes, query_sizes, kmer_size, weight_fn, z, threads, rec);
  for (size_t i = 0; i < rec.size(); i++) out[i] = rec[i];
  *n_out = rec.size();
}

// leiden_model_sums: k[n], tot[n_clusters], size[n_clusters], *m2; -1 where a record or a label is out of range
int rtch_leiden_model_sums(const rtc_wedge* records, uint64_t m, const int32_t* labels, uint32_t n, uint32_t n_clusters, uint64_t* k, uint64_t* tot,
                           uint64_t* size, uint64_t* m2) {
  LeidenModelSums s;
  if (!leiden_model_sums(records, m, labels, n, n_clusters, s)) return -1;
  std::copy(s.k.begin(), s.k.end(), k);
  std::copy(s.tot.begin(), s.tot.end(), tot);
  std::copy(s.size.begin(), s.size.end(), size);
  *m2 = s.m2;
  return 0;
}

// a clust-leiden --db model written from its parts (tests, tools): head = {algorithm, objective, width, sketch_by_file, kmer_size,
// half_k, half_subk, drlevel, knn, n_clusters, scale}, genome q named names[q] with lens[q] bases and the hashes
// hashes[off[q] .. off[q + 1]) in the model's width.  0, or -2 where the file was not written.
int rtch_leiden_model_save(const char* path, const int32_t* head, uint64_t min_len, double threshold, double resolution, double lo, double range,
                           uint64_t m2, uint32_t n, const int32_t* labels, const uint64_t* tot, const char** names, const uint64_t* lens,
                           const void* hashes, const uint64_t* off) {
  LeidenModel m;
  m.algorithm = head[0]; m.objective = head[1]; m.width = head[2]; m.sketch_by_file = head[3] != 0; m.kmer_size = head[4]; m.half_k = head[5];
  m.half_subk = head[6]; m.drlevel = head[7]; m.knn = head[8]; m.n_clusters = head[9]; m.scale = head[10] != 0;
  m.min_len = min_len; m.threshold = threshold; m.resolution = resolution; m.lo = lo; m.range = range; m.m2 = m2;
  m.labels.assign(labels, labels + n);
  m.tot.assign(tot, tot + m.n_clusters);
  m.genomes.resize(n);
  for (uint32_t q = 0; q < n; q++) {
    GenomeInfo& g = m.genomes[q];
    g.id = (int)q; g.fileName = names[q]; g.seq0.name = names[q]; g.seq0.length = (int)lens[q]; g.totalSeqLength = lens[q]; g.use64 = m.width == 8;
    if (m.width == 8) m.h64.emplace_back((const uint64_t*)hashes + off[q], (const uint64_t*)hashes + off[q + 1]);
    else m.h32.emplace_back((const uint32_t*)hashes + off[q], (const uint32_t*)hashes + off[q + 1]);
  }
  return save_leiden_model(path, m) ? 0 : -2;
}

// a clust-leiden --db model read and written back; -1 with the loader's reason in why[why_cap] where it does not load
int rtch_leiden_model_resave(const char* in_path, const char* out_path, char* why, int why_cap) {
  LeidenModel m;
  std::string w;
  if (!load_leiden_model(in_path, m, &w)) {
    if (why && why_cap > 0) { strncpy(why, w.c_str(), (size_t)why_cap - 1); why[why_cap - 1] = 0; }
    return -1;
  }
  return save_leiden_model(out_path, m) ? 0 : -2;
}
// get_nj_newick over plain arrays: labels[g] for every genome index the members name, members[m] ascending, joins[n_joins] with
// genome indices.  Returns the text's length; the text itself when it fits cap (no terminator).
long rtch_nj_newick(const char* const* labels, const uint32_t* members, uint64_t m, const rtc_njoin* joins, uint64_t n_joins, char* out, long cap) {
  const std::string text = nj_newick_text([&](uint32_t v) { return std::string(labels[v]); }, members, (size_t)m, joins, (size_t)n_joins);
  if (out && (long)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (long)text.size();
}

// nj_support_newick_text over plain arrays, as rtch_nj_newick; support[n_joins]
long rtch_nj_support_newick(const char* const* labels, const uint32_t* members, uint64_t m, const rtc_njoin* joins, uint64_t n_joins,
                            const uint32_t* support, uint32_t replicates, char* out, long cap) {
  if (!support || replicates == 0) return -1;
  const std::string text = nj_support_newick_text([&](uint32_t v) { return std::string(labels[v]); }, members, (size_t)m, joins, (size_t)n_joins, support, replicates);
  if (out && (long)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (long)text.size();
}

// upgma_newick_text over plain arrays, as rtch_nj_newick
long rtch_upgma_newick(const char* const* labels, const uint32_t* members, uint64_t m, const rtc_umerge* merges, uint64_t n_merges, char* out, long cap) {
  const std::string text = upgma_newick_text([&](uint32_t v) { return std::string(labels[v]); }, members, (size_t)m, merges, (size_t)n_merges);
  if (out && (long)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (long)text.size();
}

int rtch_upgma_keep(uint64_t sum, uint32_t size_a, uint32_t size_b, double threshold) { return upgma_keep(sum, size_a, size_b, threshold) ? 1 : 0; }

// upgma_report over plain arrays: cluster_of[g] in [0, n_clusters) for every genome, merges and first as rtc_upgma_clusters gives
// them for that labelling.  refined_of[n]: the refined cluster of every genome, numbered in order of smallest member; *kept the
// merges kept.  Returns -1 for a cluster_of outside that range, else the length of the linkage text; the text itself when it fits
// cap (no terminator).
long rtch_upgma_report(const int32_t* cluster_of, uint32_t n_clusters, uint32_t n, const rtc_umerge* merges, const uint64_t* first, double threshold,
                       int32_t* refined_of, uint64_t* kept, char* out, long cap) {
  std::vector<std::vector<int>> clusters(n_clusters);
  for (uint32_t g = 0; g < n; g++) {
    if (cluster_of[g] < 0 || (uint32_t)cluster_of[g] >= n_clusters) return -1;
    clusters[cluster_of[g]].push_back((int)g);
  }
  for (const auto& c : clusters) if (c.empty()) return -1;
  std::string text;
  std::vector<std::vector<int>> refined;
  const uint64_t k = upgma_report(n, clusters, merges, first, threshold, &text, &refined);
  if (kept) *kept = k;
  if (refined_of)
    for (size_t c = 0; c < refined.size(); c++) for (int g : refined[c]) refined_of[g] = (int32_t)c;
  if (out && (long)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (long)text.size();
}

// quality_report_text over plain arrays: names[g], cluster_of[g] in [0, n_clusters) for every genome, rec[g] (rtc_sil) and sil[g].
// which 0: the cluster report, 1: the genome report.  Returns -1 for a cluster_of outside that range, else the text's length; the text itself when it fits cap (no terminator).
long rtch_quality_report(const char* const* names, const int32_t* cluster_of, uint32_t n_clusters, const rtc_sil* rec, const double* sil, uint32_t n,
                         int which, char* out, long cap) {
  std::vector<std::vector<int>> clusters(n_clusters);
  for (uint32_t g = 0; g < n; g++) {
    if (cluster_of[g] < 0 || (uint32_t)cluster_of[g] >= n_clusters) return -1;  // every genome of a run is in a cluster
    clusters[cluster_of[g]].push_back((int)g);
  }
  std::string q, s;
  quality_report_text([&](uint32_t g) { return std::string(names[g]); }, clusters, rec, sil, n, &q, &s);
  const std::string& text = which ? s : q;
  if (out && (long)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (long)text.size();
}

// support_report_text over plain arrays: names[g], cluster_of[g] in [0, n_clusters) for every genome, rec[n_clusters] (rtc_csupport, in
// the order of the clusters' smallest members) and together[g].  which 0: the cluster report, 1: the genome report.  Returns -1
// for a cluster_of outside that range, a cluster without members or replicates == 0, else the text's length; the text itself when it fits cap.
long rtch_support_report(const char* const* names, const int32_t* cluster_of, uint32_t n_clusters, const rtc_csupport* rec, const uint64_t* together,
                         uint32_t n, uint32_t replicates, int which, char* out, long cap) {
  if (replicates == 0) return -1;
  std::vector<std::vector<int>> clusters(n_clusters);
  for (uint32_t g = 0; g < n; g++) {
    if (cluster_of[g] < 0 || (uint32_t)cluster_of[g] >= n_clusters) return -1;
    clusters[cluster_of[g]].push_back((int)g);
  }
  for (const std::vector<int>& c : clusters) if (c.empty()) return -1;
  std::string a, b;
  support_report_text([&](uint32_t g) { return std::string(names[g]); }, clusters, rec, together, n, replicates, &a, &b);
  const std::string& text = which ? b : a;
  if (out && (long)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (long)text.size();
}

// pangenome_report_text over plain arrays: names[g], cluster_of[g] in [0, n_clusters) for every genome, rec[n_clusters] (rtc_pan) and
// hist[n] in the order of the clusters' smallest members, gen[g] (rtc_pan_genome), growth_fn rtc_pan_growth.  which 0: the cluster
// report, 1: the genome report, 2: the histogram, 3: the curves.  Returns -1 for a cluster_of outside that range, a cluster
// without members or a record whose size is not its cluster's, else the text's length; the text itself when it fits cap.
long rtch_pangenome_report(const char* const* names, const int32_t* cluster_of, uint32_t n_clusters, const rtc_pan* rec, const uint64_t* hist,
                           const rtc_pan_genome* gen, uint32_t n, pan_growth_fn growth_fn, int which, char* out, long cap) {
  std::vector<std::vector<int>> clusters(n_clusters);
  for (uint32_t g = 0; g < n; g++) {
    if (cluster_of[g] < 0 || (uint32_t)cluster_of[g] >= n_clusters) return -1;
    clusters[cluster_of[g]].push_back((int)g);
  }
  std::vector<std::pair<int, size_t>> by_first;
  for (const std::vector<int>& c : clusters) {
    if (c.empty()) return -1;
    by_first.push_back({c[0], c.size()});
  }
  std::sort(by_first.begin(), by_first.end());
  for (uint32_t q = 0; q < n_clusters; q++) if (rec[q].size != by_first[q].second) return -1;
  std::string t[4];
  pangenome_report_text([&](uint32_t g) { return std::string(names[g]); }, clusters, rec, hist, gen, n, 1, growth_fn, &t[0], &t[1], &t[2], &t[3]);
  const std::string& text = t[which & 3];
  if (out && (long)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (long)text.size();
}

// screen_report_text with the caller's identity function (rtc_screen_identity) over plain arrays: names[n_queries] (an empty name: query_<q>), rep_names / cluster_id / cluster_size by slot
// (n_reps of each), hits sorted by sample, sums[n_queries].  which 0: the hit report, 1: the summary.  Returns -1 for a hit whose
// sample or slot is out of range or out of order, else the text's length; the text itself when it fits cap (no terminator).
long rtch_screen_report(const char* const* names, uint32_t n_queries, const char* const* rep_names, const int32_t* cluster_id,
                        const int32_t* cluster_size, uint32_t n_reps, const rtc_screen_hit* hits, uint64_t n_hits, const rtc_screen_sum* sums,
                        int kmer_size, double (*identity_fn)(uint32_t, uint32_t, int), int which, char* out, long cap) {
  for (uint64_t h = 0; h < n_hits; h++)
    if (hits[h].query >= n_queries || hits[h].slot >= n_reps || (h && hits[h].query < hits[h - 1].query)) return -1;
  std::vector<std::string> nm(names, names + n_queries), rn(rep_names, rep_names + n_reps);
  const std::vector<int> id(cluster_id, cluster_id + n_reps), sz(cluster_size, cluster_size + n_reps);
  std::string a, b;
  screen_report_text(nm, rn, id, sz, hits, (size_t)n_hits, sums, kmer_size, identity_fn, &a, &b);
  const std::string& text = which ? b : a;
  if (out && (long)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (long)text.size();
}

}
