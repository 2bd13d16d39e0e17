// main.cpp -- clust-mst / clust-greedy command lines on top of the MI355X C ABI.
//
// Mirrors the flag surface and workflow dispatch of the reference's src/main.cpp:113-254,291-671
// for the sketch + all-pairs + cluster path: list-mode input (-l) or one FASTA file whose
// records are the genomes (no -l), MinHash
// and KSSD (--fast) sketching, --presketched / --premsted resume, -e/--no-save, and the same
// intermediate folder (info.sketch, hash.sketch, minhash.sketch.index, kssd.*, info.mst,
// edge.mst).  Built four times: -DGREEDY_CLUST gives clust-greedy, -DDBSCAN_CLUST clust-dbscan (KSSD only, src/main.cpp:478-522;
// rtc_dbscan), -DLEIDEN_CLUST clust-leiden (src/main.cpp:391-477; rtc_graph_build + rtc_louvain), otherwise clust-mst
// (CMakeLists.txt:40-58 of the reference does the same).
// GPUs: every visible MI355X is used (--gpus LIST / RTC_GPUS to choose): one context + one host thread
// per GPU, file batches go round-robin to the GPUs, the sketches stay in HBM (copied to the host only
// to write hash.sketch), are shared among the GPUs with RCCL broadcasts, and the MST runs
// row-sharded with one all-reduce per Boruvka round (rtc_mst_sharded).  Also here: --append (clust-mst, and
// clust-greedy --fast with or without a stored state), --dense, the tree / linkage writers, clust-greedy's
// --save-rep cluster state (KSSD and MinHash) and representative database (--db ..., KSSD and MinHash), clust-greedy
// --append on MinHash sketches, the dense estimator loops (--inverted-index=false: modifyMST / greedyCluster), and
// clust-mst's --save-rep state and its MST representative database (--db ..., the search on the GPU: rtc_rep_topk).
// Single-FASTA input to --append and to --db --build / --append is outside this path and exits with a message.
#ifdef LEIDEN_CLUST
// clust-leiden sketches, saves and loads KSSD sketches as clust-dbscan does (compute_kssd_sketches keeps the sketches alone), so
// it shares that build's plumbing; its own flags, checks and clustering are the LEIDEN_CLUST branches inside
#define DBSCAN_CLUST
#endif
#include <math.h>
#include <iomanip>
#include <limits>
#include <sys/stat.h>
#include <omp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <fstream>
#include <iostream>
#include <numeric>
#include <functional>
#include <mutex>
#include <thread>

#include "rtc_host.h"

using namespace std;
using namespace rtc;

static double get_sec() { struct timeval tv; gettimeofday(&tv, NULL); return (double)tv.tv_sec + (double)tv.tv_usec / 1000000; }

// RTC_METRICS_JSON=<file>: the phase times the reference prints under -DTimer (same labels) and the sizes of the run,
// as one JSON object written when everything else has been written ("metrics / logging").
struct Metrics {
  vector<pair<string, string>> kv;  // in order of arrival; a key set twice keeps the last value
  void put(const string& k, const string& raw) {
    for (auto& e : kv) if (e.first == k) { e.second = raw; return; }
    kv.emplace_back(k, raw);
  }
  void num(const string& k, double v) { char b[64]; snprintf(b, sizeof b, "%.9g", v); put(k, b); }
  void str(const string& k, const string& v) {
    string q = "\"";
    for (char c : v) { if (c == '"' || c == '\\') q += '\\'; if ((unsigned char)c >= 0x20) q += c; }
    put(k, q + "\"");
  }
  void write() const {
    const char* path = getenv("RTC_METRICS_JSON");
    if (!path || !*path) return;
    FILE* f = fopen(path, "w");
    if (!f) { fprintf(stderr, "Warning: cannot write %s\n", path); return; }
    fputs("{", f);
    for (size_t i = 0; i < kv.size(); i++) fprintf(f, "%s\n  \"%s\": %s", i ? "," : "", kv[i].first.c_str(), kv[i].second.c_str());
    fputs("\n}\n", f);
    fclose(f);
  }
};
static Metrics g_metrics;

// The warm-up helper thread (rtc_warmup beside the sketch phase) is joined before the process leaves through exit():
// static destructors and the HIP runtime's teardown must not run while it is still inside a HIP call.
static std::thread* g_gpu_thread = nullptr;  // main's GPU bring-up thread while it runs
#ifdef RTC_MEASURE
// Measurement build only (`make measure` -> bin/clust-mst-measure, tools/cli_timeline.py; the shipped binaries hold none of
// this).  RTC_EXIT_PROBE=1: what the process leaves to the kernel at _exit -- the pageable staging ring and the lanes' device
// staging -- is released by hand, timed, before leaving: says which of them the time between _exit and the parent's wait()
// belongs to.  RTC_EXIT_DELAY_MS / RTC_START_DELAY_MS: a sleep before leaving / before anything else.  RTC_NO_THP=1: staging
// memory without transparent huge pages.
extern "C" int rtc_debug_device_reset(int device);
static std::vector<char*> g_exit_probe_host;
static std::vector<std::pair<rtc_ctx*, void*>> g_exit_probe_dev;
#endif
static std::thread g_warmup_thread;
static std::mutex g_warmup_mutex;
static void join_warmup() {
  std::lock_guard<std::mutex> lk(g_warmup_mutex);
  if (g_warmup_thread.joinable() && g_warmup_thread.get_id() != std::this_thread::get_id()) g_warmup_thread.join();
}
#define CHECK(ctx, call)                                                                         \
  do {                                                                                           \
    int st__ = (call);                                                                           \
    if (st__ != RTC_OK) {                                                                        \
      fprintf(stderr, "ERROR: %s failed (%d): %s\n", #call, st__, rtc_last_error(ctx));          \
      join_warmup();                                                                             \
      exit(1);                                                                                   \
    }                                                                                            \
  } while (0)

struct DeviceSketches {  // sketches resident in HBM in the CSR the pair kernels read
  void* d_hashes = nullptr; uint64_t* d_start = nullptr; uint32_t* d_len = nullptr;
  uint32_t n = 0; int width = 8;
};

struct Gpu {  // one per GPU in use: context, communicator, staging and the resident sketch rows
  rtc_ctx* ctx = nullptr; rtc_comm* comm = nullptr;
  int device = 0;
  void* d_sk = nullptr;         // resident sketches: row g (genome id g) at d_sk + g*stride*width
  uint32_t* d_cnt = nullptr;    // hashes per genome
};

// Sketches produced by sketch_files and left in HBM (every GPU holds all rows after the share step)
struct Resident {
  bool ok = false;              // false: fall back to the host vectors (gzip retry round, KSSD row overflow)
  uint32_t stride = 0; int width = 8;
  std::vector<uint32_t> counts; // per genome id
};

// run fn(g) on one host thread per GPU and wait (a context is used by one thread at a time)
template <typename F>
static void on_all_gpus(std::vector<Gpu>& gpus, F fn) {
  std::vector<std::thread> th;
  for (size_t g = 1; g < gpus.size(); g++) th.emplace_back([&fn, g]() { fn(g); });
  fn(0);
  for (auto& t : th) t.join();
}

static void upload_sketches(rtc_ctx* ctx, const vector<vector<uint64_t>>* h64, const vector<vector<uint32_t>>* h32,
                            DeviceSketches& ds) {
  const uint32_t n = (uint32_t)(h64 ? h64->size() : h32->size());
  ds.n = n; ds.width = h64 ? 8 : 4;
  vector<uint64_t> start(n); vector<uint32_t> len(n);
  uint64_t tot = 0;
  for (uint32_t g = 0; g < n; g++) { start[g] = tot; len[g] = (uint32_t)(h64 ? (*h64)[g].size() : (*h32)[g].size()); tot += len[g]; }
  vector<unsigned char> flat((size_t)tot * ds.width);
  for (uint32_t g = 0; g < n; g++) {
    if (!len[g]) continue;
    if (h64) memcpy(flat.data() + start[g] * 8, (*h64)[g].data(), (size_t)len[g] * 8);
    else memcpy(flat.data() + start[g] * 4, (*h32)[g].data(), (size_t)len[g] * 4);
  }
  CHECK(ctx, rtc_dev_alloc(ctx, flat.size() + 64, &ds.d_hashes));
  CHECK(ctx, rtc_dev_alloc(ctx, (size_t)n * 8 + 64, (void**)&ds.d_start));
  CHECK(ctx, rtc_dev_alloc(ctx, (size_t)n * 4 + 64, (void**)&ds.d_len));
  CHECK(ctx, rtc_copy_h2d(ctx, ds.d_hashes, flat.data(), flat.size()));
  CHECK(ctx, rtc_copy_h2d(ctx, ds.d_start, start.data(), (size_t)n * 8));
  CHECK(ctx, rtc_copy_h2d(ctx, ds.d_len, len.data(), (size_t)n * 4));
}

// the CSR over the resident rows: start[g] = order[g]*stride (order: processing order -> genome id), len from the counts
static void resident_sketches(rtc_ctx* ctx, const Gpu& gp, const Resident& rs, const vector<uint32_t>* order, DeviceSketches& ds) {
  const uint32_t n = (uint32_t)rs.counts.size();
  ds.n = n; ds.width = rs.width; ds.d_hashes = gp.d_sk;
  vector<uint64_t> start(n); vector<uint32_t> len(n);
  for (uint32_t g = 0; g < n; g++) { const uint32_t src = order ? (*order)[g] : g; start[g] = (uint64_t)src * rs.stride; len[g] = rs.counts[src]; }
  CHECK(ctx, rtc_dev_alloc(ctx, (size_t)n * 8 + 64, (void**)&ds.d_start));
  CHECK(ctx, rtc_dev_alloc(ctx, (size_t)n * 4 + 64, (void**)&ds.d_len));
  CHECK(ctx, rtc_copy_h2d(ctx, ds.d_start, start.data(), (size_t)n * 8));
  CHECK(ctx, rtc_copy_h2d(ctx, ds.d_len, len.data(), (size_t)n * 4));
}

static vector<string> read_list(const string& inputFile) {
  fprintf(stderr, "-----input fileList, sketch by file\n");
  ifstream fs(inputFile);
  if (!fs) { fprintf(stderr, "error open the inputFile: %s\n", inputFile.c_str()); exit(1); }
  vector<string> fileList; string fileName;
  while (getline(fs, fileName)) if (!fileName.empty()) fileList.push_back(fileName);
  return fileList;
}

// sketchFiles / sketchFileWithKssd (src/SketchInfo.cpp:865-992, :994-1252): parse on the host
// cores (OpenMP over files), sketch on the GPU in batches of a few GiB of bases.
struct SketchJob {
  bool kssd = false; int kmerSize = 21; int sketchSize = 1000; bool isContainment = false; int containCompress = 1000;
  int drlevel = 3; uint64_t minLen = 10000; int threads = 1;
};

// One batch of consecutive list entries: file f gets the slot [slot_off, slot_off + slot_len) of the
// page-locked staging buffer; parser threads write the bases straight into it.
static char* alloc_pageable(size_t bytes) {  // 2 MiB-aligned, transparent huge pages if the host allows
  void* p = nullptr;
  if (posix_memalign(&p, (size_t)2 << 20, bytes) != 0) return nullptr;
#ifdef RTC_MEASURE
  if (getenv("RTC_NO_THP")) return (char*)p;  // (without huge pages the parse is 15 % slower and the exit 0.04 s longer)
#endif
  madvise(p, bytes, MADV_HUGEPAGE);
  return (char*)p;
}

struct Batch { vector<size_t> files; vector<uint64_t> slot_off, slot_len; uint64_t bytes = 0; };

struct FileResult {           // indexed by list position, so late (retried) files keep list order
  SequenceInfo first; uint64_t total = 0; int flen = 0; bool kept = false;
  vector<uint64_t> h64; vector<uint32_t> h32;
  bool on_host = false;  // h64 / h32 hold the sketch (otherwise it lives in HBM only)
};

// gpus_ready (optional): the HIP runtime and the contexts are still coming up on another thread (main); wait() returns
// when `gpus` is filled, *done says whether it already is.  Everything the host can do alone happens before wait() is
// called -- the list, the slot sizes, the plan, and the PARSING: batch after batch into staging buffers of their own for
// as long as the GPUs are not there (0.05-0.24 s of runtime start-up = 6-28 GB of FASTA at the parser's rate), which
// the lanes then take back to back.
struct GpusReady { std::function<void()> wait; const std::atomic<bool>* done; };
static void sketch_files(vector<Gpu>& gpus, const string& inputFile, const SketchJob& job, vector<GenomeInfo>& genomes,
                         MinHashSketchFile* mh, KssdSketchFile* ks, Resident& rs, bool need_host_hashes,
                         const GpusReady* gpus_ready = nullptr) {
  const double tp00 = get_sec();
  const vector<string> fileList = read_list(inputFile);
  const size_t nfiles = fileList.size();
  const bool verbose = getenv("RTC_VERBOSE") != nullptr;
  // Staging format: the parser threads pack the bases to 2 bits and list everything that is not ACGT as runs
  // (rtc_host: read_genome_file_packed); the GPU expands the batch again in HBM (rtc_unpack_bases_dev) in front of the
  // sketch kernel.  A quarter of the bytes cross PCIe, which is what bounds this command line.  RTC_STAGE_ASCII=1
  // stages the characters themselves (the former path; tests compare the two).
  const bool packed = getenv("RTC_STAGE_ASCII") == nullptr;
  uint64_t BATCH_BYTES = (uint64_t)1 << 30;  // measured best on a 16-core quota: 0.5-1 GiB
  if (const char* e = getenv("RTC_BATCH_BYTES")) BATCH_BYTES = std::max<uint64_t>(strtoull(e, nullptr, 10), 1 << 20);
  vector<int32_t> shuffled;
  std::thread shuffle_thread;  // the 2^24-entry glibc-rand shuffle takes ~0.7 s: built while batch 0 is parsed
  int half_subk = 6;
  if (job.kssd) {
    const int half_k = (job.kmerSize + 1) / 2;
    half_subk = 6 - job.drlevel >= 2 ? 6 : job.drlevel + 2;
    shuffle_thread = std::thread([&shuffled, half_subk]() { shuffled = generate_shuffle_dim(half_subk); });
    ks->info.half_k = half_k; ks->info.half_subk = half_subk; ks->info.drlevel = job.drlevel;
    ks->info.id = (half_k << 8) + (half_subk << 4) + job.drlevel;        // :1030
    ks->info.genomeNumber = (int)fileList.size();                         // :1031
    ks->use64 = half_k - job.drlevel > 8;
  }
  const bool use64 = job.kssd ? ks->use64 : true;
  if (verbose) fprintf(stderr, "[init]  list + shuffle table in %.3fs\n", get_sec() - tp00);

  // ---- slot sizes (upper bound of the bases a file yields), batches of ~BATCH_BYTES ----
  const double tp0 = get_sec();
  vector<uint64_t> slot(nfiles);
  vector<FileResult> res(nfiles);
#pragma omp parallel for num_threads(job.threads) schedule(static)
  for (long i = 0; i < (long)nfiles; i++) {
    slot[i] = genome_slot_bytes(fileList[i]);
    res[i].flen = job.isContainment ? file_length_for_containment(fileList[i]) : 0;
  }
  for (size_t i = 0; i < nfiles; i++)
    if (slot[i] == 0) { fprintf(stderr, "cannot open the genome file: %s\n", fileList[i].c_str()); exit(1); }
  auto plan = [&](const vector<size_t>& files, const vector<uint64_t>& need) {
    vector<Batch> out;
    for (size_t q = 0; q < files.size(); q++) {
      if (out.empty() || (out.back().bytes + need[q] + 64 > BATCH_BYTES && !out.back().files.empty())) out.emplace_back();
      Batch& b = out.back();
      const uint64_t nd = packed ? (need[q] + 63) & ~(uint64_t)63 : need[q];  // packed slots start on 16-byte boundaries
      b.files.push_back(files[q]); b.slot_off.push_back(b.bytes); b.slot_len.push_back(nd);
      b.bytes += nd;
    }
    return out;
  };
  vector<size_t> all(nfiles);
  iota(all.begin(), all.end(), 0);
  vector<Batch> batches = plan(all, slot);
  uint64_t maxb = 0;
  for (const Batch& b : batches) maxb = std::max(maxb, b.bytes);

  // ---- the parser side of one batch: every file of it into its slot of `buf`, the runs of the packed format collected ----
  vector<size_t> retry_files; vector<uint64_t> retry_need;
  vector<size_t> row_file;  // row (= genome id) -> list position
  double parse_s = 0;       // wall time the parser threads took, summed over the batches (the GPU lanes work beside it)
  uint64_t parse_bytes = 0;
  std::atomic<uint64_t> gpu_copy_us{0}, gpu_sketch_us{0}, gpu_batches{0}, runs_total{0};  // the lanes' side of the batches (metrics)
  auto parse_batch = [&](const Batch& b, size_t bi, char* buf, vector<uint64_t>& bruns, int round) -> uint32_t {
    const double t0 = get_sec();
    vector<uint64_t> need(b.files.size(), 0);
    vector<vector<uint64_t>> fruns(packed ? b.files.size() : 0);
#pragma omp parallel for num_threads(job.threads) schedule(dynamic)
    for (long q = 0; q < (long)b.files.size(); q++) {
      FileResult& r = res[b.files[q]];
      uint64_t used = 0, nrec = 0;
      int st;
      if (packed) st = read_genome_file_packed(fileList[b.files[q]], (uint8_t*)buf + b.slot_off[q] / 4, b.slot_len[q], used, fruns[q], r.first, r.total, nrec);
      else st = read_genome_file_flat(fileList[b.files[q]], buf + b.slot_off[q], b.slot_len[q], used, r.first, r.total, nrec);
      if (st == 1) { fprintf(stderr, "cannot open the genome file: %s\n", fileList[b.files[q]].c_str()); exit(1); }
      if (st == 2) { need[q] = used + 1; used = 0; r.kept = false; }
      else r.kept = r.total >= job.minLen;                                 // :963
      if (!r.kept) used = 0;
      // no k-mers in the gap behind the genome, nor in dropped genomes
      if (!packed) memset(buf + b.slot_off[q] + used, 'N', b.slot_len[q] - used);
      else {
        vector<uint64_t>& fr = fruns[q];
        while (!fr.empty() && fr[fr.size() - 2] >= used) { fr.pop_back(); fr.pop_back(); }
        if (!fr.empty() && fr[fr.size() - 2] + fr[fr.size() - 1] > used) fr[fr.size() - 1] = used - fr[fr.size() - 2];
        if (b.slot_len[q] > used) { fr.push_back(used); fr.push_back(b.slot_len[q] - used); }
      }
    }
    if (!packed) memset(buf + b.bytes, 'N', 64);
    else {
      bruns.clear();
      for (size_t q = 0; q < b.files.size(); q++)
        for (size_t e = 0; e + 1 < fruns[q].size(); e += 2) { bruns.push_back(b.slot_off[q] + fruns[q][e]); bruns.push_back(fruns[q][e + 1]); }
      bruns.push_back(b.bytes); bruns.push_back(64);
    }
    uint32_t nkept = 0;
    for (size_t q = 0; q < b.files.size(); q++) {
      if (need[q]) { retry_files.push_back(b.files[q]); retry_need.push_back(need[q]); }
      if (res[b.files[q]].kept) { nkept++; if (round == 0) row_file.push_back(b.files[q]); }
    }
    parse_s += get_sec() - t0;
    parse_bytes += b.bytes;
    if (verbose) fprintf(stderr, "[parse] batch %zu: %zu files, %.2f GB in %.3fs\n", bi, b.files.size(), b.bytes / 1e9, get_sec() - t0);
    return nkept;
  };
  // Pageable staging by default: page-locking costs ~0.15 s/GB up front while the pageable PCIe copy
  // already runs at > 30 GB/s on the MI355X hosts measured; RTC_STAGE_PINNED=1 page-locks instead.
  bool pinned = getenv("RTC_STAGE_PINNED") != nullptr;
  // batches parsed while the GPUs come up (pageable staging only: page-locking needs a context).  The first PRE_RING of
  // them go straight into what becomes the staging ring (every configuration has at least three ring buffers: two lanes
  // + the one being parsed), so they cost no memory of their own -- every GiB of staging a run touches is 0.06 s at
  // process exit (the kernel frees it page by page), which is what a fourth pre-parsed 1-GiB batch in a buffer of its
  // own used to cost a 0.5 s run while saving it 0.05 s.  RTC_PREPARSE_BYTES (default: the three ring buffers) allows
  // more batches, each in a buffer of its own; 0 = parse only once the GPUs are there.
  struct PreBatch { char* buf; vector<uint64_t> runs; uint32_t kept; };
  vector<PreBatch> pre;
  const size_t PRE_RING = 3;
  const uint64_t ring_host_bytes = packed ? maxb / 4 + 64 : maxb + 64;
  if (gpus_ready && !pinned) {
    uint64_t budget = PRE_RING * ring_host_bytes, used = 0;
    if (const char* e = getenv("RTC_PREPARSE_BYTES")) budget = strtoull(e, nullptr, 10);
    while (pre.size() < batches.size() && !gpus_ready->done->load(std::memory_order_acquire)) {
      const Batch& b = batches[pre.size()];
      const uint64_t host_bytes = pre.size() < PRE_RING ? ring_host_bytes : packed ? b.bytes / 4 + 64 : b.bytes + 64;
      if (used + host_bytes > budget) break;
      char* buf = alloc_pageable(host_bytes);
      if (!buf) break;
      used += host_bytes;
      pre.push_back(PreBatch{buf, {}, 0});
      pre.back().kept = parse_batch(b, pre.size() - 1, buf, pre.back().runs, 0);
    }
    if (verbose) fprintf(stderr, "[init]  %zu of %zu batches parsed before the GPUs were up\n", pre.size(), batches.size());
  }
  if (gpus_ready) gpus_ready->wait();
  rtc_ctx* ctx = gpus[0].ctx;
  const size_t G = gpus.size();
  // Two lanes per GPU: lane 0 is the GPU's own context, lane 1 a second context on the same device with a
  // stream of its own, each driven by its own host thread -- the PCIe copy of one batch runs beside the
  // sketch kernel of the previous one.  Both lanes write rows of the same resident sketch buffer.
  struct Lane { rtc_ctx* ctx; void* d_seq; std::thread worker; size_t gpu; bool owned; void* d_packed = nullptr; void* d_runs = nullptr; size_t runs_cap = 0; };
  const size_t LPG = getenv("RTC_SINGLE_LANE") ? 1 : 2;
  vector<Lane> lanes(G * LPG);
  for (size_t l = 0; l < lanes.size(); l++) {
    lanes[l].gpu = l % G; lanes[l].d_seq = nullptr; lanes[l].owned = l >= G; lanes[l].ctx = gpus[l % G].ctx;
    if (lanes[l].owned) {
      CHECK(ctx, rtc_ctx_create(gpus[l % G].device, &lanes[l].ctx));
      CHECK(lanes[l].ctx, rtc_ctx_own_stream(lanes[l].ctx));
    }
  }
  const size_t NL = lanes.size();

  // ---- staging: G+1 host buffers (one being parsed, one per GPU in flight) and one device buffer per GPU ----
  const size_t NSTAGE = NL + 1;
  uint64_t buf_bytes = 0;
  vector<char*> stage(NSTAGE, nullptr);
  vector<vector<uint64_t>> stage_runs(NSTAGE);  // packed staging: the batch's runs of characters outside ACGT, batch coordinates
  auto free_stage = [&]() {
    for (size_t i = 0; i < NSTAGE; i++) {
      if (stage[i] && pinned) CHECK(ctx, rtc_host_free(ctx, stage[i]));
      else free(stage[i]);
      stage[i] = nullptr;
    }
  };
  auto ensure_buffers = [&](uint64_t need) {
    if (need <= buf_bytes) return;
    free_stage();
    for (Lane& l : lanes) {
      if (l.d_seq) { CHECK(l.ctx, rtc_dev_free(l.ctx, l.d_seq)); l.d_seq = nullptr; }
      if (l.d_packed) { CHECK(l.ctx, rtc_dev_free(l.ctx, l.d_packed)); l.d_packed = nullptr; }
    }
    const bool first = buf_bytes == 0;
    buf_bytes = need;
    const uint64_t host_bytes = packed ? buf_bytes / 4 + 64 : buf_bytes + 64;
    for (int i = 0; i < (int)NSTAGE; i++) {
      // the buffers the first batches were parsed into while the GPUs came up ARE ring slots 0 .. PRE_RING - 1 (batch i
      // of the pipeline below lives in slot i % NSTAGE, NSTAGE >= PRE_RING)
      if (first && !pinned && (size_t)i < PRE_RING && (size_t)i < pre.size() && host_bytes == ring_host_bytes) { stage[i] = pre[i].buf; continue; }
      if (pinned && rtc_host_alloc(ctx, host_bytes, (void**)&stage[i]) != RTC_OK) {
        // the host refuses to page-lock this much (ulimit -l): stage through pageable memory instead
        fprintf(stderr, "-----cannot page-lock %.2f GB (%s), staging through pageable memory\n", buf_bytes / 1e9, rtc_last_error(ctx));
        free_stage();
        pinned = false; i = -1;
        continue;
      }
      if (!pinned && !(stage[i] = alloc_pageable(host_bytes))) { fprintf(stderr, "ERROR: cannot allocate %.2f GB of staging memory\n", buf_bytes / 1e9); exit(1); }
    }
    // (the device staging buffers are allocated by the lanes themselves when their first batch arrives: lane_buffers)
  };
  // A lane's device staging, allocated on the lane's own host thread in front of its first copy: the two lanes of a GPU do
  // it side by side and the main thread is already parsing (two 1-GiB hipMallocs and two of 256 MiB used to sit between
  // "the GPUs are there" and the first batch).  The character buffer only where something reads characters.
  auto lane_buffers = [&](Lane& l, bool need_chars) {
    const uint64_t host_bytes = packed ? buf_bytes / 4 + 64 : buf_bytes + 64;
    if (packed && !l.d_packed) CHECK(l.ctx, rtc_dev_alloc(l.ctx, host_bytes, &l.d_packed));
    if (need_chars && !l.d_seq) CHECK(l.ctx, rtc_dev_alloc(l.ctx, buf_bytes + 128, &l.d_seq));
  };
  // Sketching over packed staging: the kernels read the 2-bit stream themselves -- rtc_sketch_minhash_packed_dev for every k,
  // rtc_sketch_kssd_packed_dev for the k-mer lengths the prefilter kernel covers.  RTC_SKETCH_UNPACK=1 (for --fast also the
  // older RTC_KSSD_UNPACK=1) expands every batch to characters in HBM first (the former path; tests compare the stagings)
  std::atomic<bool> direct{packed && getenv("RTC_SKETCH_UNPACK") == nullptr &&
                           (!job.kssd || (getenv("RTC_KSSD_UNPACK") == nullptr && half_subk == 6 && job.drlevel >= 3 &&
                                          (job.kmerSize + 1) / 2 * 2 >= 18 && (job.kmerSize + 1) / 2 * 2 <= 28))};
  ensure_buffers(maxb);
  // Each lane's first PCIe copy costs 17-29 ms instead of 6 (the runtime sets up the stream's copy path) and its buffers 5 ms:
  // the lanes do both now, on their worker threads, while this thread sizes and allocates the resident rows; the pipeline
  // joins a lane's worker before it hands it a batch.
  if (!getenv("RTC_NO_WARMUP"))
    for (size_t l = 0; l < NL; l++) {
      Lane* lp = &lanes[l];
      const char* src = stage[l % NSTAGE];
      const uint64_t warm_bytes = std::min<uint64_t>((uint64_t)8 << 20, packed ? buf_bytes / 4 : buf_bytes);
      lp->worker = std::thread([&lane_buffers, &direct, lp, src, warm_bytes, packed]() {
        lane_buffers(*lp, !direct.load());
        CHECK(lp->ctx, rtc_copy_h2d(lp->ctx, packed ? lp->d_packed : lp->d_seq, src, warm_bytes));
      });
    }
  if (verbose) fprintf(stderr, "[plan] %zu files, %zu batches, %zu GPU(s), staging %zu x %.2f GB, %.3fs\n", nfiles, batches.size(), G, NSTAGE, buf_bytes / 1e9, get_sec() - tp0);

  // ---- resident sketch rows: genome id g (list order among the kept files) owns row g on every GPU ----
  auto size_of = [&](size_t file) -> uint32_t {
    return job.isContainment ? (uint32_t)std::max(res[file].flen / job.containCompress, 100) : (uint32_t)job.sketchSize;  // :919-924
  };
  rs.width = job.kssd ? (use64 ? 8 : 4) : 8;
  rs.stride = 1;
  if (!job.kssd) for (size_t i = 0; i < nfiles; i++) rs.stride = std::max(rs.stride, size_of(i));
  else { uint64_t ms = 0; for (size_t i = 0; i < nfiles; i++) ms = std::max(ms, slot[i]); rs.stride = (uint32_t)(ms / (1ull << (4 * job.drlevel)) * 3 / 2 + 256); }
  rs.ok = getenv("RTC_HOST_SKETCHES") == nullptr;  // the switch forces the upload path (tests compare the two)
  rs.counts.assign(nfiles, 0);
  // The rows share ONE stride (the largest sketch any file can yield), so a single outlier -- one 3 Gbp assembly among
  // 100 000 bacterial genomes -- inflates every row.  The buffer has to fit beside the staging buffers with room left
  // for the clustering phase; when it does not (or the allocation fails) the run keeps per-batch temporary buffers
  // and clusters from the host vectors instead of stopping.
  if (rs.ok) {
    const size_t want = (size_t)nfiles * rs.stride * rs.width + (size_t)nfiles * 4 + 128;
    size_t budget = 0;
    if (const char* e = getenv("RTC_RESIDENT_BUDGET")) budget = strtoull(e, nullptr, 10);  // bytes (tests of the fallback)
    for (Gpu& g : gpus) {
      size_t fr = 0, tot = 0;
      CHECK(g.ctx, rtc_dev_mem_info(g.ctx, &fr, &tot));
      const size_t staging = NL / G * (size_t)(buf_bytes + buf_bytes / 4 + 256);  // the lanes allocate theirs with their first batch
      const size_t lim = budget ? budget : (fr > staging ? fr - staging : 0) / 2;
      if (want > lim) {
        fprintf(stderr, "-----resident sketch rows would take %.2f GB (%zu genomes x %u hashes, the largest genome sets the row) of %.2f GB free: "
                        "sketches go through host memory instead\n", want / 1e9, nfiles, rs.stride, fr / 1e9);
        rs.ok = false;
        break;
      }
    }
  }
  if (rs.ok)
    for (Gpu& g : gpus) {
      if (rtc_dev_alloc(g.ctx, (size_t)nfiles * rs.stride * rs.width + 64, &g.d_sk) != RTC_OK ||
          rtc_dev_alloc(g.ctx, (size_t)nfiles * 4 + 64, (void**)&g.d_cnt) != RTC_OK) {
        fprintf(stderr, "-----cannot keep the sketches resident (%s): sketches go through host memory instead\n", rtc_last_error(g.ctx));
        rs.ok = false;
        break;
      }
      // every count is written by the sketch kernels of its batch; rows of dropped files are never read
    }
  if (!rs.ok)
    for (Gpu& g : gpus) {
      if (g.d_sk) CHECK(g.ctx, rtc_dev_free(g.ctx, g.d_sk));
      if (g.d_cnt) CHECK(g.ctx, rtc_dev_free(g.ctx, g.d_cnt));
      g.d_sk = nullptr; g.d_cnt = nullptr;
    }
  std::atomic<bool> resident_ok{rs.ok};
  struct Placed { uint32_t row0, rows; int gpu; };  // where a batch's sketches live (share step)
  vector<Placed> placed;

  // ---- GPU side of one batch (runs on that GPU's host thread while the next batch is parsed) ----
  // row0 < 0: not resident (retry round), results only go to the host vectors.
  auto gpu_batch = [&](Lane& ln, const Batch& b, const char* h_seq, const vector<uint64_t>* h_runs, long row0) {
    Gpu& gp = gpus[ln.gpu];
    rtc_ctx* c = ln.ctx;
    const double t0 = get_sec();
    vector<uint64_t> off; vector<uint32_t> sizes; vector<size_t> kept;
    for (size_t q = 0; q < b.files.size(); q++) {
      FileResult& r = res[b.files[q]];
      if (!r.kept) continue;
      kept.push_back(b.files[q]);
      off.push_back(b.slot_off[q]);  // a genome extends to the next kept one: the gap holds only 'N'
      sizes.push_back(size_of(b.files[q]));
    }
    const uint32_t nb = (uint32_t)kept.size();
    if (!nb) return;
    off.push_back(b.bytes);
    bool dir = direct.load();  // read once per batch: another lane may switch the run to the unpack path meanwhile
    lane_buffers(ln, !dir);
    const double t0b = get_sec();
    if (packed) {
      const size_t nr = h_runs->size() / 2;
      if (nr > ln.runs_cap) {
        if (ln.d_runs) CHECK(c, rtc_dev_free(c, ln.d_runs));
        ln.runs_cap = nr + nr / 2 + 1024;
        CHECK(c, rtc_dev_alloc(c, ln.runs_cap * 16, &ln.d_runs));
      }
      CHECK(c, rtc_copy_h2d(c, ln.d_packed, h_seq, b.bytes / 4 + 16));
      CHECK(c, rtc_copy_h2d(c, ln.d_runs, h_runs->data(), nr * 16));
      if (!dir)
        CHECK(c, rtc_unpack_bases_dev(c, (const uint8_t*)ln.d_packed, b.bytes + 64, (const uint64_t*)ln.d_runs, nr, (uint8_t*)ln.d_seq));
    } else {
      CHECK(c, rtc_copy_h2d(c, ln.d_seq, h_seq, b.bytes + 64));
    }
    const double t1 = get_sec();
    const bool resident = row0 >= 0 && resident_ok.load();
    const bool to_host = need_host_hashes || !resident;
    const int w = rs.width;
    uint32_t* d_cnt = nullptr;
    if (resident) d_cnt = gp.d_cnt + row0;
    else CHECK(c, rtc_dev_alloc(c, (size_t)nb * 4, (void**)&d_cnt));
    vector<uint32_t> cnt(nb);
    uint32_t stride = rs.stride;
    void* d_out = nullptr;
    if (resident) d_out = (char*)gp.d_sk + (size_t)row0 * rs.stride * w;
    bool row_overflow = false;
    if (!job.kssd) {
      if (!resident) { stride = *std::max_element(sizes.begin(), sizes.end()); CHECK(c, rtc_dev_alloc(c, (size_t)nb * stride * 8, &d_out)); }
      // the batch is sketched as it crossed PCIe (the records update() is handed, src/SketchInfo.cpp:928-948, at 2 bits a base)
      if (dir) CHECK(c, rtc_sketch_minhash_packed_dev(c, (const uint8_t*)ln.d_packed, b.bytes + 64, (const uint64_t*)ln.d_runs, h_runs->size() / 2,
                                                      off.data(), nb, job.kmerSize, 42, sizes.data(), stride, (uint64_t*)d_out, stride, d_cnt));
      else CHECK(c, rtc_sketch_minhash_dev(c, (const uint8_t*)ln.d_seq, off.data(), nb, job.kmerSize, 42, sizes.data(), stride,
                                           (uint64_t*)d_out, stride, d_cnt));
    } else {
      if (!resident) {
        uint64_t maxlen = 0;
        for (uint32_t g = 0; g < nb; g++) maxlen = std::max(maxlen, off[g + 1] - off[g]);
        stride = (uint32_t)(maxlen / (1ull << (4 * job.drlevel)) * 3 / 2 + 256);
        CHECK(c, rtc_dev_alloc(c, (size_t)nb * stride * w, &d_out));
      }
      while (true) {
        int width = 0; uint32_t need = 0;
        int st;
        if (dir) {
          // the batch is sketched as it crossed PCIe; configurations the packed kernel does not serve (a shuffle table
          // its exact index cannot hold) are expanded in HBM after all, from here on for every batch
          st = rtc_sketch_kssd_packed_dev(c, (const uint8_t*)ln.d_packed, b.bytes + 64, (const uint64_t*)ln.d_runs, h_runs->size() / 2,
                                          off.data(), nb, job.kmerSize, job.drlevel, shuffled.data(), d_out, stride, d_cnt, &width, &need);
          if (st == RTC_ERR_UNSUPPORTED) {
            direct.store(false);
            dir = false;
            lane_buffers(ln, true);
            CHECK(c, rtc_unpack_bases_dev(c, (const uint8_t*)ln.d_packed, b.bytes + 64, (const uint64_t*)ln.d_runs, h_runs->size() / 2, (uint8_t*)ln.d_seq));
            continue;
          }
        } else {
          st = rtc_sketch_kssd_dev(c, (const uint8_t*)ln.d_seq, off.data(), nb, job.kmerSize, job.drlevel, shuffled.data(),
                                   d_out, stride, d_cnt, &width, &need);
        }
        if (st == RTC_ERR_OVERFLOW) {
          // a genome with more tuples than a resident row: this batch goes to a wider temporary buffer and
          // the run falls back to the host vectors (the other batches are pulled from HBM at the end)
          if (resident && !row_overflow) { row_overflow = true; resident_ok.store(false); CHECK(c, rtc_dev_alloc(c, (size_t)nb * 4, (void**)&d_cnt)); }
          else CHECK(c, rtc_dev_free(c, d_out));
          stride = need + 64;
          CHECK(c, rtc_dev_alloc(c, (size_t)nb * stride * w, &d_out));
          continue;
        }
        CHECK(c, st);
        break;
      }
    }
    const bool temp = !resident || row_overflow;
    CHECK(c, rtc_copy_d2h(c, cnt.data(), d_cnt, (size_t)nb * 4));
    if (dir) CHECK(c, rtc_ctx_sync(c));  // the stream is idle after the copy: this only reports a run list that broke its contract, against THIS batch
    if (row0 >= 0) for (uint32_t g = 0; g < nb; g++) rs.counts[row0 + g] = cnt[g];
    if (to_host || temp) {
      vector<unsigned char> out((size_t)nb * stride * w);
      CHECK(c, rtc_copy_d2h(c, out.data(), d_out, out.size()));
      for (uint32_t g = 0; g < nb; g++) {
        FileResult& r = res[kept[g]];
        if (w == 8) { const uint64_t* p = (const uint64_t*)out.data() + (size_t)g * stride; r.h64.assign(p, p + cnt[g]); }
        else { const uint32_t* p = (const uint32_t*)out.data() + (size_t)g * stride; r.h32.assign(p, p + cnt[g]); }
        r.on_host = true;
      }
    }
    if (temp) { CHECK(c, rtc_dev_free(c, d_out)); CHECK(c, rtc_dev_free(c, d_cnt)); }
    gpu_copy_us += (uint64_t)((t1 - t0b) * 1e6);
    gpu_sketch_us += (uint64_t)((get_sec() - t1) * 1e6);
    gpu_batches++;
    if (h_runs) runs_total += h_runs->size() / 2;
    if (verbose) fprintf(stderr, "[gpu %d.%d] %u genomes, %.2f GB: alloc %.3fs h2d %.3fs sketch%s %.3fs\n", (int)ln.gpu, (int)ln.owned, nb, b.bytes / 1e9, t0b - t0, t1 - t0b,
                         to_host || temp ? "+d2h" : "", get_sec() - t1);
  };

  // ---- pipeline: parse batch i into stage[i % (G+1)] while the GPU threads work on batches i-1 .. i-G ----
  size_t done_files = 0, bi = 0;
  uint32_t next_row = 0;
  for (int round = 0; round < 2; round++) {  // round 1: files whose slot guess was too small (gzip ISIZE)
    for (const Batch& b : batches) {
      const bool preparsed = round == 0 && bi < pre.size();  // parsed while the GPUs came up, in a buffer of its own
      char* buf = preparsed ? pre[bi].buf : stage[bi % NSTAGE];
      vector<uint64_t>& bruns = preparsed ? pre[bi].runs : stage_runs[bi % NSTAGE];
      const uint32_t nkept = preparsed ? pre[bi].kept : parse_batch(b, bi, buf, bruns, round);
      if (!retry_files.empty()) resident_ok.store(false);  // retried files arrive out of list order: ids are no longer row numbers
      Lane& ln = lanes[bi % NL];
      if (ln.worker.joinable()) ln.worker.join();
      if (shuffle_thread.joinable()) shuffle_thread.join();
      const Batch* bp = &b;
      const long row0 = round == 0 ? (long)next_row : -1;
      if (round == 0) { placed.push_back(Placed{next_row, nkept, (int)ln.gpu}); next_row += nkept; }
      Lane* lnp = &ln;
      const vector<uint64_t>* brp = &bruns;
      ln.worker = std::thread([&gpu_batch, lnp, bp, buf, brp, row0]() { gpu_batch(*lnp, *bp, buf, brp, row0); });
      for (size_t q = 0; q < b.files.size(); q++, done_files++) if (done_files % 10000 == 0) cerr << "---finished sketching: " << done_files << " genomes" << endl;
      bi++;
    }
    for (Lane& l : lanes) if (l.worker.joinable()) l.worker.join();
    if (round == 1 || retry_files.empty()) break;
    batches = plan(retry_files, retry_need);
    maxb = 0;
    for (const Batch& b : batches) maxb = std::max(maxb, b.bytes);
    ensure_buffers(maxb);
    done_files -= retry_files.size();
    retry_files.clear(); retry_need.clear();
  }
  if (shuffle_thread.joinable()) shuffle_thread.join();
  if (parse_s > 0) {  // the host feed: what ONE host can parse bounds what it can hand to 8 GPUs
    g_metrics.num("parse_s", parse_s);
    g_metrics.num("parse_gbp_per_s", (double)parse_bytes / parse_s / 1e9);
    g_metrics.num("parse_gbp_per_s_per_thread", (double)parse_bytes / parse_s / 1e9 / std::max(1, job.threads));
  }
  if (gpu_batches.load()) {  // per batch, on the lane's host thread: copy (+ unpack where a path still needs characters), sketch + read-back of the counts
    g_metrics.num("batches", (double)gpu_batches.load());
    g_metrics.num("gpu_copy_ms_per_batch", gpu_copy_us.load() / 1e3 / gpu_batches.load());
    g_metrics.num("gpu_sketch_ms_per_batch", gpu_sketch_us.load() / 1e3 / gpu_batches.load());
    g_metrics.num("runs_per_genome", (double)runs_total.load() / std::max<size_t>(1, nfiles));
  }
  {
    double inf_s = 0; uint64_t inf_b = 0;
    rtc_host_inflate_stats(&inf_s, &inf_b);
    if (inf_b) { g_metrics.num("inflate_s_all_threads", inf_s); g_metrics.num("inflate_gb_per_s_per_thread", (double)inf_b / inf_s / 1e9); }
  }
  const double tf0 = get_sec();
  // (the second lanes' contexts and every device staging buffer live until the process ends, see below)
  if (pinned) free_stage();
  // Pageable staging is NOT returned here: munmap of GBs of touched pages takes ~0.1 s and holds the
  // address-space lock, which stalls every hipMalloc of the clustering phase that follows (measured:
  // candidate edges 117 ms instead of 3 ms).  The pages go back when the process ends.
#ifdef RTC_MEASURE
  for (auto& p : stage) if (p) g_exit_probe_host.push_back(p);
  for (Lane& l : lanes) { if (l.d_seq) g_exit_probe_dev.push_back({l.ctx, l.d_seq}); if (l.d_packed) g_exit_probe_dev.push_back({l.ctx, l.d_packed}); }
#endif
  for (auto& p : stage) p = nullptr;
  // The device staging buffers stay allocated until the process ends: hipFree of a multi-GB buffer
  // costs ~0.4 s here and the clustering phase needs far less than the 288 GB that are there.
  if (verbose) fprintf(stderr, "[free]  host staging %.3fs\n", get_sec() - tf0);

  rs.ok = resident_ok.load();
  if (!rs.ok) {
    // fall back to the host vectors: pull the batches whose rows were left in HBM only
    for (const Placed& pl : placed) {
      if (!pl.rows || !gpus[pl.gpu].d_sk || res[row_file[pl.row0]].on_host) continue;
      Gpu& gp = gpus[pl.gpu];
      vector<unsigned char> out((size_t)pl.rows * rs.stride * rs.width);
      CHECK(gp.ctx, rtc_copy_d2h(gp.ctx, out.data(), (char*)gp.d_sk + (size_t)pl.row0 * rs.stride * rs.width, out.size()));
      for (uint32_t g = 0; g < pl.rows; g++) {
        FileResult& r = res[row_file[pl.row0 + g]];
        const uint32_t c = rs.counts[pl.row0 + g];
        if (rs.width == 8) { const uint64_t* q = (const uint64_t*)out.data() + (size_t)g * rs.stride; r.h64.assign(q, q + c); }
        else { const uint32_t* q = (const uint32_t*)out.data() + (size_t)g * rs.stride; r.h32.assign(q, q + c); }
        r.on_host = true;
      }
    }
    for (Gpu& g : gpus) {
      if (g.d_sk) CHECK(g.ctx, rtc_dev_free(g.ctx, g.d_sk));
      if (g.d_cnt) CHECK(g.ctx, rtc_dev_free(g.ctx, g.d_cnt));
      g.d_sk = nullptr; g.d_cnt = nullptr;
    }
  } else if (G > 1 || gpus[0].comm) {
    // ---- share: every batch's rows travel from the GPU that sketched them to all others (RCCL broadcast) ----
    const double ts0 = get_sec();
    on_all_gpus(gpus, [&](size_t g) {
      Gpu& gp = gpus[g];
      for (const Placed& pl : placed) {
        if (!pl.rows) continue;
        CHECK(gp.ctx, rtc_comm_broadcast(gp.comm, (char*)gp.d_sk + (size_t)pl.row0 * rs.stride * rs.width,
                                         (size_t)pl.rows * rs.stride * rs.width, pl.gpu));
        CHECK(gp.ctx, rtc_comm_broadcast(gp.comm, gp.d_cnt + pl.row0, (size_t)pl.rows * 4, pl.gpu));
      }
      CHECK(gp.ctx, rtc_ctx_sync(gp.ctx));
    });
    if (verbose) fprintf(stderr, "[share] %zu batches over %zu GPUs (%s) in %.3fs\n", placed.size(), G, rtc_comm_backend(gpus[0].comm), get_sec() - ts0);
  }
  rs.counts.resize(next_row);

  // ---- assemble in list order ----
  for (size_t i = 0; i < nfiles; i++) {
    FileResult& r = res[i];
    if (!r.kept) continue;
    GenomeInfo gi;
    gi.id = (int)genomes.size();                                        // :964-965 (list order here)
    gi.fileName = fileList[i];
    gi.totalSeqLength = r.total;
    gi.seq0 = r.first;
    gi.use64 = job.kssd ? ks->use64 : false;
    genomes.push_back(std::move(gi));
    if (!job.kssd) mh->hashes.push_back(std::move(r.h64));
    else if (use64) ks->h64.push_back(std::move(r.h64));
    else ks->h32.push_back(std::move(r.h32));
  }
}

// "all CPUs of the platform" (src/main.cpp:75-76,113), bounded by what this process may actually
// use: the affinity mask (omp_get_num_procs) and a cgroup-v2 CPU quota.  Oversubscribing a quota
// makes the parser threads time-slice against each other.
// sketchSequences / sketchSequencesWithKssd (src/SketchInfo.cpp:554-862, consumers :205-272, :274-436): without -l the
// input is ONE FASTA file and every record of at least minLen bases is a genome of its own (SequenceInfo{name, comment,
// strand 0, length}).  Records keep their file order (the reference's RabbitFX consumers merge per-thread vectors, so
// its order depends on the thread count; one consumer gives file order).  The records travel to the GPU back to back
// -- the offsets are the genome boundaries -- in batches; the sketches come back to the host vectors.
struct SeqModeSizes { uint64_t maxSize = 1, minSize = 1u << 31, totalSize = 0; int number = 0, badNumber = 0; };

static bool read_sequences(const string& inputFile, uint64_t minLen, vector<FastaRecord>& kept, SeqModeSizes& sz) {
  const size_t dot = inputFile.find_last_of('.');
  const string suf = dot == string::npos ? string() : inputFile.substr(dot + 1);
  if (suf != "fasta" && suf != "fna" && suf != "fa") {
    cerr << "error input format file: " << inputFile << endl << "Only support FASTA files" << endl;
    exit(1);
  }
  vector<FastaRecord> recs;
  if (!read_fasta(inputFile, recs)) { fprintf(stderr, "ERROR: sketchSequences(), cannot open the genome file, %s\n", inputFile.c_str()); return false; }
  for (FastaRecord& r : recs) {   // calSize, sequence branch (src/SketchInfo.cpp:484-535)
    const uint64_t len = r.seq.size();
    if (len < minLen) { sz.badNumber++; continue; }
    sz.maxSize = std::max(sz.maxSize, len); sz.minSize = std::min(sz.minSize, len); sz.totalSize += len; sz.number++;
    kept.push_back(std::move(r));
  }
  if (sz.number == 0) { cerr << "ERROR: calSize(), no sequence passes the minimum length filter" << endl; return false; }
  const int totalNumber = sz.number + sz.badNumber;
  cerr << "\t===the genome number for clustering is: " << sz.number << endl
       << "\t===the genome number below the minimum genome length threshold is: " << sz.badNumber << endl
       << "\t===the total genome number is: " << totalNumber << endl;
  if ((double)sz.badNumber / totalNumber >= 0.2)
    fprintf(stderr, "Warning: there are %d poor quality (length < %ld) genome assemblies in the total %d genome assemblied.\n", sz.badNumber, (long)minLen, totalNumber);
  cerr << "\t===the totalSize is: " << sz.totalSize << endl << "\t===the maxSize is: " << sz.maxSize << endl
       << "\t===the minSize is: " << sz.minSize << endl << "\t===the averageSize is: " << sz.totalSize / sz.number << endl;
  return true;
}

static void sketch_sequences(vector<Gpu>& gpus, vector<FastaRecord>& recs, const SketchJob& job, vector<GenomeInfo>& genomes,
                             MinHashSketchFile* mh, KssdSketchFile* ks) {
  rtc_ctx* c = gpus[0].ctx;
  const size_t n = recs.size();
  vector<int32_t> shuffled;
  int half_subk = 0;
  if (job.kssd) {
    half_subk = 6 - job.drlevel >= 2 ? 6 : job.drlevel + 2;
    shuffled = generate_shuffle_dim(half_subk);
    const int half_k = (job.kmerSize + 1) / 2;
    ks->info.half_k = half_k; ks->info.half_subk = half_subk; ks->info.drlevel = job.drlevel;
    ks->info.id = (half_k << 8) + (half_subk << 4) + job.drlevel; ks->info.genomeNumber = (int)n;
    ks->use64 = half_k - job.drlevel > 8;
  }
  genomes.resize(n);
  for (size_t i = 0; i < n; i++) {
    GenomeInfo& g = genomes[i];
    g.id = (int)i; g.totalSeqLength = recs[i].seq.size(); g.use64 = job.kssd && ks->use64;
    g.seq0.name = recs[i].name; g.seq0.comment = recs[i].has_comment ? recs[i].comment : string();
    g.seq0.strand = 0; g.seq0.length = (int)recs[i].seq.size();
  }
  if (job.kssd) { if (ks->use64) ks->h64.resize(n); else ks->h32.resize(n); } else mh->hashes.resize(n);
  const uint64_t BATCH = (uint64_t)1 << 30;
  void* d_seq = nullptr; uint64_t d_seq_bytes = 0;
  for (size_t i0 = 0; i0 < n;) {
    size_t i1 = i0; uint64_t bytes = 0;
    while (i1 < n && (i1 == i0 || bytes + recs[i1].seq.size() <= BATCH)) bytes += recs[i1++].seq.size();
    const uint32_t nb = (uint32_t)(i1 - i0);
    if (bytes + 64 > d_seq_bytes) { if (d_seq) CHECK(c, rtc_dev_free(c, d_seq)); d_seq_bytes = bytes + 64; CHECK(c, rtc_dev_alloc(c, d_seq_bytes, &d_seq)); }
    vector<char> h_seq(bytes + 64, 'N');
    vector<uint64_t> off(nb + 1, 0);
    vector<uint32_t> sizes(nb);
    for (uint32_t q = 0; q < nb; q++) {
      const string& sq = recs[i0 + q].seq;
      memcpy(h_seq.data() + off[q], sq.data(), sq.size());
      off[q + 1] = off[q] + sq.size();
      sizes[q] = job.isContainment ? (uint32_t)std::max((int)sq.size() / job.containCompress, 100) : (uint32_t)job.sketchSize;   // :224-231
    }
    CHECK(c, rtc_copy_h2d(c, d_seq, h_seq.data(), bytes + 64));
    uint32_t* d_cnt = nullptr; void* d_out = nullptr;
    CHECK(c, rtc_dev_alloc(c, (size_t)nb * 4 + 64, (void**)&d_cnt));
    uint32_t stride = 0; int w = 8;
    if (!job.kssd) {
      stride = *std::max_element(sizes.begin(), sizes.end());
      CHECK(c, rtc_dev_alloc(c, (size_t)nb * stride * 8 + 64, &d_out));
      CHECK(c, rtc_sketch_minhash_dev(c, (const uint8_t*)d_seq, off.data(), nb, job.kmerSize, 42, sizes.data(), stride, (uint64_t*)d_out, stride, d_cnt));
    } else {
      w = ks->use64 ? 8 : 4;
      uint64_t maxlen = 0;
      for (uint32_t q = 0; q < nb; q++) maxlen = std::max(maxlen, off[q + 1] - off[q]);
      stride = (uint32_t)(maxlen / (1ull << (4 * job.drlevel)) * 3 / 2 + 256);
      CHECK(c, rtc_dev_alloc(c, (size_t)nb * stride * w + 64, &d_out));
      while (true) {
        int width = 0; uint32_t need = 0;
        const int st = rtc_sketch_kssd_dev(c, (const uint8_t*)d_seq, off.data(), nb, job.kmerSize, job.drlevel, shuffled.data(), d_out, stride, d_cnt,
                                           &width, &need);
        if (st == RTC_ERR_OVERFLOW) {
          CHECK(c, rtc_dev_free(c, d_out));
          stride = need + 64;
          CHECK(c, rtc_dev_alloc(c, (size_t)nb * stride * w + 64, &d_out));
          continue;
        }
        CHECK(c, st);
        break;
      }
    }
    vector<uint32_t> cnt(nb);
    CHECK(c, rtc_copy_d2h(c, cnt.data(), d_cnt, (size_t)nb * 4));
    vector<unsigned char> out((size_t)nb * stride * w);
    CHECK(c, rtc_copy_d2h(c, out.data(), d_out, out.size()));
    for (uint32_t q = 0; q < nb; q++) {
      if (w == 8) {
        const uint64_t* p = (const uint64_t*)out.data() + (size_t)q * stride;
        if (job.kssd) ks->h64[i0 + q].assign(p, p + cnt[q]); else mh->hashes[i0 + q].assign(p, p + cnt[q]);
      } else {
        const uint32_t* p = (const uint32_t*)out.data() + (size_t)q * stride;
        ks->h32[i0 + q].assign(p, p + cnt[q]);
      }
    }
    CHECK(c, rtc_dev_free(c, d_out)); CHECK(c, rtc_dev_free(c, d_cnt));
    for (size_t i = i0; i < i1; i++) { string().swap(recs[i].seq); }
    i0 = i1;
  }
  if (d_seq) CHECK(c, rtc_dev_free(c, d_seq));
}

static int default_threads() {
  int n = omp_get_num_procs();
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0}; long period = 0;
    if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
      const long quota = atol(q);
      if (quota > 0) n = (int)std::min<long>(n, std::max<long>(1, (quota + period - 1) / period));
    }
    fclose(f);
  }
  return std::max(n, 1);
}

struct Options {
  string inputFile, outputFile, folder_path, premsted;
  bool newick = false, phylip = false, nexus = false, linkage = false;  // --newick-tree / --phylip-tree / --nexus-tree / --linkage-matrix
  bool dense = false;       // --dense: density maps, ANI histogram and the MST noise-removal pass
  bool has_append = false;  // --append LIST: inputFile holds the genomes to add to --presketched/--premsted DIR
  bool saveRep = false;     // clust-greedy --fast --save-rep: cluster_state.bin beside the sketches
  string repdb_path;        // clust-greedy --fast --db FILE with one of --build / --query / --assign / --append / --stats
  bool db_build = false, db_query = false, db_assign = false, db_stats = false;
  bool db_update = false;   // clust-dbscan --db FILE --update
  int topk = 5;             // --top-k of --query
  bool has_topk = false;
  int threads = default_threads();
  bool sketchByFile = false, noSave = false, is_fast = false, isContainment = false, isJaccard = false, isSetKmer = false;
  bool has_threshold = false, has_input = false, has_presketched = false, has_premsted = false, has_output = false;
  double threshold = 0.05;
  int kmerSize = 19, sketchSize = 1000, containCompress = 1000, drlevel = 3;
  uint64_t minLen = 10000;
  bool useIndex = true;  // --inverted-index=false: the dense estimator loops (modifyMST / greedyCluster) instead of the index path
  // clust-mst post-processing (src/main.cpp:205-209): the MST edge-length analysis, its stability, the near-duplicate groups
  // and the representatives per cluster.  Each acts in the flows where the reference honours it and is accepted elsewhere.
  bool autoThreshold = false, stability = false;
  double dedupDist = -1.0;
  int repsPerCluster = 0;
  string gpus;  // --gpus / RTC_GPUS: "all" (default), a count, or a comma list of device ordinals
  double dbscanEps = 0.05;  // clust-dbscan --eps / --minpts / --max-posting (src/main.cpp:173-182)
  int dbscanMinPts = 5, maxPosting = 0;
  vector<double> epsSweep;  // clust-dbscan --eps-sweep: further eps values served by the pair phase of --eps (rtc_dbscan_sweep)
  bool kdist = false;       // clust-dbscan --kdist: the k-distance curve, k = minPts - 1
  bool hierarchy = false;   // clust-dbscan --hierarchy: the density hierarchy below --eps (rtc_dbscan_hierarchy) and its flat clustering
  bool hasMinClusterSize = false;
  bool minhash = false;     // clust-dbscan --minhash: MinHashDBSCAN over MinHash sketches (rtc_dbscan_mash) instead of --fast;
                            // clust-leiden --minhash: the graph over MinHash sketches (rtc_graph_build_mash) instead of --fast
  bool hasMaxPosting = false;
  int minClusterSize = 0;   // --min-cluster-size (default: --minpts)
  int dbscanKnn = 0;        // clust-dbscan --knn: KssdDBSCAN over the k-NN graph (rtc_dbscan_knn); 0: the run without the flag
  // clust-leiden (src/main.cpp:184-198)
  double resolution = 1.0;
  bool has_resolution = false, louvain = false, leiden = false, has_pregraph = false, saveGraph = false;
  int knn = 0;
  string objective = "cpm";  // --objective, with --leiden: cpm as the reference calls igraph, or modularity
  bool has_objective = false;
  // clust-leiden --mcl: Markov clustering (rtc_mcl) as the third algorithm
  bool mcl = false;
  string inflation = "2.0", mclSelect = "1024", mclIterations = "100";  // as spelled: the refusals name them
  const char* mclOnly = nullptr;  // the first of --inflation / --mcl-select / --mcl-iterations, which only --mcl gives a meaning
  // clust-leiden --snn: shared-neighbour edge weights (rtc_graph_snn) in place of the pairs' own similarities
  bool snn = false, hasSnnPrune = false;
  string snnPrune = "0";  // as spelled
  bool hasDrlevel = false;
  string minhashOnly;        // clust-leiden: the first of -s / -c as spelled, which only --minhash gives a meaning
  bool linkageComplete = false;  // clust-mst --linkage complete: complete linkage inside every cluster (rtc_linkage_complete)
  bool quality = false;  // clust-mst --quality: silhouette, diameter and separation of the run's clusters (rtc_cluster_quality)
  bool orderDegree = false;  // clust-greedy --order degree: representatives by how many genomes they cover (rtc_greedy_degree)
  bool upgma = false;  // clust-mst --upgma: average linkage inside every cluster (rtc_upgma_clusters)
  bool njTree = false, njAll = false;  // clust-mst --nj-tree / --nj-all: neighbour-joining trees of the clusters / of all genomes (rtc_nj_clusters)
  bool has_njSupport = false, has_njSeed = false;  // clust-mst --nj-support B [--nj-seed S]: jackknife support values for those trees (rtc_nj_support)
  long long njSupport = 0;
  uint64_t njSeed = 0;
  bool has_clusterSupport = false, has_supportSeed = false;  // clust-mst --cluster-support B [--support-seed S]: jackknife support of the clusters themselves (rtc_cluster_support)
  long long clusterSupport = 0;
  uint64_t supportSeed = 0;
  bool pangenome = false, has_panSoft = false, has_panCloud = false;  // clust-mst --fast --pangenome [--pan-soft P] [--pan-cloud P]: core and accessory hashes of the clusters (rtc_pangenome)
  long long panSoft = 95, panCloud = 15;
  // clust-mst --fast --db FILE --screen: which clusters a sample contains (rtc_rep_screen)
  bool db_screen = false;
  string minContainment = "0.05", minShared = "2", minUnique = "2", screenPicks = "0";  // as spelled: the refusals read them
  const char* screenOnly = nullptr;  // the first of --min-containment / --min-shared / --min-unique / --screen-picks, which only --screen gives a meaning
};

#ifdef LEIDEN_CLUST
// q of rtc_wedge for a weight: max(1, llround(weight * 2^20)), as include/rtclust.h asks of the callers
static uint32_t leiden_weight_units(double weight) {
  const long long q = llround(weight * 1048576.0);
  return (uint32_t)std::min<long long>(std::max<long long>(q, 1), 0xffffffffll);
}
// leiden.graph in the reference's text layout (save_graph_to_file, src/leiden.cpp:474-491): "n m", then "u v weight" per edge,
// the weight as operator<< prints a double (6 significant digits)
static bool save_leiden_graph(const string& path, uint32_t n, const vector<rtc_gedge>& edges, const vector<double>& weights) {
  std::ofstream out(path);
  if (!out.is_open()) { cerr << "ERROR: Cannot open graph file for writing: " << path << endl; return false; }
  out << n << " " << edges.size() << "\n";
  for (size_t e = 0; e < edges.size(); e++) out << edges[e].u << " " << edges[e].v << " " << weights[e] << "\n";
  out.close();
  return !out.fail();
}
// the file back: every weight becomes q on the value the file holds (weights: the values themselves, for --leiden's own
// quantisation); a weight <= 0 cannot be an edge's
static bool load_leiden_graph(const string& path, vector<rtc_wedge>& edges, vector<double>& weights, uint64_t& n, string* why) {
  std::ifstream in(path);
  if (!in.is_open()) { *why = "cannot open " + path; return false; }
  uint64_t m = 0;
  if (!(in >> n >> m) || n >= 0x7fffffffull) { *why = path + ": no 'nodes edges' header"; return false; }
  edges.clear();
  weights.clear();
  edges.reserve((size_t)std::min<uint64_t>(m, (uint64_t)1 << 28));
  for (uint64_t e = 0; e < m; e++) {
    uint64_t u = 0, v = 0;
    double w = 0.0;
    if (!(in >> u >> v >> w)) { *why = path + ": " + std::to_string(e) + " of " + std::to_string(m) + " edges"; return false; }
    if (u >= n || v >= n || !(w > 0.0) || !(w <= 4095.0)) { *why = path + ": edge " + std::to_string(e) + " is out of range"; return false; }
    edges.push_back(rtc_wedge{(uint32_t)u, (uint32_t)v, leiden_weight_units(w)});
    weights.push_back(w);
  }
  return true;
}
#endif

static void unsupported(const char* what) {
  fprintf(stderr, "ERROR: %s is outside the sketch + all-pairs path this build implements\n", what);
  exit(1);
}

static Options parse(int argc, char** argv) {
  Options o;
  auto need = [&](int& i) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "ERROR: option %s requires a value\n", argv[i]); exit(1); } return argv[++i]; };
  for (int i = 1; i < argc; i++) {
    const string a = argv[i];
#ifdef LEIDEN_CLUST
    // the options of the Leiden build (src/main.cpp:184-198) and this build's own --save-graph; none of clust-dbscan's
    if (a == "--resolution") { o.resolution = atof(need(i)); o.has_resolution = true; continue; }
    if (a == "--louvain") { o.louvain = true; continue; }
    if (a == "--leiden") { o.leiden = true; continue; }
    if (a == "--objective") { o.objective = need(i); o.has_objective = true; continue; }
    if (a == "--mcl") { o.mcl = true; continue; }
    if (a == "--inflation") { o.inflation = need(i); if (!o.mclOnly) o.mclOnly = "--inflation"; continue; }
    if (a == "--mcl-select") { o.mclSelect = need(i); if (!o.mclOnly) o.mclOnly = "--mcl-select"; continue; }
    if (a == "--mcl-iterations") { o.mclIterations = need(i); if (!o.mclOnly) o.mclOnly = "--mcl-iterations"; continue; }
    if (a == "--snn") { o.snn = true; continue; }
    if (a == "--snn-prune") { o.snnPrune = need(i); o.hasSnnPrune = true; continue; }
    if (a == "--knn") { o.knn = atoi(need(i)); continue; }
    if (a == "--pregraph") { o.folder_path = need(i); o.has_pregraph = true; continue; }
    if (a == "--save-graph") { o.saveGraph = true; continue; }
    if (a == "--minhash") { o.minhash = true; continue; }
    if ((a == "-s" || a == "--sketch-size" || a == "-c" || a == "--containment") && o.minhashOnly.empty()) o.minhashOnly = a;
    if (a == "--append" || a == "--save-rep" || a == "--query" ||
        a == "--top-k" || a == "--dense" || a == "--premsted" || a == "--auto-threshold" || a == "--stability" || a == "--dedup-dist" ||
        a == "--reps-per-cluster" || a == "--newick-tree" || a == "--phylip-tree" || a == "--nexus-tree" || a == "--linkage-matrix" ||
        a == "--buildDB" || a.rfind("--inverted-index", 0) == 0) {
      fprintf(stderr, "ERROR: unknown option %s\n", a.c_str());
      exit(1);
    }
#elif defined(DBSCAN_CLUST)
    // the options of the DBSCAN build (src/main.cpp:173-182); the MST / greedy ones are not defined there.  The common options
    // -c (given to the KSSD tuner, as src/main.cpp:516 does), -s and --save-rep (no effect on DBSCAN) are parsed below.
    if (a == "--eps") { o.dbscanEps = atof(need(i)); continue; }
    if (a == "--minpts") { o.dbscanMinPts = atoi(need(i)); continue; }
    if (a == "--max-posting") { o.maxPosting = atoi(need(i)); o.hasMaxPosting = true; continue; }
    if (a == "--minhash") { o.minhash = true; continue; }
    if (a == "--eps-sweep") {
      // e1,e2,...: at most 32 values, each > 0 as atof reads it
      const string v = need(i);
      for (size_t p0 = 0; p0 <= v.size();) {
        size_t p1 = v.find(',', p0);
        if (p1 == string::npos) p1 = v.size();
        if (p1 == p0) { fprintf(stderr, "ERROR: --eps-sweep %s: empty element\n", v.c_str()); exit(1); }
        const double e = atof(v.substr(p0, p1 - p0).c_str());
        if (!(e > 0.0)) { fprintf(stderr, "ERROR: --eps-sweep %s: every value must be > 0\n", v.c_str()); exit(1); }
        o.epsSweep.push_back(e);
        p0 = p1 + 1;
      }
      if (o.epsSweep.size() > 32) { fprintf(stderr, "ERROR: --eps-sweep takes at most 32 values, got %zu\n", o.epsSweep.size()); exit(1); }
      continue;
    }
    if (a == "--kdist") { o.kdist = true; continue; }
    if (a == "--hierarchy") { o.hierarchy = true; continue; }
    if (a == "--min-cluster-size") { o.minClusterSize = atoi(need(i)); o.hasMinClusterSize = true; continue; }
    if (a == "--knn") { o.dbscanKnn = atoi(need(i)); continue; }
    if (a == "--update") { o.db_update = true; continue; }
    if (a == "--query" || a == "--top-k" || a == "--dense" ||
        a == "--premsted" || a == "--auto-threshold" || a == "--stability" || a == "--dedup-dist" || a == "--reps-per-cluster" ||
        a == "--newick-tree" || a == "--phylip-tree" || a == "--nexus-tree" || a == "--linkage-matrix" || a == "--buildDB") {
      fprintf(stderr, "ERROR: unknown option %s\n", a.c_str());
      exit(1);
    }
#endif
    if (a == "-t" || a == "--threads") { o.threads = atoi(need(i)); }
    else if (a == "-m" || a == "--min-length") { o.minLen = strtoull(need(i), nullptr, 10); fprintf(stderr, "-----set the filter minimum length: %ld\n", (long)o.minLen); }
    else if (a == "-c" || a == "--containment") { o.containCompress = atoi(need(i)); o.isContainment = true; fprintf(stderr, "-----use AAF distance with containment coefficient, the sketch size is in porportion with 1/%d\n", o.containCompress); }
    else if (a == "-k" || a == "--kmer-size") { o.kmerSize = atoi(need(i)); o.isSetKmer = true; fprintf(stderr, "-----set kmerSize: %d\n", o.kmerSize); }
    else if (a == "-s" || a == "--sketch-size") { o.sketchSize = atoi(need(i)); o.isJaccard = true; fprintf(stderr, "-----set sketchSize:  %d\n", o.sketchSize); }
    else if (a == "-l" || a == "--list") o.sketchByFile = true;
    else if (a == "-e" || a == "--no-save") o.noSave = true;
    else if (a == "-d" || a == "--threshold") { o.threshold = atof(need(i)); o.has_threshold = true; fprintf(stderr, "-----set threshold:  %g\n", o.threshold); }
    else if (a == "-o" || a == "--output") { o.outputFile = need(i); o.has_output = true; }
    else if (a == "-i" || a == "--input") { o.inputFile = need(i); o.has_input = true; }
    else if (a == "--presketched") { o.folder_path = need(i); o.has_presketched = true; }
    else if (a == "--append") { o.inputFile = need(i); o.has_append = true; }
    else if (a == "--fast") o.is_fast = true;
#ifdef GREEDY_CLUST
    else if (a == "--save-rep") o.saveRep = true;
    else if (a == "--order") {
      if (strcmp(need(i), "degree") != 0) { fprintf(stderr, "ERROR: --order must be degree\n"); exit(1); }
      o.orderDegree = true;
    }
#endif
    else if (a == "--db") o.repdb_path = need(i);
    else if (a == "--build") o.db_build = true;
    else if (a == "--query") o.db_query = true;
    else if (a == "--assign") o.db_assign = true;
    else if (a == "--stats") o.db_stats = true;
    else if (a == "--top-k") { o.topk = atoi(need(i)); o.has_topk = true; }
    else if (a == "--drlevel") { o.drlevel = atoi(need(i)); o.hasDrlevel = true; }
    else if (a == "--gpus") o.gpus = need(i);
#ifndef GREEDY_CLUST
    else if (a == "--dense") o.dense = true;
    else if (a == "--newick-tree") o.newick = true;
    else if (a == "--phylip-tree") o.phylip = true;
    else if (a == "--nexus-tree") o.nexus = true;
    else if (a == "--linkage-matrix") o.linkage = true;
#endif
    else if (a == "--inverted-index") { /* on by default, as in the reference (src/main.cpp:104,129) */ }
    else if (a.rfind("--inverted-index=", 0) == 0) {  // the flag's CLI11 form with a value: =false / =0 switches the index path off
      const string v = a.substr(17);
      o.useIndex = !(v == "false" || v == "0" || v == "off" || v == "no");
    }
#ifndef GREEDY_CLUST
    else if (a == "--save-rep") o.saveRep = true;
    else if (a == "--premsted") { o.folder_path = need(i); o.has_premsted = true; }
    else if (a == "--auto-threshold") o.autoThreshold = true;
    else if (a == "--stability") o.stability = true;
    else if (a == "--dedup-dist") o.dedupDist = atof(need(i));
    else if (a == "--reps-per-cluster") o.repsPerCluster = atoi(need(i));
#endif
#if !defined(GREEDY_CLUST) && !defined(DBSCAN_CLUST) && !defined(LEIDEN_CLUST)
    else if (a == "--linkage") {
      if (strcmp(need(i), "complete") != 0) { fprintf(stderr, "ERROR: --linkage must be complete\n"); exit(1); }
      o.linkageComplete = true;
    }
    else if (a == "--nj-tree") o.njTree = true;
    else if (a == "--nj-all") o.njAll = true;
    else if (a == "--nj-support") { o.njSupport = atoll(need(i)); o.has_njSupport = true; }
    else if (a == "--nj-seed") { o.njSeed = strtoull(need(i), nullptr, 10); o.has_njSeed = true; }
    else if (a == "--quality") o.quality = true;
    else if (a == "--cluster-support") { o.clusterSupport = atoll(need(i)); o.has_clusterSupport = true; }
    else if (a == "--support-seed") { o.supportSeed = strtoull(need(i), nullptr, 10); o.has_supportSeed = true; }
    else if (a == "--upgma") o.upgma = true;
    else if (a == "--pangenome") o.pangenome = true;
    else if (a == "--pan-soft") { o.panSoft = atoll(need(i)); o.has_panSoft = true; }
    else if (a == "--pan-cloud") { o.panCloud = atoll(need(i)); o.has_panCloud = true; }
    else if (a == "--screen") o.db_screen = true;
    else if (a == "--min-containment") { o.minContainment = need(i); if (!o.screenOnly) o.screenOnly = "--min-containment"; }
    else if (a == "--min-shared") { o.minShared = need(i); if (!o.screenOnly) o.screenOnly = "--min-shared"; }
    else if (a == "--min-unique") { o.minUnique = need(i); if (!o.screenOnly) o.screenOnly = "--min-unique"; }
    else if (a == "--screen-picks") { o.screenPicks = need(i); if (!o.screenOnly) o.screenOnly = "--screen-picks"; }
#endif
    else if (a == "-h" || a == "--help") {
#ifdef GREEDY_CLUST
      puts("clust-greedy (MI355X build): greedy incremental clustering module");
#elif defined(LEIDEN_CLUST)
      puts("clust-leiden (MI355X build): graph-based community detection (Leiden, Louvain) clustering module, KSSD sketches (--fast)\n"
           "or MinHash sketches (--minhash)");
      puts("  -t,--threads N  -m,--min-length N  -k,--kmer-size N (default 19)  -l,--list  -e,--no-save  -d,--threshold X (default 0.05:\n"
           "  a pair is an edge when its distance is below it)  -o,--output FILE  -i,--input FILE  --presketched DIR\n"
           "  --fast | --minhash (one of the two is required)  --drlevel N (--fast)\n"
           "  --gpus all|N|i,j,.. (sketching on every GPU, graph and clustering on the first)\n"
           "  --minhash (instead of --fast: MinHash sketches as clust-mst makes and saves them, -k / -s,--sketch-size / -m and the\n"
           "             tuner as there, or a MinHash --presketched DIR, k and s from it; a pair is an edge when MinHash::distance()\n"
           "             on the union-truncated counts is below -d, 0 < d <= 1, with no size-ratio rule; --knn ranks by common / denom;\n"
           "             not with --fast, -c, --drlevel or --db)\n"
           "  --leiden | --louvain (one of the two is required; they exclude each other)  --resolution X (default 1.0; higher: more\n"
           "  clusters)\n"
           "  --leiden: the deterministic Leiden of include/rtclust.h (move phase, refinement into connected well-connected pieces,\n"
           "           aggregation on the refined partition, iterations until the labels repeat)\n"
           "  --objective cpm|modularity (with --leiden; default cpm, as the reference calls igraph: node weight 1, the weights\n"
           "           normalised to [0, 1] when their range is below 0.5, the lightest edge dropping out.  Under cpm a --resolution\n"
           "           of 1 or more -- the default included -- moves nothing and leaves every genome in its own cluster, which is\n"
           "           what the reference's call does too: use --resolution below 1, or --objective modularity, to get clusters)\n"
           "  --mcl (the third algorithm: Markov clustering in the fixed point of include/rtclust.h -- expansion, inflation and\n"
           "         selection of the graph's flow matrix until it repeats; no objective and no resolution: not with --louvain,\n"
           "         --leiden, --resolution, --objective or --db --build)\n"
           "  --inflation X (with --mcl; default 2.0; a multiple of 0.5 between 1.5 and 8; higher: more clusters)\n"
           "  --mcl-select S (with --mcl; default 1024; a column of the matrix keeps its S largest entries, 1 .. 4096)\n"
           "  --mcl-iterations T (with --mcl; default 100; a run that has not converged by then warns and writes what it has)\n"
           "  --snn (with any of the three algorithms: the weight of an edge becomes the shared-neighbour weight of include/rtclust.h,\n"
           "         the Jaccard index of its two ends' closed neighbourhoods in the graph, (shared + 2) / (deg u + deg v - shared),\n"
           "         counted on the GPU, in place of the pair's own 1 - distance; --save-graph still writes the similarity graph, and\n"
           "         --pregraph DIR --snn gives the direct --snn run's result; not with --db)\n"
           "  --snn-prune X (with --snn; default 0; 0 <= X < 1: the edges whose new weight is below X drop out, in one pass -- a\n"
           "                 dropped edge still counted in the neighbourhoods)\n"
           "  --knn K (every genome keeps its K best edges among the higher-numbered genomes; 0 or absent: 1000 with --louvain, 500\n"
           "           with --leiden and --mcl; 1..9: 50 with a warning, as the reference defaults it, so the filter cannot be\n"
           "           switched off)\n"
           "  --save-graph (leiden.graph into the sketch folder: 'n m', then 'u v weight' per edge; the weights carry 6 significant\n"
           "                digits, so a --pregraph run is defined on the file's weights, not on the sketches')\n"
           "  --pregraph DIR (DIR/leiden.graph and the KSSD sketches of DIR -- with --minhash its MinHash sketches: the clustering\n"
           "                  alone, for another --resolution)\n"
           "  --db FILE --build (with the flags above: the run as without --db, then the model -- labels, community totals, the\n"
           "                     run's parameters and quantisation, genome records and all sketches -- into FILE; not with --pregraph)\n"
           "  --db FILE --assign (-l -i LIST | -i FASTA) -o assign.tsv (new genomes placed into the model's communities on the GPU:\n"
           "                     k, sketch parameters, threshold, knn, objective and resolution come from FILE; per query its\n"
           "                     cluster or novel, the runner-up, edges kept, communities touched, the weight to the cluster and\n"
           "                     its share, the nearest genome and its distance; the model is not changed)\n"
           "  --db FILE --stats (algorithm, parameters, genomes and clusters of FILE; no GPU, no -o)");
      exit(0);
#elif defined(DBSCAN_CLUST)
      puts("clust-dbscan (MI355X build): DBSCAN density-based clustering module (KSSD with --fast, MinHash with --minhash)");
      puts("  -t,--threads N  -m,--min-length N  -k,--kmer-size N  -l,--list  -e,--no-save  -d,--threshold X (KSSD tuner)\n"
           "  -o,--output FILE  -i,--input FILE  --presketched DIR  --fast  --drlevel N  --gpus all|N|i,j,..\n"
           "  --eps X (default 0.05)  --minpts N (default 5)  --max-posting M (0: off)\n"
           "  --eps-sweep e1,e2,.. (at most 32 further eps values from the same pair phase: FILE.eps_<value>, FILE.eps_sweep.tsv)\n"
           "  --kdist (FILE.kdist.tsv: every genome's distance to its (minpts - 1)-th nearest candidate, largest first)\n"
           "  --hierarchy (the density hierarchy of every eps up to --eps from the same pair phase: FILE.hierarchy.tsv, FILE.core.tsv,\n"
           "               and FILE.hdbscan, a flat clustering that needs no eps)  --min-cluster-size M (default: --minpts, >= 2)\n"
           "  --minhash (instead of --fast: MinHash sketches as clust-mst makes and saves them, -k / -s / -m as there, or a MinHash\n"
           "             --presketched DIR; neighbours by MinHash::distance() <= eps, 0 <= eps < 1, a core point has minpts neighbours\n"
           "             besides itself; with --eps-sweep, not with --kdist, --hierarchy, --min-cluster-size, --max-posting or -c)\n"
           "  --db FILE --build (with the flags above: the run as without --db, then the model of --eps -- labels, core flags, genome\n"
           "                     records and all sketches -- into FILE; not with --max-posting)\n"
           "  --db FILE --assign (-l -i LIST | -i FASTA) -o assign.tsv (new genomes placed into the model on the GPU: kind, k, sketch\n"
           "                     parameters, eps and minpts come from FILE; per query its cluster or novel, bridges, neighbours, core\n"
           "                     neighbours, would_be_core, the nearest genome and its distance)\n"
           "  --db FILE --update -l -i LIST -o updated.dbscan (new genomes ADDED to the model: sketched as --assign sketches them, the\n"
           "                     clustering of all genomes as --build over the old list followed by LIST gives it, byte for byte,\n"
           "                     but only the new genomes and the old noise and border genomes are measured again; FILE is\n"
           "                     rewritten in place; -l as the model was built; not with --knn, --eps-sweep, --kdist, --hierarchy or\n"
           "                     --max-posting, nor for a model built with --max-posting)\n"
           "  --db FILE --stats (kind, parameters, genomes, clusters, noise and core points of FILE; no GPU)\n"
           "  -c,--containment N (KSSD tuner)  -s,--sketch-size N  --save-rep (accepted, no effect on DBSCAN)\n"
           "  --knn K (the reference's approximate k-NN DBSCAN, label-identical: every genome keeps its K best-scoring candidates, then\n"
           "           those within eps; 0: off; K < minpts - 1 is raised to it.  The GPU gains no time from it -- the pair phase\n"
           "           already produces every candidate -- it is there to reproduce the reference's clusters.  With --fast, lists,\n"
           "           a single FASTA, --presketched, --max-posting and -c; not with --minhash, --eps-sweep, --kdist, --hierarchy,\n"
           "           --min-cluster-size or --db)");
      exit(0);
#else
      puts("clust-mst (MI355X build): minimum-spanning-tree-based module");
#endif
      puts("  -t,--threads N  -m,--min-length N  -c,--containment N  -k,--kmer-size N  -s,--sketch-size N\n"
           "  -l,--list  -e,--no-save  -d,--threshold X  -o,--output FILE  -i,--input FILE\n"
           "  --presketched DIR  --fast  --drlevel N  --gpus all|N|i,j,.. (default all visible MI355X)\n"
           "  --inverted-index=false (MinHash: the dense loops modifyMST / greedyCluster with MinHash::distance())"
#ifndef GREEDY_CLUST
           "  --premsted DIR  --append LIST (with --presketched/--premsted DIR)\n"
           "  --auto-threshold  --stability  --dedup-dist D  --reps-per-cluster K (with --fast: <output>.dedup / .reps)\n"
           "  --save-rep (mst_cluster_state.bin beside the sketches; a later --append measures against its representatives)\n"
           "  --linkage complete (complete linkage inside every cluster of the run: <output>.complete, where every two members of\n"
           "             a cluster are within -d, and <output>.complete.linkage.txt; with --fast or MinHash on the index path)\n"
           "  --nj-tree (a neighbour-joining tree of every cluster over the exact set-Jaccard distances, joined on the GPU:\n"
           "             <output>.nj.newick, one tree a line in the order of <output>; with --fast or MinHash on the index path)\n"
           "  --nj-all (one neighbour-joining tree over all genomes: <output>.nj.all.newick; genomes that share no hash are at distance 1)\n"
           "  --nj-support B [--nj-seed S] (with --nj-tree / --nj-all: B = 1 .. 256 delete-half jackknife replicates over the sketch\n"
           "             hashes, counted on the GPU; <output>.nj.support.newick / .nj.all.support.newick carry every inner branch's\n"
           "             support in percent, <output>.nj.support.tsv / .nj.all.support.tsv the counts; S: the mask seed, default 0)\n"
           "  --quality (how good the partition is, over the exact set-Jaccard distances, scored on the GPU: <output>.quality.tsv, a\n"
           "             line a cluster with its mean and least silhouette, mean intra-cluster distance, diameter, separation and\n"
           "             nearest cluster, and <output>.silhouette.tsv, a line a genome; with --fast or MinHash on the index path)\n"
           "  --cluster-support B [--support-seed S] (which clusters survive resampling: B = 1 .. 256 delete-half jackknife replicates\n"
           "             over the sketch hashes, each with its own single-linkage components at -d, formed on the GPU;\n"
           "             <output>.support.tsv, a line a cluster with the replicates that recover, split, merge and mix it, and\n"
           "             <output>.support.genomes.tsv, a line a genome; S: the mask seed, default 0)\n"
           "  --upgma (average linkage, UPGMA, inside every cluster of the run, in exact integers on the GPU: <output>.upgma, the\n"
           "             clusters cut at -d by mean distance; <output>.upgma.linkage.txt, every merge; <output>.upgma.newick, one\n"
           "             ultrametric tree a line in the order of <output>; with --fast or MinHash on the index path)\n"
           "  --fast --pangenome [--pan-soft P] [--pan-cloud P] (what the members of every cluster hold in common: how many members\n"
           "             hold each sketch hash, counted on the GPU; <output>.pangenome.tsv, a line a cluster with its pan, core,\n"
           "             soft-core (held by at least P %, default 95), shell and cloud (by less than P %, default 15) hashes and its\n"
           "             most typical member; <output>.pangenome.genomes.tsv, a line a genome; <output>.pangenome.hist.tsv, hashes by\n"
           "             the number of members that hold them; <output>.pangenome.curve.tsv, the expected pan and core size after j\n"
           "             members; KSSD sketches only)\n"
           "  [--fast] --db FILE --build|--query|--assign|--append LIST|--stats [--top-k N] (MST representative database)\n"
           "  --fast --db FILE --screen -i SAMPLES [--min-containment C] [--min-shared N] [--min-unique N] [--screen-picks N] (which\n"
           "             clusters a mixture holds: the containment of every representative in every sample and a winner-takes-all\n"
           "             decomposition of the sample, on the GPU; <output>, a line a hit, and <output>.summary.tsv, a line a sample;\n"
           "             defaults 0.05, 2, 2 and 0 = no limit; KSSD databases only)"
#else
           "  --append LIST (with --presketched DIR)  --save-rep (cluster_state.bin beside the sketches)\n"
           "  --order degree (clusters that do not depend on the order of the genomes: two genomes are neighbours when they are\n"
           "             within -d, the genomes are walked by their number of neighbours, most first, the larger genome first among\n"
           "             equals, one becomes a representative when no earlier representative is its neighbour, and every other\n"
           "             genome joins its most similar neighbouring representative -- all on the GPU; <output>.order.tsv lists the\n"
           "             genomes in that order with degree, role, representative and distance; with --fast or MinHash sketches\n"
           "             (0 <= d < 1), lists, a single FASTA and --presketched; not with -c, --inverted-index=false, --append,\n"
           "             --db or --save-rep)\n"
           "  [--fast] --db FILE --build|--query|--assign|--append LIST|--stats [--top-k N] (representative database)"
#endif
      );
      exit(0);
    }
    else if (
#ifdef GREEDY_CLUST
             a == "--dense" || a == "--auto-threshold" || a == "--stability" || a == "--dedup-dist" || a == "--reps-per-cluster" ||
#endif
              a == "--newick-tree" || a == "--phylip-tree" ||
             a == "--nexus-tree" || a == "--linkage-matrix" || a == "--buildDB")
      unsupported(a.c_str());
    else { fprintf(stderr, "ERROR: unknown option %s\n", a.c_str()); exit(1); }
  }
  return o;
}

[[maybe_unused]] static void cluster_from_mst(const vector<rtc_edge>& mst, const vector<GenomeInfo>& genomes, bool sketchByFile,
                             const string& outputFile, double threshold, vector<rtc_edge>* forest_out = nullptr,
                             vector<vector<int>>* clusters_out = nullptr) {
  vector<rtc_edge> forest = generate_forest(mst, threshold);
  vector<vector<int>> cl = generate_cluster_with_bfs(forest, (int)genomes.size());
  print_result(cl, genomes, sketchByFile, outputFile, threshold);
  if (forest_out) *forest_out = forest;
  if (clusters_out) *clusters_out = cl;
  cerr << "-----write the cluster result into: " << outputFile << endl;
  cerr << "-----the cluster number of: " << outputFile << " is: " << cl.size() << endl;
  g_metrics.num("clusters", (double)cl.size());
}

struct Options;
static void write_trees(const Options& o, const vector<GenomeInfo>& genomes, const vector<rtc_edge>& mst, bool byFile);

// --dense noise removal (src/sub_command.cpp:3071-3103): drop the forest edges of low-density nodes, cluster again
[[maybe_unused]] static void remove_noise_and_print(const vector<rtc_edge>& mst, const vector<GenomeInfo>& genomes, bool sketchByFile,
                                                    const string& outputFile, double threshold, const vector<int32_t>& dense, int span,
                                                    vector<rtc_edge>* forest_out = nullptr, vector<vector<int>>* clusters_out = nullptr) {
  vector<rtc_edge> forest = generate_forest(mst, threshold);
  vector<vector<int>> cl = generate_cluster_with_bfs(forest, (int)genomes.size());
  vector<int> noise = noise_nodes(cl, dense, span, (int)genomes.size(), threshold);
  cerr << "-----the total noiseArr size is: " << noise.size() << endl;
  forest = modify_forest(forest, noise);
  vector<vector<int>> cluster = generate_cluster_with_bfs(forest, (int)genomes.size());
  const string outputFileNew = outputFile + ".removeNoise";
  print_result(cluster, genomes, sketchByFile, outputFileNew);
  cerr << "-----write the cluster without noise into: " << outputFileNew << endl;
  cerr << "-----the cluster number of: " << outputFileNew << " is: " << cluster.size() << endl;
  if (forest_out) *forest_out = forest;
  if (clusters_out) *clusters_out = cluster;
}

// --dedup-dist / --reps-per-cluster after a clustering (src/sub_command.cpp:2089-2103, :2130-2144, :2583-2597, :2624-2638):
// <base>.dedup holds every cluster's representatives of its near-duplicate groups, <base>.reps up to K of them chosen
// farthest-first on the forest's tree metric.  The groups' tree medoids come from rtc_tree_medoids (large groups on the GPU).
[[maybe_unused]] static void dedup_and_reps(rtc_ctx* ctx, double dedup_dist, int reps_per_cluster, int threads, const vector<rtc_edge>& forest,
                                            const vector<vector<int>>& clusters, const vector<GenomeInfo>& genomes, bool sketchByFile,
                                            const string& base) {
  if (!(dedup_dist > 0) && !(reps_per_cluster > 0)) return;
  const int n = (int)genomes.size();
  vector<int> node_to_rep(n);
  for (int i = 0; i < n; i++) node_to_rep[i] = i;
  if (dedup_dist > 0) {
    vector<uint64_t> lens(n);  // get_seq_len (src/cluster_postprocess.cpp:13-19): the medoid ties go to the longer sequence
    for (int i = 0; i < n; i++) lens[i] = sketchByFile ? genomes[i].totalSeqLength : (uint64_t)genomes[i].seq0.length;
    vector<int32_t> rep(n);
    CHECK(ctx, rtc_ctx_set_host_threads(ctx, threads));
    CHECK(ctx, rtc_tree_medoids(ctx, (uint32_t)n, forest.data(), forest.size(), dedup_dist, lens.data(), rep.data()));
    for (int i = 0; i < n; i++) node_to_rep[i] = rep[i];
  }
  const vector<vector<int>> candidates = dedup_candidates(clusters, node_to_rep, dedup_dist);
  if (dedup_dist > 0) {
    const string f = base + ".dedup";
    print_result(candidates, genomes, sketchByFile, f);
    cerr << "-----write the deduped cluster result into: " << f << endl;
  }
  if (reps_per_cluster > 0) {
    const string f = base + ".reps";
    print_result(select_k_reps(clusters, candidates, forest, n, node_to_rep, reps_per_cluster), genomes, sketchByFile, f);
    cerr << "-----write the reps-per-cluster result into: " << f << endl;
  }
}

[[maybe_unused]] static vector<vector<int>> clusters_from_rep_of(const vector<int32_t>& rep_of) {
  // cluster list in representative-creation order: [rep, members...] (src/greedy.cpp:1355-1367)
  vector<vector<int>> cl; vector<int> cid(rep_of.size(), -1);
  for (size_t i = 0; i < rep_of.size(); i++) if (rep_of[i] == (int32_t)i) { cid[i] = (int)cl.size(); cl.push_back({(int)i}); }
  for (size_t i = 0; i < rep_of.size(); i++) if (rep_of[i] != (int32_t)i) cl[cid[rep_of[i]]].push_back((int)i);
  return cl;
}

// src/sub_command.cpp:3010-3029 (and the same block in the --premsted / --append flows)
[[maybe_unused]] static void write_trees(const Options& o, const vector<GenomeInfo>& genomes, const vector<rtc_edge>& mst, bool byFile) {
  if (o.newick) { const string f = o.outputFile + ".newick.tree"; print_newick_tree(genomes, mst, byFile, f); cerr << "-----write the newick tree into: " << f << endl; }
  if (o.phylip) { const string f = o.outputFile + ".phylip.tree"; print_phylip_tree(genomes, mst, byFile, f); cerr << "-----write the PHYLIP tree into: " << f << endl; }
  if (o.nexus) { const string f = o.outputFile + ".nexus.tree"; print_nexus_tree(genomes, mst, byFile, f); cerr << "-----write the NEXUS tree into: " << f << endl; }
  if (o.linkage) { const string f = o.outputFile + ".linkage.txt"; print_linkage_matrix((int)genomes.size(), mst, f); cerr << "-----write the linkage matrix into: " << f << endl; }
}

#if !defined(GREEDY_CLUST) && !defined(DBSCAN_CLUST) && !defined(LEIDEN_CLUST)
// --linkage complete: complete linkage inside every cluster of the plain run (include/rtclust.h has the definition).  The device
// hands back every component's merges on exact keys; the host gives each its distance through the function that weighs the
// MST's edges and applies a component's merges up to, not including, the first one past the threshold (generate_forest's <=).
// <base>.complete: the refined clusters in print_result's layout, by smallest member; <base>.complete.linkage.txt: the kept
// merges as print_linkage_matrix writes them, leaves as genome indices, new ids N, N + 1, ... in file order.
static void linkage_complete_and_print(rtc_ctx* ctx, const DeviceSketches& ds, const vector<vector<int>>& clusters, const vector<GenomeInfo>& genomes,
                                       bool sketchByFile, const string& base, double threshold, int kmer_size) {
  const uint32_t n = (uint32_t)genomes.size();
  vector<uint32_t> comp(n, 0);
  for (size_t c = 0; c < clusters.size(); c++) for (int g : clusters[c]) comp[g] = (uint32_t)c;
  // the stop bound: conservative, any bound at or below the true one gives the same cut
  const double j = 1.0 / (2.0 * exp((double)kmer_size * threshold) - 1.0) * (1.0 - 1.0 / 1048576.0);
  const double jn = floor(j * 2147483648.0);
  const uint32_t kmin_num = !(jn > 0.0) ? 0u : jn >= 2147483648.0 ? 2147483648u : (uint32_t)jn;
  vector<rtc_lmerge> merges(n > 1 ? n - 1 : 1);
  vector<uint64_t> first((size_t)n + 1, 0);
  uint64_t n_merges = 0;
  CHECK(ctx, rtc_linkage_complete(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, n, comp.data(), kmin_num, 2147483648u, merges.data(), merges.size(),
                                  &n_merges, first.data()));
  uint64_t cnt[10];
  CHECK(ctx, rtc_linkage_counters(ctx, cnt));
  // components arrive in order of their smallest member; so do the clusters generate_cluster_with_bfs numbers, but do not rely on it
  vector<size_t> order(clusters.size());
  for (size_t c = 0; c < order.size(); c++) order[c] = c;
  vector<int> smallest(clusters.size());
  for (size_t c = 0; c < clusters.size(); c++) smallest[c] = *std::min_element(clusters[c].begin(), clusters[c].end());
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return smallest[x] < smallest[y]; });
  const string f_lk = base + ".complete.linkage.txt";
  FILE* fp = fopen(f_lk.c_str(), "w");
  if (!fp) { cerr << "ERROR: cannot open file: " << f_lk << endl; join_warmup(); exit(1); }
  vector<vector<int>> out;
  vector<int> cid(n), head(n);  // the linkage id of the cluster named g; the result cluster (index into out) named g
  for (uint32_t g = 0; g < n; g++) cid[g] = (int)g;
  int next_id = (int)n;
  uint64_t kept = 0;
  for (size_t q = 0; q < order.size(); q++) {
    const vector<int>& mem = clusters[order[q]];
    vector<int> sorted_mem(mem);
    std::sort(sorted_mem.begin(), sorted_mem.end());
    const size_t out0 = out.size();
    for (int g : sorted_mem) { head[g] = (int)out.size(); out.push_back({g}); }
    for (uint64_t e = first[q]; e < first[q + 1]; e++) {
      const rtc_lmerge& mg = merges[e];
      const double dist = rtc_linkage_distance(mg.common, mg.denom, kmer_size);
      if (dist > threshold) break;
      fprintf(fp, "%d\t%d\t%.6f\t%d\n", cid[mg.a], cid[mg.b], dist, (int)mg.size);
      cid[mg.a] = next_id++;
      vector<int>& A = out[head[mg.a]];
      vector<int>& Bv = out[head[mg.b]];
      A.insert(A.end(), Bv.begin(), Bv.end());
      Bv.clear();
      kept++;
    }
    // the component's clusters: members ascending, clusters by smallest member
    vector<vector<int>> part;
    for (size_t i = out0; i < out.size(); i++) if (!out[i].empty()) { std::sort(out[i].begin(), out[i].end()); part.push_back(std::move(out[i])); }
    std::sort(part.begin(), part.end(), [](const vector<int>& x, const vector<int>& y) { return x[0] < y[0]; });
    out.resize(out0);
    for (auto& c : part) out.push_back(std::move(c));
  }
  fclose(fp);
  std::sort(out.begin(), out.end(), [](const vector<int>& x, const vector<int>& y) { return x[0] < y[0]; });
  const string f_cl = base + ".complete";
  print_result(out, genomes, sketchByFile, f_cl, threshold);
  cerr << "-----write the complete-linkage cluster result into: " << f_cl << endl;
  cerr << "-----the cluster number of: " << f_cl << " is: " << out.size() << endl;
  cerr << "-----write the complete-linkage matrix into: " << f_lk << endl;
  g_metrics.num("linkage_fill_s", 1e-9 * (double)cnt[6]);
  g_metrics.num("linkage_agglomerate_s", 1e-9 * (double)cnt[7]);
  g_metrics.num("linkage_components", (double)cnt[0]);
  g_metrics.num("linkage_merges", (double)kept);
  g_metrics.num("linkage_clusters", (double)out.size());
}

// --nj-tree / --nj-all: neighbour joining (include/rtclust.h has the definition) over the distances the host forms from the exact
// keys of the index path.  --nj-tree: every cluster of the plain run is a component, <base>.nj.newick holds one tree a line in
// the order <base> lists the clusters; --nj-all: all genomes are one component, <base>.nj.all.newick.  A tree that does not fit
// the device (RTC_ERR_NOMEM, no fallback) is reported after everything else has been written: returns 1.
static int nj_trees_and_print(rtc_ctx* ctx, const DeviceSketches& ds, const vector<vector<int>>& clusters, const vector<GenomeInfo>& genomes,
                              bool sketchByFile, const string& base, int kmer_size, int threads, bool per_cluster, bool all, uint32_t replicates,
                              uint64_t seed) {
  const uint32_t n = (uint32_t)genomes.size();
  CHECK(ctx, rtc_ctx_set_host_threads(ctx, threads > 0 ? threads : 1));
  uint64_t sum[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, ssum[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int pass = 0; pass < 2; pass++) {
    if (!(pass == 0 ? per_cluster : all)) continue;
    vector<uint32_t> comp(n, 0);
    vector<vector<int>> whole(1);
    if (pass == 0) { for (size_t c = 0; c < clusters.size(); c++) for (int g : clusters[c]) comp[g] = (uint32_t)c; }
    else for (uint32_t g = 0; g < n; g++) whole[0].push_back((int)g);
    vector<rtc_njoin> joins(n > 0 ? n : 1);
    vector<uint64_t> first((size_t)n + 1, 0);
    uint64_t n_joins = 0;
    vector<uint32_t> support(replicates ? joins.size() : 0);
    const int st = replicates ? rtc_nj_support(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, n, comp.data(), kmer_size, replicates, seed, joins.data(),
                                               joins.size(), &n_joins, first.data(), support.data())
                              : rtc_nj_clusters(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, n, comp.data(), kmer_size, joins.data(), joins.size(),
                                                &n_joins, first.data());
    if (st == RTC_ERR_NOMEM) { cerr << "ERROR: " << rtc_last_error(ctx) << endl; return 1; }
    CHECK(ctx, st);
    uint64_t cnt[10];
    CHECK(ctx, rtc_nj_counters(ctx, cnt));
    for (int i = 0; i < 10; i++) sum[i] += cnt[i];
    const string f = base + (pass == 0 ? ".nj.newick" : ".nj.all.newick");
    print_nj_newick(genomes, pass == 0 ? clusters : whole, joins, first, sketchByFile, f);
    cerr << "-----write the neighbour-joining " << (pass == 0 ? "trees of the clusters" : "tree of all genomes") << " into: " << f << endl;
    if (replicates) {
      // the same trees with the support of every inner branch, and the counts as a table
      uint64_t scnt[10];
      CHECK(ctx, rtc_nj_support_counters(ctx, scnt));
      for (int i = 0; i < 10; i++) ssum[i] += scnt[i];
      const string stem = base + (pass == 0 ? ".nj" : ".nj.all");
      print_nj_support(genomes, pass == 0 ? clusters : whole, joins, first, support, replicates, sketchByFile, stem + ".support.newick", stem + ".support.tsv");
      cerr << "-----write the jackknife support of the neighbour-joining " << (pass == 0 ? "trees of the clusters" : "tree of all genomes")
           << " into: " << stem << ".support.newick and " << stem << ".support.tsv" << endl;
    }
  }
  if (replicates) {
    const double mean = ssum[8] ? (double)ssum[9] / (double)ssum[8] : 0.0;
    cerr << "-----jackknife support: " << sum[0] << " trees, " << ssum[8] << " splits, " << replicates << " replicates, mean count " << mean << endl;
    g_metrics.num("nj_support_count_s", 1e-9 * (double)ssum[2]);
    g_metrics.num("nj_support_distance_s", 1e-9 * (double)ssum[3]);
    g_metrics.num("nj_support_join_s", 1e-9 * (double)ssum[4]);
    g_metrics.num("nj_support_split_s", 1e-9 * (double)ssum[5]);
    g_metrics.num("nj_support_replicates", (double)replicates);
    g_metrics.num("nj_support_mean", mean);
  }
  g_metrics.num("nj_fill_s", 1e-9 * (double)sum[6]);
  g_metrics.num("nj_distance_s", 1e-9 * (double)sum[7]);
  g_metrics.num("nj_join_s", 1e-9 * (double)sum[8]);
  g_metrics.num("nj_components", (double)sum[0]);
  g_metrics.num("nj_records", (double)sum[4]);
  return 0;
}
// --upgma: average linkage inside every cluster of the plain run (include/rtclust.h has the definition).  The device hands back
// every cluster's whole dendrogram on exact integer sums; upgma_report cuts it at the threshold by the integer rule.
// <base>.upgma: the refined clusters in print_result's layout, by smallest member; <base>.upgma.linkage.txt: all merges;
// <base>.upgma.newick: one ultrametric tree a line in the order <base> lists the clusters.  A cluster that does not fit the
// device (RTC_ERR_NOMEM, no fallback) is reported after everything else has been written: returns 1.
static int upgma_and_print(rtc_ctx* ctx, const DeviceSketches& ds, const vector<vector<int>>& clusters, const vector<GenomeInfo>& genomes,
                           bool sketchByFile, const string& base, double threshold, int kmer_size, int threads) {
  const uint32_t n = (uint32_t)genomes.size();
  CHECK(ctx, rtc_ctx_set_host_threads(ctx, threads > 0 ? threads : 1));
  vector<uint32_t> comp(n, 0);
  for (size_t c = 0; c < clusters.size(); c++) for (int g : clusters[c]) comp[g] = (uint32_t)c;
  vector<rtc_umerge> merges(n > 0 ? n : 1);
  vector<uint64_t> first((size_t)n + 1, 0);
  uint64_t n_merges = 0;
  const int st = rtc_upgma_clusters(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, n, comp.data(), kmer_size, merges.data(), merges.size(), &n_merges,
                                    first.data());
  if (st == RTC_ERR_NOMEM) { cerr << "ERROR: " << rtc_last_error(ctx) << endl; return 1; }
  CHECK(ctx, st);
  uint64_t cnt[10];
  CHECK(ctx, rtc_upgma_counters(ctx, cnt));
  string linkage_txt;
  vector<vector<int>> out;
  upgma_report(n, clusters, merges.data(), first.data(), threshold, &linkage_txt, &out);
  const string f_cl = base + ".upgma", f_lk = base + ".upgma.linkage.txt", f_nw = base + ".upgma.newick";
  FILE* fp = fopen(f_lk.c_str(), "w");
  if (!fp) { cerr << "ERROR: cannot open file: " << f_lk << endl; join_warmup(); exit(1); }
  fwrite(linkage_txt.data(), 1, linkage_txt.size(), fp);
  fclose(fp);
  print_result(out, genomes, sketchByFile, f_cl, threshold);
  print_upgma_newick(genomes, clusters, merges, first, sketchByFile, f_nw);
  cerr << "-----write the average-linkage cluster result into: " << f_cl << endl;
  cerr << "-----the cluster number of: " << f_cl << " is: " << out.size() << endl;
  cerr << "-----write the average-linkage matrix into: " << f_lk << endl;
  cerr << "-----write the average-linkage trees of the clusters into: " << f_nw << endl;
  g_metrics.num("upgma_fill_s", 1e-9 * (double)cnt[6]);
  g_metrics.num("upgma_distance_s", 1e-9 * (double)cnt[7]);
  g_metrics.num("upgma_agglomerate_s", 1e-9 * (double)cnt[8]);
  g_metrics.num("upgma_components", (double)cnt[0]);
  g_metrics.num("upgma_merges", (double)cnt[4]);
  g_metrics.num("upgma_clusters", (double)out.size());
  return 0;
}
// --quality: the silhouette of every genome under the run's clusters and, per cluster, its diameter and its separation from the
// nearest other cluster (include/rtclust.h has the definition), over the distances the host forms from the exact keys of the
// index path; pairs that share no hash are at distance 1.  <base>.quality.tsv: a line a cluster in the order and with the numbers
// <base> prints; <base>.silhouette.tsv: a line a genome in input order (quality_report_text, rtc_host.h).  A candidate list that does not fit the device (RTC_ERR_NOMEM, no fallback) is reported: returns 1.
static int quality_and_print(rtc_ctx* ctx, const DeviceSketches& ds, const vector<vector<int>>& clusters, const vector<GenomeInfo>& genomes,
                             bool sketchByFile, const string& base, int kmer_size, int threads) {
  const uint32_t n = (uint32_t)genomes.size();
  CHECK(ctx, rtc_ctx_set_host_threads(ctx, threads > 0 ? threads : 1));
  vector<int32_t> label(n, -1);
  for (size_t c = 0; c < clusters.size(); c++) for (int g : clusters[c]) label[g] = (int32_t)c;
  vector<rtc_sil> rec(n > 0 ? n : 1);
  const int st = rtc_cluster_quality(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, n, label.data(), kmer_size, rec.data());
  if (st == RTC_ERR_NOMEM) { cerr << "ERROR: " << rtc_last_error(ctx) << endl; return 1; }
  CHECK(ctx, st);
  uint64_t cnt[10];
  CHECK(ctx, rtc_cluster_quality_counters(ctx, cnt));
  vector<double> sil(n);
  for (uint32_t g = 0; g < n; g++) sil[g] = rtc_silhouette_value(&rec[g]);
  string q_text, s_text;
  const double all_mean = quality_report_text([&](uint32_t g) { return sketchByFile ? genomes[g].fileName : genomes[g].seq0.name; }, clusters,
                                              rec.data(), sil.data(), n, &q_text, &s_text);
  const string f_q = base + ".quality.tsv", f_s = base + ".silhouette.tsv";
  for (int which = 0; which < 2; which++) {
    const string& f = which ? f_s : f_q;
    const string& text = which ? s_text : q_text;
    FILE* fp = fopen(f.c_str(), "w");
    if (!fp) { cerr << "ERROR: cannot open file: " << f << endl; join_warmup(); exit(1); }
    fwrite(text.data(), 1, text.size(), fp);
    fclose(fp);
  }
  cerr << "-----write the cluster quality into: " << f_q << endl;
  cerr << "-----write the silhouettes into: " << f_s << endl;
  cerr << "-----the mean silhouette of: " << base << " is: " << all_mean << endl;
  g_metrics.num("quality_pair_s", 1e-9 * (double)cnt[5]);
  g_metrics.num("quality_distance_s", 1e-9 * (double)cnt[6]);
  g_metrics.num("quality_score_s", 1e-9 * (double)cnt[7]);
  g_metrics.num("quality_candidates", (double)cnt[1]);
  g_metrics.num("quality_silhouette_mean", all_mean);
  return 0;
}
// --cluster-support B: which of the run's clusters survive a delete-half jackknife over the sketch hashes (include/rtclust.h has
// the definition): B replicates, each with its own single-linkage components over the MST's candidates at the run's threshold,
// tallied against the run's clusters.  <base>.support.tsv: a line a cluster in the order and with the numbers <base> prints;
// <base>.support.genomes.tsv: a line a genome in input order (support_report_text, rtc_host.h).  State that does not fit the
// device (RTC_ERR_NOMEM, no fallback) is reported: returns 1.
static int cluster_support_and_print(rtc_ctx* ctx, const DeviceSketches& ds, const vector<vector<int>>& clusters, const vector<GenomeInfo>& genomes,
                                     bool sketchByFile, const string& base, double threshold, int kmer_size, uint32_t replicates, uint64_t seed) {
  const uint32_t n = (uint32_t)genomes.size();
  vector<uint32_t> comp(n, 0);
  for (size_t c = 0; c < clusters.size(); c++) for (int g : clusters[c]) comp[g] = (uint32_t)c;
  vector<rtc_csupport> rec(clusters.size() > 0 ? clusters.size() : 1);
  vector<uint64_t> together(n > 0 ? n : 1, 0);
  const int st = rtc_cluster_support(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, n, comp.data(), kmer_size, threshold, replicates, seed, rec.data(),
                                     together.data());
  if (st == RTC_ERR_NOMEM || st == RTC_ERR_UNSUPPORTED) { cerr << "ERROR: " << rtc_last_error(ctx) << endl; return 1; }
  CHECK(ctx, st);
  uint64_t cnt[10];
  CHECK(ctx, rtc_cluster_support_counters(ctx, cnt));
  string c_text, g_text;
  const double mean = support_report_text([&](uint32_t g) { return sketchByFile ? genomes[g].fileName : genomes[g].seq0.name; }, clusters, rec.data(),
                                          together.data(), n, replicates, &c_text, &g_text);
  const string f_c = base + ".support.tsv", f_g = base + ".support.genomes.tsv";
  for (int which = 0; which < 2; which++) {
    const string& f = which ? f_g : f_c;
    const string& text = which ? g_text : c_text;
    FILE* fp = fopen(f.c_str(), "w");
    if (!fp) { cerr << "ERROR: cannot open file: " << f << endl; join_warmup(); exit(1); }
    fwrite(text.data(), 1, text.size(), fp);
    fclose(fp);
  }
  cerr << "-----write the jackknife support of the clusters into: " << f_c << " and " << f_g << endl;
  cerr << "-----cluster support: " << clusters.size() << " clusters, " << replicates << " replicates, " << cnt[1] << " candidates, " << cnt[4]
       << " hooking passes, mean recovered " << mean << endl;
  g_metrics.num("support_pair_s", 1e-9 * (double)cnt[5]);
  g_metrics.num("support_count_s", 1e-9 * (double)cnt[6]);
  g_metrics.num("support_components_s", 1e-9 * (double)cnt[7]);
  g_metrics.num("support_tally_s", 1e-9 * (double)cnt[8]);
  g_metrics.num("support_replicates", (double)replicates);
  g_metrics.num("support_recovered_mean", mean);
  return 0;
}
// --pangenome: how many members of its cluster hold each hash of every genome (include/rtclust.h has the definition), counted on
// the GPU over the run's clusters.  <base>.pangenome.tsv: a line a cluster in the order and with the numbers <base> prints;
// <base>.pangenome.genomes.tsv: a line a genome in input order; <base>.pangenome.hist.tsv and <base>.pangenome.curve.tsv: the
// clusters' histograms and growth curves (pangenome_report_text, rtc_host.h).  Tables that do not fit the device (RTC_ERR_NOMEM, no
// fallback) are reported: returns 1.
static int pangenome_and_print(rtc_ctx* ctx, const DeviceSketches& ds, const vector<vector<int>>& clusters, const vector<GenomeInfo>& genomes,
                               bool sketchByFile, const string& base, uint32_t soft_pct, uint32_t cloud_pct, int threads) {
  const uint32_t n = (uint32_t)genomes.size();
  vector<int32_t> label(n, -1);
  for (size_t c = 0; c < clusters.size(); c++) for (int g : clusters[c]) label[g] = (int32_t)c;
  vector<rtc_pan> rec(n > 0 ? n : 1);
  vector<uint64_t> hist(n > 0 ? n : 1, 0);
  vector<rtc_pan_genome> gen(n > 0 ? n : 1);
  uint32_t n_cl = 0;
  const int st = rtc_pangenome(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, n, label.data(), soft_pct, cloud_pct, rec.data(), hist.data(), gen.data(),
                               &n_cl);
  if (st == RTC_ERR_NOMEM || st == RTC_ERR_UNSUPPORTED) { cerr << "ERROR: " << rtc_last_error(ctx) << endl; return 1; }
  CHECK(ctx, st);
  uint64_t cnt[10], phase[3];
  CHECK(ctx, rtc_pangenome_counters(ctx, cnt));
  CHECK(ctx, rtc_pangenome_phases(ctx, phase));
  string text[4];
  const double share = pangenome_report_text([&](uint32_t g) { return sketchByFile ? genomes[g].fileName : genomes[g].seq0.name; }, clusters, rec.data(),
                                             hist.data(), gen.data(), n, threads > 0 ? threads : 1, rtc_pan_growth, &text[0], &text[1], &text[2], &text[3]);
  const string files[4] = {base + ".pangenome.tsv", base + ".pangenome.genomes.tsv", base + ".pangenome.hist.tsv", base + ".pangenome.curve.tsv"};
  for (int which = 0; which < 4; which++) {
    FILE* fp = fopen(files[which].c_str(), "w");
    if (!fp) { cerr << "ERROR: cannot open file: " << files[which] << endl; join_warmup(); exit(1); }
    fwrite(text[which].data(), 1, text[which].size(), fp);
    fclose(fp);
  }
  cerr << "-----write the pangenome of the clusters into: " << files[0] << ", " << files[1] << ", " << files[2] << " and " << files[3] << endl;
  cerr << "-----pangenome: " << cnt[0] << " clusters, " << cnt[2] << " hashes of " << cnt[1] << " genomes, " << cnt[3] << " distinct, " << cnt[4] << " / "
       << cnt[5] << " / " << cnt[6] << " clusters on the wave / workgroup / arena path, " << cnt[7] << " group(s), mean core share " << share << endl;
  g_metrics.num("pangenome_count_s", 1e-9 * (double)phase[0]);
  g_metrics.num("pangenome_sweep_s", 1e-9 * (double)phase[1]);
  g_metrics.num("pangenome_genome_s", 1e-9 * (double)phase[2]);
  g_metrics.num("pangenome_clusters", (double)cnt[0]);
  g_metrics.num("pangenome_hashes", (double)cnt[3]);
  g_metrics.num("pangenome_core_share_mean", share);
  return 0;
}
#endif

#if !defined(GREEDY_CLUST) && !defined(DBSCAN_CLUST)
// append_clust_mst / append_clust_mst_fast (src/sub_command.cpp:1532-1759): sketch the new genomes with the
// stored folder's parameters, evaluate only the pairs that involve a new genome (rows >= start_index,
// src/MST.cpp:1375-1383 -- rtc_mst_append), merge that forest with the stored MST (sort + Kruskal,
// :1693-1700), cut, print, and write the combined folder.
static int append_mst_from_state(const Options& o, vector<Gpu>& gpus, MstState& st, const string& state_path, bool db = false);
static int append_clust_mst(const Options& o, vector<Gpu>& gpus) {
  rtc_ctx* ctx = gpus[0].ctx;
  {  // a --save-rep state beside the sketches: the new genomes are measured against its representatives (src/sub_command.cpp:1289-1316, :1533-1560)
    const string state_path = o.folder_path + "/mst_cluster_state.bin";
    struct stat sb;
    if (stat(state_path.c_str(), &sb) == 0) {
      cerr << "===== clust-mst " << (o.is_fast ? "--fast " : "") << "append (inverted-index state) =====" << endl;
      MstState st;
      if (!load_mst_state(state_path, o.is_fast, st)) cerr << "ERROR: failed to load " << state_path << ", falling back to classic append" << endl;
      else return append_mst_from_state(o, gpus, st, state_path);
    }
  }
  vector<GenomeInfo> genomes; MinHashSketchFile mh; KssdSketchFile ks; bool byFile = true;
  double t0 = get_sec();
  if (o.is_fast) { if (!load_kssd_sketches(o.folder_path, genomes, ks, byFile)) return 1; }
  else if (!load_minhash_sketches(o.folder_path, genomes, mh, byFile)) return 1;
  vector<rtc_edge> pre_mst;
  if (!load_mst(o.folder_path, pre_mst)) return 1;
  const size_t n_pre = genomes.size();
  if (byFile != o.sketchByFile) {
    cerr << "Warning: append_clust_mst(), the input format of append genomes and pre-sketched genome is not same (single input genome vs. genome list)" << endl;
    cerr << "the output cluster file may not have the genome file name" << endl;
  }
  if (!o.sketchByFile) unsupported("single-FASTA input (run with -l and a genome list)");
  cerr << "-----use the same sketch parameters with pre-generated sketches" << endl;
  SketchJob job;
  job.kssd = o.is_fast; job.minLen = o.minLen; job.threads = o.threads;
  if (o.is_fast) {
    job.kmerSize = ks.info.half_k * 2; job.drlevel = ks.info.drlevel;
    cerr << "---use the KSSD sketches" << endl << "---the half_k is: " << ks.info.half_k << endl
         << "---the half_subk is: " << ks.info.half_subk << endl << "---the drlevel is: " << ks.info.drlevel << endl;
  } else {
    job.kmerSize = mh.kmerSize; job.sketchSize = mh.sketchSize; job.isContainment = mh.isContainment; job.containCompress = mh.containCompress;
    cerr << "---the kmer size is: " << mh.kmerSize << endl;
    if (mh.isContainment) cerr << "---use the AAF distance (variable-sketch-size), the sketch size is in proportion with 1/" << mh.containCompress << endl;
    else cerr << "---use the Mash distance (fixed-sketch-size), the sketch size is: " << mh.sketchSize << endl;
  }
  cerr << "---the thread number is: " << o.threads << endl << "---the threshold is: " << o.threshold << endl;
  vector<GenomeInfo> add; MinHashSketchFile mh2; KssdSketchFile ks2; Resident rs2;
  sketch_files(gpus, o.inputFile, job, add, &mh2, &ks2, rs2, true);
  for (size_t i = 0; i < add.size(); i++) {
    add[i].id = (int)(n_pre + i);
    genomes.push_back(add[i]);
    if (!o.is_fast) mh.hashes.push_back(std::move(mh2.hashes[i]));
    else if (ks.use64) ks.h64.push_back(std::move(ks2.h64[i]));
    else ks.h32.push_back(std::move(ks2.h32[i]));
  }
  ks.info.genomeNumber = (int)genomes.size();
  cerr << "-----the size of sketches (number of genomes or sequences) is: " << genomes.size() << endl;
  cerr << "========time of computing sketch is: " << get_sec() - t0 << "========" << endl;
  const string new_folder = current_date_time();
  if (!o.noSave) {
    string command = "mkdir -p " + new_folder;
    if (system(command.c_str()) != 0) { cerr << "ERROR: cannot create " << new_folder << endl; return 1; }
    if (o.is_fast) { save_kssd_sketches(genomes, ks, new_folder, true); save_kssd_index(ks, new_folder); }
    else { save_minhash_sketches(genomes, mh, new_folder, true); save_minhash_index(mh, new_folder); }
  }
  double t2 = get_sec();
  DeviceSketches ds;
  if (o.is_fast) upload_sketches(ctx, ks.use64 ? &ks.h64 : nullptr, ks.use64 ? nullptr : &ks.h32, ds);
  else upload_sketches(ctx, &mh.hashes, nullptr, ds);
  const int kmer_size = o.is_fast ? ks.info.half_k * 2 : mh.kmerSize;
  const int is_containment = o.is_fast ? (int)o.isContainment : (int)mh.isContainment;
  vector<rtc_edge> append_mst(genomes.size());
  uint64_t ne = 0;
  cerr << "---the start_index is: " << n_pre << endl;
  if (!o.useIndex && !o.is_fast)  // the fallback of append_clust_mst (src/sub_command.cpp:1680): modifyMST from start_index
    CHECK(ctx, rtc_mst_mash(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, (uint32_t)n_pre, kmer_size, is_containment, (uint32_t)mh.sketchSize,
                            append_mst.data(), &ne, 0, nullptr, nullptr));
  else
    CHECK(ctx, rtc_mst_append(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, (uint32_t)n_pre, kmer_size, is_containment, o.threshold,
                              append_mst.data(), &ne));
  append_mst.resize(ne);
  cerr << "========time of generateMST is: " << get_sec() - t2 << "========" << endl;
  vector<rtc_edge> final_graph(pre_mst);
  final_graph.insert(final_graph.end(), append_mst.begin(), append_mst.end());
  std::sort(final_graph.begin(), final_graph.end(), [](const rtc_edge& a, const rtc_edge& b) { return a.dist < b.dist; });  // cmpEdge
  vector<rtc_edge> final_mst = kruskal_algorithm(final_graph, (int)genomes.size());
  write_trees(o, genomes, final_mst, byFile);
  cluster_from_mst(final_mst, genomes, byFile, o.outputFile, o.threshold);
  if (!o.noSave) { save_genome_info(genomes, new_folder, "mst", true, o.is_fast); save_mst(final_mst, new_folder); }
  return 0;
}

// The state path of append_clust_mst[_fast]: sketch the new genomes with the state's parameters, measure them against the
// representatives and against each other on the GPU (rtc_rep_match), replay the decisions in list order on the host
// (append_mst_state), print the live clusters (printMstStateClusterResult), and write the state back with --save-rep and no -e.
static int append_mst_from_state(const Options& o, vector<Gpu>& gpus, MstState& st, const string& state_path, bool db) {
  rtc_ctx* ctx = gpus[0].ctx;
  if (!o.sketchByFile) unsupported("single-FASTA input (run with -l and a genome list)");
  SketchJob job;
  job.kssd = st.kssd; job.minLen = o.minLen; job.threads = o.threads;
  if (st.kssd) { job.kmerSize = st.half_k * 2; job.drlevel = st.drlevel; }
  else if (db) {  // mst_repdb_append: contain_compress > 0 ? contain_compress : 1000 (src/sub_command.cpp:1238-1242)
    job.kmerSize = st.kmer_size; job.sketchSize = st.sketch_size; job.isContainment = st.is_containment;
    job.containCompress = st.contain_compress > 0 ? st.contain_compress : 1000;
  } else {
    // the reference stores contain_compress = 0 (src/sub_command.cpp:2821, :3065) and sketches the new genomes with it
    if (st.is_containment && st.contain_compress <= 0) {
      cerr << "ERROR: is_containment is true but contain_compress is " << st.contain_compress << endl;
      return 1;
    }
    job.kmerSize = st.kmer_size; job.sketchSize = st.sketch_size; job.isContainment = st.is_containment; job.containCompress = st.contain_compress;
  }
  const double t0 = get_sec();
  vector<GenomeInfo> add; MinHashSketchFile mh2; KssdSketchFile ks2; Resident rs2;
  sketch_files(gpus, o.inputFile, job, add, &mh2, &ks2, rs2, true);
  const bool q64 = st.kssd ? ks2.use64 : true;
  if (!add.empty() && q64 != st.use64) {
    cerr << "ERROR: the new sketches have use64=" << q64 << " but the state has use64=" << st.use64 << endl;
    return 1;
  }
  const vector<vector<uint64_t>>& qh64 = st.kssd ? ks2.h64 : mh2.hashes;
  const vector<vector<uint32_t>>& qh32 = ks2.h32;
  cerr << "========time of computing sketch is: " << get_sec() - t0 << "========" << endl;
  cerr << "\n[clust-mst" << (st.kssd ? " --fast" : "") << " append] using inverted-index state" << endl;
  cerr << "  existing members: " << st.N << ", existing reps: " << st.reps() << ", new sketches: " << add.size() << endl;
  const double t1 = get_sec();
  const uint32_t R = (uint32_t)st.reps(), Q = (uint32_t)add.size();
  vector<rtc_rep_pair> pairs;
  if (Q) {
    DeviceSketches ds;
    if (st.use64) { vector<vector<uint64_t>> all(st.h64); all.insert(all.end(), qh64.begin(), qh64.end()); upload_sketches(ctx, &all, nullptr, ds); }
    else { vector<vector<uint32_t>> all(st.h32); all.insert(all.end(), qh32.begin(), qh32.end()); upload_sketches(ctx, nullptr, &all, ds); }
    const int kmer_size = st.kssd ? st.half_k * 2 : st.kmer_size;
    uint64_t np = 0;
    pairs.resize((size_t)Q * 8);
    CHECK(ctx, rtc_rep_match(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, R, Q, kmer_size, (int)st.kssd, (int)st.is_containment, st.threshold, 0,
                             pairs.data(), pairs.size(), &np));
    if (np > pairs.size()) {
      pairs.resize(np);
      CHECK(ctx, rtc_rep_match(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, R, Q, kmer_size, (int)st.kssd, (int)st.is_containment, st.threshold, 0,
                               pairs.data(), pairs.size(), &np));
    }
    pairs.resize(np);
    (void)rtc_dev_free(ctx, ds.d_hashes); (void)rtc_dev_free(ctx, ds.d_start); (void)rtc_dev_free(ctx, ds.d_len);
  }
  const double t2 = get_sec();
  vector<string> names; vector<uint64_t> lens;
  for (const GenomeInfo& g : add) { names.push_back(g.fileName); lens.push_back(st.sketch_by_file ? g.totalSeqLength : (uint64_t)g.seq0.length); }
  const vector<vector<int>> live = append_mst_state(st, names, lens, st.use64 ? &qh64 : nullptr, st.use64 ? nullptr : &qh32, pairs);
  const double t3 = get_sec();
  cerr << "========time of rep match (GPU) is: " << t2 - t1 << "========" << endl;
  cerr << "========time of append replay (host) is: " << t3 - t2 << "========" << endl;
  g_metrics.num("rep_match_s", t2 - t1);
  g_metrics.num("append_replay_s", t3 - t2);
  print_mst_state_clusters(live, st.member_names, st.member_lens, st.sketch_by_file, o.outputFile, st.threshold);
  cerr << "-----write the cluster result into: " << o.outputFile << endl;
  cerr << "-----the cluster number of: " << o.outputFile << " is: " << live.size() << endl;
  if (db) {  // mst_repdb_append[_fast]: the database is always saved back
    if (!save_mst_state(state_path, st)) { cerr << "ERROR: failed to save updated MST RepDB state to: " << state_path << endl; return 1; }
    cerr << "  Live clusters:       " << live.size() << endl << "  Total genomes:       " << st.N << endl << "  RepDB updated:       " << state_path << endl;
    return 0;
  }
  if (!o.noSave && o.saveRep && !save_mst_state(state_path, st)) return 1;
  return 0;
}

// mst_repdb_query[_fast] / mst_repdb_assign[_fast] (src/sub_command.cpp:942-1050, :1152-1236): the queries (-l LIST, or the
// records of one FASTA file, named query_<i>) sketched with the database's parameters, every query's best representatives
// from rtc_rep_topk on the GPU (assign: the best one, kept within the database's threshold), the TSV.
static int mst_db_search(const Options& o, vector<Gpu>& gpus) {
  rtc_ctx* ctx = gpus[0].ctx;
  MstState st;
  if (!load_mst_state(o.repdb_path, o.is_fast, st)) { cerr << "ERROR: failed to load MST RepDB from: " << o.repdb_path << endl; return 1; }
  SketchJob job;
  job.kssd = st.kssd; job.minLen = o.minLen; job.threads = o.threads;
  if (st.kssd) { job.kmerSize = st.kmer_size > 0 ? st.kmer_size : st.half_k * 2; job.drlevel = st.drlevel; }
  else {
    job.kmerSize = st.kmer_size; job.sketchSize = st.sketch_size; job.isContainment = st.is_containment;
    job.containCompress = st.contain_compress > 0 ? st.contain_compress : 1000;
  }
  const double t0 = get_sec();
  vector<GenomeInfo> q; MinHashSketchFile mh; KssdSketchFile ks; Resident rs;
  if (o.sketchByFile) sketch_files(gpus, o.inputFile, job, q, &mh, &ks, rs, true);
  else {
    vector<FastaRecord> recs; SeqModeSizes sz;
    if (!read_sequences(o.inputFile, o.minLen, recs, sz)) return 1;
    sketch_sequences(gpus, recs, job, q, &mh, &ks);
  }
  const double t1 = get_sec();
  g_metrics.num("sketch_queries_s", t1 - t0);
  const bool q64 = st.kssd ? ks.use64 : true;
  if (!q.empty() && q64 != st.use64) {
    cerr << "ERROR: the query sketches have use64=" << q64 << " but the MST RepDB has use64=" << st.use64 << " (different hash width)" << endl;
    return 1;
  }
  vector<string> names;
  for (size_t i = 0; i < q.size(); i++) names.push_back(o.sketchByFile ? q[i].fileName : string());  // single FASTA: fileName is empty
  const uint32_t R = (uint32_t)st.reps(), Q = (uint32_t)q.size();
  const uint32_t topk = o.db_assign ? 1u : (uint32_t)std::max(o.topk, 0);
  cerr << "===== MST RepDB " << (o.db_assign ? "Assignment" : "Query") << " (" << (st.kssd ? "KSSD" : "MinHash") << ") =====" << endl
       << "  Query genomes:  " << Q << endl;
  if (!o.db_assign) cerr << "  Top-k:          " << o.topk << endl;
  cerr << "  DB reps:        " << R << endl;
  if (o.db_assign) cerr << "  Threshold:      " << st.threshold << endl;
  vector<rtc_rep_hit> hits;
  vector<uint32_t> per(Q, 0);
  if (Q && R) {
    vector<uint8_t> live(R);
    for (uint32_t r = 0; r < R; r++) live[r] = st.clusters[r].empty() ? 0 : 1;
    DeviceSketches ds;
    if (st.use64) {
      vector<vector<uint64_t>> all(st.h64);
      const vector<vector<uint64_t>>& qh = st.kssd ? ks.h64 : mh.hashes;
      all.insert(all.end(), qh.begin(), qh.end());
      upload_sketches(ctx, &all, nullptr, ds);
    } else {
      vector<vector<uint32_t>> all(st.h32);
      all.insert(all.end(), ks.h32.begin(), ks.h32.end());
      upload_sketches(ctx, nullptr, &all, ds);
    }
    uint64_t nh = 0;
    hits.resize((size_t)Q * (topk ? std::min<uint32_t>(topk, 64) : 16));
    CHECK(ctx, rtc_rep_topk(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, R, Q, live.data(), mst_query_wmode(st), topk, 0, hits.data(),
                            hits.size(), &nh, per.data()));
    if (nh > hits.size()) {
      hits.resize(nh);
      CHECK(ctx, rtc_rep_topk(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, R, Q, live.data(), mst_query_wmode(st), topk, 0, hits.data(),
                              hits.size(), &nh, per.data()));
    }
    hits.resize(nh);
    (void)rtc_dev_free(ctx, ds.d_hashes); (void)rtc_dev_free(ctx, ds.d_start); (void)rtc_dev_free(ctx, ds.d_len);
  }
  const double t2 = get_sec();
  g_metrics.num("rep_topk_s", t2 - t1);
  cerr << "========time of rep top-k (GPU) is: " << t2 - t1 << "========" << endl;
  if (o.db_assign) {
    int assigned = 0;
    if (!write_mst_assign_tsv(o.outputFile, st, names, hits, per, &assigned)) return 1;
    cerr << "===== Assignment Results =====" << endl;
    if (Q) cerr << "  Assigned:    " << assigned << " (" << std::fixed << std::setprecision(1) << (100.0 * assigned / Q) << "%)" << endl
                << "  Novel:       " << Q - assigned << " (" << std::fixed << std::setprecision(1) << (100.0 * (Q - assigned) / Q) << "%)" << endl;
    cerr << "  Output:      " << o.outputFile << endl << "==============================" << endl;
  } else {
    if (!write_mst_query_tsv(o.outputFile, st, names, hits, per)) return 1;
    cerr << "===== Query Results =====" << endl << "  Output: " << o.outputFile << endl << "=========================" << endl;
  }
  return 0;
}

// clust-mst --fast --db FILE --screen: the samples (-l LIST, or the records of one FASTA file, named query_<i>) sketched with the
// database's parameters as --query sketches them, rtc_rep_screen on the first GPU with one retry at the reported size, the two
// reports.  The checks of main() have been through the flags: min_containment in [0, 1], the counts at least 1.
static int mst_db_screen(const Options& o, vector<Gpu>& gpus) {
  rtc_ctx* ctx = gpus[0].ctx;
  MstState st;
  if (!load_mst_state(o.repdb_path, true, st)) { cerr << "ERROR: failed to load MST RepDB from: " << o.repdb_path << endl; return 1; }
  SketchJob job;
  job.kssd = true; job.minLen = o.minLen; job.threads = o.threads;
  job.kmerSize = st.kmer_size > 0 ? st.kmer_size : st.half_k * 2; job.drlevel = st.drlevel;
  const double t0 = get_sec();
  vector<GenomeInfo> q; MinHashSketchFile mh; KssdSketchFile ks; Resident rs;
  if (o.sketchByFile) sketch_files(gpus, o.inputFile, job, q, &mh, &ks, rs, true);
  else {
    vector<FastaRecord> recs; SeqModeSizes sz;
    if (!read_sequences(o.inputFile, o.minLen, recs, sz)) return 1;
    sketch_sequences(gpus, recs, job, q, &mh, &ks);
  }
  const double t1 = get_sec();
  g_metrics.num("sketch_queries_s", t1 - t0);
  if (!q.empty() && ks.use64 != st.use64) {
    cerr << "ERROR: the query sketches have use64=" << ks.use64 << " but the MST RepDB has use64=" << st.use64 << " (different hash width)" << endl;
    return 1;
  }
  vector<string> names;
  for (size_t i = 0; i < q.size(); i++) names.push_back(o.sketchByFile ? q[i].fileName : string());  // single FASTA: fileName is empty
  const uint32_t R = (uint32_t)st.reps(), Q = (uint32_t)q.size();
  const double min_cont = atof(o.minContainment.c_str());
  const uint32_t min_cont_q20 = (uint32_t)llround(min_cont * 1048576.0);
  const uint32_t min_shared = (uint32_t)std::min<long long>(atoll(o.minShared.c_str()), 0x7fffffff);
  const uint32_t min_unique = (uint32_t)std::min<long long>(atoll(o.minUnique.c_str()), 0x7fffffff);
  const uint32_t picks = (uint32_t)std::min<long long>(std::max<long long>(atoll(o.screenPicks.c_str()), 0), 0x7fffffff);
  cerr << "===== MST RepDB Screen (KSSD) =====" << endl << "  Samples:          " << Q << endl << "  DB reps:          " << R << endl
       << "  Min containment:  " << min_cont << endl << "  Min shared:       " << min_shared << endl << "  Min unique:       " << min_unique << endl;
  vector<rtc_screen_hit> hits;
  vector<rtc_screen_sum> sums(Q);
  for (uint32_t i = 0; i < Q; i++) sums[i] = rtc_screen_sum{(uint32_t)(st.use64 ? ks.h64[i].size() : ks.h32[i].size()), 0, 0, 0, 0, 0};
  uint64_t cnt[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (Q && R) {
    vector<uint8_t> live(R);
    for (uint32_t r = 0; r < R; r++) live[r] = st.clusters[r].empty() ? 0 : 1;
    DeviceSketches ds;
    if (st.use64) {
      vector<vector<uint64_t>> all(st.h64);
      all.insert(all.end(), ks.h64.begin(), ks.h64.end());
      upload_sketches(ctx, &all, nullptr, ds);
    } else {
      vector<vector<uint32_t>> all(st.h32);
      all.insert(all.end(), ks.h32.begin(), ks.h32.end());
      upload_sketches(ctx, nullptr, &all, ds);
    }
    uint64_t nh = 0;
    hits.resize((size_t)Q * 64);
    CHECK(ctx, rtc_rep_screen(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, R, Q, live.data(), min_shared, min_cont_q20, min_unique, picks, 0,
                              hits.data(), hits.size(), &nh, sums.data()));
    if (nh > hits.size()) {
      hits.resize(nh);
      CHECK(ctx, rtc_rep_screen(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, R, Q, live.data(), min_shared, min_cont_q20, min_unique, picks, 0,
                                hits.data(), hits.size(), &nh, sums.data()));
    }
    hits.resize(nh);
    CHECK(ctx, rtc_rep_screen_counters(ctx, cnt));
    (void)rtc_dev_free(ctx, ds.d_hashes); (void)rtc_dev_free(ctx, ds.d_start); (void)rtc_dev_free(ctx, ds.d_len);
  }
  const double t2 = get_sec();
  g_metrics.num("rep_screen_s", t2 - t1);
  g_metrics.num("screen_hits", (double)hits.size());
  g_metrics.num("screen_picks", (double)cnt[4]);
  g_metrics.num("screen_rounds_max", (double)cnt[5]);
  cerr << "========time of rep screen (GPU) is: " << t2 - t1 << "========" << endl;
  const string f_sum = o.outputFile + ".summary.tsv";
  if (!write_mst_screen_tsv(o.outputFile, st, names, hits, sums, rtc_screen_identity)) return 1;
  if (!write_mst_screen_summary_tsv(f_sum, st, names, hits, sums)) return 1;
  cerr << "===== Screen Results =====" << endl << "  Hits:    " << hits.size() << endl << "  Picks:   " << cnt[4] << endl << "  Output:  " << o.outputFile << endl
       << "  Summary: " << f_sum << endl << "==========================" << endl;
  return 0;
}

// mst_repdb_append[_fast] (src/sub_command.cpp:1051-1100, :1237-1280): the --append machinery against the database, saved in place
static int mst_db_append(const Options& o, vector<Gpu>& gpus) {
  MstState st;
  if (!load_mst_state(o.repdb_path, o.is_fast, st)) { cerr << "ERROR: failed to load MST RepDB from: " << o.repdb_path << endl; return 1; }
  cerr << "===== MST RepDB Append (" << (o.is_fast ? "KSSD" : "MinHash") << ") =====" << endl << "  Existing reps:    " << st.reps() << endl
       << "  Existing genomes: " << st.N << endl;
  return append_mst_from_state(o, gpus, st, o.repdb_path, true);
}

// MinHashInitialMstState / KssdInitialMstState + save (src/sub_command.cpp:2083-2087, :2577-2581, :2814-2823, :3058-3068): every
// cluster of the forest collapsed to its tree medoid (rtc_tree_medoids with dedup_dist = +inf), written to
// <folder>/mst_cluster_state.bin
static int save_initial_mst_state(rtc_ctx* ctx, const Options& o, const string& state_path, const vector<GenomeInfo>& genomes, bool sketchByFile,
                                  const vector<rtc_edge>& forest, const vector<vector<int>>& clusters, const MinHashSketchFile& mh,
                                  const KssdSketchFile& ks, bool from_sketches, int contain_compress = 0) {
  const int n = (int)genomes.size();
  const size_t nh = o.is_fast ? (ks.use64 ? ks.h64.size() : ks.h32.size()) : mh.hashes.size();
  if ((int)nh != n) { cerr << "ERROR: --save-rep needs the sketches on the host (" << nh << " of " << n << ")" << endl; return 1; }
  const double inf = std::numeric_limits<double>::max();
  vector<uint64_t> lens(n);
  for (int i = 0; i < n; i++) lens[i] = sketchByFile ? genomes[i].totalSeqLength : (uint64_t)genomes[i].seq0.length;
  vector<int32_t> rep(n);
  CHECK(ctx, rtc_ctx_set_host_threads(ctx, o.threads));
  CHECK(ctx, rtc_tree_medoids(ctx, (uint32_t)n, forest.data(), forest.size(), inf, lens.data(), rep.data()));
  const vector<vector<int>> cands = dedup_candidates(clusters, vector<int>(rep.begin(), rep.end()), inf);
  vector<int> rep_of_cluster(clusters.size());
  for (size_t c = 0; c < clusters.size(); c++) rep_of_cluster[c] = cands[c].empty() ? (clusters[c].empty() ? -1 : clusters[c][0]) : cands[c][0];
  MstState st;
  st.kssd = o.is_fast;
  st.threshold = o.threshold;
  if (o.is_fast) {
    st.half_k = ks.info.half_k; st.half_subk = ks.info.half_subk; st.drlevel = ks.info.drlevel; st.kmer_size = ks.info.half_k * 2;
    init_mst_state(st, genomes, sketchByFile, clusters, rep_of_cluster, ks.use64 ? &ks.h64 : nullptr, ks.use64 ? nullptr : &ks.h32);
  } else {
    // sketches[0].minHash->getSketchSize(): the fixed size, or in containment mode genome 0's own size when it was sketched
    // here (src/SketchInfo.cpp) and containCompress when it was loaded (src/Sketch_IO.cpp:334)
    st.kmer_size = mh.kmerSize;
    st.is_containment = mh.isContainment;
    st.contain_compress = contain_compress;
    st.sketch_size = !mh.isContainment ? mh.sketchSize
                     : from_sketches ? mh.containCompress
                     : sketchByFile ? std::max(file_length_for_containment(genomes[0].fileName) / mh.containCompress, 100)
                                    : std::max(genomes[0].seq0.length / mh.containCompress, 100);
    init_mst_state(st, genomes, sketchByFile, clusters, rep_of_cluster, &mh.hashes, nullptr);
  }
  if (!save_mst_state(state_path, st)) return 1;
  if (!o.repdb_path.empty()) {  // build_and_save_{kssd,minhash}_mst_db's summary
    cerr << "\n===== MST RepDB Build Summary (" << (o.is_fast ? "KSSD" : "MinHash") << ") =====" << endl << "  Total genomes:    " << n << endl
         << "  Representatives:  " << st.reps() << endl;
    if (n) cerr << "  Compression:      " << std::fixed << std::setprecision(2) << (1.0 - (double)st.reps() / n) * 100.0 << "%" << endl;
    cerr << "  RepDB saved to:   " << state_path << endl;
  }
  return 0;
}
#endif

#ifdef GREEDY_CLUST
// calculate_mash_distance over a known intersection (src/greedy.cpp:103-160)
static double kssd_mash_distance(int cm, int sizeRef, int sizeQry, int kmer_size) {
  const uint64_t uni = (uint64_t)sizeRef + (uint64_t)sizeQry - (uint64_t)cm;
  const double jac = uni == 0 ? 0.0 : (double)cm / (double)uni;
  double dist = 0.0;
  if (jac != 1.0) { dist = -log(2 * jac / (1.0 + jac)) / (double)kmer_size; if (dist > 1.0) dist = 1.0; }
  return dist;
}

// minhash_mash_distance (src/greedy.cpp:2771-2787)
static double minhash_mash_distance(int common, int sizeQry, int sizeRef, int kmer_size, bool is_containment) {
  if (common <= 0) return 1.0;
  double jaccard;
  if (is_containment) {
    const int minSize = std::min(sizeQry, sizeRef);
    if (minSize == 0) return 1.0;
    jaccard = (double)common / minSize;
  } else {
    const int denom = sizeQry + sizeRef - common;
    if (denom == 0) return 0.0;
    jaccard = (double)common / denom;
  }
  if (jaccard >= 1.0) return 0.0;
  if (jaccard <= 0.0) return 1.0;
  const double dist = -log(2.0 * jaccard / (1.0 + jaccard)) / kmer_size;
  return dist > 1.0 ? 1.0 : dist;
}

// one (new genome or query, representative) pair with cm > 0 shared hashes: is it a candidate, and at which distance?
// KSSD: size-ratio and minimum-common filters, then calculate_mash_distance (src/greedy.cpp:1815-1843, :2583-2606).
// MinHash, incremental step: minimum-common filter only (:2040-2076); MinHash query: no filter (:3003-3012).
static bool rep_candidate(const KssdClusterState& st, bool query, int cm, int sizeQry, int sizeRef, double radio, double jaccard_min,
                          double& dist) {
  if (!st.minhash) {
    const double ratio = (double)sizeQry / sizeRef;
    if (ratio > radio || ratio < 1.0 / radio) return false;
    const int min_common_needed = (int)(jaccard_min * (sizeQry + sizeRef) / (1.0 + jaccard_min));
    if (cm < min_common_needed) return false;
    dist = kssd_mash_distance(cm, sizeRef, sizeQry, st.kmer_size);
    return true;
  }
  if (!query) {
    if (sizeRef == 0) return false;
    const int min_common_needed = st.is_containment ? (int)(jaccard_min * std::min(sizeQry, sizeRef))
                                                    : (int)(jaccard_min * (sizeQry + sizeRef) / (1.0 + jaccard_min));
    if (cm < min_common_needed) return false;
    if (!st.is_containment && sizeQry + sizeRef - cm == 0) return false;
  }
  dist = minhash_mash_distance(cm, sizeQry, sizeRef, st.kmer_size, st.is_containment);
  return true;
}

static size_t sketch_count(const KssdSketchFile& f) { return f.use64 ? f.h64.size() : f.h32.size(); }
static size_t sketch_len(const KssdSketchFile& f, size_t i) { return f.use64 ? f.h64[i].size() : f.h32[i].size(); }
static void push_sketch(KssdSketchFile& dst, const KssdSketchFile& src, size_t i) {
  if (dst.use64) dst.h64.push_back(src.h64[i]); else dst.h32.push_back(src.h32[i]);
}

// the representatives' sketches followed by `tail`'s: the set one rectangular intersection launch works on
static void reps_then(const KssdClusterState& st, const KssdSketchFile& tail, KssdSketchFile& work) {
  work = st.reps;
  if (sketch_count(work) == 0) work.use64 = tail.use64;
  for (size_t i = 0; i < sketch_count(tail); i++) push_sketch(work, tail, i);
}

// KssdIncrementalCluster (src/greedy.cpp:1736-1900): every new genome, in order, joins the representative at the
// smallest Mash distance <= threshold among those that share a hash with it and pass the size-ratio and
// minimum-common filters, or becomes a representative itself.  The GPU supplies |A ∩ B| of each new genome against
// the stored representatives and the new genomes before it; the rule runs on the host.  Ties in distance go to the
// earliest representative (the reference's choice depends on hash-map iteration and thread order).  As in the
// reference (:1861-1864) a genome that opens a cluster is recorded as its representative but is not listed among
// the cluster's members -- the cluster starts empty.
static int kssd_incremental_cluster(rtc_ctx* ctx, KssdClusterState& st, const vector<GenomeInfo>& add, const KssdSketchFile& ks2,
                                    bool keep_sketches) {
  const size_t R0 = st.rep_ids.size(), m = add.size(), n_old = st.genomes.size(), n_work = R0 + m;
  const double threshold = st.threshold;
  cerr << "Existing clusters: " << R0 << endl << "New genomes: " << m << endl;
  if (st.minhash && m == 0) { cerr << "ERROR: No new sketches to process" << endl; return 0; }       // src/greedy.cpp:1973-1981
  if (st.minhash && R0 == 0) { cerr << "ERROR: No existing representatives" << endl; return 0; }
  if (m == 0) return 0;
  if (R0 && ks2.use64 != st.reps.use64) { cerr << "ERROR: appended sketches and stored sketches differ in hash width" << endl; return 1; }
  KssdSketchFile work;
  reps_then(st, ks2, work);
  st.reps.use64 = work.use64; if (keep_sketches && n_old == 0) st.sk.use64 = work.use64;
  DeviceSketches ds;
  upload_sketches(ctx, work.use64 ? &work.h64 : nullptr, work.use64 ? nullptr : &work.h32, ds);
  const double radio = 2.0 * exp(threshold * st.kmer_size) - 1.0;                 // calculateMaxSizeRatio, src/greedy.cpp:162-173
  const double x = exp(-threshold * st.kmer_size), jaccard_min = x / (2.0 - x);   // :1751-1753
  const size_t max_block_bytes = (size_t)256 << 20;
  const size_t B = std::max<size_t>(1, std::min<size_t>(m, max_block_bytes / (n_work * 4)));
  uint32_t* d_common = nullptr;
  CHECK(ctx, rtc_dev_alloc(ctx, B * n_work * 4 + 64, (void**)&d_common));
  vector<uint32_t> common(B * n_work);
  vector<int> rep_of_col(n_work, -1);  // column of `work` -> representative index (new genomes: once they open a cluster)
  for (size_t r = 0; r < R0; r++) rep_of_col[r] = (int)r;
  int new_clusters = 0, assigned = 0;
  for (size_t r0 = R0; r0 < n_work; r0 += B) {
    const size_t r1 = std::min(n_work, r0 + B);
    CHECK(ctx, rtc_pair_common_dev(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, (uint32_t)n_work, (uint32_t)r0, (uint32_t)r1, 0,
                                   (uint32_t)n_work, d_common, (uint64_t)n_work, 1, 0));
    CHECK(ctx, rtc_copy_d2h(ctx, common.data(), d_common, (r1 - r0) * n_work * 4));
    for (size_t q = r0; q < r1; q++) {
      const uint32_t* row = common.data() + (q - r0) * n_work;
      const int genome_idx = (int)(n_old + (q - R0));
      const int sizeQry = (int)sketch_len(work, q);
      double best_dist = std::numeric_limits<double>::max();
      int best = -1;
      for (size_t c = 0; c < q; c++) {
        if (rep_of_col[c] < 0 || row[c] == 0) continue;  // candidates: representatives sharing a hash (:1768-1790)
        double dist;
        if (!rep_candidate(st, false, (int)row[c], sizeQry, (int)sketch_len(work, c), radio, jaccard_min, dist)) continue;
        if (dist <= threshold && dist < best_dist) { best_dist = dist; best = rep_of_col[c]; }
      }
      if (best >= 0) { st.clusters[best].push_back(genome_idx); assigned++; }
      else {
        rep_of_col[q] = (int)st.rep_ids.size();
        st.rep_ids.push_back(genome_idx);
        st.rep_genomes.push_back(add[q - R0]);
        push_sketch(st.reps, work, q);
        st.clusters.push_back(vector<int>());
        new_clusters++;
      }
    }
  }
  for (size_t i = 0; i < m; i++) {
    st.genomes.push_back(add[i]);
    if (keep_sketches) push_sketch(st.sk, ks2, i);
  }
  st.info.genomeNumber = (int)st.genomes.size();
  CHECK(ctx, rtc_dev_free(ctx, d_common));
  CHECK(ctx, rtc_dev_free(ctx, ds.d_hashes)); CHECK(ctx, rtc_dev_free(ctx, ds.d_start)); CHECK(ctx, rtc_dev_free(ctx, ds.d_len));
  cerr << "===== Incremental Clustering Results =====" << endl << "Assigned to existing clusters: " << assigned << endl
       << "New clusters created: " << new_clusters << endl << "Total clusters now: " << st.clusters.size() << endl;
  return 0;
}

// the representative part of a state, from clusters whose first member is the representative (src/greedy.cpp:924-934)
static void fill_cluster_state(KssdClusterState& st, double threshold, int kmer_size, const KssdParameters& info,
                               const vector<GenomeInfo>& genomes, const KssdSketchFile& sk, const vector<vector<int>>& cluster) {
  st.threshold = threshold; st.kmer_size = kmer_size; st.info = info; st.genomes = genomes; st.sk = sk; st.clusters = cluster;
  st.rep_ids.clear(); st.rep_genomes.clear();
  st.reps = KssdSketchFile(); st.reps.info = info; st.reps.use64 = sk.use64;
  for (const auto& c : cluster) if (!c.empty()) {
    st.rep_ids.push_back(c[0]);
    st.rep_genomes.push_back(genomes[c[0]]);
    push_sketch(st.reps, sk, c[0]);
  }
}

// KssdInitialClusterWithState (src/greedy.cpp:900-958): the stored sketches sorted by hash count, descending
// (comparator without tie-break, :594-597), clustered as clust-greedy --fast does, kept as a state
static int kssd_initial_state(rtc_ctx* ctx, vector<GenomeInfo>& pre, KssdSketchFile& ks, double threshold, KssdClusterState& st) {
  const size_t n_pre = pre.size();
  struct Item { size_t idx; size_t c; };
  vector<Item> items(n_pre);
  for (size_t i = 0; i < n_pre; i++) items[i] = Item{i, sketch_len(ks, i)};
  std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.c > b.c; });
  vector<GenomeInfo> genomes; KssdSketchFile all; all.info = ks.info; all.use64 = ks.use64;
  for (const Item& it : items) {
    genomes.push_back(pre[it.idx]);
    if (ks.use64) all.h64.push_back(std::move(ks.h64[it.idx])); else all.h32.push_back(std::move(ks.h32[it.idx]));
  }
  const int kmer_size = ks.info.half_k * 2;
  vector<vector<int>> cluster;
  if (n_pre) {
    DeviceSketches ds;
    upload_sketches(ctx, all.use64 ? &all.h64 : nullptr, all.use64 ? nullptr : &all.h32, ds);
    vector<int32_t> rep_of(n_pre, -1);
    uint32_t ncl = 0;
    CHECK(ctx, rtc_greedy(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, (uint32_t)n_pre, nullptr, kmer_size, 0, 1, threshold,
                          rep_of.data(), &ncl));
    CHECK(ctx, rtc_dev_free(ctx, ds.d_hashes)); CHECK(ctx, rtc_dev_free(ctx, ds.d_start)); CHECK(ctx, rtc_dev_free(ctx, ds.d_len));
    cluster = clusters_from_rep_of(rep_of);
  }
  fill_cluster_state(st, threshold, kmer_size, ks.info, genomes, all, cluster);
  return 0;
}

// compute_kssd_sketches with a state's parameters: the genomes of `list` on the GPU sketcher
static void sketch_for_state(vector<Gpu>& gpus, const Options& o, const string& list, int kmer_size, int drlevel,
                             vector<GenomeInfo>& add, KssdSketchFile& ks2) {
  SketchJob job;
  job.kssd = true; job.kmerSize = kmer_size; job.drlevel = drlevel; job.minLen = o.minLen; job.threads = o.threads;
  MinHashSketchFile mh2; Resident rs2;
  sketch_files(gpus, list, job, add, &mh2, &ks2, rs2, true);
}

// compute_sketches with a MinHash RepDB's parameters (contain_compress is the literal 1000 of mh_repdb_query / _assign /
// _append, src/sub_command.cpp:609,657,717); the sketches come back in the u64 arm of a KssdSketchFile
static void sketch_for_mh_state(vector<Gpu>& gpus, const Options& o, const string& list, const KssdClusterState& st,
                                vector<GenomeInfo>& add, KssdSketchFile& out) {
  SketchJob job;
  job.kssd = false; job.kmerSize = st.kmer_size; job.sketchSize = st.sketch_size; job.isContainment = st.is_containment;
  job.containCompress = 1000; job.minLen = o.minLen; job.threads = o.threads;
  MinHashSketchFile mh2; KssdSketchFile unused; Resident rs2;
  sketch_files(gpus, list, job, add, &mh2, &unused, rs2, true);
  out = KssdSketchFile(); out.use64 = true; out.h64 = std::move(mh2.hashes);
}

static int save_sketch_folder(const vector<GenomeInfo>& g, const KssdSketchFile& ks, string& folder) {
  folder = current_date_time();
  string command = "mkdir -p " + folder;
  if (system(command.c_str()) != 0) { cerr << "ERROR: cannot create " << folder << endl; return 1; }
  save_kssd_sketches(g, ks, folder, true);
  return 0;
}

// append_clust_greedy_fast (src/sub_command.cpp:192-270).  With DIR/cluster_state.bin ("Incremental Update Mode"):
// the stored state's sketches, clusters, threshold and k; the new genomes are clustered against its
// representatives.  Without it ("Initial State Building Mode"): the stored KSSD sketches are clustered as
// clust-greedy --fast would (KssdInitialClusterWithState), then the new genomes as above.  --save-rep (and no -e)
// writes the state back.
static int append_clust_greedy_fast(const Options& o, vector<Gpu>& gpus) {
  rtc_ctx* ctx = gpus[0].ctx;
  const string state_file = o.folder_path + "/cluster_state.bin";
  double t0 = get_sec();
  if (!o.sketchByFile) unsupported("single-FASTA input (run with -l and a genome list)");
  KssdClusterState st;
  struct stat sb;
  bool has_state = stat(state_file.c_str(), &sb) == 0;
  bool byFile = true;
  if (has_state) {
    cerr << "===== Incremental Update Mode (KSSD) =====" << endl << "Found existing cluster state, loading..." << endl;
    has_state = load_kssd_cluster_state(state_file, st);
  }
  if (has_state) {
    cerr << "---the threshold is: " << o.threshold << endl << "---the thread number is: " << o.threads << endl;
  } else {
    vector<GenomeInfo> pre; KssdSketchFile ks;
    if (!load_kssd_sketches(o.folder_path, pre, ks, byFile)) return 1;
    if (byFile != o.sketchByFile) cerr << "Warning: the input format of append genomes and pre-sketched genome is not same" << endl;
    cerr << "===== Initial State Building Mode (KSSD) =====" << endl;
    cerr << "No existing state found, building state from pre-sketched genomes..." << endl;
    cerr << "-----use the same sketch parameters with pre-generated sketches" << endl << "---use the KSSD sketches" << endl
         << "---the half_k is: " << ks.info.half_k << endl << "---the half_subk is: " << ks.info.half_subk << endl
         << "---the drlevel is: " << ks.info.drlevel << endl << "---the threshold is: " << o.threshold << endl;
    if (kssd_initial_state(ctx, pre, ks, o.threshold, st) != 0) return 1;
  }
  // ---- the new genomes, with the stored parameters (KssdIncrementalCluster works with the state's threshold and k) ----
  vector<GenomeInfo> add; KssdSketchFile ks2;
  sketch_for_state(gpus, o, o.inputFile, st.kmer_size, st.info.drlevel, add, ks2);
  cerr << "New genomes sketched: " << add.size() << endl;
  cerr << "========time of computing sketch is: " << get_sec() - t0 << "========" << endl;
  if (!o.noSave) {  // compute_kssd_sketches(isSave): the appended sketches get a folder of their own
    string folder;
    if (save_sketch_folder(add, ks2, folder) != 0) return 1;
  }
  double t2 = get_sec();
  if (kssd_incremental_cluster(ctx, st, add, ks2, true) != 0) return 1;
  if (!o.noSave && o.saveRep) {
    if (!save_kssd_cluster_state(state_file, st)) return 1;
    cerr << "-----saved cluster state (with inverted index) for future incremental updates" << endl;
  }
  print_result(st.clusters, st.genomes, byFile, o.outputFile);
  cerr << "-----write the cluster result into: " << o.outputFile << endl;
  cerr << "-----the cluster number of " << o.outputFile << " is: " << st.clusters.size() << endl;
  cerr << "========time of greedyCluster is: " << get_sec() - t2 << "========" << endl;
  return 0;
}

// ---- RepDB of clust-greedy --fast --db (src/sub_command.cpp:276-475, src/main.cpp:300-334) ----
static void repdb_build_summary(size_t total, size_t reps, const string& db) {
  cerr << "\n===== RepDB Build Summary =====" << endl << "  Total genomes:    " << total << endl << "  Representatives:  " << reps << endl
       << "  Compression:      " << std::fixed << std::setprecision(2) << (1.0 - (double)reps / total) * 100.0 << "%" << endl
       << "  RepDB saved to:   " << db << endl << "===============================" << endl;
}

// repdb_build_from_sketch / repdb_build_from_genome (src/sub_command.cpp:278-334)
static int repdb_build(const Options& o, vector<Gpu>& gpus) {
  rtc_ctx* ctx = gpus[0].ctx;
  vector<GenomeInfo> pre; KssdSketchFile ks; bool byFile = true;
  if (o.has_presketched) {
    if (!load_kssd_sketches(o.folder_path, pre, ks, byFile)) return 1;
    cerr << "===== RepDB Build (from pre-sketched) =====" << endl;
  } else {
    if (!o.sketchByFile) unsupported("single-FASTA input (run with -l and a genome list)");
    int kmerSize = o.kmerSize;
    if (!o.isSetKmer) { kmerSize = 19; cerr << "-----use default kmerSize: " << kmerSize << endl; }
    sketch_for_state(gpus, o, o.inputFile, kmerSize, o.drlevel, pre, ks);
    string folder;
    if (save_sketch_folder(pre, ks, folder) != 0) return 1;   // compute_kssd_sketches(isSave = true)
    cerr << "===== RepDB Build (from genomes) =====" << endl;
  }
  cerr << "  Genomes:    " << pre.size() << endl << "  Threshold:  " << o.threshold << endl << "  Kmer size:  " << ks.info.half_k * 2 << endl;
  if (pre.empty()) { cerr << "ERROR: no genome to cluster" << endl; return 1; }
  KssdClusterState st;
  if (kssd_initial_state(ctx, pre, ks, o.threshold, st) != 0) return 1;
  if (!save_kssd_repdb(o.repdb_path, st)) return 1;
  if (!o.outputFile.empty()) {
    print_result(st.clusters, st.genomes, byFile, o.outputFile, o.threshold);
    cerr << "-----write the cluster result into: " << o.outputFile << endl;
  }
  repdb_build_summary(st.genomes.size(), st.rep_ids.size(), o.repdb_path);
  return 0;
}

struct RepHit { int rep_idx; double distance; };

// KssdClusterState::query_topk for every query (src/greedy.cpp:2539-2637): the representatives that share a hash
// with the query and pass the size-ratio and minimum-common filters, ordered by Mash distance (ties: earlier
// representative first -- the reference's std::sort leaves them in hash-map order), the first `topk` kept.  One
// rectangular intersection launch (rows = queries, columns = representatives) stands in for the index walk.
static int repdb_query_topk(rtc_ctx* ctx, const KssdClusterState& st, const KssdSketchFile& qs, int topk, vector<vector<RepHit>>& out) {
  const size_t R = st.rep_ids.size(), Q = sketch_count(qs);
  out.assign(Q, vector<RepHit>());
  if (R == 0 || Q == 0) return 0;
  if (qs.use64 != st.reps.use64) { cerr << "ERROR: query sketches and the RepDB differ in hash width" << endl; return 1; }
  KssdSketchFile work;
  reps_then(st, qs, work);
  DeviceSketches ds;
  upload_sketches(ctx, work.use64 ? &work.h64 : nullptr, work.use64 ? nullptr : &work.h32, ds);
  const double radio = 2.0 * exp(st.threshold * st.kmer_size) - 1.0;
  const double x = exp(-st.threshold * st.kmer_size), jaccard_min = x / (2.0 - x);
  const size_t B = std::max<size_t>(1, std::min<size_t>(Q, ((size_t)256 << 20) / (R * 4)));
  uint32_t* d_common = nullptr;
  CHECK(ctx, rtc_dev_alloc(ctx, B * R * 4 + 64, (void**)&d_common));
  vector<uint32_t> common(B * R);
  for (size_t q0 = 0; q0 < Q; q0 += B) {
    const size_t q1 = std::min(Q, q0 + B);
    CHECK(ctx, rtc_pair_common_dev(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, (uint32_t)(R + Q), (uint32_t)(R + q0), (uint32_t)(R + q1), 0,
                                   (uint32_t)R, d_common, (uint64_t)R, 0, 0));
    CHECK(ctx, rtc_copy_d2h(ctx, common.data(), d_common, (q1 - q0) * R * 4));
    for (size_t q = q0; q < q1; q++) {
      const uint32_t* row = common.data() + (q - q0) * R;
      const int sizeQry = (int)sketch_len(qs, q);
      vector<RepHit> scored;
      for (size_t r = 0; r < R; r++) {
        if (row[r] == 0) continue;
        double dist;
        if (!rep_candidate(st, true, (int)row[r], sizeQry, (int)sketch_len(st.reps, r), radio, jaccard_min, dist)) continue;
        scored.push_back(RepHit{(int)r, dist});
      }
      std::stable_sort(scored.begin(), scored.end(), [](const RepHit& a, const RepHit& b) { return a.distance < b.distance; });
      if ((int)scored.size() > topk) scored.resize(std::max(topk, 0));
      out[q] = std::move(scored);
    }
  }
  CHECK(ctx, rtc_dev_free(ctx, d_common));
  CHECK(ctx, rtc_dev_free(ctx, ds.d_hashes)); CHECK(ctx, rtc_dev_free(ctx, ds.d_start)); CHECK(ctx, rtc_dev_free(ctx, ds.d_len));
  return 0;
}

static int repdb_load_and_sketch(const Options& o, vector<Gpu>& gpus, KssdClusterState& st, vector<GenomeInfo>& q, KssdSketchFile& qs) {
  if (o.is_fast) { if (!load_kssd_repdb(o.repdb_path, st)) { cerr << "ERROR: Failed to load RepDB from: " << o.repdb_path << endl; return 1; } }
  else if (!load_minhash_repdb(o.repdb_path, st)) { cerr << "ERROR: Failed to load MinHash RepDB from: " << o.repdb_path << endl; return 1; }
  if (!o.sketchByFile) unsupported("single-FASTA input (run with -l and a genome list)");
  if (o.is_fast) sketch_for_state(gpus, o, o.inputFile, st.kmer_size, st.info.drlevel, q, qs);
  else sketch_for_mh_state(gpus, o, o.inputFile, st, q, qs);
  return 0;
}

// mh_repdb_build_from_sketch / mh_repdb_build_from_genome (src/sub_command.cpp:502-586): the sketches in stored /
// list order (no size sort here), MinHashInitialClusterWithState = the MinHash greedy pass, saved as MHREPDB1
static int mh_repdb_build(const Options& o, vector<Gpu>& gpus) {
  rtc_ctx* ctx = gpus[0].ctx;
  vector<GenomeInfo> genomes; MinHashSketchFile mh; bool byFile = true;
  vector<uint32_t> size_cfg;
  if (o.has_presketched) {
    if (!load_minhash_sketches(o.folder_path, genomes, mh, byFile)) return 1;
    if (genomes.empty()) { cerr << "ERROR: no genome to cluster" << endl; return 1; }
    // loadSketches builds MinHash(k, containCompress) in containment mode (src/Sketch_IO.cpp:334): getSketchSize() reports that
    size_cfg.assign(genomes.size(), mh.isContainment ? (uint32_t)mh.containCompress : (uint32_t)mh.sketchSize);
    cerr << "===== MinHash RepDB Build (from pre-sketched) =====" << endl;
  } else {
    if (!o.sketchByFile) unsupported("single-FASTA input (run with -l and a genome list)");
    mh.kmerSize = o.kmerSize; mh.sketchSize = o.sketchSize; mh.isContainment = o.isContainment; mh.containCompress = o.containCompress;
    if (!o.isSetKmer) { mh.kmerSize = 21; cerr << "-----use default kmerSize: " << mh.kmerSize << endl; }
    if (!o.isJaccard) mh.sketchSize = 1000;
    SketchJob job;
    job.kssd = false; job.kmerSize = mh.kmerSize; job.sketchSize = mh.sketchSize; job.isContainment = mh.isContainment;
    job.containCompress = mh.containCompress; job.minLen = o.minLen; job.threads = o.threads;
    KssdSketchFile unused; Resident rs;
    sketch_files(gpus, o.inputFile, job, genomes, &mh, &unused, rs, true);
    cerr << "-----the size of sketches (number of genomes or sequences) is: " << genomes.size() << endl;
    if (genomes.empty()) { cerr << "ERROR: no genome to cluster" << endl; return 1; }
    const string folder = current_date_time();   // compute_sketches(isSave = true)
    string command = "mkdir -p " + folder;
    if (system(command.c_str()) != 0) { cerr << "ERROR: cannot create " << folder << endl; return 1; }
    save_minhash_sketches(genomes, mh, folder, true);
    size_cfg.resize(genomes.size());
    for (size_t i = 0; i < genomes.size(); i++)
      size_cfg[i] = mh.isContainment ? (uint32_t)std::max(file_length_for_containment(genomes[i].fileName) / mh.containCompress, 100)
                                     : (uint32_t)mh.sketchSize;
    cerr << "===== MinHash RepDB Build (from genomes) =====" << endl;
  }
  KssdClusterState st;
  st.minhash = true; st.threshold = o.threshold; st.kmer_size = mh.kmerSize; st.sketch_size = (int)size_cfg[0]; st.is_containment = mh.isContainment;
  cerr << "  Genomes:       " << genomes.size() << endl << "  Threshold:     " << o.threshold << endl << "  Kmer size:     " << st.kmer_size << endl
       << "  Sketch size:   " << st.sketch_size << endl;
  if (o.has_presketched) cerr << "  Containment:   " << (st.is_containment ? "yes" : "no") << endl;
  DeviceSketches ds;
  upload_sketches(ctx, &mh.hashes, nullptr, ds);
  vector<int32_t> rep_of(genomes.size(), -1);
  uint32_t ncl = 0;
  CHECK(ctx, rtc_greedy(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, size_cfg.data(), st.kmer_size, (int)st.is_containment, 0,
                        o.threshold, rep_of.data(), &ncl));
  CHECK(ctx, rtc_dev_free(ctx, ds.d_hashes)); CHECK(ctx, rtc_dev_free(ctx, ds.d_start)); CHECK(ctx, rtc_dev_free(ctx, ds.d_len));
  st.clusters = clusters_from_rep_of(rep_of);
  st.genomes = genomes; st.reps.use64 = true;
  for (const auto& c : st.clusters) if (!c.empty()) {
    st.rep_ids.push_back(c[0]);
    st.rep_genomes.push_back(genomes[c[0]]);
    st.reps.h64.push_back(mh.hashes[c[0]]);
  }
  if (!save_minhash_repdb(o.repdb_path, st)) return 1;
  if (!o.outputFile.empty()) {
    print_result(st.clusters, st.genomes, byFile, o.outputFile);
    cerr << "-----write the cluster result into: " << o.outputFile << endl;
  }
  cerr << "\n===== MinHash RepDB Build Summary =====" << endl << "  Total genomes:    " << genomes.size() << endl
       << "  Representatives:  " << st.rep_ids.size() << endl
       << "  Compression:      " << std::fixed << std::setprecision(2) << (1.0 - (double)st.rep_ids.size() / genomes.size()) * 100.0 << "%" << endl
       << "  RepDB saved to:   " << o.repdb_path << endl << "===============================" << endl;
  return 0;
}

// repdb_query (src/sub_command.cpp:337-393)
static int repdb_query(const Options& o, vector<Gpu>& gpus) {
  KssdClusterState st; vector<GenomeInfo> q; KssdSketchFile qs;
  if (repdb_load_and_sketch(o, gpus, st, q, qs) != 0) return 1;
  cerr << (o.is_fast ? "===== RepDB Query =====" : "===== MinHash RepDB Query =====") << endl << "  Query genomes:  " << q.size() << endl << "  Top-k:          " << o.topk << endl
       << "  DB reps:        " << st.rep_ids.size() << endl;
  vector<vector<RepHit>> hits;
  if (repdb_query_topk(gpus[0].ctx, st, qs, o.topk, hits) != 0) return 1;
  FILE* fp = fopen(o.outputFile.c_str(), "w");
  if (!fp) { cerr << "ERROR: Cannot open output file: " << o.outputFile << endl; return 1; }
  fprintf(fp, "#query\trank\trep_name\tdistance\tcluster_id\tcluster_size\n");
  for (size_t i = 0; i < q.size(); i++) {
    string qname = q[i].fileName;
    if (qname.empty()) qname = "query_" + std::to_string(i);
    if (hits[i].empty()) fprintf(fp, "%s\t0\tno_match\t-1\t-1\t0\n", qname.c_str());
    else for (size_t r = 0; r < hits[i].size(); r++) {
      const int ri = hits[i][r].rep_idx;
      fprintf(fp, "%s\t%d\t%s\t%.6f\t%d\t%d\n", qname.c_str(), (int)r + 1, st.rep_genomes[ri].fileName.c_str(), hits[i][r].distance, ri,
              (int)st.clusters[ri].size());
    }
  }
  fclose(fp);
  cerr << "===== Query Results =====" << endl << "  Output: " << o.outputFile << endl << "=========================" << endl;
  return 0;
}

// repdb_assign (src/sub_command.cpp:395-452; KssdClusterState::assign, src/greedy.cpp:2639-2654)
static int repdb_assign(const Options& o, vector<Gpu>& gpus) {
  KssdClusterState st; vector<GenomeInfo> q; KssdSketchFile qs;
  if (repdb_load_and_sketch(o, gpus, st, q, qs) != 0) return 1;
  cerr << (o.is_fast ? "===== RepDB Assignment =====" : "===== MinHash RepDB Assignment =====") << endl << "  Query genomes:  " << q.size() << endl << "  DB reps:        " << st.rep_ids.size() << endl
       << "  Threshold:      " << st.threshold << endl;
  vector<vector<RepHit>> hits;
  if (repdb_query_topk(gpus[0].ctx, st, qs, 1, hits) != 0) return 1;
  FILE* fp = fopen(o.outputFile.c_str(), "w");
  if (!fp) { cerr << "ERROR: Cannot open output file: " << o.outputFile << endl; return 1; }
  fprintf(fp, "#query\tassigned_cluster\trep_name\tdistance\tcluster_size\tstatus\n");
  int assigned = 0, unassigned = 0;
  for (size_t i = 0; i < q.size(); i++) {
    string qname = q[i].fileName;
    if (qname.empty()) qname = "query_" + std::to_string(i);
    if (!hits[i].empty() && hits[i][0].distance <= st.threshold) {
      const int ri = hits[i][0].rep_idx;
      fprintf(fp, "%s\t%d\t%s\t%.6f\t%d\tassigned\n", qname.c_str(), ri, st.rep_genomes[ri].fileName.c_str(), hits[i][0].distance,
              (int)st.clusters[ri].size());
      assigned++;
    } else {
      fprintf(fp, "%s\t-1\tunassigned\t-1\t0\tnovel\n", qname.c_str());
      unassigned++;
    }
  }
  fclose(fp);
  cerr << "===== Assignment Results =====" << endl
       << "  Assigned:    " << assigned << " (" << std::fixed << std::setprecision(1) << (100.0 * assigned / q.size()) << "%)" << endl
       << "  Novel:       " << unassigned << " (" << std::fixed << std::setprecision(1) << (100.0 * unassigned / q.size()) << "%)" << endl
       << "  Output:      " << o.outputFile << endl << "==============================" << endl;
  return 0;
}

// repdb_append (src/sub_command.cpp:454-500)
static int repdb_append(const Options& o, vector<Gpu>& gpus) {
  KssdClusterState st; vector<GenomeInfo> add; KssdSketchFile ks2;
  if (repdb_load_and_sketch(o, gpus, st, add, ks2) != 0) return 1;
  const size_t old_reps = st.rep_ids.size(), old_total = st.genomes.size();
  cerr << (o.is_fast ? "===== RepDB Append =====" : "===== MinHash RepDB Append =====") << endl << "  Existing reps:    " << old_reps << endl << "  Existing genomes: " << old_total << endl
       << "  New genomes:      " << add.size() << endl;
  if (kssd_incremental_cluster(gpus[0].ctx, st, add, ks2, false) != 0) return 1;
  if (!(st.minhash ? save_minhash_repdb(o.repdb_path, st) : save_kssd_repdb(o.repdb_path, st))) return 1;
  if (!o.outputFile.empty()) {   // printKssdResult / printRepDBClusterResult (src/sub_command.cpp:672-702): the same layout
    print_result(st.clusters, st.genomes, true, o.outputFile, st.threshold);
    cerr << "-----write the cluster result into: " << o.outputFile << endl;
  }
  cerr << "\n===== Append Summary =====" << endl << "  New reps added:   " << st.rep_ids.size() - old_reps << endl
       << "  Total reps now:   " << st.rep_ids.size() << endl << "  Total genomes:    " << st.genomes.size() << endl
       << "  RepDB updated:    " << o.repdb_path << endl << "==========================" << endl;
  return 0;
}
// append_clust_greedy (src/sub_command.cpp:23-190): `clust-greedy --append LIST --presketched DIR` on MinHash sketches.
// Without a stored state the old and the new sketches are put together, sorted by genome size (cmpGenomeSize) and
// clustered by the legacy greedyCluster -- every representative, MinHash::distance() (rtc_greedy_mash).  With a
// cluster_state.bin the representatives are taken from the folder's sketches by the stored ids (the reference
// re-reads the folder, :100-139) and the new genomes go through MinHashIncrementalCluster.
static int append_clust_greedy(const Options& o, vector<Gpu>& gpus) {
  rtc_ctx* ctx = gpus[0].ctx;
  const string state_file = o.folder_path + "/cluster_state.bin";
  if (!o.sketchByFile) unsupported("single-FASTA input (run with -l and a genome list)");
  KssdClusterState st;
  struct stat sb;
  bool has_state = stat(state_file.c_str(), &sb) == 0;
  if (has_state) {
    cerr << "===== Incremental Update Mode (MinHash) =====" << endl << "Found existing cluster state, loading..." << endl;
    has_state = load_minhash_cluster_state(state_file, st);
  }
  vector<GenomeInfo> pre; MinHashSketchFile mh; bool byFile = true;
  if (!load_minhash_sketches(o.folder_path, pre, mh, byFile)) return 1;
  auto sketch_new = [&](int kmer, int sketch_size, bool containment, vector<GenomeInfo>& add, MinHashSketchFile& mh2) {
    SketchJob job;
    job.kssd = false; job.kmerSize = kmer; job.sketchSize = sketch_size; job.isContainment = containment;
    job.containCompress = mh.containCompress; job.minLen = o.minLen; job.threads = o.threads;
    KssdSketchFile unused; Resident rs2;
    sketch_files(gpus, o.inputFile, job, add, &mh2, &unused, rs2, true);
  };
  if (!has_state) {
    if (byFile != o.sketchByFile) {
      cerr << "ERROR: append_clust_greedy(), the input format of append genomes and pre-sketched genome is not same (single input genome vs. genome list)" << endl;
      return 1;
    }
    cerr << "-----use the same sketch parameters with pre-generated sketches" << endl << "---the kmer size is: " << mh.kmerSize << endl;
    if (mh.isContainment) cerr << "---use the AAF distance (variable-sketch-size), the sketch size is in proportion with 1/" << mh.containCompress << endl;
    else cerr << "---use the Mash distance (fixed-sketch-size), the sketch size is: " << mh.sketchSize << endl;
    cerr << "---the thread number is: " << o.threads << endl << "---the threshold is: " << o.threshold << endl;
    vector<GenomeInfo> add; MinHashSketchFile mh2;
    sketch_new(mh.kmerSize, mh.sketchSize, mh.isContainment, add, mh2);
    cerr << "-----the size of sketches (number of genomes or sequences) is: " << add.size() << endl;
    // final_sketches = pre + append, sorted by genome size (length descending, id ascending; ids restart in the appended part)
    vector<GenomeInfo> all(pre);
    all.insert(all.end(), add.begin(), add.end());
    vector<size_t> perm(all.size());
    iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) {
      if (all[a].totalSeqLength != all[b].totalSeqLength) return all[a].totalSeqLength > all[b].totalSeqLength;
      return all[a].id < all[b].id;
    });
    vector<GenomeInfo> genomes; MinHashSketchFile fin = mh; fin.hashes.clear();
    for (size_t q : perm) {
      genomes.push_back(all[q]);
      fin.hashes.push_back(q < pre.size() ? mh.hashes[q] : mh2.hashes[q - pre.size()]);
    }
    if (!o.noSave) {
      const string folder = current_date_time();
      string command = "mkdir -p " + folder;
      if (system(command.c_str()) != 0) { cerr << "ERROR: cannot create " << folder << endl; return 1; }
      save_minhash_sketches(genomes, fin, folder, byFile);
    }
    if (genomes.empty()) { cerr << "ERROR: no genome to cluster" << endl; return 1; }
    DeviceSketches ds;
    upload_sketches(ctx, &fin.hashes, nullptr, ds);
    vector<int32_t> rep_of(genomes.size());
    uint32_t ncl = 0;
    // (sketches loaded from a containment folder report containCompress as their sketch size, src/Sketch_IO.cpp:334;
    // containDistance() does not use it)
    CHECK(ctx, rtc_greedy_mash(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, mh.kmerSize, (int)mh.isContainment,
                               (uint32_t)mh.sketchSize, o.threshold, rep_of.data(), &ncl));
    vector<vector<int>> cluster = clusters_from_rep_of(rep_of);
    print_result(cluster, genomes, byFile, o.outputFile);
    cerr << "-----write the cluster result into: " << o.outputFile << endl;
    cerr << "-----the cluster number of " << o.outputFile << " is: " << cluster.size() << endl;
    return 0;
  }
  cerr << "---the threshold is: " << o.threshold << endl << "---the thread number is: " << o.threads << endl;
  if (byFile != o.sketchByFile) cerr << "Warning: the input format of append genomes and pre-sketched genome is not same" << endl;
  st.genomes = pre; st.sk = KssdSketchFile(); st.sk.use64 = true; st.sk.h64 = mh.hashes;
  st.reps = KssdSketchFile(); st.reps.use64 = true; st.rep_genomes.clear();
  for (int rep_id : st.rep_ids) {
    if (rep_id < 0 || (size_t)rep_id >= pre.size()) {
      cerr << "ERROR: Representative ID " << rep_id << " out of range [0, " << pre.size() << "), cannot continue" << endl;
      return 1;
    }
    st.rep_genomes.push_back(pre[rep_id]);
    st.reps.h64.push_back(mh.hashes[rep_id]);
  }
  cerr << "Successfully loaded " << st.rep_ids.size() << " representatives" << endl << "Rebuilding inverted index..." << endl;
  if (st.kmer_size <= 0 || st.sketch_size <= 0) {
    cerr << "ERROR: Invalid kmer_size or sketch_size: kmer=" << st.kmer_size << ", sketch=" << st.sketch_size << endl;
    return 1;
  }
  if (st.is_containment && mh.containCompress <= 0) { cerr << "ERROR: is_containment is true but contain_compress is " << mh.containCompress << endl; return 1; }
  cerr << "Computing sketches for new genomes..." << endl << "  Parameters: kmer_size=" << st.kmer_size << ", sketch_size=" << st.sketch_size
       << ", is_containment=" << st.is_containment << ", contain_compress=" << mh.containCompress << endl;
  vector<GenomeInfo> add; MinHashSketchFile mh2;
  sketch_new(st.kmer_size, st.sketch_size, st.is_containment, add, mh2);
  cerr << "New genomes sketched: " << add.size() << endl;
  if (add.empty()) { cerr << "ERROR: No new sketches generated" << endl; return 0; }
  cerr << "Starting incremental clustering..." << endl;
  KssdSketchFile ks2; ks2.use64 = true; ks2.h64 = std::move(mh2.hashes);
  if (kssd_incremental_cluster(ctx, st, add, ks2, true) != 0) return 1;
  cerr << "Incremental clustering completed" << endl;
  if (!o.noSave && o.saveRep && !save_minhash_cluster_state(state_file, st)) return 1;
  print_result(st.clusters, st.genomes, o.sketchByFile, o.outputFile);
  cerr << "-----write the cluster result into: " << o.outputFile << endl;
  cerr << "-----the cluster number of " << o.outputFile << " is: " << st.clusters.size() << endl;
  cerr << "-----updated cluster state saved" << endl;
  return 0;
}
#endif

#ifdef DBSCAN_CLUST
// The -i input of --db --assign / --update sketched as the model's genomes were: kind, k, sketch parameters and minimum length
// from the model (clust-dbscan's and clust-leiden's alike).  what: whose sketches, for the messages.
struct ModelSketching { bool minhash; int width, kmer_size, sketch_size, half_k, half_subk, drlevel; uint64_t min_len; };
static int model_db_sketch(const Options& o, vector<Gpu>& gpus, const ModelSketching& md, const char* what, vector<GenomeInfo>& q,
                           MinHashSketchFile& mh, KssdSketchFile& ks) {
  SketchJob job;
  job.kssd = !md.minhash; job.kmerSize = md.kmer_size; job.minLen = md.min_len; job.threads = o.threads;
  if (md.minhash) job.sketchSize = md.sketch_size;
  else job.drlevel = md.drlevel;
  Resident rs;
  if (o.sketchByFile) sketch_files(gpus, o.inputFile, job, q, &mh, &ks, rs, true);
  else {
    vector<FastaRecord> recs; SeqModeSizes sz;
    if (!read_sequences(o.inputFile, md.min_len, recs, sz)) return 1;
    sketch_sequences(gpus, recs, job, q, &mh, &ks);
  }
  const int qwidth = md.minhash ? 8 : (ks.use64 ? 8 : 4);
  if (!q.empty() && qwidth != md.width) {
    cerr << "ERROR: the " << what << " sketches have hash width " << qwidth << " but the model has " << md.width << endl;
    return 1;
  }
  if (!md.minhash && !q.empty() && (ks.info.half_k != md.half_k || ks.info.half_subk != md.half_subk)) {
    cerr << "ERROR: the " << what << " sketches have half_k " << ks.info.half_k << ", half_subk " << ks.info.half_subk << " but the model has " << md.half_k
         << ", " << md.half_subk << endl;
    return 1;
  }
  return 0;
}
#endif

#ifdef LEIDEN_CLUST
// clust-leiden --db FILE --assign: the queries sketched as the model's genomes were; rtc_graph_query, the host's weights on the
// host threads, rtc_leiden_place; one TSV line each.  The model is read only.
static int leiden_db_assign(const Options& o, vector<Gpu>& gpus, const LeidenModel& md) {
  rtc_ctx* ctx = gpus[0].ctx;
  const double t0 = get_sec();
  vector<GenomeInfo> q; MinHashSketchFile mh; KssdSketchFile ks;
  if (const int rc = model_db_sketch(o, gpus, ModelSketching{false, md.width, md.kmer_size, 0, md.half_k, md.half_subk, md.drlevel, md.min_len},
                                     "query", q, mh, ks))
    return rc;
  const double t1 = get_sec();
  g_metrics.num("sketch_queries_s", t1 - t0);
  const uint32_t N = (uint32_t)md.labels.size(), Q = (uint32_t)q.size();
  cerr << "===== Leiden model assignment (" << (md.algorithm == 1 ? "Leiden" : "Louvain") << ", " << (md.objective == 0 ? "cpm" : "modularity") << ") =====" << endl
       << "  Query genomes:  " << Q << endl << "  Model genomes:  " << N << endl << "  Threshold, knn: " << md.threshold << ", " << md.knn << endl;
  vector<rtc_graph_near> near(Q);
  vector<rtc_leiden_placement> place(Q);
  vector<uint32_t> msize(N), qsize(Q);
  for (uint32_t p = 0; p < N; p++) msize[p] = (uint32_t)(md.width == 8 ? md.h64[p].size() : md.h32[p].size());
  uint64_t gc[10] = {0}, pc[10] = {0};
  double t_weights = 0.0;
  if (Q) {
    DeviceSketches ds;
    if (md.width == 8) {
      vector<vector<uint64_t>> all(md.h64);
      all.insert(all.end(), ks.h64.begin(), ks.h64.end());
      upload_sketches(ctx, &all, nullptr, ds);
    } else {
      vector<vector<uint32_t>> all(md.h32);
      all.insert(all.end(), ks.h32.begin(), ks.h32.end());
      upload_sketches(ctx, nullptr, &all, ds);
    }
    if (ds.n != N + Q) { cerr << "ERROR: --assign needs the query sketches on the host (" << ds.n - N << " of " << Q << ")" << endl; return 1; }
    for (uint32_t i = 0; i < Q; i++) qsize[i] = (uint32_t)(md.width == 8 ? ks.h64[i].size() : ks.h32[i].size());
    vector<rtc_qedge> edges((size_t)std::max<uint64_t>(1, (uint64_t)Q * std::min<uint64_t>(md.knn > 0 ? (uint64_t)md.knn : 64, 64)));
    uint64_t n_edges = 0;
    int st = rtc_graph_query(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, N, Q, md.threshold, md.kmer_size, (uint32_t)md.knn, 0, edges.data(),
                             edges.size(), &n_edges, near.data());
    if (st == RTC_ERR_OVERFLOW) {  // the count is known now
      edges.resize(n_edges);
      st = rtc_graph_query(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, N, Q, md.threshold, md.kmer_size, (uint32_t)md.knn, 0, edges.data(),
                           edges.size(), &n_edges, near.data());
    }
    CHECK(ctx, st);
    edges.resize(n_edges);
    rtc_graph_query_counters(ctx, gc);
    (void)rtc_dev_free(ctx, ds.d_hashes); (void)rtc_dev_free(ctx, ds.d_start); (void)rtc_dev_free(ctx, ds.d_len);
    const double tw = get_sec();
    LeidenQuant z;
    z.objective = md.objective; z.scale = md.scale; z.lo = md.lo; z.range = md.range;
    vector<rtc_wedge> records;
    leiden_assign_weights(edges.data(), n_edges, msize.data(), qsize.data(), md.kmer_size, rtc_graph_weight, z, o.threads, records);
    t_weights = get_sec() - tw;
    CHECK(ctx, rtc_leiden_place(ctx, N, md.labels.data(), (uint32_t)md.n_clusters, md.objective == RTC_LEIDEN_MODULARITY ? md.tot.data() : nullptr, md.m2,
                                md.resolution, md.objective, Q, records.data(), records.size(), place.data()));
    rtc_leiden_place_counters(ctx, pc);
  }
  if (getenv("RTC_VERBOSE"))
    fprintf(stderr, "[assign] %llu candidates in %llu chunk(s), %llu passing, %llu kept; query %.3f ms, weights %.3f ms, place %.3f ms\n",
            (unsigned long long)gc[1], (unsigned long long)gc[0], (unsigned long long)gc[2], (unsigned long long)gc[3], gc[9] / 1e6, t_weights * 1e3, pc[9] / 1e6);
  uint64_t placed = 0;
  for (uint32_t i = 0; i < Q; i++) placed += place[i].label >= 0;
  g_metrics.num("leiden_assign_query_s", gc[9] / 1e9);
  g_metrics.num("leiden_assign_weights_s", t_weights);
  g_metrics.num("leiden_assign_place_s", pc[9] / 1e9);
  g_metrics.num("leiden_assign_placed", (double)placed);
  g_metrics.num("leiden_assign_novel", (double)(Q - placed));
  g_metrics.num("genomes", (double)Q);
  FILE* fp = fopen(o.outputFile.c_str(), "w");
  if (!fp) { cerr << "ERROR: cannot open file: " << o.outputFile << endl; return 1; }
  fprintf(fp, "query\tcluster\trunner_up\tedges\tcommunities\tweight\tshare\tnearest\tdistance\n");
  for (uint32_t i = 0; i < Q; i++) {
    const rtc_leiden_placement& r = place[i];
    const string& name = o.sketchByFile ? q[i].fileName : q[i].seq0.name;
    char cluster[16] = "novel", runner[16] = "-", dist[32] = "inf";
    if (r.label >= 0) snprintf(cluster, sizeof cluster, "%d", r.label);
    if (r.runner_up >= 0) snprintf(runner, sizeof runner, "%d", r.runner_up);
    const double share = (r.label >= 0 && r.k_x) ? (double)r.e_label / (double)r.k_x : 0.0;
    string nearest = "-";
    if (near[i].nearest != UINT32_MAX) {
      const GenomeInfo& g = md.genomes[near[i].nearest];
      nearest = md.sketch_by_file ? g.fileName : g.seq0.name;
      snprintf(dist, sizeof dist, "%.6f", 1.0 - rtc_graph_weight(near[i].common, qsize[i], msize[near[i].nearest], md.kmer_size));
    }
    fprintf(fp, "%s\t%s\t%s\t%u\t%u\t%.6f\t%.6f\t%s\t%s\n", name.c_str(), cluster, runner, r.n_edges, r.n_comms, (double)r.e_label / 1048576.0, share,
            nearest.c_str(), dist);
  }
  fclose(fp);
  cerr << "===== Assignment Results =====" << endl << "  Placed:      " << placed << endl << "  Novel:       " << Q - placed << endl
       << "  Output:      " << o.outputFile << endl << "==============================" << endl;
  return 0;
}
#endif

#if defined(DBSCAN_CLUST) && !defined(LEIDEN_CLUST)
// KssdDBSCAN's closing lines (src/dbscan.cpp:951-980).  Its progress lines (:918-930) leave std::fixed and precision 1 on cerr
// once one has been printed, and the core-point percentage comes out in that format then: the walk is replayed from the labels
// to learn whether it printed one.  After cluster c (opened at its smallest core index s_c) the walk has visited
// {0 .. s_c} and the members of clusters 0 .. c; it reports when that count has grown by max(1000, n / 100) since its last
// report or equals n.
static void dbscan_report(const vector<int32_t>& labels, const vector<uint8_t>& core, uint32_t ncl, uint32_t nnoise) {
  const int n = (int)labels.size();
  vector<int> seed(ncl, -1);
  vector<vector<int>> members(ncl);
  uint64_t n_core = 0;
  for (int v = 0; v < n; v++) {
    if (core[v]) { n_core++; if (seed[labels[v]] < 0) seed[labels[v]] = v; }
    if (labels[v] >= 0) members[labels[v]].push_back(v);
  }
  vector<int> bit(n + 1, 0);  // Fenwick tree over the indices of the members placed so far
  auto add = [&](int i) { for (i++; i <= n; i += i & -i) bit[i]++; };
  auto prefix = [&](int i) { int r = 0; for (i++; i > 0; i -= i & -i) r += bit[i]; return r; };
  const int interval = std::max(1000, n / 100);
  int last = 0, placed = 0;
  bool fixed_fmt = false;
  for (uint32_t c = 0; c < ncl; c++) {
    for (int v : members[c]) add(v);
    placed += (int)members[c].size();
    const int processed = seed[c] + 1 + (placed - prefix(seed[c]));
    if (processed - last >= interval || processed == n) { fixed_fmt = true; last = processed; }
  }
  cerr << "-----DBSCAN clustering complete!" << endl;
  cerr << "-----Found " << ncl << " clusters" << endl;
  cerr << "-----Found " << nnoise << " noise points (outliers)" << endl;
  if (n_core > 0) {
    if (fixed_fmt) cerr << std::fixed << std::setprecision(1);
    cerr << "-----Core points: " << n_core << " (" << (100.0 * n_core / n) << "%)" << endl;
    cerr.unsetf(std::ios_base::floatfield);
    cerr << std::setprecision(6);
  }
}

// printKssdDBSCANResult (src/dbscan.cpp:1212-1310): the clusters with their members in ascending index order, then every noise
// point as a cluster of its own.  mismatch: the sketches were stored in the other layout than -l asks for (the warning of
// :3237-3240).  The reference then prints fields it never loaded: with -l an empty fileSeqs gives the names "N/A" (:1246-1250)
// beside an empty file name, without -l an empty seqInfo gives empty names.  The lengths it prints there are whatever the
// unloaded field holds; this prints 0.
static void print_dbscan_result(const vector<int32_t>& labels, uint32_t ncl, const vector<GenomeInfo>& g, bool sketchByFile, bool mismatch,
                                const string& outputFile, double eps, int minPts, int minClusterSize = 0) {
  FILE* fp = fopen(outputFile.c_str(), "w");
  if (!fp) { cerr << "Error in printKssdDBSCANResult(), cannot open file: " << outputFile << endl; exit(1); }
  vector<vector<int>> clusters(ncl);
  vector<int> noise;
  for (size_t i = 0; i < labels.size(); i++) {
    if (labels[i] < 0) noise.push_back((int)i);
    else clusters[labels[i]].push_back((int)i);
  }
  // minClusterSize > 0: the flat clustering of --hierarchy (rtc_hierarchy_flat), eps the ceiling the hierarchy was built under
  if (minClusterSize > 0) fprintf(fp, "# HDBSCAN* flat clustering parameters: min_cluster_size=%d, minPts=%d, eps_max=%.6f\n", minClusterSize, minPts, eps);
  else fprintf(fp, "# DBSCAN clustering parameters: eps=%.6f, minPts=%d\n", eps, minPts);
  fprintf(fp, "# Total clusters: %d\n", (int)ncl);
  if (!noise.empty()) fprintf(fp, "# Total noise points (outliers): %d\n", (int)noise.size());
  fprintf(fp, "#\n");
  auto line = [&](int j, int curId) {
    const GenomeInfo& s = g[curId];
    if (sketchByFile && mismatch)
      fprintf(fp, "\t%5d\t%6d\t%12dnt\t%20s\t%20s\t%s\n", j, curId, 0, "", "N/A", "N/A");
    else if (sketchByFile)
      fprintf(fp, "\t%5d\t%6d\t%12dnt\t%20s\t%20s\t%s\n", j, curId, (int)s.totalSeqLength, s.fileName.c_str(), s.seq0.name.c_str(),
              s.seq0.comment.c_str());
    else if (mismatch)
      fprintf(fp, "\t%6d\t%6d\t%12dnt\t%20s\t%s\n", j, curId, 0, "", "");
    else
      fprintf(fp, "\t%6d\t%6d\t%12dnt\t%20s\t%s\n", j, curId, s.seq0.length, s.seq0.name.c_str(), s.seq0.comment.c_str());
  };
  for (size_t i = 0; i < clusters.size(); i++) {
    fprintf(fp, "the cluster %d is: \n", (int)i);
    for (size_t j = 0; j < clusters[i].size(); j++) line((int)j, clusters[i][j]);
    fprintf(fp, "\n");
  }
  for (size_t i = 0; i < noise.size(); i++) {
    fprintf(fp, "the cluster %d is: \n", (int)(clusters.size() + i));
    line(0, noise[i]);
    fprintf(fp, "\n");
  }
  fclose(fp);
}

static int dbscan_db_sketch(const Options& o, vector<Gpu>& gpus, const DbscanModel& md, const char* what, vector<GenomeInfo>& q,
                            MinHashSketchFile& mh, KssdSketchFile& ks) {
  return model_db_sketch(o, gpus, ModelSketching{md.minhash, md.width, md.kmer_size, md.sketch_size, md.half_k, md.half_subk, md.drlevel, md.min_len},
                         what, q, mh, ks);
}

// clust-dbscan --db FILE --assign: the queries sketched as the model's genomes were, placed by rtc_dbscan_assign, one TSV line each
static int dbscan_db_assign(const Options& o, vector<Gpu>& gpus, const DbscanModel& md) {
  rtc_ctx* ctx = gpus[0].ctx;
  const double t0 = get_sec();
  vector<GenomeInfo> q; MinHashSketchFile mh; KssdSketchFile ks;
  if (const int rc = dbscan_db_sketch(o, gpus, md, "query", q, mh, ks)) return rc;
  const double t1 = get_sec();
  g_metrics.num("sketch_queries_s", t1 - t0);
  const uint32_t N = (uint32_t)md.labels.size(), Q = (uint32_t)q.size();
  cerr << "===== DBSCAN model assignment (" << (md.minhash ? "MinHash" : "KSSD") << ") =====" << endl
       << "  Query genomes:  " << Q << endl << "  Model genomes:  " << N << endl << "  Eps, minPts:    " << md.eps << ", " << md.min_pts << endl;
  vector<rtc_dbscan_place> place(Q);
  uint64_t c[10] = {0};
  if (Q) {
    DeviceSketches ds;
    if (md.width == 8) {
      vector<vector<uint64_t>> all(md.h64);
      const vector<vector<uint64_t>>& qh = md.minhash ? mh.hashes : ks.h64;
      all.insert(all.end(), qh.begin(), qh.end());
      upload_sketches(ctx, &all, nullptr, ds);
    } else {
      vector<vector<uint32_t>> all(md.h32);
      all.insert(all.end(), ks.h32.begin(), ks.h32.end());
      upload_sketches(ctx, nullptr, &all, ds);
    }
    if (ds.n != N + Q) { cerr << "ERROR: --assign needs the query sketches on the host (" << ds.n - N << " of " << Q << ")" << endl; return 1; }
    CHECK(ctx, rtc_dbscan_assign(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, N, Q, md.labels.data(), md.core.data(), md.minhash ? 1 : 0,
                                 (uint32_t)md.sketch_size, md.eps, md.min_pts, md.kmer_size, 0, place.data()));
    rtc_dbscan_assign_counters(ctx, c);
    (void)rtc_dev_free(ctx, ds.d_hashes); (void)rtc_dev_free(ctx, ds.d_start); (void)rtc_dev_free(ctx, ds.d_len);
  }
  const double t2 = get_sec();
  if (getenv("RTC_VERBOSE"))
    fprintf(stderr, "[assign] %llu candidates in %llu chunk(s), %llu neighbours; join %.3f ms, predicate %.3f ms, fold %.3f ms\n", (unsigned long long)c[1],
            (unsigned long long)c[0], (unsigned long long)c[2], c[6] / 1e6, c[7] / 1e6, c[8] / 1e6);
  g_metrics.num("dbscan_assign_s", t2 - t1);
  g_metrics.num("dbscan_assign_join_s", c[6] / 1e9);
  g_metrics.num("dbscan_assign_predicate_s", c[7] / 1e9);
  g_metrics.num("dbscan_assign_fold_s", c[8] / 1e9);
  g_metrics.num("dbscan_assign_placed", (double)c[3]);
  g_metrics.num("dbscan_assign_novel", (double)c[4]);
  g_metrics.num("dbscan_assign_bridging", (double)c[5]);
  g_metrics.num("genomes", (double)Q);
  FILE* fp = fopen(o.outputFile.c_str(), "w");
  if (!fp) { cerr << "ERROR: cannot open file: " << o.outputFile << endl; return 1; }
  fprintf(fp, "query\tcluster\tbridges\tneighbours\tcore_neighbours\twould_be_core\tnearest\tdistance\n");
  for (uint32_t i = 0; i < Q; i++) {
    const rtc_dbscan_place& r = place[i];
    const string& name = o.sketchByFile ? q[i].fileName : q[i].seq0.name;
    char cluster[16] = "novel", dist[32] = "inf";
    if (r.label >= 0) snprintf(cluster, sizeof cluster, "%d", r.label);
    string nearest = "-";
    if (r.nearest != UINT32_MAX) {
      const GenomeInfo& g = md.genomes[r.nearest];
      nearest = md.sketch_by_file ? g.fileName : g.seq0.name;
      double d;
      if (md.minhash) d = rtc_mash_distance(r.common, r.denom, (uint32_t)md.sketch_size, md.kmer_size);
      else if (r.common == r.denom) d = 0.0;
      else { const double j = (double)r.common / (double)r.denom; d = -log(2.0 * j / (1.0 + j)) / md.kmer_size; }
      snprintf(dist, sizeof dist, "%.6f", d);
    }
    fprintf(fp, "%s\t%s\t%d\t%u\t%u\t%u\t%s\t%s\n", name.c_str(), cluster, r.label != r.label_max ? 1 : 0, r.n_neighbours, r.n_core, r.flags & 1u,
            nearest.c_str(), dist);
  }
  fclose(fp);
  cerr << "===== Assignment Results =====" << endl << "  Placed:      " << c[3] << endl << "  Novel:       " << c[4] << endl << "  Bridging:    " << c[5] << endl
       << "  Output:      " << o.outputFile << endl << "==============================" << endl;
  return 0;
}

// clust-dbscan --db FILE --update: the new genomes sketched as --assign sketches its queries, rtc_dbscan_update over the model's
// sketches followed by theirs, the clustering of all genomes in result.dbscan's layout, and the model rewritten in place
static int dbscan_db_update(const Options& o, vector<Gpu>& gpus, DbscanModel& md) {
  rtc_ctx* ctx = gpus[0].ctx;
  const double t0 = get_sec();
  vector<GenomeInfo> add; MinHashSketchFile mh; KssdSketchFile ks;
  if (const int rc = dbscan_db_sketch(o, gpus, md, "new", add, mh, ks)) return rc;
  const double t1 = get_sec();
  g_metrics.num("sketch_new_s", t1 - t0);
  const uint32_t N = (uint32_t)md.labels.size(), M = (uint32_t)add.size();
  cerr << "===== DBSCAN model update (" << (md.minhash ? "MinHash" : "KSSD") << ") =====" << endl
       << "  New genomes:    " << M << endl << "  Model genomes:  " << N << endl << "  Eps, minPts:    " << md.eps << ", " << md.min_pts << endl;
  const vector<vector<uint64_t>>& a64 = md.minhash ? mh.hashes : ks.h64;
  if ((md.width == 8 ? a64.size() : ks.h32.size()) != M) {
    cerr << "ERROR: --update needs the new sketches on the host (" << (md.width == 8 ? a64.size() : ks.h32.size()) << " of " << M << ")" << endl;
    return 1;
  }
  vector<int32_t> labels((size_t)N + M);
  vector<uint8_t> core((size_t)N + M);
  uint32_t ncl = 0, nnoise = 0;
  uint64_t c[12] = {0};
  {
    DeviceSketches ds;
    if (md.width == 8) {
      vector<vector<uint64_t>> all(md.h64);
      all.insert(all.end(), a64.begin(), a64.end());
      upload_sketches(ctx, &all, nullptr, ds);
    } else {
      vector<vector<uint32_t>> all(md.h32);
      all.insert(all.end(), ks.h32.begin(), ks.h32.end());
      upload_sketches(ctx, nullptr, &all, ds);
    }
    CHECK(ctx, rtc_dbscan_update(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, N, M, md.labels.data(), md.core.data(), md.minhash ? 1 : 0,
                                 (uint32_t)md.sketch_size, md.eps, md.min_pts, md.kmer_size, labels.data(), core.data(), &ncl, &nnoise));
    rtc_dbscan_update_counters(ctx, c);
    (void)rtc_dev_free(ctx, ds.d_hashes); (void)rtc_dev_free(ctx, ds.d_start); (void)rtc_dev_free(ctx, ds.d_len);
  }
  const double t2 = get_sec();
  if (getenv("RTC_VERBOSE"))
    fprintf(stderr, "[update] rows %llu + %llu, %llu candidates in %llu chunk(s), %llu kept; join %.3f ms, predicate %.3f ms, components %.3f ms\n",
            (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[3], (unsigned long long)c[2], (unsigned long long)c[4], c[8] / 1e6,
            c[9] / 1e6, c[10] / 1e6);
  g_metrics.num("dbscan_update_s", t2 - t1);
  g_metrics.num("dbscan_update_join_s", c[8] / 1e9);
  g_metrics.num("dbscan_update_predicate_s", c[9] / 1e9);
  g_metrics.num("dbscan_update_components_s", c[10] / 1e9);
  g_metrics.num("dbscan_update_rows", (double)(c[0] + c[1]));
  g_metrics.num("dbscan_update_promoted", (double)c[5]);
  g_metrics.num("dbscan_update_merged", (double)c[6]);
  g_metrics.num("genomes", (double)N + M);
  g_metrics.num("clusters", (double)ncl);
  g_metrics.num("noise", (double)nnoise);
  if (!update_dbscan_model(md, add, &ks.h32, &a64, labels, core, (int)ncl)) { cerr << "ERROR: --update: the new sketches do not fit the model" << endl; return 1; }
  print_dbscan_result(labels, ncl, md.genomes, md.sketch_by_file, false, o.outputFile, md.eps, md.min_pts);
  if (!save_dbscan_model(o.repdb_path, md)) return 1;
  cerr << "===== Update Results =====" << endl << "  Genomes:     " << (size_t)N + M << endl << "  Clusters:    " << ncl << endl << "  Noise:       " << nnoise << endl
       << "  Re-measured: " << c[1] << " of " << N << " model genomes" << endl << "  Promoted:    " << c[5] << endl << "  Merged away: " << c[6] << endl
       << "  Output:      " << o.outputFile << endl << "  Model:       " << o.repdb_path << endl << "==========================" << endl;
  return 0;
}
#endif

// Will this run use exactly one GPU?  Answered without the HIP runtime (its environment must be final before it starts): a
// --gpus / RTC_GPUS choice that names one device, or "all" on a host whose driver topology lists one GPU node.
static bool single_gpu_run(const string& spec) {
  if (spec != "all") {  // as the spec is parsed further down: digits alone are a COUNT (--gpus 4 = four GPUs), a comma list names devices
    if (spec.find(',') == string::npos && spec.find_first_not_of("0123456789") == string::npos && atoi(spec.c_str()) > 0) return atoi(spec.c_str()) == 1;
    int named = 0;
    for (size_t p0 = 0; p0 <= spec.size();) { size_t p1 = spec.find(',', p0); if (p1 == string::npos) p1 = spec.size(); if (p1 > p0) named++; p0 = p1 + 1; }
    return named == 1;
  }
  for (const char* v : {"HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"})
    if (const char* e = getenv(v)) return *e != 0 && strchr(e, ',') == nullptr;
  int gpus = 0;
  for (int node = 0; node < 64; node++) {
    FILE* f = fopen(("/sys/class/kfd/kfd/topology/nodes/" + std::to_string(node) + "/properties").c_str(), "r");
    if (!f) break;
    char key[64]; unsigned long long val;
    while (fscanf(f, "%63s %llu", key, &val) == 2)
      if (strcmp(key, "simd_count") == 0 && val > 0) gpus++;
    fclose(f);
  }
  return gpus == 1;
}

int main(int argc, char** argv) {
#ifdef RTC_MEASURE
  if (const char* e = getenv("RTC_START_DELAY_MS")) usleep(1000 * atoi(e));
#endif
  const double t_main = get_sec();
  Options o = parse(argc, argv);
  // The staging batches leave pageable memory 15 % faster through the runtime's copy kernels than through the SDMA engines
  // (2 048 x 5 Mbp: output 0.112-0.127 s after the runtime is up against 0.128-0.153 s, tools/cli_timeline.py) and the
  // sketch kernels leave the CUs idle two thirds of the time anyway.  Measured on ONE GPU only, so only a run on one GPU
  // gets it: with several, RCCL's collectives and the share step's peer copies would land on the CUs beside the sketch
  // kernels, which nobody has timed.  Has to be in the environment before the runtime starts (hence the look at the
  // driver's topology instead of a device count); a value the user has set is left alone.
  if (single_gpu_run(o.gpus.empty() ? (getenv("RTC_GPUS") ? getenv("RTC_GPUS") : "all") : o.gpus)) setenv("HSA_ENABLE_SDMA", "0", 0);
  if (!o.has_output && !o.db_stats) { cerr << "ERROR: option -o/--output is required (unless --buildDB or --stats is used)" << endl; return 1; }
  if (o.threads < 1) { fprintf(stderr, "-----Invalid thread number %d\n", o.threads); return 1; }
  fprintf(stderr, "-----set the thread number %d\n", o.threads);
  if (!o.has_threshold) { o.threshold = 0.05; cerr << "-----use default threshold: " << o.threshold << endl; }

#ifdef GREEDY_CLUST
  // ---- --order degree: what it does not go with, before any GPU is asked for ----
  if (o.orderDegree) {
    const char* bad = o.isContainment ? "-c/--containment" : !o.useIndex ? "--inverted-index=false" : o.has_append ? "--append"
                      : !o.repdb_path.empty() ? "--db" : o.saveRep ? "--save-rep" : nullptr;
    if (bad) { cerr << "ERROR: --order does not go with " << bad << endl; return 1; }
    if (!o.is_fast && !(o.threshold >= 0.0 && o.threshold < 1.0)) {
      cerr << "ERROR: --order degree on MinHash sketches needs 0 <= -d/--threshold < 1, got " << o.threshold << endl;
      return 1;
    }
  }
  // ---- RepDB mode (src/main.cpp:160-170, :300-370) ----
  const bool db_action = o.db_build || o.db_query || o.db_assign || o.db_stats;
  if (db_action && o.repdb_path.empty()) { cerr << "ERROR: --build / --query / --assign / --stats require --db" << endl; return 1; }
  if ((int)o.db_build + (int)o.db_query + (int)o.db_assign + (int)o.db_stats > 1) { cerr << "ERROR: --build, --query, --assign and --stats exclude each other" << endl; return 1; }
  if (!o.repdb_path.empty()) {
    if (o.db_stats) {
      KssdClusterState st;
      if (o.is_fast) { if (!load_kssd_repdb(o.repdb_path, st)) { cerr << "ERROR: Failed to load RepDB from: " << o.repdb_path << endl; return 1; } }
      else if (!load_minhash_repdb(o.repdb_path, st)) { cerr << "ERROR: Failed to load MinHash RepDB from: " << o.repdb_path << endl; return 1; }
      print_kssd_repdb_stats(st, std::cout);
      return 0;
    }
    if (o.db_build && !o.has_presketched && !o.has_input) { cerr << "ERROR: --build requires --presketched <folder> or -i <genome_list> -l" << endl; return 1; }
    if (o.db_query && !o.has_input) { cerr << "ERROR: --query requires -i <input_file>" << endl; return 1; }
    if (o.db_assign && !o.has_input) { cerr << "ERROR: --assign requires -i <input_file>" << endl; return 1; }
    if (!db_action && !o.has_append) { cerr << "ERROR: --db requires one of: --build, --query, --assign, --append, --stats" << endl; return 1; }
  }
  if (o.has_append && o.has_input) { cerr << "ERROR: --append and -i/--input exclude each other" << endl; return 1; }
  if (o.has_append && !o.has_presketched && o.repdb_path.empty()) { cerr << "ERROR option --append, option --presketched needed" << endl; return 1; }  // src/main.cpp:378-381
#endif
#ifdef LEIDEN_CLUST
  // ---- clust-leiden: the checks of src/main.cpp:391-477 in that order, all before any GPU context exists (the default
  // threshold 0.05 is set above, as for every command) ----
  // ---- clust-leiden --minhash: this build's own flag, what it excludes named first.  -s and -c mean something beside it alone
  if (!o.minhash && !o.minhashOnly.empty()) { fprintf(stderr, "ERROR: unknown option %s\n", o.minhashOnly.c_str()); return 1; }
  if (o.minhash) {
    const char* bad = o.is_fast ? "--fast (the two sketch kinds exclude each other)" : o.isContainment ? "-c/--containment" : o.hasDrlevel ? "--drlevel"
                      : !o.repdb_path.empty() ? "--db (models of MinHash sketches are out of scope)" : nullptr;
    if (bad) { cerr << "ERROR: --minhash does not go with " << bad << endl; return 1; }
    if (!(o.threshold > 0.0 && o.threshold <= 1.0)) { cerr << "ERROR: --minhash needs 0 < -d/--threshold <= 1, got " << o.threshold << endl; return 1; }
  }
  // ---- clust-leiden --mcl: the third algorithm has neither an objective nor a resolution, and the placement rule of --db is
  // defined on modularity / CPM scores.  Beside --assign / --stats it has no effect, as --louvain / --leiden have none there.
  int mcl_h = 4;
  uint32_t mcl_select = 1024, mcl_iterations = 100;
  if (!o.mcl && o.mclOnly) { cerr << "ERROR: " << o.mclOnly << " needs --mcl" << endl; return 1; }
  if (o.mcl) {
    const char* bad = o.louvain ? "--louvain" : o.leiden ? "--leiden" : o.has_resolution ? "--resolution" : o.has_objective ? "--objective"
                      : o.db_build ? "--db --build" : nullptr;
    if (bad) { cerr << "ERROR: --mcl does not go with " << bad << endl; return 1; }
    char* end = nullptr;
    const double x2 = strtod(o.inflation.c_str(), &end) * 2.0;
    if (end == o.inflation.c_str() || *end || !(x2 >= 3.0 && x2 <= 16.0) || x2 != floor(x2)) {
      cerr << "ERROR: --inflation must be a multiple of 0.5 between 1.5 and 8, got " << o.inflation << endl;
      return 1;
    }
    mcl_h = (int)x2;
    const long long sel = strtoll(o.mclSelect.c_str(), &end, 10);
    if (end == o.mclSelect.c_str() || *end || sel < 1 || sel > 4096) { cerr << "ERROR: --mcl-select must be between 1 and 4096, got " << o.mclSelect << endl; return 1; }
    mcl_select = (uint32_t)sel;
    const long long its = strtoll(o.mclIterations.c_str(), &end, 10);
    if (end == o.mclIterations.c_str() || *end || its < 0 || its > 0x7fffffffll) { cerr << "ERROR: --mcl-iterations must be 0 or more, got " << o.mclIterations << endl; return 1; }
    mcl_iterations = (uint32_t)its;
  }
  // ---- clust-leiden --snn: a query has no neighbourhood in the model's graph, so no placement rule follows from these weights
  double snn_prune = 0.0;
  if (!o.snn && o.hasSnnPrune) { cerr << "ERROR: --snn-prune needs --snn" << endl; return 1; }
  if (o.snn) {
    if (!o.repdb_path.empty() || o.db_build || o.db_assign || o.db_stats) { cerr << "ERROR: --snn does not go with --db" << endl; return 1; }
    char* end = nullptr;
    snn_prune = strtod(o.snnPrune.c_str(), &end);
    if (end == o.snnPrune.c_str() || *end || !(snn_prune >= 0.0 && snn_prune < 1.0)) { cerr << "ERROR: --snn-prune must be in [0, 1)" << endl; return 1; }
  }
  // ---- clust-leiden --db: the model file's flows, their flag errors first ----
  LeidenModel ld_model;
  {
    const int actions = (int)o.db_build + (int)o.db_assign + (int)o.db_stats;
    if (actions > 1) { cerr << "ERROR: --build, --assign and --stats exclude each other" << endl; return 1; }
    if (actions && o.repdb_path.empty()) { cerr << "ERROR: --build / --assign / --stats require --db" << endl; return 1; }
    if (!o.repdb_path.empty() && actions != 1) { cerr << "ERROR: --db requires one of --build, --assign, --stats" << endl; return 1; }
    if (o.db_build && o.has_pregraph) { cerr << "ERROR: --db --build does not go with --pregraph" << endl; return 1; }
    if (o.db_assign && !o.has_input) { cerr << "ERROR: --assign requires -i <input_file>" << endl; return 1; }
    if (o.db_assign && (o.has_pregraph || o.saveGraph)) {
      cerr << "ERROR: --assign does not go with " << (o.has_pregraph ? "--pregraph" : "--save-graph") << endl;
      return 1;
    }
    if (o.db_stats || o.db_assign) {
      string why;
      if (!load_leiden_model(o.repdb_path, ld_model, &why)) { cerr << "ERROR: --db " << o.repdb_path << ": " << why << endl; return 1; }
    }
    if (o.db_stats) {
      print_leiden_model_stats(ld_model, std::cout);
      std::cout.flush();
      return 0;
    }
    if (o.db_assign) {
      // -k, -d, --resolution, --knn, --objective, --louvain and --leiden beside --assign have no effect: the model's hold
      o.louvain = ld_model.algorithm == 0; o.leiden = !o.louvain; o.mcl = false;
      o.objective = ld_model.objective == 0 ? "cpm" : "modularity";
      o.resolution = ld_model.resolution; o.has_resolution = false;
      o.threshold = ld_model.threshold; o.knn = ld_model.knn;
      o.is_fast = true; o.has_presketched = false;
      o.kmerSize = ld_model.kmer_size; o.isSetKmer = true; o.drlevel = ld_model.drlevel;
    }
  }
  if (o.has_resolution) cerr << "-----Resolution parameter: " << o.resolution << endl;
  if (o.leiden && o.louvain) { cerr << "ERROR: --leiden and --louvain exclude each other" << endl; return 1; }
  if (!o.louvain && !o.leiden && !o.mcl) {
    cerr << "ERROR: Leiden refinement is not in this build; run with --louvain" << endl;
    cerr << "NOTE: the line above is kept for scripts that match it; name the algorithm: --leiden (the deterministic Leiden), --louvain or --mcl (Markov clustering)" << endl;
    return 1;
  }
  if (o.objective != "cpm" && o.objective != "modularity") { cerr << "ERROR: --objective must be cpm or modularity, got " << o.objective << endl; return 1; }
  if (!(o.resolution > 0.0) || !(o.resolution < 65536.0)) { cerr << "ERROR: --resolution must be > 0 and below 65536, got " << o.resolution << endl; return 1; }
  if (!(o.threshold > 0.0)) { cerr << "ERROR: -d/--threshold must be > 0, got " << o.threshold << endl; return 1; }
  if (o.knn < 0) { cerr << "ERROR: --knn must be >= 0, got " << o.knn << endl; return 1; }
  if (o.knn == 0 && o.louvain) { o.knn = 1000; cerr << "-----Auto-enabled: edge-parallel + warm-start + knn=" << o.knn << endl; }
  if (o.knn == 0) { o.knn = 500; cerr << "-----Auto-selecting k-NN: k=" << o.knn << " (use --knn 0 to disable)" << endl; }
  if (o.knn > 0 && o.knn < 10) { cerr << "WARNING: --knn value too small (" << o.knn << "), recommend at least 50. Using 50." << endl; o.knn = 50; }
  if (o.mcl) cerr << "-----Algorithm: MCL (inflation " << mcl_h / 2.0 << ", select " << mcl_select << ")" << endl;
  else cerr << (o.louvain ? "-----Algorithm: Louvain (Optimized)" : "-----Algorithm: Leiden") << endl;
  cerr << "  - k-NN filtering (k=" << o.knn << ")" << endl;
  vector<rtc_wedge> pregraph;
  vector<double> pregraph_weights;
  if (o.has_pregraph) {
    cerr << "-----Clustering from pre-built graph (fast resolution adjustment)" << endl;
    // the sketches of the folder name the genomes (clust_from_pregraph_leiden, src/sub_command.cpp:3200-3225): KSSD ones, with
    // --minhash the MinHash ones
    o.has_presketched = true;
    o.is_fast = !o.minhash;
    o.saveGraph = false;
  } else if (!o.is_fast && !o.minhash) {
    cerr << "ERROR: clust-leiden requires --fast option" << endl;
    return 1;
  } else if (!o.has_presketched) {
    if (!o.isSetKmer) { o.kmerSize = 19; cerr << "-----use default kmerSize: " << o.kmerSize << endl; }  // as clust-dbscan, --minhash included
    if (o.drlevel < 0 || o.drlevel > 8) { cerr << "ERROR: invalid drlevel " << o.drlevel << ", should be in [0, 8]" << endl; return 1; }
  }
  if (o.saveGraph && o.noSave && !o.has_presketched) { cerr << "ERROR: --save-graph writes into the sketch folder, which -e/--no-save leaves out" << endl; return 1; }
  uint64_t pregraph_nodes = 0;
  if (o.has_pregraph) {
    string why;
    if (!load_leiden_graph(o.folder_path + "/leiden.graph", pregraph, pregraph_weights, pregraph_nodes, &why)) {
      cerr << "ERROR: --pregraph " << o.folder_path << ": " << why << endl;
      return 1;
    }
  }
#elif defined(DBSCAN_CLUST)
  // ---- clust-dbscan --knn: defined on the directed k-NN relation, so nothing built on the symmetric one goes with it, and
  // --assign's border rule reads full neighbourhoods.  Its -i input is opened here: the GPU comes up beside the reading of the
  // list, and a run that cannot start must say so before any context exists.
  if (o.dbscanKnn > 0) {
    const char* bad = o.minhash ? "--minhash" : !o.epsSweep.empty() ? "--eps-sweep" : o.kdist ? "--kdist" : o.hierarchy ? "--hierarchy"
                      : o.hasMinClusterSize ? "--min-cluster-size" : !o.repdb_path.empty() ? "--db" : nullptr;
    if (bad) { cerr << "ERROR: --knn does not go with " << bad << endl; return 1; }
    if (o.has_input && !o.has_presketched && !std::ifstream(o.inputFile)) {
      cerr << "ERROR: --knn: cannot open the input " << o.inputFile << endl;
      return 1;
    }
  }
  // ---- clust-dbscan --db: the model file's flows, their flag errors before any GPU context exists ----
  DbscanModel db_model;
  {
    const int actions = (int)o.db_build + (int)o.db_assign + (int)o.db_stats + (int)o.db_update;
    if (o.db_update && o.repdb_path.empty()) { cerr << "ERROR: --update requires --db" << endl; return 1; }
    if (actions && o.repdb_path.empty()) { cerr << "ERROR: --build / --assign / --stats require --db" << endl; return 1; }
    if (!o.repdb_path.empty() && o.has_append) { cerr << "ERROR: --append not supported for DBSCAN clustering" << endl; return 1; }
    if (!o.repdb_path.empty() && actions != 1) { cerr << "ERROR: --db requires exactly one of --build, --assign, --stats, --update" << endl; return 1; }
    if (o.db_update) {
      const char* bad = !o.epsSweep.empty() ? "--eps-sweep" : o.kdist ? "--kdist" : o.hierarchy ? "--hierarchy" : o.hasMaxPosting ? "--max-posting" : nullptr;
      if (bad) { cerr << "ERROR: --update does not go with " << bad << endl; return 1; }
      if (!o.has_input) { cerr << "ERROR: --update requires -i <input_file>" << endl; return 1; }
    }
    if (o.db_build && o.hasMaxPosting && o.maxPosting > 0) {
      cerr << "ERROR: --build does not go with --max-posting (its pruning depends on posting counts that new genomes would change)" << endl;
      return 1;
    }
    if (o.db_stats || o.db_assign || o.db_update) {
      string why;
      if (!load_dbscan_model(o.repdb_path, db_model, &why)) { cerr << "ERROR: --db " << o.repdb_path << ": " << why << endl; return 1; }
    }
    if (o.db_stats) {
      print_dbscan_model_stats(db_model, std::cout);
      std::cout.flush();
      return 0;
    }
    if (o.db_assign) {
      // -k, -s, --eps and --minpts beside --assign have no effect, as clust-mst --db --assign treats -k and -s: the model's hold
      if (o.is_fast && db_model.minhash) { cerr << "ERROR: --assign: --fast given, but " << o.repdb_path << " is a MinHash model" << endl; return 1; }
      if (o.minhash && !db_model.minhash) { cerr << "ERROR: --assign: --minhash given, but " << o.repdb_path << " is a KSSD model" << endl; return 1; }
      if (db_model.max_posting > 0) {
        cerr << "ERROR: --assign: " << o.repdb_path << " was built with --max-posting " << db_model.max_posting << ", which is out of scope" << endl;
        return 1;
      }
      if (!o.has_input) { cerr << "ERROR: --assign requires -i <input_file>" << endl; return 1; }
      o.is_fast = !db_model.minhash;
      o.minhash = db_model.minhash;
      o.epsSweep.clear(); o.kdist = o.hierarchy = o.hasMinClusterSize = o.isContainment = false;
      o.dbscanEps = db_model.eps; o.dbscanMinPts = db_model.min_pts;
    }
    if (o.db_update) {  // -k, -s, --eps and --minpts have no effect, as beside --assign: the model's hold
      if (o.is_fast && db_model.minhash) { cerr << "ERROR: --update: --fast given, but " << o.repdb_path << " is a MinHash model" << endl; return 1; }
      if (o.minhash && !db_model.minhash) { cerr << "ERROR: --update: --minhash given, but " << o.repdb_path << " is a KSSD model" << endl; return 1; }
      if (db_model.max_posting > 0) {
        cerr << "ERROR: --update: " << o.repdb_path << " was built with --max-posting " << db_model.max_posting << ", which is out of scope" << endl;
        return 1;
      }
      if (o.sketchByFile != db_model.sketch_by_file) {
        cerr << "ERROR: --update: " << o.repdb_path << " was built " << (db_model.sketch_by_file ? "with" : "without") << " -l, the new genomes must come the same way"
             << endl;
        return 1;
      }
      o.is_fast = !db_model.minhash;
      o.minhash = db_model.minhash;
      o.hasMinClusterSize = o.isContainment = false;
      o.dbscanEps = db_model.eps; o.dbscanMinPts = db_model.min_pts;
    }
  }
  // ---- clust-dbscan --minhash: this build's own flag, what it excludes named before any GPU context exists ----
  if (o.minhash) {
    const char* bad = o.is_fast ? "--fast (the two sketch kinds exclude each other)" : o.kdist ? "--kdist" : o.hierarchy ? "--hierarchy"
                      : o.hasMinClusterSize ? "--min-cluster-size" : o.hasMaxPosting ? "--max-posting" : o.isContainment ? "-c/--containment" : nullptr;
    if (bad) { cerr << "ERROR: --minhash does not go with " << bad << endl; return 1; }
    vector<double> all = o.epsSweep;
    all.push_back(o.dbscanEps);
    for (double e : all)
      if (!(e >= 0.0 && e < 1.0)) { cerr << "ERROR: --minhash needs 0 <= eps < 1, got " << e << endl; return 1; }
  }
  // ---- clust-dbscan --hierarchy: this build's own flags, checked before anything of the reference's ----
  if (o.hasMinClusterSize && !o.hierarchy) { cerr << "ERROR: --min-cluster-size needs --hierarchy" << endl; return 1; }
  if (o.hierarchy && !o.hasMinClusterSize) o.minClusterSize = o.dbscanMinPts;
  if (o.hierarchy && o.minClusterSize < 2) {
    cerr << "ERROR: --min-cluster-size must be >= 2, got " << o.minClusterSize << (o.hasMinClusterSize ? "" : " (from --minpts)") << endl;
    return 1;
  }
  // ---- clust-dbscan: the checks of src/main.cpp:478-517, in that order ----
  if (!o.is_fast && !o.minhash) { cerr << "ERROR: clust-dbscan requires --fast option" << endl; return 1; }
  cerr << "-----Using DBSCAN clustering" << endl;
  cerr << "-----DBSCAN parameters: eps=" << o.dbscanEps << ", minPts=" << o.dbscanMinPts;
  if (o.maxPosting > 0) cerr << ", max-posting=" << o.maxPosting;
  if (o.dbscanKnn > 0) cerr << ", knn=" << o.dbscanKnn;
  cerr << endl;
  if (!o.isSetKmer) { o.kmerSize = 19; cerr << "-----use default kmerSize: " << o.kmerSize << endl; }
  if (o.drlevel < 0 || o.drlevel > 8) { cerr << "ERROR: invalid drlevel " << o.drlevel << ", should be in [0, 8]" << endl; return 1; }
  if (o.has_append) { cerr << "ERROR: --append not supported for DBSCAN clustering" << endl; return 1; }
#endif
#if !defined(GREEDY_CLUST) && !defined(DBSCAN_CLUST)
#ifndef LEIDEN_CLUST
  // ---- --linkage complete: what it does not go with, before any GPU is asked for ----
  if (o.linkageComplete) {
    const char* bad = o.isContainment ? "-c/--containment" : !o.useIndex ? "--inverted-index=false" : o.has_append ? "--append"
                      : o.has_premsted ? "--premsted" : !o.repdb_path.empty() ? "--db" : o.dense ? "--dense"
                      : o.autoThreshold ? "--auto-threshold" : o.stability ? "--stability" : nullptr;
    if (bad) { cerr << "ERROR: --linkage does not go with " << bad << endl; return 1; }
  }
  // ---- --nj-tree / --nj-all: the same company, refused before any GPU is asked for ----
  if (o.njTree || o.njAll) {
    const char* bad = o.isContainment ? "-c/--containment" : !o.useIndex ? "--inverted-index=false" : o.has_append ? "--append"
                      : o.has_premsted ? "--premsted" : !o.repdb_path.empty() ? "--db" : o.dense ? "--dense"
                      : o.autoThreshold ? "--auto-threshold" : o.stability ? "--stability" : nullptr;
    if (bad) { cerr << "ERROR: " << (o.njTree ? "--nj-tree" : "--nj-all") << " does not go with " << bad << endl; return 1; }
  }
  // ---- --nj-support / --nj-seed: what they need, before any GPU is asked for ----
  if (o.has_njSupport && !(o.njTree || o.njAll)) { cerr << "ERROR: --nj-support needs --nj-tree or --nj-all" << endl; return 1; }
  if (o.has_njSupport && (o.njSupport < 1 || o.njSupport > 256)) { cerr << "ERROR: --nj-support must lie in 1 .. 256, not " << o.njSupport << endl; return 1; }
  if (o.has_njSeed && !o.has_njSupport) { cerr << "ERROR: --nj-seed needs --nj-support" << endl; return 1; }
  // ---- --quality: the same company again ----
  if (o.quality) {
    const char* bad = o.isContainment ? "-c/--containment" : !o.useIndex ? "--inverted-index=false" : o.has_append ? "--append"
                      : o.has_premsted ? "--premsted" : !o.repdb_path.empty() ? "--db" : o.dense ? "--dense"
                      : o.autoThreshold ? "--auto-threshold" : o.stability ? "--stability" : nullptr;
    if (bad) { cerr << "ERROR: --quality does not go with " << bad << endl; return 1; }
  }
  // ---- --cluster-support / --support-seed: the same company, and what they need ----
  if (o.has_clusterSupport) {
    const char* bad = o.isContainment ? "-c/--containment" : !o.useIndex ? "--inverted-index=false" : o.has_append ? "--append"
                      : o.has_premsted ? "--premsted" : !o.repdb_path.empty() ? "--db" : o.dense ? "--dense"
                      : o.autoThreshold ? "--auto-threshold" : o.stability ? "--stability" : nullptr;
    if (bad) { cerr << "ERROR: --cluster-support does not go with " << bad << endl; return 1; }
    if (o.clusterSupport < 1 || o.clusterSupport > 256) { cerr << "ERROR: --cluster-support must lie in 1 .. 256, not " << o.clusterSupport << endl; return 1; }
  }
  if (o.has_supportSeed && !o.has_clusterSupport) { cerr << "ERROR: --support-seed needs --cluster-support" << endl; return 1; }
  // ---- --upgma: and again ----
  if (o.upgma) {
    const char* bad = o.isContainment ? "-c/--containment" : !o.useIndex ? "--inverted-index=false" : o.has_append ? "--append"
                      : o.has_premsted ? "--premsted" : !o.repdb_path.empty() ? "--db" : o.dense ? "--dense"
                      : o.autoThreshold ? "--auto-threshold" : o.stability ? "--stability" : nullptr;
    if (bad) { cerr << "ERROR: --upgma does not go with " << bad << endl; return 1; }
  }
  // ---- --pangenome / --pan-soft / --pan-cloud: the same company, and what they need ----
  if (o.pangenome) {
    const char* bad = o.isContainment ? "-c/--containment" : !o.useIndex ? "--inverted-index=false" : o.has_append ? "--append"
                      : o.has_premsted ? "--premsted" : !o.repdb_path.empty() ? "--db" : o.dense ? "--dense"
                      : o.autoThreshold ? "--auto-threshold" : o.stability ? "--stability" : nullptr;
    if (bad) { cerr << "ERROR: --pangenome does not go with " << bad << endl; return 1; }
    // a bottom-s MinHash sketch says nothing about the hashes above its own cut
    if (!o.is_fast) { cerr << "ERROR: --pangenome needs --fast (KSSD sketches)" << endl; return 1; }
    if (!(1 <= o.panCloud && o.panCloud <= o.panSoft && o.panSoft <= 100)) {
      cerr << "ERROR: --pan-soft and --pan-cloud must satisfy 1 <= cloud <= soft <= 100, not soft " << o.panSoft << " and cloud " << o.panCloud << endl;
      return 1;
    }
  } else if (o.has_panSoft || o.has_panCloud) {
    cerr << "ERROR: " << (o.has_panSoft ? "--pan-soft" : "--pan-cloud") << " needs --pangenome" << endl;
    return 1;
  }
#endif
  // ---- MST RepDB mode: --db FILE (src/main.cpp:213-254, :525-600) ----
  if (o.has_topk && !o.db_query) { cerr << "ERROR: --top-k requires --query" << endl; return 1; }
  const bool db_action = o.db_build || o.db_query || o.db_assign || o.db_stats;
  if (db_action && o.repdb_path.empty()) { cerr << "ERROR: --build / --query / --assign / --stats require --db" << endl; return 1; }
  if ((int)o.db_build + (int)o.db_query + (int)o.db_assign + (int)o.db_stats > 1) { cerr << "ERROR: --build, --query, --assign and --stats exclude each other" << endl; return 1; }
  // ---- --screen: what it needs and does not go with, before any GPU is asked for and before --stats prints ----
  if (o.db_screen) {
    if (o.repdb_path.empty()) { cerr << "ERROR: --screen requires --db" << endl; return 1; }
    if (!o.is_fast) { cerr << "ERROR: --screen needs --fast (a KSSD database)" << endl; return 1; }
    const char* bad = o.db_build ? "--build" : o.db_query ? "--query" : o.db_assign ? "--assign" : o.db_stats ? "--stats" : o.has_append ? "--append" : nullptr;
    if (bad) { cerr << "ERROR: --screen does not go with " << bad << endl; return 1; }
    if (!o.has_input) { cerr << "ERROR: --screen requires -i <input_file>" << endl; return 1; }
    char* end = nullptr;
    const double c = strtod(o.minContainment.c_str(), &end);
    if (o.minContainment.empty() || *end != 0 || !(c >= 0.0 && c <= 1.0)) { cerr << "ERROR: --min-containment must be in [0, 1]" << endl; return 1; }
    if (atoll(o.minShared.c_str()) < 1) { cerr << "ERROR: --min-shared must be at least 1" << endl; return 1; }
    if (atoll(o.minUnique.c_str()) < 1) { cerr << "ERROR: --min-unique must be at least 1" << endl; return 1; }
  } else if (o.screenOnly) { cerr << "ERROR: " << o.screenOnly << " needs --screen" << endl; return 1; }
  if (!o.repdb_path.empty()) {
    if (o.db_stats) {  // mst_repdb_stats[_fast]: before any GPU context
      MstState st;
      if (!load_mst_state(o.repdb_path, o.is_fast, st)) { cerr << "ERROR: failed to load MST RepDB from: " << o.repdb_path << endl; return 1; }
      print_mst_state_stats(st, std::cout);
      std::cout.flush();
      return 0;
    }
    if (o.db_build && !o.has_presketched && !o.has_input) { cerr << "ERROR: --build requires --presketched <folder> or -i <genome_list> -l" << endl; return 1; }
    if (o.db_query && !o.has_input) { cerr << "ERROR: --query requires -i <input_file>" << endl; return 1; }
    if (o.db_assign && !o.has_input) { cerr << "ERROR: --assign requires -i <input_file>" << endl; return 1; }
    if (!db_action && !o.has_append && !o.db_screen) { cerr << "ERROR: --db requires one of: --build, --query, --assign, --append, --stats" << endl; return 1; }
    if (o.db_build && !o.has_presketched && !o.sketchByFile) unsupported("single-FASTA input (run with -l and a genome list)");
    // the tree writers, --dense and the post-processing flags have no effect here; the build keeps no sketch folder
    // (isSave = false) and takes -k or 21, -s or 1000, without the tuner
    o.newick = o.phylip = o.nexus = o.linkage = o.dense = o.autoThreshold = o.stability = o.saveRep = false;
    o.dedupDist = -1.0; o.repsPerCluster = 0; o.useIndex = true;
    if (o.db_build && !o.has_presketched) {
      o.noSave = true;
      if (!o.isSetKmer) { o.kmerSize = 21; cerr << "-----use default kmerSize: " << o.kmerSize << endl; }
      if (!o.is_fast && !o.isJaccard) o.sketchSize = 1000;
    }
  }
  // ---- --premsted: no sketching, no GPU (clust_from_mst[_fast], src/sub_command.cpp:1760-1934) ----
  if (o.has_append && o.has_input) { cerr << "ERROR: --append and -i/--input exclude each other" << endl; return 1; }
  if (o.has_append && !o.has_presketched && !o.has_premsted && o.repdb_path.empty()) { cerr << "ERROR option --append, option --presketched or --premsted needed" << endl; return 1; }
  if (o.has_premsted && !o.has_append) {
    vector<GenomeInfo> genomes; vector<rtc_edge> mst; bool byFile = true;
    if (!load_genome_info(o.folder_path, "mst", genomes, o.is_fast, byFile)) return 1;
    if (!load_mst(o.folder_path, mst)) return 1;
    write_trees(o, genomes, mst, byFile);
    // clust_from_mst (src/sub_command.cpp:1852-1893) runs the edge-length analysis; clust_from_mst_fast (--fast, :1760-1822)
    // has none, so there the two flags have no effect
    if (!o.is_fast && o.autoThreshold) auto_threshold_report(mst, (int)genomes.size(), o.outputFile, 0.05, o.stability);
    else if (!o.is_fast && o.stability) stability_report(mst, (int)genomes.size(), o.threshold);
    cluster_from_mst(mst, genomes, byFile, o.outputFile, o.threshold);
    if (o.dense) {  // clust_from_mst with !no_dense: the stored mst.dense drives the noise pass (src/sub_command.cpp:1795-1822)
      vector<int32_t> dense; int span = 0, gn = 0;
      if (!load_dense(o.folder_path, dense, span, gn) || gn != (int)genomes.size()) return 1;
      remove_noise_and_print(mst, genomes, byFile, o.outputFile, o.threshold, dense, span);
    }
    return 0;
  }
#endif

  // ---- GPUs: one context (and one host thread when it works) per device; RCCL communicators among them ----
  // The HIP runtime, the contexts and the communicators come up on a thread of their own (0.05-0.24 s): a run from a genome
  // list reads the list, sizes its slots and PARSES ITS FIRST BATCH meanwhile (sketch_files); every other flow waits here.
  vector<Gpu> gpus;
  auto init_gpus = [&]() -> int {
    string spec = o.gpus.empty() ? (getenv("RTC_GPUS") ? getenv("RTC_GPUS") : "all") : o.gpus;
    const int ndev = rtc_device_count();
    bool gpus_by_default = false, single_gpu_flow = false;
    vector<int> devs;
    // Sketching from genome files spreads over every GPU of the choice in every flow (lanes on all of them, the rows
    // shared afterwards); of the clustering steps only the row-sharded MST does.  Greedy clustering has a serial
    // dependency on the representative set, --dense / --inverted-index=false evaluate their pairs on one GPU: those
    // cluster on the first GPU.  Flows that sketch little or nothing here (--presketched, --append, --db) take the first
    // GPU of the choice alone and never open a communicator.
    single_gpu_flow =
#ifdef GREEDY_CLUST
        o.has_append || !o.repdb_path.empty() || o.has_presketched;
#elif defined(DBSCAN_CLUST)
        o.has_presketched || o.db_assign || o.db_update;
#else
        o.has_append || ((o.dense || !o.useIndex) && o.has_presketched) || !o.repdb_path.empty();
#endif
    if (spec == "all") { gpus_by_default = true; for (int d = 0; d < ndev; d++) devs.push_back(d); }
    else if (spec.find(',') == string::npos && atoi(spec.c_str()) > 0 && spec.find_first_not_of("0123456789") == string::npos) {
      const int want = atoi(spec.c_str());
      if (want > ndev) { fprintf(stderr, "ERROR: --gpus %d but only %d GPU(s) are visible\n", want, ndev); return 1; }
      for (int d = 0; d < want; d++) devs.push_back(d);
    } else {
      size_t p0 = 0;
      while (p0 <= spec.size()) { size_t p1 = spec.find(',', p0); if (p1 == string::npos) p1 = spec.size(); if (p1 > p0) devs.push_back(atoi(spec.substr(p0, p1 - p0).c_str())); p0 = p1 + 1; }
    }
    if (single_gpu_flow && devs.size() > 1) {
      if (!gpus_by_default) fprintf(stderr, "-----this flow runs on one GPU: using GPU %d of the %zu named\n", devs[0], devs.size());
      devs.resize(1);
    }
    if (devs.empty()) { fprintf(stderr, "ERROR: no MI355X context: %s (%d devices)\n", rtc_last_error(nullptr), ndev); return 1; }
    gpus.resize(devs.size());
    vector<rtc_ctx*> ctxs;
    for (size_t g = 0; g < devs.size(); g++) {
      gpus[g].device = devs[g];
      int st = rtc_ctx_create(devs[g], &gpus[g].ctx);
      if (st != RTC_OK) { fprintf(stderr, "ERROR: no MI355X context on device %d: %s\n", devs[g], rtc_last_error(nullptr)); return 1; }
      ctxs.push_back(gpus[g].ctx);
    }
    // RTC_COMM_FORCE_RCCL=1 opens an RCCL communicator also for ONE GPU and sends the run through the share step and
    // rtc_mst_sharded: the loader and every collective of the multi-GPU path, driven from this binary on a one-GPU box
    if (gpus.size() > 1 || (getenv("RTC_COMM_FORCE_RCCL") && !single_gpu_flow)) {
      vector<rtc_comm*> comms(gpus.size(), nullptr);
      const int st = rtc_comm_init_all(ctxs.data(), (int)ctxs.size(), comms.data());
      if (st != RTC_OK) {
        // the default ("all") must not turn a missing or broken RCCL into a dead command line: one GPU does the whole
        // job, as it would on a one-GPU host.  A user who named several GPUs asked for them: that is an error.
        if (!gpus_by_default) { fprintf(stderr, "ERROR: rtc_comm_init_all failed (%d): %s\n", st, rtc_last_error(ctxs[0])); return 1; }
        fprintf(stderr, "Warning: no communicator among the %zu visible GPU(s) (%s); running on GPU %d alone\n", gpus.size(), rtc_last_error(ctxs[0]), gpus[0].device);
        for (size_t g = 1; g < gpus.size(); g++) rtc_ctx_destroy(gpus[g].ctx);
        gpus.resize(1);
      } else {
        for (size_t g = 0; g < gpus.size(); g++) gpus[g].comm = comms[g];
        fprintf(stderr, "-----use %zu GPUs (%s exchange)\n", gpus.size(), rtc_comm_backend(comms[0]));
      }
    }
    return 0;
  };
  int gpu_rc = 0;
  double t_gpus = 0;
  std::atomic<bool> gpus_done{false};
  std::thread gpu_thread([&]() { gpu_rc = init_gpus(); t_gpus = get_sec(); gpus_done.store(true, std::memory_order_release); });
  // whichever way this function is left before the GPUs were asked for (return, exit()): not with that thread inside HIP
  g_gpu_thread = &gpu_thread;
  atexit([]() { if (g_gpu_thread && g_gpu_thread->joinable()) g_gpu_thread->join(); });
  struct GpuJoin { std::thread& t; ~GpuJoin() { if (t.joinable()) t.join(); g_gpu_thread = nullptr; } } gpu_join{gpu_thread};
  rtc_ctx* ctx = nullptr;
  struct Joiner { ~Joiner() { join_warmup(); } } warm;
  bool gpus_up = false;
  const std::function<void()> wait_gpus = [&]() {
    if (gpus_up) return;
    const double t_asked = get_sec();
    gpu_thread.join();
    gpus_up = true;
    if (gpu_rc != 0) { fflush(nullptr); _exit(gpu_rc); }
    ctx = gpus[0].ctx;
    g_metrics.num("hip_init_s", t_gpus - t_main);
    g_metrics.num("hip_init_exposed_s", std::max(0.0, t_gpus - t_asked));  // what the main thread still had to wait for
    if (getenv("RTC_VERBOSE")) fprintf(stderr, "[ctx]   HIP runtime + %zu GPU context(s) in %.3fs (asked for at t+%.3fs, waited %.3fs)\n", gpus.size(),
                                       t_gpus - t_main, t_asked - t_main, std::max(0.0, t_gpus - t_asked));
    // The device code of the pair / MST / greedy phases is mapped at its first launch (~27 ms): a helper thread does
    // that with a toy clustering while this one reads and sketches (rtc_warmup; RTC_NO_WARMUP=1 leaves it out).
    if (!getenv("RTC_NO_WARMUP")) {
      std::vector<int> wdev;
      for (const Gpu& g : gpus) wdev.push_back(g.device);
      g_warmup_thread = std::thread([wdev]() { for (int d : wdev) (void)rtc_warmup(d); });
    }
  };
  const bool list_run = !o.has_presketched && !o.has_append && o.has_input && o.sketchByFile
#if defined(GREEDY_CLUST) || defined(DBSCAN_CLUST)
                        && o.repdb_path.empty()
#else
                        && (o.repdb_path.empty() || o.db_build)
#endif
      ;
  const GpusReady gpus_ready{wait_gpus, &gpus_done};
  if (!list_run) wait_gpus();
  Resident rs;
#if !defined(GREEDY_CLUST) && !defined(DBSCAN_CLUST)
  if (!o.repdb_path.empty() && !o.db_build) {  // --build goes on through the MST flow below
    const int rc = o.db_screen ? mst_db_screen(o, gpus) : (o.db_query || o.db_assign) ? mst_db_search(o, gpus) : mst_db_append(o, gpus);
    g_metrics.str("command", "clust-mst");
    g_metrics.str("sketch", o.is_fast ? "kssd" : "minhash");
    g_metrics.write();
    for (Gpu& g : gpus) { if (g.comm) rtc_comm_destroy(g.comm); }
    for (Gpu& g : gpus) rtc_ctx_destroy(g.ctx);
    return rc;
  }
  if (o.has_append) return append_clust_mst(o, gpus);
#elif defined(GREEDY_CLUST)
  if (!o.repdb_path.empty()) {
    const int rc = o.db_build ? (o.is_fast ? repdb_build(o, gpus) : mh_repdb_build(o, gpus)) : o.db_query ? repdb_query(o, gpus) : o.db_assign ? repdb_assign(o, gpus) : repdb_append(o, gpus);
    for (Gpu& g : gpus) { if (g.comm) rtc_comm_destroy(g.comm); }
    for (Gpu& g : gpus) rtc_ctx_destroy(g.ctx);
    return rc;
  }
  if (o.has_append) {  // src/main.cpp:378-387
    const int rc = o.is_fast ? append_clust_greedy_fast(o, gpus) : append_clust_greedy(o, gpus);
    for (Gpu& g : gpus) { if (g.comm) rtc_comm_destroy(g.comm); }
    for (Gpu& g : gpus) rtc_ctx_destroy(g.ctx);
    return rc;
  }
#elif defined(LEIDEN_CLUST)
  if (o.db_assign) {
    const int rc = leiden_db_assign(o, gpus, ld_model);
    g_metrics.str("command", "clust-leiden");
    g_metrics.str("sketch", "kssd");
    g_metrics.write();
    for (Gpu& g : gpus) { if (g.comm) rtc_comm_destroy(g.comm); }
    for (Gpu& g : gpus) rtc_ctx_destroy(g.ctx);
    return rc;
  }
#else
  if (o.db_assign || o.db_update) {
    const int rc = o.db_assign ? dbscan_db_assign(o, gpus, db_model) : dbscan_db_update(o, gpus, db_model);
    g_metrics.str("command", "clust-dbscan");
    g_metrics.str("sketch", db_model.minhash ? "minhash" : "kssd");
    g_metrics.write();
    for (Gpu& g : gpus) { if (g.comm) rtc_comm_destroy(g.comm); }
    for (Gpu& g : gpus) rtc_ctx_destroy(g.ctx);
    return rc;
  }
#endif

  vector<GenomeInfo> genomes;
  MinHashSketchFile mh; KssdSketchFile ks;
  bool sketchByFile = true;
  string folder_path = o.folder_path;
  const bool from_sketches = o.has_presketched;
  bool greedy =
#ifdef GREEDY_CLUST
      true;
#else
      false;
#endif
  const bool dbscan =
#ifdef DBSCAN_CLUST
      true;
#else
      false;
#endif
  [[maybe_unused]] bool dbscan_format_mismatch = false;

  double t0 = get_sec();
  if (from_sketches) {
    if (o.is_fast) { if (!load_kssd_sketches(folder_path, genomes, ks, sketchByFile)) return 1; }
    else { if (!load_minhash_sketches(folder_path, genomes, mh, sketchByFile)) return 1; }
#if defined(DBSCAN_CLUST) && !defined(LEIDEN_CLUST)
    // clust_from_sketch_dbscan prints with the -l of the command line, not the one stored with the sketches (:3237-3240)
    if (sketchByFile != o.sketchByFile) { cerr << "Warning: sketch format mismatch" << endl; dbscan_format_mismatch = true; }
    sketchByFile = o.sketchByFile;
#endif
    cerr << "-----the size of sketches is: " << genomes.size() << endl;
    cerr << "========time of load genome Infos and sketch Infos is: " << get_sec() - t0 << endl;
  } else {
    if (!o.has_input) { cerr << "ERROR: -i/--input is required" << endl; return 1; }
    sketchByFile = o.sketchByFile;
    uint64_t maxSize, minSize, averageSize;
    vector<FastaRecord> seq_recs;
    if (o.sketchByFile) { if (!cal_size(o.inputFile, o.minLen, maxSize, minSize, averageSize)) return 1; }
    else {
      SeqModeSizes sz;
      if (!read_sequences(o.inputFile, o.minLen, seq_recs, sz)) return 1;
      maxSize = sz.maxSize; minSize = sz.minSize; averageSize = sz.totalSize / sz.number;
    }
    // main.cpp:632 (clust-mst --fast uses the kssd tuner) / :659 (everything else)
    if (o.db_build && !dbscan) { /* mst_repdb_build_from_genome[_fast]: the parameters as given, no tuner */ }
    else if (o.is_fast && !greedy) { if (!tune_kssd_parameters(o.isSetKmer, maxSize, minSize, averageSize, o.isContainment, o.kmerSize, o.threshold, o.drlevel)) return 1; }
    else if (!tune_parameters(greedy, o.isSetKmer, maxSize, minSize, averageSize, o.isContainment, o.isJaccard, o.kmerSize, o.threshold, o.containCompress, o.sketchSize)) return 1;
    SketchJob job;
    job.kssd = o.is_fast; job.kmerSize = o.kmerSize; job.sketchSize = o.sketchSize; job.isContainment = o.isContainment;
    job.containCompress = o.containCompress; job.drlevel = o.drlevel; job.minLen = o.minLen; job.threads = o.threads;
    if (getenv("RTC_VERBOSE")) fprintf(stderr, "[tune]  cal_size + tune_parameters in %.3fs\n", get_sec() - t0);
    if (o.sketchByFile) sketch_files(gpus, o.inputFile, job, genomes, &mh, &ks, rs, !o.noSave || o.db_build, &gpus_ready);
    else { wait_gpus(); sketch_sequences(gpus, seq_recs, job, genomes, &mh, &ks); }
    wait_gpus();
    mh.kmerSize = o.kmerSize; mh.isContainment = o.isContainment; mh.containCompress = o.containCompress; mh.sketchSize = o.sketchSize;
    cerr << "-----the size of sketches (number of genomes or sequences) is: " << genomes.size() << endl;
    double t1 = get_sec();
    cerr << "========time of computing sketch is: " << t1 - t0 << "========" << endl;
    {
      uint64_t bases = 0;
      for (const GenomeInfo& gi : genomes) bases += o.sketchByFile ? gi.totalSeqLength : (uint64_t)gi.seq0.length;
      g_metrics.num("computing_sketch_s", t1 - t0);
      g_metrics.num("bases", (double)bases);
      g_metrics.num("sketch_gbp_per_s", (double)bases / (t1 - t0) / 1e9);
    }
    folder_path = current_date_time();
    if (!o.noSave) {
      string command = "mkdir -p " + folder_path;
      if (system(command.c_str()) != 0) { cerr << "ERROR: cannot create " << folder_path << endl; return 1; }
      // compute_kssd_sketches (clust-dbscan, src/sub_command.cpp:2154-2188) keeps the sketches alone
      if (o.is_fast) { save_kssd_sketches(genomes, ks, folder_path, sketchByFile); if (!greedy && !dbscan) save_kssd_index(ks, folder_path); }
      else { save_minhash_sketches(genomes, mh, folder_path, sketchByFile); save_minhash_index(mh, folder_path); }
      cerr << "========time of saveSketches is: " << get_sec() - t1 << "========" << endl;
      g_metrics.num("saveSketches_s", get_sec() - t1);
    }
  }
  if (genomes.empty()) { cerr << "ERROR: no genome to cluster" << endl; return 1; }
  // clust-dbscan from genomes takes the tuned / given k, from a sketch folder half_k * 2 (src/sub_command.cpp:3247, :3278)
  const int kmer_size = (dbscan && !from_sketches) ? o.kmerSize : o.is_fast ? ks.info.half_k * 2 : mh.kmerSize;

  double t2 = get_sec();
#ifdef GREEDY_CLUST
  // ---- clust-greedy: compute_clusters GREEDY branch (src/sub_command.cpp:2894-2922, :1963-1986) ----
  vector<uint32_t> size_cfg, kssd_order;
  if (o.is_fast) {
    // src/greedy.cpp:594-597: sort by hash count, descending, comparator without tie-break
    vector<size_t> perm(genomes.size());
    iota(perm.begin(), perm.end(), 0);
    auto cnt = [&](size_t i) { return rs.ok ? (size_t)rs.counts[i] : (ks.use64 ? ks.h64[i].size() : ks.h32[i].size()); };
    struct Item { size_t idx; size_t c; };
    vector<Item> items(genomes.size());
    for (size_t i = 0; i < items.size(); i++) items[i] = Item{i, cnt(i)};
    std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.c > b.c; });
    vector<GenomeInfo> g2; KssdSketchFile k2; k2.info = ks.info; k2.use64 = ks.use64;
    for (const Item& it : items) {
      g2.push_back(genomes[it.idx]);
      kssd_order.push_back((uint32_t)it.idx);  // resident rows are addressed through this order, not moved
      if (!rs.ok || (o.saveRep && !o.noSave)) { if (ks.use64) k2.h64.push_back(ks.h64[it.idx]); else k2.h32.push_back(ks.h32[it.idx]); }
    }
    genomes.swap(g2); ks = std::move(k2);
  } else {
    if (from_sketches) {
      // clust_from_sketches GREEDY branch: sort by genome size desc, id asc (src/sub_command.cpp:2657-2660)
      vector<size_t> perm(genomes.size());
      iota(perm.begin(), perm.end(), 0);
      std::sort(perm.begin(), perm.end(), [&](size_t a, size_t b) {
        if (!sketchByFile) {  // cmpSeqSize (src/SketchInfo.cpp:54-58)
          if (genomes[a].seq0.length != genomes[b].seq0.length) return genomes[a].seq0.length > genomes[b].seq0.length;
          return genomes[a].id < genomes[b].id;
        }
        if (genomes[a].totalSeqLength != genomes[b].totalSeqLength) return genomes[a].totalSeqLength > genomes[b].totalSeqLength;
        return genomes[a].id < genomes[b].id;
      });
      vector<GenomeInfo> g2; vector<vector<uint64_t>> h2;
      for (size_t p : perm) { g2.push_back(genomes[p]); h2.push_back(mh.hashes[p]); }
      genomes.swap(g2); mh.hashes.swap(h2);
      // loadSketches builds MinHash(k, containCompress) in containment mode, so getSketchSize() reports
      // containCompress there (src/Sketch_IO.cpp:334); fixed mode reports sketchSize
      size_cfg.assign(genomes.size(), mh.isContainment ? (uint32_t)mh.containCompress : (uint32_t)mh.sketchSize);
    } else {
      size_cfg.resize(genomes.size());
      for (size_t i = 0; i < genomes.size(); i++)
        size_cfg[i] = !mh.isContainment ? (uint32_t)mh.sketchSize
                      : sketchByFile ? (uint32_t)std::max(file_length_for_containment(genomes[i].fileName) / mh.containCompress, 100)
                                     : (uint32_t)std::max(genomes[i].seq0.length / mh.containCompress, 100);
    }
  }
  // greedy has a serial dependency on the representative set: one GPU clusters (replicas only)
  DeviceSketches ds;
  if (rs.ok) resident_sketches(ctx, gpus[0], rs, o.is_fast ? &kssd_order : nullptr, ds);
  else if (o.is_fast) upload_sketches(ctx, ks.use64 ? &ks.h64 : nullptr, ks.use64 ? nullptr : &ks.h32, ds);
  else upload_sketches(ctx, &mh.hashes, nullptr, ds);
  vector<int32_t> rep_of(genomes.size());
  uint32_t ncl = 0;
  if (o.orderDegree) {
    // --order degree: the genomes keep the numbering of the size sort above, the clustering is include/rtclust.h's
    // (rtc_greedy_degree); <output>.order.tsv lists them in the order the definition walks them
    const uint32_t s_mh = o.is_fast ? 0u : size_cfg[0];
    vector<rtc_degree_place> place(genomes.size());
    CHECK(ctx, rtc_greedy_degree(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, o.is_fast ? 0 : 1, s_mh, o.threshold, kmer_size,
                                 place.data(), &ncl));
    for (size_t v = 0; v < place.size(); v++) rep_of[v] = (int32_t)place[v].rep;
    const string tsv = o.outputFile + ".order.tsv";
    FILE* fp = fopen(tsv.c_str(), "w");
    if (!fp) { cerr << "ERROR: cannot open file: " << tsv << endl; return 1; }
    vector<uint32_t> order(place.size());
    iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return place[a].degree != place[b].degree ? place[a].degree > place[b].degree : a < b; });
    auto name_of = [&](uint32_t v) -> const string& { return sketchByFile ? genomes[v].fileName : genomes[v].seq0.name; };
    fprintf(fp, "name\tdegree\trole\trepresentative\tdistance\n");
    for (uint32_t v : order) {
      const rtc_degree_place& p = place[v];
      double dist = 0.0;
      if (p.rep != v) {
        if (!o.is_fast) dist = rtc_mash_distance(p.common, p.denom, s_mh, kmer_size);
        else if (p.denom != p.common) { const double j = (double)p.common / (double)p.denom; dist = -log(2.0 * j / (1.0 + j)) / kmer_size; }
      }
      fprintf(fp, "%s\t%u\t%s\t%s\t%.6f\n", name_of(v).c_str(), p.degree, p.rep == v ? "rep" : "member", name_of(p.rep).c_str(), dist);
    }
    fclose(fp);
    cerr << "-----write the processing order into: " << tsv << endl;
    uint64_t dc[12];
    if (rtc_greedy_degree_counters(ctx, dc) == RTC_OK) {
      g_metrics.num("greedy_degree_pair_s", 1e-9 * (double)(dc[7] + dc[8]));
      g_metrics.num("greedy_degree_select_s", 1e-9 * (double)dc[9]);
      g_metrics.num("greedy_degree_assign_s", 1e-9 * (double)dc[10]);
      g_metrics.num("greedy_degree_rounds", (double)(dc[5] & 0xffffffffull));
      g_metrics.num("greedy_degree_edges", (double)dc[3]);
    }
  } else if (!o.is_fast && !o.useIndex)  // greedyCluster: every representative, MinHash::distance() (src/sub_command.cpp:2683,2914)
    CHECK(ctx, rtc_greedy_mash(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, kmer_size, (int)mh.isContainment, size_cfg[0], o.threshold,
                               rep_of.data(), &ncl));
  else
    CHECK(ctx, rtc_greedy(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, o.is_fast ? nullptr : size_cfg.data(), kmer_size,
                          o.is_fast ? 0 : (int)mh.isContainment, o.is_fast ? 1 : 0, o.threshold, rep_of.data(), &ncl));
  vector<vector<int>> cluster = clusters_from_rep_of(rep_of);
  if (!o.is_fast && o.useIndex && o.saveRep && (from_sketches || !o.noSave)) {
    // MinHashInitialClusterWithState + save (src/sub_command.cpp:2673-2679, :2904-2909; src/greedy.cpp:1904-1960)
    KssdClusterState st;
    st.minhash = true; st.threshold = o.threshold; st.kmer_size = kmer_size; st.sketch_size = (int)size_cfg[0]; st.is_containment = mh.isContainment;
    st.genomes = genomes; st.sk.use64 = true; st.sk.h64 = mh.hashes; st.clusters = cluster; st.reps.use64 = true;
    cerr << "Building inverted index from " << cluster.size() << " representatives..." << endl;
    for (const auto& c : cluster) if (!c.empty()) { st.rep_ids.push_back(c[0]); st.rep_genomes.push_back(genomes[c[0]]); st.reps.h64.push_back(mh.hashes[c[0]]); }
    const string state_file = folder_path + "/cluster_state.bin";
    if (!save_minhash_cluster_state(state_file, st)) return 1;
    cerr << "-----saved cluster state (with inverted index) to: " << state_file << endl;
  }
  if (o.is_fast && o.saveRep && !o.noSave && !from_sketches) {  // compute_kssd_clusters, src/sub_command.cpp:1962-1967
    KssdClusterState st;
    KssdParameters info = ks.info;
    info.genomeNumber = (int)genomes.size();
    fill_cluster_state(st, o.threshold, kmer_size, info, genomes, ks, cluster);
    const string state_file = folder_path + "/cluster_state.bin";
    if (!save_kssd_cluster_state(state_file, st)) return 1;
    cerr << "-----saved cluster state (with inverted index) to: " << state_file << endl;
  }
  print_result(cluster, genomes, sketchByFile, o.outputFile);
  cerr << "-----write the cluster result into: " << o.outputFile << endl;
  cerr << "-----the cluster number of " << o.outputFile << " is: " << cluster.size() << endl;
  cerr << "========time of greedyCluster is: " << get_sec() - t2 << "========" << endl;
  g_metrics.num("greedyCluster_s", get_sec() - t2);
  g_metrics.num("clusters", (double)cluster.size());
#elif defined(LEIDEN_CLUST)
  // ---- clust-leiden --louvain: the graph of KssdLeidenCluster (src/leiden.cpp:168-293) and the library's Louvain on the first
  // GPU, printKssdResult with the clusters in label order ----
  const uint32_t n_nodes = (uint32_t)genomes.size();
  vector<rtc_wedge> wedges;
  vector<double> weights;
  if (o.has_pregraph) {
    if (pregraph_nodes != n_nodes) {
      cerr << "ERROR: --pregraph " << folder_path << ": leiden.graph has " << pregraph_nodes << " nodes, the folder " << n_nodes << " sketches" << endl;
      return 1;
    }
    wedges.swap(pregraph);
    weights.swap(pregraph_weights);
    cerr << "-----Loaded graph: " << n_nodes << " nodes, " << wedges.size() << " edges" << endl;
  } else {
    if (o.minhash && mh.isContainment) { cerr << "ERROR: --minhash: " << folder_path << " holds containment sketches (-c), which are out of scope" << endl; return 1; }
    DeviceSketches ds;
    if (rs.ok) resident_sketches(ctx, gpus[0], rs, nullptr, ds);
    else if (o.minhash) upload_sketches(ctx, &mh.hashes, nullptr, ds);
    else upload_sketches(ctx, ks.use64 ? &ks.h64 : nullptr, ks.use64 ? nullptr : &ks.h32, ds);
    cerr << "-----Building similarity graph" << (o.minhash ? " (MinHash)" : "") << "..." << endl;
    vector<rtc_gedge> edges((size_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_nodes * (uint64_t)o.knn, (uint64_t)16 * n_nodes)));
    uint64_t n_edges = 0;
    auto build = [&]() {  // --minhash: the edge rule and the rank on MinHash::distance()'s (common, denom)
      return o.minhash ? rtc_graph_build_mash(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, (uint32_t)mh.sketchSize, o.threshold, kmer_size,
                                              (uint32_t)o.knn, edges.data(), edges.size(), &n_edges)
                       : rtc_graph_build(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, o.threshold, kmer_size, (uint32_t)o.knn, edges.data(),
                                         edges.size(), &n_edges);
    };
    int st = build();
    if (st == RTC_ERR_OVERFLOW) {  // the count is known now
      edges.resize(n_edges);
      st = build();
    }
    CHECK(ctx, st);
    edges.resize(n_edges);
    uint64_t gc[10] = {0};
    rtc_graph_counters(ctx, gc);
    cerr << "-----Comparisons: " << gc[1] << endl;
    cerr << "-----Edges created: " << n_edges << endl;
    if (getenv("RTC_VERBOSE") && o.minhash)
      fprintf(stderr, "[minhash] %llu candidate edges in %llu chunk(s), %llu merged, %llu passing, %llu edges; pair %.3f ms, filter + merge %.3f ms, "
              "select %.3f ms\n", (unsigned long long)gc[1], (unsigned long long)gc[0], (unsigned long long)gc[8], (unsigned long long)gc[2],
              (unsigned long long)gc[3], gc[5] / 1e6, gc[6] / 1e6, gc[7] / 1e6);
    vector<uint32_t> sizes(n_nodes);
    CHECK(ctx, rtc_copy_d2h(ctx, sizes.data(), ds.d_len, (size_t)n_nodes * 4));
    weights.resize(n_edges);
    wedges.resize(n_edges);
    for (uint64_t e = 0; e < n_edges; e++) {
      weights[e] = o.minhash ? rtc_graph_weight_mash(edges[e].common, edges[e].pad, (uint32_t)mh.sketchSize, kmer_size)
                             : rtc_graph_weight(edges[e].common, sizes[edges[e].u], sizes[edges[e].v], kmer_size);
      wedges[e] = rtc_wedge{edges[e].u, edges[e].v, leiden_weight_units(weights[e])};
    }
    g_metrics.num("leiden_graph_s", gc[9] / 1e9);
    g_metrics.num("leiden_graph_merged", (double)gc[8]);
    if (o.saveGraph) {
      const string graph_file = folder_path + "/leiden.graph";
      if (!save_leiden_graph(graph_file, n_nodes, edges, weights)) return 1;
      cerr << "-----Graph saved to: " << graph_file << endl;
    }
  }
  uint64_t snn_c[10] = {0}, snn_pruned = 0;
  if (o.snn) {
    // --snn: every record's weight becomes the shared-neighbour weight of its edge, before anything is quantised; the graph
    // saved above stays the similarity graph.  A record of a vertex with itself (a --pregraph file may hold one) keeps its own.
    vector<rtc_snn> sn(wedges.size());
    CHECK(ctx, rtc_graph_snn(ctx, n_nodes, wedges.data(), wedges.size(), sn.data()));
    rtc_graph_snn_counters(ctx, snn_c);
    size_t kept = 0;
    double w_lo = 0.0, w_hi = 0.0;
    for (size_t e = 0; e < wedges.size(); e++) {
      const double w = (sn[e].flags & 1u) ? weights[e] : rtc_snn_weight(sn[e].shared, sn[e].deg_u, sn[e].deg_v);
      if (w < snn_prune) { snn_pruned++; continue; }  // one pass: the dropped edge counted in the neighbourhoods
      w_lo = kept ? std::min(w_lo, w) : w;
      w_hi = kept ? std::max(w_hi, w) : w;
      wedges[kept] = rtc_wedge{wedges[e].u, wedges[e].v, leiden_weight_units(w)};
      weights[kept++] = w;
    }
    wedges.resize(kept);
    weights.resize(kept);
    cerr << "-----SNN: " << snn_c[1] << " edge(s), " << snn_c[2] << " triangle(s), " << snn_pruned << " pruned, weights [" << w_lo << ", " << w_hi << "]" << endl;
  }
  if (wedges.empty()) cerr << "-----Warning: No edges! Each sequence in its own cluster." << endl;
  vector<int32_t> labels(n_nodes);
  uint32_t ncl = 0;
  double modularity = 0.0;
  uint64_t lc[10] = {0};
  const size_t graph_edges = wedges.size();
  LeidenQuant quant;  // --louvain: modularity's, nothing scaled
  uint32_t mcl_its = 0;
  int mcl_converged = 0;
  if (o.mcl) {
    // --mcl: --louvain's records; the labels name a cluster by its smallest member, in rtc_louvain's cluster order
    CHECK(ctx, rtc_mcl(ctx, n_nodes, wedges.data(), wedges.size(), mcl_h, mcl_select, mcl_iterations, labels.data(), &ncl, &mcl_its, &mcl_converged,
                       nullptr, 0, nullptr));
    rtc_mcl_counters(ctx, lc);
    cerr << "-----MCL: " << mcl_its << " iteration(s), " << (mcl_converged ? "converged" : "NOT converged") << ", " << lc[3] << " attractor(s)" << endl;
    if (!mcl_converged)
      cerr << "-----Warning: MCL did not converge in " << mcl_iterations << " iteration(s) (--mcl-iterations); the clusters are those of the last matrix" << endl;
    vector<int32_t> dense(n_nodes, -1);  // cluster c of the result: the c-th smallest label
    int32_t next = 0;
    for (uint32_t x = 0; x < n_nodes; x++)
      if (labels[x] == (int32_t)x) dense[x] = next++;
    for (uint32_t x = 0; x < n_nodes; x++) labels[x] = dense[labels[x]];
  } else if (o.leiden) {
    // --leiden: q from the weights anew (CPM: normalised as src/leiden.cpp:343-366, the records at q == 0 dropped)
    const int objective = o.objective == "cpm" ? RTC_LEIDEN_CPM : RTC_LEIDEN_MODULARITY;
    vector<uint32_t> eu(graph_edges), ev(graph_edges);
    for (size_t e = 0; e < graph_edges; e++) { eu[e] = wedges[e].u; ev[e] = wedges[e].v; }
    double w_min = 0.0, w_max = 0.0;
    (void)leiden_quantiser(weights.data(), graph_edges, objective, &quant, nullptr, nullptr);  // what --db --build keeps of it
    if (leiden_quantise(eu.data(), ev.data(), weights.data(), graph_edges, objective, wedges, &w_min, &w_max))
      cerr << "-----Edge weights normalized: [" << w_min << ", " << w_max << "] -> [0, 1]" << endl;
    if (objective == RTC_LEIDEN_CPM && o.resolution >= 1.0)
      cerr << "-----Note: under --objective cpm a --resolution of 1 or more leaves every genome in its own cluster" << endl;
    CHECK(ctx, rtc_leiden(ctx, n_nodes, wedges.data(), wedges.size(), o.resolution, objective, labels.data(), &ncl, &modularity));
    rtc_leiden_counters(ctx, lc);
    cerr << "-----Leiden (" << o.objective << "): " << lc[0] << " iteration(s), " << lc[1] << " level(s), " << lc[5] << " merge(s), quality " << modularity << endl;
  } else {
    CHECK(ctx, rtc_louvain(ctx, n_nodes, wedges.data(), wedges.size(), o.resolution, labels.data(), &ncl, &modularity));
    rtc_louvain_counters(ctx, lc);
    cerr << "-----Louvain: " << lc[0] << " level(s), " << lc[1] << " round(s), modularity " << modularity << endl;
  }
  vector<vector<int>> cluster(ncl);
  for (uint32_t x = 0; x < n_nodes; x++) cluster[labels[x]].push_back((int)x);
  print_result(cluster, genomes, sketchByFile, o.outputFile);
  cerr << "-----write the cluster result into: " << o.outputFile << endl;
  cerr << "-----the cluster number of " << o.outputFile << " is: " << cluster.size() << endl;
  if (o.db_build) {  // the model: what --db --assign places new genomes into
    LeidenModel md;
    md.algorithm = o.leiden ? 1 : 0;
    md.objective = o.leiden && o.objective == "cpm" ? RTC_LEIDEN_CPM : RTC_LEIDEN_MODULARITY;
    md.width = ks.use64 ? 8 : 4; md.sketch_by_file = sketchByFile; md.kmer_size = kmer_size;
    md.half_k = ks.info.half_k; md.half_subk = ks.info.half_subk; md.drlevel = ks.info.drlevel;
    md.knn = o.knn; md.n_clusters = (int)ncl; md.min_len = o.minLen; md.threshold = o.threshold; md.resolution = o.resolution;
    md.scale = quant.scale; md.lo = quant.lo; md.range = quant.range;
    LeidenModelSums sums;
    if (!leiden_model_sums(wedges.data(), wedges.size(), labels.data(), n_nodes, ncl, sums)) { cerr << "ERROR: --build: the labels do not fit the graph" << endl; return 1; }
    md.m2 = md.objective == RTC_LEIDEN_MODULARITY ? sums.m2 : 0;
    md.tot = md.objective == RTC_LEIDEN_MODULARITY ? sums.tot : sums.size;
    md.labels = labels; md.genomes = genomes;
    if (ks.use64) md.h64 = ks.h64; else md.h32 = ks.h32;
    if ((md.width == 8 ? md.h64.size() : md.h32.size()) != genomes.size()) {
      cerr << "ERROR: --build needs the sketches on the host (" << (md.width == 8 ? md.h64.size() : md.h32.size()) << " of " << genomes.size() << ")" << endl;
      return 1;
    }
    if (!save_leiden_model(o.repdb_path, md)) return 1;
    cerr << "-----write the Leiden model (" << genomes.size() << " genomes, " << ncl << " clusters) into: " << o.repdb_path << endl;
  }
  cerr << "========time of Leiden clustering is: " << get_sec() - t2 << "========" << endl;
  g_metrics.num("leiden_louvain_s", lc[9] / 1e9);  // the clustering call, whichever algorithm
  g_metrics.num("leiden_edges", (double)graph_edges);
  if (o.snn) {
    g_metrics.num("leiden_snn_s", snn_c[9] / 1e9);
    g_metrics.num("leiden_snn_triangles", (double)snn_c[2]);
    g_metrics.num("leiden_snn_pruned", (double)snn_pruned);
  }
  if (o.mcl) {
    g_metrics.num("mcl_iterations", (double)mcl_its);
    g_metrics.num("mcl_converged", (double)mcl_converged);
    g_metrics.num("mcl_entries", (double)lc[2]);
    g_metrics.num("mcl_expand_s", lc[8] / 1e9);
  } else {
    g_metrics.num("leiden_levels", (double)(o.leiden ? lc[1] : lc[0]));
  }
  if (o.leiden) {
    g_metrics.num("leiden_refine_s", lc[8] / 1e9);
    g_metrics.num("leiden_iterations", (double)lc[0]);
    g_metrics.num("leiden_merges", (double)lc[5]);
  }
  g_metrics.num("leiden_clusters", (double)ncl);
  if (!o.mcl) g_metrics.num("leiden_modularity", modularity);
#elif defined(DBSCAN_CLUST)
  // ---- clust-dbscan: KssdDBSCAN (src/dbscan.cpp:725-985) on the first GPU, printKssdDBSCANResult (:1212-1310); with
  // --minhash MinHashDBSCAN (:987-1096) and printDBSCANResult (:1102-1210), whose layout is the same ----
  if (o.minhash && mh.isContainment) { cerr << "ERROR: --minhash: " << folder_path << " holds containment sketches (-c), which are out of scope" << endl; return 1; }
  DeviceSketches ds;
  if (rs.ok) resident_sketches(ctx, gpus[0], rs, nullptr, ds);
  else if (o.minhash) upload_sketches(ctx, &mh.hashes, nullptr, ds);
  else upload_sketches(ctx, ks.use64 ? &ks.h64 : nullptr, ks.use64 ? nullptr : &ks.h32, ds);
  auto dbscan_mash = [&](const double* eps, size_t L, int32_t* lab, uint8_t* cr, uint32_t* nc, uint32_t* nn) {
    CHECK(ctx, rtc_dbscan_mash(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, (uint32_t)mh.sketchSize, eps, (uint32_t)L, o.dbscanMinPts,
                               kmer_size, lab, cr, nc, nn));
    uint64_t mc[10] = {0};
    rtc_dbscan_mash_counters(ctx, mc);
    if (getenv("RTC_VERBOSE"))
      fprintf(stderr, "[minhash] %zu levels: %llu candidate edges in %llu chunk(s), %llu merged, %llu kept; pair %.3f ms, predicate %.3f ms, "
              "components %.3f ms\n", L, (unsigned long long)mc[1], (unsigned long long)mc[0], (unsigned long long)mc[2], (unsigned long long)mc[3],
              mc[6] / 1e6, mc[7] / 1e6, mc[8] / 1e6);
    g_metrics.num("dbscan_mash_pair_s", mc[6] / 1e9);
    g_metrics.num("dbscan_mash_predicate_s", mc[7] / 1e9);
    g_metrics.num("dbscan_mash_components_s", mc[8] / 1e9);
  };
  cerr << "-----Running DBSCAN clustering (" << (o.minhash ? "MinHash" : "KSSD") << ")..." << endl;
  cerr << "-----Parameters: eps=" << o.dbscanEps << ", minPts=" << o.dbscanMinPts << endl;
  vector<int32_t> labels(genomes.size());
  vector<uint8_t> core(genomes.size());
  uint32_t ncl = 0, nnoise = 0;
  vector<rtc_hedge> forest(o.hierarchy ? genomes.size() : 0);  // --hierarchy: n - 1 slots, the core triples beside them
  vector<rtc_kdist> hcore(o.hierarchy ? genomes.size() : 0);
  uint64_t n_forest = 0;
  if (o.dbscanKnn > 0) {  // KssdDBSCAN's lines on its k (src/dbscan.cpp:754-761, :774), then the k-NN call
    int knn_k = o.dbscanKnn;
    if (knn_k < o.dbscanMinPts - 1) {
      cerr << "-----WARNING: knn_k (" << knn_k << ") < minPts-1 (" << (o.dbscanMinPts - 1) << "). Adjusting knn_k to " << (o.dbscanMinPts - 1) << "." << endl;
      knn_k = o.dbscanMinPts - 1;
    } else if (knn_k < 5 * (o.dbscanMinPts - 1)) {
      cerr << "-----WARNING: knn_k (" << knn_k << ") may be too small for stable DBSCAN. Consider knn_k >= " << (5 * (o.dbscanMinPts - 1)) << "." << endl;
    }
    cerr << "-----WARNING: k-NN acceleration is approximate for DBSCAN (may miss eps neighbors if k is small)." << endl;
    CHECK(ctx, rtc_dbscan_knn(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, o.dbscanEps, o.dbscanMinPts, kmer_size, o.maxPosting, knn_k,
                              labels.data(), core.data(), &ncl, &nnoise));
    uint64_t kc[10] = {0};
    rtc_dbscan_knn_counters(ctx, kc);
    if (getenv("RTC_VERBOSE"))
      fprintf(stderr, "[knn] k %d: %llu candidate edges in %llu chunk(s), %llu passers, %llu rows truncated (%llu by arrival order), %llu neighbour "
              "edges, %llu rounds; selection %.3f ms, propagation %.3f ms\n", knn_k, (unsigned long long)kc[1], (unsigned long long)kc[0],
              (unsigned long long)kc[2], (unsigned long long)kc[3], (unsigned long long)kc[4], (unsigned long long)kc[5], (unsigned long long)kc[7],
              kc[8] / 1e6, rtc_dbscan_knn_propagate_ns(ctx) / 1e6);
    g_metrics.num("dbscan_knn_k", (double)knn_k);
    g_metrics.num("dbscan_knn_select_s", kc[8] / 1e9);
    g_metrics.num("dbscan_knn_propagate_s", rtc_dbscan_knn_propagate_ns(ctx) / 1e9);
    g_metrics.num("dbscan_knn_truncated_rows", (double)kc[3]);
  } else if (o.minhash && o.epsSweep.empty()) {
    dbscan_mash(&o.dbscanEps, 1, labels.data(), core.data(), &ncl, &nnoise);
  } else if (o.epsSweep.empty() && !o.kdist && !o.hierarchy) {
    CHECK(ctx, rtc_dbscan(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, o.dbscanEps, o.dbscanMinPts, kmer_size, o.maxPosting,
                          labels.data(), core.data(), &ncl, &nnoise));
  } else {
    // --eps is one more level of the sweep: one pair phase for the whole run.  An --eps that repeats a sweep value shares its
    // level; 32 sweep values and a 33rd --eps are past rtc_dbscan_sweep's 32 levels, and --eps then takes a call of its own.
    const size_t n = genomes.size(), S = o.epsSweep.size();
    vector<double> levels = o.epsSweep;
    size_t eps_level = std::find(levels.begin(), levels.end(), o.dbscanEps) - levels.begin();
    const bool own_call = eps_level == S && S == 32;
    if (eps_level == S && !own_call) levels.push_back(o.dbscanEps);
    const size_t L = levels.size();
    vector<int32_t> all_labels(L * n);
    vector<uint8_t> all_core(L * n);
    vector<uint32_t> all_ncl(L), all_nnoise(L);
    vector<rtc_kdist> kd(o.kdist ? n : 0);
    if (o.minhash) {
      dbscan_mash(levels.data(), L, all_labels.data(), all_core.data(), all_ncl.data(), all_nnoise.data());
    } else if (o.hierarchy) {  // the hierarchy below --eps from the sweep's pair phase
      CHECK(ctx, rtc_dbscan_sweep_hierarchy(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, levels.data(), (uint32_t)L, o.dbscanMinPts,
                                            kmer_size, o.maxPosting, all_labels.data(), all_core.data(), all_ncl.data(), all_nnoise.data(),
                                            o.kdist ? kd.data() : nullptr, o.dbscanEps, forest.data(), &n_forest, hcore.data()));
      uint64_t hc[10] = {0};
      rtc_dbscan_hierarchy_counters(ctx, hc);
      if (getenv("RTC_VERBOSE"))
        fprintf(stderr, "[hierarchy] %llu candidate edges in %llu chunk(s), %llu kept at eps %g, %llu forest edges in %llu round(s); pair %.3f ms, "
                "k-distance %.3f ms, weights and ranking %.3f ms, forest %.3f ms\n", (unsigned long long)hc[1], (unsigned long long)hc[0],
                (unsigned long long)hc[2], o.dbscanEps, (unsigned long long)hc[3], (unsigned long long)hc[4], hc[5] / 1e6, hc[6] / 1e6, hc[7] / 1e6,
                hc[8] / 1e6);
      g_metrics.num("dbscan_hierarchy_pair_s", hc[5] / 1e9);
      g_metrics.num("dbscan_hierarchy_kdist_s", hc[6] / 1e9);
      g_metrics.num("dbscan_hierarchy_forest_s", (hc[7] + hc[8]) / 1e9);
      g_metrics.num("dbscan_hierarchy_edges", (double)hc[3]);
    } else {
      CHECK(ctx, rtc_dbscan_sweep(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, levels.data(), (uint32_t)L, o.dbscanMinPts, kmer_size,
                                  o.maxPosting, all_labels.data(), all_core.data(), all_ncl.data(), all_nnoise.data(), o.kdist ? kd.data() : nullptr));
    }
    uint64_t sc[10] = {0};
    if (!o.minhash) rtc_dbscan_sweep_counters(ctx, sc);
    if (getenv("RTC_VERBOSE") && !o.minhash)
      fprintf(stderr, "[sweep] %zu levels: %llu candidate edges in %llu chunk(s), %llu kept; pair %.3f ms, predicate %.3f ms, components %.3f ms, "
              "k-distance %.3f ms\n", L, (unsigned long long)sc[1], (unsigned long long)sc[0], (unsigned long long)sc[2], sc[5] / 1e6, sc[6] / 1e6,
              sc[7] / 1e6, sc[8] / 1e6);
    g_metrics.num("dbscan_sweep_levels", (double)L);
    if (!o.minhash) {
      g_metrics.num("dbscan_sweep_pair_s", sc[5] / 1e9);
      g_metrics.num("dbscan_sweep_predicate_s", sc[6] / 1e9);
      g_metrics.num("dbscan_sweep_components_s", sc[7] / 1e9);
      g_metrics.num("dbscan_sweep_kdist_s", sc[8] / 1e9);
    }
    if (own_call && o.minhash) {
      dbscan_mash(&o.dbscanEps, 1, labels.data(), core.data(), &ncl, &nnoise);
    } else if (own_call) {
      CHECK(ctx, rtc_dbscan(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, o.dbscanEps, o.dbscanMinPts, kmer_size, o.maxPosting,
                            labels.data(), core.data(), &ncl, &nnoise));
    } else {
      std::copy(all_labels.begin() + eps_level * n, all_labels.begin() + (eps_level + 1) * n, labels.begin());
      std::copy(all_core.begin() + eps_level * n, all_core.begin() + (eps_level + 1) * n, core.begin());
      ncl = all_ncl[eps_level]; nnoise = all_nnoise[eps_level];
    }
    if (S) {
      const string tsv = o.outputFile + ".eps_sweep.tsv";
      FILE* fp = fopen(tsv.c_str(), "w");
      if (!fp) { cerr << "ERROR: cannot open file: " << tsv << endl; return 1; }
      fprintf(fp, "eps\tclusters\tnoise\tcore_points\tlargest_cluster\tborder_points\n");
      for (size_t e = 0; e < S; e++) {
        const vector<int32_t> lab(all_labels.begin() + e * n, all_labels.begin() + (e + 1) * n);
        char name[64];
        snprintf(name, sizeof name, ".eps_%.6f", levels[e]);
        print_dbscan_result(lab, all_ncl[e], genomes, sketchByFile, dbscan_format_mismatch, o.outputFile + name, levels[e], o.dbscanMinPts);
        vector<uint32_t> size(all_ncl[e], 0);
        uint64_t n_core = 0, n_border = 0;
        for (size_t v = 0; v < n; v++) {
          if (lab[v] >= 0) size[lab[v]]++;
          if (all_core[e * n + v]) n_core++;
          else if (lab[v] >= 0) n_border++;
        }
        fprintf(fp, "%.6f\t%u\t%u\t%llu\t%u\t%llu\n", levels[e], all_ncl[e], all_nnoise[e], (unsigned long long)n_core,
                size.empty() ? 0u : *std::max_element(size.begin(), size.end()), (unsigned long long)n_border);
      }
      fclose(fp);
      cerr << "-----write the eps sweep (" << S << " values) into: " << tsv << endl;
    }
    if (o.kdist) {
      // the curve as one plots it: the distances in descending order (no k-th candidate: inf, first), ties by index
      const string tsv = o.outputFile + ".kdist.tsv";
      FILE* fp = fopen(tsv.c_str(), "w");
      if (!fp) { cerr << "ERROR: cannot open file: " << tsv << endl; return 1; }
      vector<double> dist(n);
      for (size_t v = 0; v < n; v++) {
        const rtc_kdist& r = kd[v];
        const uint64_t denom = (uint64_t)r.size_p + r.size_q - r.common;
        if (r.neighbour == UINT32_MAX) dist[v] = INFINITY;
        else if (denom == r.common) dist[v] = 0.0;  // j = 1, two empty u64 sketches included
        else { const double j = (double)r.common / (double)denom; dist[v] = -log(2.0 * j / (1.0 + j)) / kmer_size; }
      }
      vector<uint32_t> order(n);
      for (size_t v = 0; v < n; v++) order[v] = (uint32_t)v;
      std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return dist[a] != dist[b] ? dist[a] > dist[b] : a < b; });
      fprintf(fp, "index\tkth_neighbour\tcommon\tsize\tsize_neighbour\tdistance\n");
      for (uint32_t v : order) {
        const rtc_kdist& r = kd[v];
        if (r.neighbour == UINT32_MAX) fprintf(fp, "%u\t-1\t0\t%u\t0\tinf\n", v, r.size_p);
        else fprintf(fp, "%u\t%u\t%u\t%u\t%u\t%.10g\n", v, r.neighbour, r.common, r.size_p, r.size_q, dist[v]);
      }
      fclose(fp);
      cerr << "-----write the k-distance curve (k=" << o.dbscanMinPts - 1 << ") into: " << tsv << endl;
    }
  }
  if (o.hierarchy) {
    const size_t n = genomes.size();
    auto dist_of = [&](uint32_t common, uint32_t a, uint32_t b) {
      const uint64_t denom = (uint64_t)a + b - common;
      if (denom == common) return 0.0;  // m = 1, two empty u64 sketches included
      const double j = (double)common / (double)denom;
      return -log(2.0 * j / (1.0 + j)) / kmer_size;
    };
    const string htsv = o.outputFile + ".hierarchy.tsv", ctsv = o.outputFile + ".core.tsv", flat = o.outputFile + ".hdbscan";
    FILE* fp = fopen(htsv.c_str(), "w");
    if (!fp) { cerr << "ERROR: cannot open file: " << htsv << endl; return 1; }
    fprintf(fp, "p\tq\tdistance\tcommon\tsize_p\tsize_q\n");
    for (uint64_t e = 0; e < n_forest; e++) {  // the forest's order: the smallest distance first
      const rtc_hedge& h = forest[e];
      fprintf(fp, "%u\t%u\t%.6f\t%u\t%u\t%u\n", h.p, h.q, dist_of(h.common, h.size_p, h.size_q), h.common, h.size_p, h.size_q);
    }
    fclose(fp);
    fp = fopen(ctsv.c_str(), "w");
    if (!fp) { cerr << "ERROR: cannot open file: " << ctsv << endl; return 1; }
    fprintf(fp, "index\tcore_distance\n");
    for (size_t v = 0; v < n; v++) {
      if (hcore[v].neighbour == UINT32_MAX) fprintf(fp, "%zu\tinf\n", v);
      else fprintf(fp, "%zu\t%.6f\n", v, dist_of(hcore[v].common, hcore[v].size_p, hcore[v].size_q));
    }
    fclose(fp);
    vector<int32_t> flat_labels(n);
    uint32_t flat_ncl = 0;
    const int st = rtc_hierarchy_flat((uint32_t)n, forest.data(), n_forest, hcore.data(), kmer_size, o.minClusterSize, flat_labels.data(), nullptr,
                                      &flat_ncl);
    if (st != RTC_OK) { cerr << "ERROR: rtc_hierarchy_flat failed with status " << st << endl; return 1; }
    print_dbscan_result(flat_labels, flat_ncl, genomes, sketchByFile, dbscan_format_mismatch, flat, o.dbscanEps, o.dbscanMinPts, o.minClusterSize);
    cerr << "-----write the hierarchy (" << n_forest << " edges) into: " << htsv << endl;
    cerr << "-----write the core distances into: " << ctsv << endl;
    cerr << "-----write the flat clustering (min_cluster_size=" << o.minClusterSize << ", " << flat_ncl << " clusters) into: " << flat << endl;
  }
  if (o.minhash) {  // MinHashDBSCAN's closing lines (:1091-1093): it counts no core points
    cerr << "-----DBSCAN clustering complete!" << endl;
    cerr << "-----Found " << ncl << " clusters" << endl;
    cerr << "-----Found " << nnoise << " noise points (outliers)" << endl;
  } else {
    dbscan_report(labels, core, ncl, nnoise);
  }
  print_dbscan_result(labels, ncl, genomes, sketchByFile, dbscan_format_mismatch, o.outputFile, o.dbscanEps, o.dbscanMinPts);
  cerr << "-----write the cluster result into: " << o.outputFile << endl;
  cerr << "-----the cluster number of " << o.outputFile << " is: " << ncl << endl;
  cerr << "-----the noise point number is: " << nnoise << endl;
  if (o.db_build) {  // the model of --eps: what --db --assign places new genomes into
    DbscanModel md;
    md.minhash = o.minhash; md.width = ds.width; md.sketch_by_file = sketchByFile; md.kmer_size = kmer_size;
    if (!o.minhash) { md.half_k = ks.info.half_k; md.half_subk = ks.info.half_subk; md.drlevel = ks.info.drlevel; }
    else md.sketch_size = mh.sketchSize;
    md.min_pts = o.dbscanMinPts; md.max_posting = 0; md.n_clusters = (int)ncl; md.min_len = o.minLen; md.eps = o.dbscanEps;
    md.labels = labels; md.core = core; md.genomes = genomes;
    if (o.minhash) md.h64 = mh.hashes; else if (ks.use64) md.h64 = ks.h64; else md.h32 = ks.h32;
    if ((md.width == 8 ? md.h64.size() : md.h32.size()) != genomes.size()) {
      cerr << "ERROR: --build needs the sketches on the host (" << (md.width == 8 ? md.h64.size() : md.h32.size()) << " of " << genomes.size() << ")" << endl;
      return 1;
    }
    if (!save_dbscan_model(o.repdb_path, md)) return 1;
    cerr << "-----write the DBSCAN model (" << genomes.size() << " genomes, " << ncl << " clusters) into: " << o.repdb_path << endl;
  }
  g_metrics.num("dbscan_s", get_sec() - t2);
  g_metrics.num("clusters", (double)ncl);
  g_metrics.num("noise", (double)nnoise);
#else
  // ---- clust-mst: compute_clusters MST branch (src/sub_command.cpp:2924-3053, :1988-2152) ----
  const int is_containment = o.is_fast ? (int)o.isContainment : (int)mh.isContainment;
  vector<rtc_edge> mst(genomes.size());
  uint64_t nedges = 0;
  const size_t G = gpus.size();
  vector<DeviceSketches> dss(G);
  on_all_gpus(gpus, [&](size_t g) {  // every GPU holds the complete sketch set (resident rows, or an upload of the loaded folder)
    if (rs.ok) resident_sketches(gpus[g].ctx, gpus[g], rs, nullptr, dss[g]);
    else if (o.is_fast) upload_sketches(gpus[g].ctx, ks.use64 ? &ks.h64 : nullptr, ks.use64 ? nullptr : &ks.h32, dss[g]);
    else upload_sketches(gpus[g].ctx, &mh.hashes, nullptr, dss[g]);
  });
  vector<int32_t> dense; uint64_t ani[101];
  if (!o.useIndex && !o.is_fast) {  // modifyMST, the dense loop (src/sub_command.cpp:2764,2995): every pair, MinHash::distance()
    const DeviceSketches& ds = dss[0];
    if (o.dense) dense.resize((size_t)DENSE_SPAN * ds.n);
    CHECK(ctx, rtc_mst_mash(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, 0, kmer_size, is_containment, (uint32_t)mh.sketchSize, mst.data(),
                            &nedges, o.dense ? DENSE_SPAN : 0, o.dense ? dense.data() : nullptr, o.dense ? ani : nullptr));
  } else if ((G == 1 && !gpus[0].comm) || o.dense) {  // --dense: the histograms are accumulated beside the single-GPU candidate list
    const DeviceSketches& ds = dss[0];
    if (o.dense) dense.resize((size_t)DENSE_SPAN * ds.n);
    CHECK(ctx, rtc_mst_dense(ctx, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, 0, kmer_size, is_containment, o.threshold, mst.data(), &nedges,
                             o.dense ? DENSE_SPAN : 0, o.dense ? dense.data() : nullptr, o.dense ? ani : nullptr));
  } else {
    // N x N row-sharded across the GPUs, one all-reduce per Boruvka round; every rank ends with the same forest
    vector<vector<rtc_edge>> out(G, vector<rtc_edge>(genomes.size()));
    vector<uint64_t> ne(G, 0);
    vector<rtc_shard_stats> stt(G);
    on_all_gpus(gpus, [&](size_t g) {
      const DeviceSketches& ds = dss[g];
      CHECK(gpus[g].ctx, rtc_mst_sharded(gpus[g].ctx, gpus[g].comm, ds.d_hashes, ds.width, ds.d_start, ds.d_len, ds.n, kmer_size,
                                         is_containment, o.threshold, out[g].data(), &ne[g], &stt[g]));
    });
    for (size_t g = 1; g < G; g++)
      if (ne[g] != ne[0] || memcmp(out[g].data(), out[0].data(), ne[0] * sizeof(rtc_edge)) != 0) { fprintf(stderr, "ERROR: GPU %zu ended with a different forest\n", g); return 1; }
    nedges = ne[0];
    mst.swap(out[0]);
    if (getenv("RTC_VERBOSE"))
      for (size_t g = 0; g < G; g++)
        fprintf(stderr, "[mst gpu %zu] rows %u..%u, %llu candidate edges, pair %.2f ms, boruvka %.2f ms (%u rounds)\n", g, stt[g].row0, stt[g].row1,
                (unsigned long long)stt[g].cand_edges, stt[g].pair_ms, stt[g].mst_ms, stt[g].rounds);
  }
  mst.resize(nedges);
  double t3 = get_sec();
  cerr << "========time of generateMST is: " << t3 - t2 << "========" << endl;
  g_metrics.num("generateMST_s", t3 - t2);
  g_metrics.num("mst_edges", (double)nedges);
  if (!o.noSave && !from_sketches) {
    save_genome_info(genomes, folder_path, "mst", sketchByFile, o.is_fast);
    save_mst(mst, folder_path);
    cerr << "========time of saveMST is: " << get_sec() - t3 << "========" << endl;
    g_metrics.num("saveMST_s", get_sec() - t3);
  }
  write_trees(o, genomes, mst, sketchByFile);
  // the edge-length analysis: compute_kssd_clusters (--fast from genomes, src/sub_command.cpp:2032-2073) with --stability, the
  // --presketched flows (clust_from_sketch_fast :2549-2566, clust_from_sketches :2786-2803) with min_gap_ratio 0.1 and without
  // it; compute_clusters (MinHash from genomes) has it switched off (:3031-3032)
  if (o.is_fast && !from_sketches) {
    if (o.autoThreshold) auto_threshold_report(mst, (int)genomes.size(), o.outputFile, 0.05, o.stability);
    else if (o.stability) stability_report(mst, (int)genomes.size(), o.threshold);
  } else if (from_sketches && o.autoThreshold) {
    auto_threshold_report(mst, (int)genomes.size(), o.outputFile, 0.1, false);
  }
  vector<rtc_edge> forest;
  vector<vector<int>> clusters;
  cluster_from_mst(mst, genomes, sketchByFile, o.outputFile, o.threshold, &forest, &clusters);
  // --save-rep: the presketched flows always, the flows from genomes when they keep a sketch folder (-e: none)
  if (o.saveRep && (from_sketches || !o.noSave) &&
      save_initial_mst_state(ctx, o, folder_path + "/mst_cluster_state.bin", genomes, sketchByFile, forest, clusters, mh, ks, from_sketches) != 0)
    return 1;
  // --db --build: the state is the database (build_and_save_{kssd,minhash}_mst_db); a MinHash containment build from genomes
  // stores -c, a --presketched build 0
  if (o.db_build &&
      save_initial_mst_state(ctx, o, o.repdb_path, genomes, sketchByFile, forest, clusters, mh, ks, from_sketches,
                             (!o.is_fast && !from_sketches && mh.isContainment) ? o.containCompress : 0) != 0)
    return 1;
  // --dedup-dist / --reps-per-cluster: the KSSD flows only (compute_kssd_clusters, clust_from_sketch_fast)
  if (o.is_fast) dedup_and_reps(ctx, o.dedupDist, o.repsPerCluster, o.threads, forest, clusters, genomes, sketchByFile, o.outputFile);
  if (o.linkageComplete) {
    if (is_containment) { cerr << "ERROR: --linkage does not go with containment sketches" << endl; return 1; }
    linkage_complete_and_print(ctx, dss[0], clusters, genomes, sketchByFile, o.outputFile, o.threshold, kmer_size);
  }
  if (o.njTree || o.njAll) {
    if (is_containment) { cerr << "ERROR: " << (o.njTree ? "--nj-tree" : "--nj-all") << " does not go with containment sketches" << endl; return 1; }
    if (nj_trees_and_print(ctx, dss[0], clusters, genomes, sketchByFile, o.outputFile, kmer_size, o.threads, o.njTree, o.njAll,
                           o.has_njSupport ? (uint32_t)o.njSupport : 0, o.njSeed) != 0) {
      join_warmup();
      return 1;
    }
  }
  if (o.quality) {
    if (is_containment) { cerr << "ERROR: --quality does not go with containment sketches" << endl; return 1; }
    if (quality_and_print(ctx, dss[0], clusters, genomes, sketchByFile, o.outputFile, kmer_size, o.threads) != 0) {
      join_warmup();
      return 1;
    }
  }
  if (o.has_clusterSupport) {
    if (is_containment) { cerr << "ERROR: --cluster-support does not go with containment sketches" << endl; return 1; }
    if (cluster_support_and_print(ctx, dss[0], clusters, genomes, sketchByFile, o.outputFile, o.threshold, kmer_size, (uint32_t)o.clusterSupport,
                                  o.supportSeed) != 0) {
      join_warmup();
      return 1;
    }
  }
  if (o.upgma) {
    if (is_containment) { cerr << "ERROR: --upgma does not go with containment sketches" << endl; return 1; }
    if (upgma_and_print(ctx, dss[0], clusters, genomes, sketchByFile, o.outputFile, o.threshold, kmer_size, o.threads) != 0) {
      join_warmup();
      return 1;
    }
  }
  if (o.pangenome) {
    if (is_containment) { cerr << "ERROR: --pangenome does not go with containment sketches" << endl; return 1; }
    if (pangenome_and_print(ctx, dss[0], clusters, genomes, sketchByFile, o.outputFile, (uint32_t)o.panSoft, (uint32_t)o.panCloud, o.threads) != 0) {
      join_warmup();
      return 1;
    }
  }
  if (o.dense) {
    if (!o.noSave && !from_sketches) { save_ani(folder_path, ani); save_dense(folder_path, dense, DENSE_SPAN, (int)genomes.size()); }
    remove_noise_and_print(mst, genomes, sketchByFile, o.outputFile, o.threshold, dense, DENSE_SPAN, &forest, &clusters);
    if (o.is_fast)
      dedup_and_reps(ctx, o.dedupDist, o.repsPerCluster, o.threads, forest, clusters, genomes, sketchByFile, o.outputFile + ".removeNoise");
  }
#endif
  const double t_end = get_sec();
#ifdef GREEDY_CLUST
  g_metrics.str("command", "clust-greedy");
#elif defined(LEIDEN_CLUST)
  g_metrics.str("command", "clust-leiden");
#elif defined(DBSCAN_CLUST)
  g_metrics.str("command", "clust-dbscan");
#else
  g_metrics.str("command", "clust-mst");
#endif
  g_metrics.str("sketch", o.is_fast ? "kssd" : "minhash");
  g_metrics.num("gpus", (double)gpus.size());
  g_metrics.num("genomes", (double)genomes.size());
  g_metrics.num("kmer_size", (double)kmer_size);
  g_metrics.num("threshold", o.threshold);
  g_metrics.num("threads", (double)o.threads);
  g_metrics.num("from_sketches", from_sketches ? 1 : 0);
  g_metrics.num("total_s", t_end - t_main);
  g_metrics.write();
  join_warmup();
#ifdef RTC_MEASURE
  if (const char* e = getenv("RTC_EXIT_DELAY_MS")) usleep(1000 * atoi(e));
  if (getenv("RTC_EXIT_PROBE")) {
    const double p0 = get_sec();
    for (char* p : g_exit_probe_host) free(p);
    const double p1 = get_sec();
    for (auto& d : g_exit_probe_dev) (void)rtc_dev_free(d.first, d.second);
    const double p2 = get_sec();
    fprintf(stderr, "[probe] %zu host staging buffers freed in %.3fs, %zu device buffers in %.3fs\n", g_exit_probe_host.size(), p1 - p0,
            g_exit_probe_dev.size(), p2 - p1);
    if (strcmp(getenv("RTC_EXIT_PROBE"), "reset") == 0) {
      for (Gpu& g : gpus) (void)rtc_debug_device_reset(g.device);
      fprintf(stderr, "[probe] hipDeviceReset in %.3fs\n", get_sec() - p2);
      fprintf(stderr, "[exit]  output written at t+%.3fs, contexts released in %.3fs (main entered at %.6f, leaving at %.6f)\n", t_end - t_main, 0.0, t_main, get_sec());
      fflush(nullptr);
      _exit(0);
    }
  }
#endif
  for (Gpu& g : gpus) { if (g.comm) rtc_comm_destroy(g.comm); }
  for (Gpu& g : gpus) rtc_ctx_destroy(g.ctx);
  if (getenv("RTC_VERBOSE")) fprintf(stderr, "[exit]  output written at t+%.3fs, contexts released in %.3fs (main entered at %.6f, leaving at %.6f)\n", t_end - t_main,
                                     get_sec() - t_end, t_main, get_sec());
  // Everything is written and closed: leave without unmapping the GBs of staging memory page by page and without the
  // HIP runtime's own teardown (0.15 s of a 0.9 s run on 41 Gbp); the kernel reclaims both at once.
  std::cout.flush();
  fflush(nullptr);
  _exit(0);
}
