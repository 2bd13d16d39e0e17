// rtc_internal.h -- shared host-side plumbing for the HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "../../include/rtclust.h"

// The library's switches (README: environment).  Read from the environment ONCE, when the context is created -- no call path
// asks the environment again; rtc_ctx_reload_options reads them anew for a context that is already there (tests, tuning runs).
struct rtc_options {
  int verbose = 0;                 // RTC_VERBOSE
  int pair_join = 1;               // RTC_PAIR_JOIN: 0 never, 1 by the cost rule, 2 wherever its scratch fits
  int join_semi = 1;               // RTC_JOIN_SEMI: 0 never, 1 by rule, 2 always
  int join_fullsort = 0;           // RTC_JOIN_FULLSORT
  int join_debug = 0;              // RTC_JOIN_DEBUG
  int pair_force_merge = 0;        // RTC_PAIR_FORCE_MERGE
  uint32_t pair_ktarget = 0;       // RTC_PAIR_KTARGET (0: the kernel's default)
  uint64_t pair_tcols_budget = 0;  // RTC_PAIR_TCOLS_BUDGET (0: default)
  uint64_t edge_budget = 0;        // RTC_EDGE_BUDGET (0: default)
  bool has_greedy_global_pairs = false;
  uint64_t greedy_global_pairs = 0;  // RTC_GREEDY_GLOBAL_PAIRS
  int kssd_cuckoo = 0;             // RTC_KSSD_CUCKOO
  int kssd_nofast = 0;             // RTC_KSSD_NOFAST
  int sketch_packed = 0, sketch_no_packed = 0;  // RTC_SKETCH_PACKED / RTC_SKETCH_NO_PACKED (LDS table layout of the MinHash kernels)
  int sketch_rounds = 0;           // RTC_SKETCH_ROUNDS (0: planned)
  int sketch_t0_factor = -1;       // RTC_SKETCH_T0_FACTOR (-1: by rule)
  int comm_force_rccl = 0;         // RTC_COMM_FORCE_RCCL
  double comm_timeout_s = 120.0;   // RTC_COMM_TIMEOUT_S (<= 0: forever)
  int dedup_gpu = 1;               // RTC_DEDUP_GPU: 0 never, 1 groups from the measured cutoff up, 2 every group of two or more
  int dbscan_mash_serial = 0;      // RTC_DBSCAN_MASH_SERIAL: the per-thread merge instead of the wave-cooperative one
  int dbscan_mash_noprefilter = 0;  // RTC_DBSCAN_MASH_NOPREFILTER: every candidate is merged
  uint32_t linkage_span = 0;       // RTC_LINKAGE_SPAN: the rows of a band that small components share in the fill (0: default)
  uint64_t linkage_bytes = 0;      // RTC_LINKAGE_BYTES: the byte budget of a batch of rtc_linkage_complete (0: half the free HBM)
  uint64_t nj_bytes = 0;           // RTC_NJ_BYTES: the byte budget of a batch of rtc_nj_clusters (0: half the free HBM)
  uint32_t nj_grid_min = 0;        // RTC_NJ_GRID_MIN: components of at least this many points (down to 4) take the grid path (0: default)
  uint32_t nj_scan_blocks = 0;     // RTC_NJ_SCAN_BLOCKS: the most workgroups of a grid-path scan launch, 1 .. 1024 (0: 1024)
  uint64_t upgma_bytes = 0;        // RTC_UPGMA_BYTES: the byte budget of a batch of rtc_upgma_clusters (0: half the free HBM)
  uint32_t upgma_grid_min = 0;     // RTC_UPGMA_GRID_MIN: components of at least this many points (down to 4) take the grid path (0: default)
  uint32_t upgma_scan_blocks = 0;  // RTC_UPGMA_SCAN_BLOCKS: the most workgroups of a grid-path scan launch, 1 .. 1024 (0: 1024)
  int mcl_global = 0;              // RTC_MCL_GLOBAL: every column of rtc_mcl takes the long path (the table in global memory)
  int snn_global = 0;              // RTC_SNN_GLOBAL: every record of rtc_graph_snn takes the long path (the owner's row in global memory)
  int sil_global = 0;              // RTC_SIL_GLOBAL: every row of rtc_silhouette takes the long path (the table in global memory)
  uint64_t support_bytes = 0;      // RTC_SUPPORT_BYTES: the bytes rtc_cluster_support's words of 64 replicates may take at once (0: half the free HBM)
  bool has_degree_tail = false;
  uint32_t degree_tail = 0;        // RTC_DEGREE_TAIL: rtc_greedy_degree's selection goes to the one-workgroup kernel from this many open vertices down (0: never)
  int degree_block = 0;            // RTC_DEGREE_BLOCK: every row of rtc_greedy_degree's assignment takes the 256-lane path
  uint64_t screen_bytes = 0;       // RTC_SCREEN_BYTES: the bytes a chunk of rtc_rep_screen's match records and views may take (0: half the free HBM)
  int screen_global = 0;           // RTC_SCREEN_GLOBAL: every sample of rtc_rep_screen takes the long path (the counts in global memory)
  uint64_t pan_bytes = 0;          // RTC_PAN_BYTES: the bytes a group of rtc_pangenome's clusters (arena and views) may take (0: half the free HBM)
  int pan_global = 0;              // RTC_PAN_GLOBAL: every cluster of rtc_pangenome takes the arena in global memory
};
void rtc_options_from_env(rtc_options* o);

// The size-ratio bound of the MST's candidate filter: calr (src/MST.cpp:26-37) as the reference stores it, "int radio =
// calr(threshold, k - 1)" (:1292), i.e. floor(2 e^(threshold (k-1)) - 1) for threshold >= 0 -- but saturated at INT32_MAX where
// the reference's conversion is undefined.  The kernels keep a pair iff max <= radio * min with the product in 64 bits, so a
// saturated radio keeps every pair; the reference's int product wraps there instead (a deliberate divergence).
static inline int rtc_size_radio(double threshold, int kmer_size) {
  const double r = 2.0 * exp(threshold * (kmer_size - 1)) - 1.0;
  return r < 2147483647.0 ? (int)r : 2147483647;
}

struct rtc_ctx {
  int device = 0;
  rtc_options opt;
  hipStream_t stream = nullptr;
  hipStream_t owned_stream = nullptr;  // rtc_ctx_own_stream
  int num_cu = 256;
  int lds_per_wg = 65536;
  std::string err;
  // growable device scratch (segment tables, partial sketches, partition tables ...)
  void* ws[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t ws_bytes[6] = {0, 0, 0, 0, 0, 0};
  // pinned host staging for small synchronous read-backs
  void* pinned = nullptr;
  size_t pinned_bytes = 0;
  // a word of page-locked host memory the device can write: asynchronous argument checks (rtc_check_runs_async) raise it, the
  // next packed sketch call and rtc_ctx_sync report it
  uint32_t* sticky = nullptr;
  uint64_t free_hbm_cached = 0;   // rtc_free_hbm
  double free_hbm_at = -1.0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // HIP events around the last pair_tiled_kernel launch, on the stream it was launched on (rtc_pair_last_kernel_ms)
  hipEvent_t pk0 = nullptr, pk1 = nullptr;
  int pk_valid = 0;
  // tiled pair kernel: the last plan (slice offsets + transposed column copy in scratch slots 1 / 4).
  // Reused only while pair_plan_hold is set by a caller that guarantees unchanged sketches between
  // launches (the row-chunk loop of the dense candidate-edge path).
  int quiet = 0;           // rtc_warmup's context: no RTC_VERBOSE lines
  int pair_last_path = 0;  // rtc_pair_last_path
  int dedup_last_path = 0;  // rtc_dedup_last_path
  int rep_topk_path = 0;    // rtc_rep_topk_last_path
  uint64_t rep_topk[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_rep_topk_counters
  // rtc_dbscan_counters: [0] row chunks, [1] candidate edges, [2] eps edges, [3] core points, [4] asymmetric pairs, [5] hook rounds,
  // [6] pair phase ns, [7] eps filter ns, [8] components + labels ns, [9] whole call ns
  uint64_t dbscan[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t dbscan_sweep[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_dbscan_sweep_counters (include/rtclust.h lists them)
  uint64_t dbscan_hier[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // rtc_dbscan_hierarchy_counters (include/rtclust.h lists them)
  uint64_t dbscan_mash[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // rtc_dbscan_mash_counters (include/rtclust.h lists them)
  uint64_t dbscan_assign[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_dbscan_assign_counters (include/rtclust.h lists them)
  int dbscan_assign_path = 0;  // rtc_dbscan_assign_last_path
  uint64_t dbscan_update[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_dbscan_update_counters (include/rtclust.h lists them)
  uint64_t dbscan_knn[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_dbscan_knn_counters (include/rtclust.h lists them)
  uint64_t dbscan_knn_propagate_ns = 0;  // rtc_dbscan_knn_propagate_ns
  uint64_t graph[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};    // rtc_graph_counters (include/rtclust.h lists them)
  uint64_t louvain[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_louvain_counters (include/rtclust.h lists them)
  uint64_t leiden[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // rtc_leiden_counters
  uint64_t graph_query[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // rtc_graph_query_counters (include/rtclust.h lists them)
  uint64_t leiden_place[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_leiden_place_counters (include/rtclust.h lists them)
  int leiden_place_path = 0;  // rtc_leiden_place_last_path
  uint64_t linkage[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_linkage_counters (include/rtclust.h lists them)
  uint64_t nj[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_nj_counters (include/rtclust.h lists them)
  int nj_path = 0;          // rtc_nj_last_path
  uint64_t nj_support[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_nj_support_counters (include/rtclust.h lists them)
  uint64_t upgma[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_upgma_counters (include/rtclust.h lists them)
  int upgma_path = 0;       // rtc_upgma_last_path
  uint64_t mcl[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_mcl_counters (include/rtclust.h lists them)
  int mcl_path = 0;         // rtc_mcl_last_path
  uint64_t snn[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_graph_snn_counters (include/rtclust.h lists them)
  int snn_path = 0;         // rtc_graph_snn_last_path
  uint64_t sil[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_silhouette_counters (include/rtclust.h lists them)
  int sil_path = 0;         // rtc_silhouette_last_path
  uint64_t quality[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_cluster_quality_counters (include/rtclust.h lists them)
  uint64_t csupport[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_cluster_support_counters (include/rtclust.h lists them)
  uint64_t greedy_degree[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_greedy_degree_counters (include/rtclust.h lists them)
  int greedy_degree_path = 0;  // rtc_greedy_degree_last_path
  uint64_t rep_screen[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_rep_screen_counters (include/rtclust.h lists them)
  int rep_screen_path = 0;  // rtc_rep_screen_last_path
  uint64_t pan[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // rtc_pangenome_counters (include/rtclust.h lists them)
  uint64_t pan_phase[3] = {0, 0, 0};  // rtc_pangenome_phases
  int pan_path = 0;         // rtc_pangenome_last_path
  int host_threads = 1;     // rtc_ctx_set_host_threads: the host side of rtc_tree_medoids and of rtc_nj_clusters', rtc_upgma_clusters' and rtc_cluster_quality's distances
  // rtc_diag_counters: [0] pair tiles the join took, [1] tiled-kernel tiles, [2] merge-kernel tiles, [3] candidate lists contracted
  // to their forest, [4] greedy runs replayed from ONE global join, [5] greedy query blocks of the block loop, [6] estimates handed
  // back instead of a launch (rtc_pair_edges_dev's overflow protocol)
  uint64_t diag[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // the inverted join's last refusal for density: the input it counted
  // keyed on the sketch buffer, its generation (every sketch / gather call on this context bumps sketch_gen) and the tile
  struct { const void* hashes = nullptr; uint64_t gen = 0; uint32_t n = 0, row0 = 0, row1 = 0, col0 = 0, col1 = 0; uint64_t K = 0, maxkey = 0; uint64_t edges_hint = 0; /* set by a refusal from the sample, for this call only: candidate edges to expect */ } join_dense;
  uint64_t sketch_gen = 1;
  // the candidate edge list of the last clustering call (rtc_edge_list_free keeps it, rtc_candidate_edges_device takes it): a
  // command line clusters once, a service or a benchmark loop many times over sets of one size -- the second call then starts with
  // a list that held the first one's edges, no allocation and no overflow redo
  void* mst_pinned = nullptr;      // rtc_mst_bufs: page-locked sketch sizes + forest of a whole-MST call
  size_t mst_pinned_bytes = 0;
  void* edge_cache = nullptr;
  uint64_t edge_cache_cap = 0;
  void* edge_cache_count = nullptr;
  int pair_plan_hold = 0, pair_plan_valid = 0;
  uint32_t pair_plan_tc1_hint = 0;
  struct {
    const void *hashes, *start, *len;
    uint32_t n, tc0, tc1;
    int width, P, npl;
    const uint32_t* d_so;
    const uint64_t* d_tbase;
    const void* d_tcols;
    const void* d_tcols_lo;
  } pair_plan = {};
  // KSSD filter tables of this context (cuckoo index or full table), keyed by (half_subk, drlevel, checksum)
  struct {
    int half_subk = -1, drlevel = -1;
    uint64_t checksum = 0;
    void* d_index = nullptr;
    int ck1 = 13, ck2 = 13;
    int32_t* d_table = nullptr;
    void* d_bucket = nullptr;  // bucket index (64 KiB of patterns) + ranks (64 KiB)
    void* d_bloom = nullptr;   // blocked Bloom filter of the kept middle 12-mers and their reverse complements (64 KiB)
    int bvar = -1;             // which bucket bits the index uses, -1: none
  } kssd;
};

int rtc_fail(rtc_ctx* ctx, int code, const char* fmt, ...);
// returns device scratch slot `slot` grown to at least `bytes`
int rtc_ws(rtc_ctx* ctx, int slot, size_t bytes, void** out);
int rtc_pinned(rtc_ctx* ctx, size_t bytes, void** out);
// free HBM of the context's device, for the scratch budgets of the pair phase: hipMemGetInfo walks the driver's tables, so the
// answer is kept for 100 ms or until this context allocates or frees (the budgets are halves of the free memory, not margins)
// One empty launch per sketch translation unit: the HIP runtime maps a unit's device code at its first launch (~10 ms each);
// rtc_warmup does that beside the command lines' first PCIe copies instead of in front of their first sketch.
int rtc_touch_sketch_minhash(rtc_ctx* ctx);
int rtc_touch_sketch_kssd(rtc_ctx* ctx);
int rtc_touch_sketch_minhash_packed(rtc_ctx* ctx);
int rtc_touch_unpack(rtc_ctx* ctx);
// The run list's contract -- ascending by start, disjoint, inside the batch -- checked on the device in one pass, without a host
// round trip: a violation raises the context's sticky flag (rtc_unpack.hip).  rtc_sticky_error: RTC_ERR_ARG once if it is up.
int rtc_check_runs_async(rtc_ctx* ctx, const uint64_t* d_runs, uint64_t n_runs, uint64_t n_bases);
int rtc_sticky_error(rtc_ctx* ctx);
uint64_t rtc_free_hbm(rtc_ctx* ctx);

// the host's monotonic clock, for the phase times of the counters
static inline uint64_t rtc_now_ns() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

struct DevBuf {  // hipMalloc'd scratch released on every way out; the context's free-memory figure stays current, as with rtc_dev_alloc / rtc_dev_free
  rtc_ctx* ctx = nullptr;
  std::vector<void*> p;
  ~DevBuf() {
    for (void* q : p) (void)hipFree(q);
    if (ctx) ctx->free_hbm_at = -1.0;
  }
  template <class T> int get(rtc_ctx* c, size_t count, T** out) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max<size_t>(count * sizeof(T), 256));
    if (e != hipSuccess) { (void)hipGetLastError(); return rtc_fail(c, RTC_ERR_NOMEM, "device scratch: %zu bytes: %s", count * sizeof(T), hipGetErrorString(e)); }
    p.push_back(q);
    ctx = c;
    ctx->free_hbm_at = -1.0;
    *out = (T*)q;
    return RTC_OK;
  }
  void release(void* q) {
    for (auto& x : p) if (x == q) { (void)hipFree(x); x = nullptr; }
    if (ctx) ctx->free_hbm_at = -1.0;
  }
};

// ---- internal C++ interfaces shared by the translation units ----------------------------------
// all-reduce of a per-round key array across the ranks of a multi-GPU run (rtc_comm.hip);
// dtype 0 = int64, 1 = uint32, 2 = uint64; op 0 = MIN, 1 = MAX
struct rtc_reduce_hook {
  int (*all_reduce)(void* self, void* d_buf, size_t count, int dtype, int op);
  void* self;
};
struct rtc_edge_list {  // device-resident candidate edges
  rtc_cedge* d_edges = nullptr;
  uint64_t cap = 0, m = 0;
  unsigned long long* d_count = nullptr;
  int contractions = 0;
};
// on_new (optional): called with every batch of freshly produced candidate edges (device pointer, count)
// before the list may be contracted -- the --dense histograms see every candidate pair exactly once
struct rtc_edge_observer {
  int (*on_new)(void* self, const rtc_cedge* d_new, uint64_t count);
  void* self;
};
int rtc_candidate_edges_device(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start,
                               const uint32_t* d_len, uint32_t n, uint32_t row0, uint32_t row1, int kmer_size,
                               int is_containment, double threshold, uint32_t s_fixed, rtc_edge_list* el,
                               const rtc_edge_observer* obs = nullptr);
// (ctx != NULL: a list of up to 1 GiB stays with the context for its next clustering call instead of going back to the driver)
void rtc_edge_list_free(rtc_edge_list* el, rtc_ctx* ctx = nullptr);
// rtc_pairs_join.hip: candidate edges of a lower-triangle tile by the inverted join; *handled = 0 when it declines
int rtc_pair_edges_join(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                        uint32_t n, uint32_t row0, uint32_t row1, uint32_t col0, uint32_t col1, int radio,
                        rtc_cedge* d_edges, uint64_t cap, uint64_t* d_count, double tiled_scale, int* handled);
// sorted: leave the forest in the reference's output order (weight, i, j) -- rtc_sort.hip; contractions pass false.
// max_len: the longest sketch when the caller knows it (sizes vary): the edge id of a round then carries the count too
int rtc_msf_device(rtc_ctx* ctx, const rtc_cedge* d_edges, uint64_t m, const uint32_t* d_len, uint32_t n,
                   int is_containment, uint32_t s_fixed, const rtc_reduce_hook* hook, rtc_cedge* d_sel,
                   uint64_t* n_sel_out, int* rounds_out, bool sorted = true, uint32_t max_len = 0);
int rtc_sort_forest_device(rtc_ctx* ctx, rtc_cedge* d_sel, uint64_t ns, const uint32_t* d_len, int wmode);
int rtc_sort_u32_pairs(rtc_ctx* ctx, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t n);
int rtc_sort_u64_pairs(rtc_ctx* ctx, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t n);
// rtc_graph.hip: the least Jaccard quotient whose distance through the host function is below threshold (rtc_graph_build's J*)
double rtc_graph_jstar(double threshold, int kmer_size);
uint32_t rtc_fixed_size_of(const uint32_t* h_len, uint32_t n);
size_t rtc_msf_scratch_bytes(uint32_t n);
struct rtc_mst_bufs_t { uint32_t* h_len; rtc_cedge* h_sel; rtc_cedge* d_sel; };  // page-locked sizes + forest, device forest list
int rtc_mst_bufs(rtc_ctx* ctx, uint32_t n, rtc_mst_bufs_t* b);
int rtc_edges_to_mst_host_fixed(const rtc_cedge* h_sel, uint64_t m, const uint32_t* h_len, int kmer_size, int is_containment,
                                uint32_t s_fixed, rtc_edge* h_out);

// rtc_linkage.hip: the exact m x m key blocks (common, denom) of the components of a labelling, formed on the device in batches
// under a byte budget -- what rtc_linkage_complete agglomerates and rtc_nj_clusters joins.  Components are numbered by their
// smallest member, members taken in ascending genome order; the members of the components of two or more, component after
// component, are the permuted set perm, cfirst[c] where component c starts in it.
struct rtc_kb_comp {
  uint64_t key_off;      // first record of the block in the batch's buffer
  uint64_t ld;           // records per row of the block
  uint64_t merge_off;    // first output record (the consumer's)
  uint64_t scratch_off;  // the consumer's scratch
  uint32_t m, pad;
};
struct rtc_kb_batch {
  rtc_lkey* d_keys;                  // the blocks of the batch, both halves filled, the diagonal untouched; NULL: no component of two or more
  uint64_t n_keys;                   // records in d_keys
  std::vector<rtc_kb_comp>* comps;   // the components of two or more of [c, ce), key_off / ld / m set
  size_t c, ce;                      // the components of the batch, those of one member included
  uint64_t fill_ns;
  const std::vector<uint32_t>*csize, *cfirst, *perm;
  uint64_t budget;                   // the byte budget the batch was formed under
};
// on_batch is called for every batch in component order, the stream idle and the blocks complete; it may overwrite them.
// budget_opt 0: half the free HBM.  h_first[0 .. n_comp] is zeroed.  A component whose 8 m^2 bytes and one band exceed the budget:
// RTC_ERR_NOMEM, the message starting with who.  spare_copies: a batch leaves room for that many further copies of its blocks
// (rtc_nj_support's replicate blocks), and the refusal counts them.
int rtc_key_blocks(rtc_ctx* ctx, const char* who, uint64_t budget_opt, const void* d_hashes, int width, const uint64_t* d_start,
                   const uint32_t* d_len, uint32_t n, const uint32_t* h_comp, uint64_t* h_first,
                   const std::function<int(const rtc_kb_batch&)>& on_batch, uint32_t spare_copies = 0);
// How an on_batch hands its records over: those of the batch's components in component order behind *total, local indices
// turned into genome indices, h_first kept.  n_of(i, comp): the records comps[i] has at recs[comp.merge_off ..), and where the
// caller counts the component.  Once a component does not fit under cap, *overflow is up, nothing more is written and *total
// goes on counting.
template <class Rec> inline void rtc_kb_to_genomes(Rec& r, const uint32_t* g) { r.a = g[r.a]; r.b = g[r.b]; }
inline void rtc_kb_to_genomes(rtc_njoin& r, const uint32_t* g) { r.a = g[r.a]; r.b = g[r.b]; if (r.c != 0xFFFFFFFFu) r.c = g[r.c]; }
template <class Rec, class NOf>
void rtc_kb_remap(const rtc_kb_batch& b, const std::vector<Rec>& recs, NOf n_of, Rec* h_out, uint64_t cap, uint64_t* h_first, uint64_t* total,
                  bool* overflow) {
  const std::vector<uint32_t>&csize = *b.csize, &cfirst = *b.cfirst, &perm = *b.perm;
  size_t i = 0;
  for (size_t q = b.c; q < b.ce; q++) {
    if (csize[q] >= 2) {
      const rtc_kb_comp& cp = (*b.comps)[i];
      const uint64_t nr = n_of(i, cp);
      if (*total + nr > cap) *overflow = true;
      if (!*overflow)
        for (uint64_t e = 0; e < nr; e++) {
          Rec r = recs[cp.merge_off + e];
          rtc_kb_to_genomes(r, perm.data() + cfirst[q]);
          h_out[*total + e] = r;
        }
      *total += nr;
      i++;
    }
    h_first[q + 1] = *total;
  }
}

// the records of a neighbour-joining tree of m points
static inline uint64_t rtc_nj_records_of(uint32_t m) { return m >= 3 ? m - 2 : m == 2 ? 1 : 0; }
// rtc_nj.hip, for rtc_nj_support.hip.  rtc_nj_join: the records of comps[0 .. nc) (each m >= 2) over the matrices in d_dist, laid
// out by merge_off, which it sets; n_path[3]: the components of each path.  rtc_nj_clusters_impl is rtc_nj_clusters with a hook that sees every batch of two or more after its trees are joined: the
// batch (blocks overwritten), the components, their records with local indices, the records before the batch.
int rtc_nj_join(rtc_ctx* ctx, double* d_dist, std::vector<rtc_kb_comp>& comps, std::vector<rtc_njoin>& h_out, uint64_t n_path[3]);
using rtc_nj_hook = std::function<int(const rtc_kb_batch&, const std::vector<rtc_kb_comp>&, const std::vector<rtc_njoin>&, uint64_t)>;
int rtc_nj_clusters_impl(rtc_ctx* ctx, const char* who, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                         uint32_t n, const uint32_t* h_comp, int kmer_size, rtc_njoin* h_joins, uint64_t cap, uint64_t* h_n_joins,
                         uint64_t* h_first, uint32_t spare_copies, const rtc_nj_hook* hook);

#define RTC_HIP(ctx, call)                                                                  \
  do {                                                                                      \
    hipError_t e__ = (call);                                                                \
    if (e__ != hipSuccess)                                                                  \
      return rtc_fail((ctx), RTC_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call,      \
                      hipGetErrorString(e__));                                              \
  } while (0)

#define RTC_TRY(call)                  \
  do {                                 \
    int s__ = (call);                  \
    if (s__ != RTC_OK) return s__;     \
  } while (0)

// RTC_DEBUG_SYNC=1 in the environment synchronises after every launch and names it on stderr, so
// an asynchronous device fault can be pinned on a kernel
#define RTC_CHECK_LAUNCH(ctx)                                                        \
  do {                                                                               \
    RTC_HIP(ctx, hipGetLastError());                                                 \
    if (rtc_debug_sync()) {                                                          \
      fprintf(stderr, "[rtc] %s:%d launched, syncing\n", __FILE__, __LINE__);        \
      RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));                               \
      fprintf(stderr, "[rtc] %s:%d ok\n", __FILE__, __LINE__);                       \
    }                                                                                \
  } while (0)
static inline bool rtc_debug_sync() {
  static const bool on = getenv("RTC_DEBUG_SYNC") != nullptr;
  return on;
}

// ---- device helpers shared by kernels ------------------------------------------------------
__device__ __forceinline__ uint64_t rtc_rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint32_t rtc_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
