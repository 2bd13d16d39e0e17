/*
 * rtclust.h -- C ABI of the MI355X-native sketch + all-pairs-distance path of RabbitTClust.
 *
 * The reference has no FFI; the path sits behind the RabbitSketch C++ class API and the
 * intermediate-folder file formats.  Each entry point below names the reference
 * code it replaces (paths relative to the RabbitTClust tree).  Plain pointers and sizes only;
 * every function returns an rtc_status; no exceptions cross the boundary.
 *
 * Pointer naming: d_* = device (HBM) pointer, h_* = host pointer.  All device work is enqueued
 * on the context's HIP stream (rtc_ctx_set_stream); *_dev entry points do not synchronise unless
 * stated.  A context is bound to one GPU and may be used by one host thread at a time.
 */
#ifndef RTCLUST_H
#define RTCLUST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  RTC_OK = 0,
  RTC_ERR_ARG = 1,         /* bad argument (null pointer, k out of range, misaligned buffer) */
  RTC_ERR_HIP = 2,         /* HIP runtime failure; see rtc_last_error() */
  RTC_ERR_UNSUPPORTED = 3, /* valid request outside what the GPU path implements */
  RTC_ERR_OVERFLOW = 4,    /* caller-provided output capacity too small; required size reported */
  RTC_ERR_NOMEM = 5,
  RTC_ERR_COMM = 6         /* a collective did not complete within RTC_COMM_TIMEOUT_S (default 120 s) or the communicator was
                              aborted after one: every later call on that communicator returns this at once */
} rtc_status;

typedef struct rtc_ctx rtc_ctx;

/* ---- context ------------------------------------------------------------------------- */
int rtc_device_count(void); /* visible GPUs (0 when there is none or the runtime fails) */
int rtc_ctx_create(int device, rtc_ctx** out);
void rtc_ctx_destroy(rtc_ctx* ctx);
/* Loads the device code of the pair / MST / greedy phases ahead of their first use: the HIP runtime maps a
 * translation unit's code object at its first kernel launch (~27 ms for these phases together on MI355X), which a
 * one-shot command line would otherwise pay between sketching and clustering.  Runs a complete toy clustering on a
 * context of its own; meant for a helper thread beside the sketch phase (the command lines do that).  Thread-safe
 * against work on other contexts. */
int rtc_warmup(int device);
/* The library's switches (RTC_PAIR_JOIN, RTC_EDGE_BUDGET, RTC_SKETCH_T0_FACTOR, RTC_COMM_TIMEOUT_S ...: README) are read from
 * the environment once, by rtc_ctx_create; no call looks at the environment again.  This reads them anew for a context
 * that is already there (tests and tuning runs that change a switch between calls). */
int rtc_ctx_reload_options(rtc_ctx* ctx);
int rtc_ctx_set_stream(rtc_ctx* ctx, void* hip_stream); /* NULL = default stream */
/* Gives the context a non-blocking stream of its own: two contexts on one device, each driven by its
 * own host thread, then overlap (the command lines copy batch i+1 while batch i is sketched). */
int rtc_ctx_own_stream(rtc_ctx* ctx);
int rtc_ctx_sync(rtc_ctx* ctx);
const char* rtc_last_error(const rtc_ctx* ctx); /* ctx may be NULL: last context-less failure */
const char* rtc_version(void);
/* device properties: out[0]=CU count, out[1]=LDS bytes per workgroup, out[2]=wavefront size */
int rtc_device_info(rtc_ctx* ctx, int out[3]);

/* device memory for hosts that do not link a HIP runtime themselves (the C++ CLI) */
int rtc_dev_alloc(rtc_ctx* ctx, size_t bytes, void** d_ptr);
int rtc_dev_free(rtc_ctx* ctx, void* d_ptr);
/* free / total HBM of the context's GPU in bytes (the command lines size their resident sketch rows against it) */
int rtc_dev_mem_info(rtc_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
int rtc_copy_h2d(rtc_ctx* ctx, void* d_dst, const void* h_src, size_t bytes); /* synchronous */
int rtc_copy_d2h(rtc_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* synchronous */
int rtc_memset_dev(rtc_ctx* ctx, void* d_ptr, int value, size_t bytes);
/* page-locked host staging memory: the CLI parses FASTA files straight into it (the reference's
 * per-thread kseq buffers, src/SketchInfo.cpp:880-948) so the PCIe copy runs at link speed */
int rtc_host_alloc(rtc_ctx* ctx, size_t bytes, void** h_ptr);
int rtc_host_free(rtc_ctx* ctx, void* h_ptr);

/* ---- 2-bit packed staging (command lines) -------------------------------------------------- */
/* The reference feeds the sketcher ASCII records (src/SketchInfo.cpp:928-948).  The command lines send a quarter of
 * that over PCIe: base i of a batch at bits 2 (i & 3) of d_packed[i >> 2] with A, C, G, T = 0..3, and everything that
 * is not ACGT (N, IUPAC codes, record separators, the gaps between genomes) as d_runs[2 r] = start, d_runs[2 r + 1] =
 * length.  This call writes the ASCII stream the sketch kernels read to d_seq[0 .. n_bases): "ACGT"[code], 'N' over the
 * runs.  n_bases a multiple of 64, both buffers 16-byte aligned.  Context stream, asynchronous. */
int rtc_unpack_bases_dev(rtc_ctx* ctx, const uint8_t* d_packed, uint64_t n_bases, const uint64_t* d_runs, uint64_t n_runs,
                         uint8_t* d_seq);

/* ---- timing of the last launches (HIP events on the context stream) -------------------- */
/* Brackets subsequently enqueued work; rtc_timer_stop synchronises and returns milliseconds. */
int rtc_timer_start(rtc_ctx* ctx);
int rtc_timer_stop(rtc_ctx* ctx, float* ms_out);

/* ---- synthetic genomes (benchmark / test input) -------------------------- */
typedef struct {
  uint64_t fam_seed; /* ancestor stream */
  uint64_t mut_seed; /* this member's substitution stream */
  uint32_t mut_thr;  /* substitute where a 14-bit draw < mut_thr (rate = mut_thr/16384) */
  uint32_t n_every;  /* 0: none; else an 8-base run of 'N' every n_every bases */
} rtc_synth_desc;
/* Writes genome g's bases (ASCII ACGT/N) to d_seq[h_off[g] .. h_off[g+1]). */
int rtc_synth_genomes_dev(rtc_ctx* ctx, const rtc_synth_desc* h_desc, const uint64_t* h_off,
                          uint32_t n, uint8_t* d_seq);

/* ---- MinHash sketching ----------------------------------------------------------------- */
/* Replaces, for a batch of genomes, `new Sketch::MinHash(k, size)` + `update(seq)` per FASTA
 * record + `storeMinHashes()`  (src/SketchInfo.cpp:918-924, :942, :969; RabbitSketch library).
 * d_seq: concatenated genomes, 16-byte aligned; records of one genome are separated by any
 *   non-ACGT byte (k-mers never span records); lower case is folded to upper.
 * h_off[n+1]: byte offsets of the genomes in d_seq.  h_sizes[n]: sketch size per genome
 *   (fixed-size mode: all equal; containment mode: max(fileBytes/compress,100),
 *   src/SketchInfo.cpp:919-924), or NULL to use `size` for all.
 * d_out: n * stride u64; genome g's ascending distinct hashes at d_out + g*stride;
 * d_cnt[n]: number of hashes produced (< size only when the genome has fewer distinct k-mers).
 * Hash: first 64 bits of MurmurHash3_x64_128(canonical k-mer ASCII, k, seed) for k > 16,
 * first 32 bits for k <= 16 (Mash / RabbitSketch convention). 1 <= k <= 32. */
int rtc_sketch_minhash_dev(rtc_ctx* ctx, const uint8_t* d_seq, const uint64_t* h_off, uint32_t n,
                           int k, uint32_t seed, const uint32_t* h_sizes, uint32_t size,
                           uint64_t* d_out, uint32_t stride, uint32_t* d_cnt);

/* The same sketches straight from a batch in the 2-bit staging format (layout: rtc_unpack_bases_dev above) -- the records
 * `update()` is handed one by one (src/SketchInfo.cpp:928-948) as they crossed PCIe, 0.25 B per base read once, no ASCII
 * copy in HBM.  d_packed (16-byte aligned) holds n_bases / 4 bytes, n_bases a multiple of 64 and >= h_off[n];
 * d_runs[2 r], d_runs[2 r + 1] = start and length of run r of characters outside ACGT, ascending by start and disjoint
 * (record separators and the gaps between genomes are runs too): a k-mer counts exactly when none of its k characters
 * lies in a run nor outside its genome's [h_off[g], h_off[g + 1]) -- what update() does with a character outside ACGT.
 * Every k in 1..32 and every sketch size; everything else as rtc_sketch_minhash_dev, whose results it reproduces bit
 * for bit.  The run list's contract is checked on the device beside the sketching (no host round trip): a violation is
 * reported as RTC_ERR_ARG by rtc_ctx_sync -- call it before the sketches of a packed batch are consumed -- or, failing
 * that, by the next packed call on the context. */
int rtc_sketch_minhash_packed_dev(rtc_ctx* ctx, const uint8_t* d_packed, uint64_t n_bases, const uint64_t* d_runs,
                                  uint64_t n_runs, const uint64_t* h_off, uint32_t n, int k, uint32_t seed,
                                  const uint32_t* h_sizes, uint32_t size, uint64_t* d_out, uint32_t stride,
                                  uint32_t* d_cnt);

/* What the two calls above plan for a batch whose largest sketch size is `size` at this k (both plan alike): workgroups
 * per CU, whether the hash tables take the packed LDS layout, and the dynamic LDS of a workgroup.  Pure host arithmetic
 * (tests and tuning ask it where a layout boundary lies); ctx may be NULL: the options are read from the environment. */
int rtc_sketch_minhash_plan(rtc_ctx* ctx, int k, uint32_t size, int* wgs_per_cu, int* packed_tables, uint64_t* lds_bytes);

/* ---- KSSD sketching (--fast) ------------------------------------------------------------- */
/* Replaces the per-file body of sketchFileWithKssd (src/SketchInfo.cpp:994-1252): 2-bit rolling
 * k-mer (k rounded up to even, :1019-1020), canonical min, shuffled-dimension filter, dr_tuple,
 * dedup, ascending sort.  h_shuffled_dim: the 2^(4*half_subk) table of generate_shuffle_dim
 * (:91-102; built on the host with the same glibc srand/rand calls).
 * width_out: 4 (u32 hashes) or 8 (u64) as decided by half_k - drlevel > 8 (:1021).
 * d_out: n * stride elements of that width; d_cnt[n] = hashes per genome.
 * Returns RTC_ERR_OVERFLOW if some genome yields more than `stride` hashes; h_need (optional)
 * then holds the required stride. */
int rtc_sketch_kssd_dev(rtc_ctx* ctx, const uint8_t* d_seq, const uint64_t* h_off, uint32_t n,
                        int kmer_size, int drlevel, const int32_t* h_shuffled_dim, void* d_out,
                        uint32_t stride, uint32_t* d_cnt, int* width_out, uint32_t* h_need);
/* The same sketches straight from a batch in the 2-bit staging format (see rtc_unpack_bases_dev for the layout): the
 * records sketchFileWithKssd walks (src/SketchInfo.cpp:1120-1166) as they crossed PCIe, 0.25 B per base read once, no
 * ASCII copy in HBM.  d_packed (16-byte aligned) holds n_bases / 4 bytes, n_bases a multiple of 64; d_runs[2 r],
 * d_runs[2 r + 1] = start and length of run r of characters outside ACGT, ascending by start and disjoint -- a k-mer
 * counts exactly when none of its characters lies in a run (:1136-1139, :1160-1164) nor outside its genome's
 * [h_off[g], h_off[g + 1]).  Everything else as rtc_sketch_kssd_dev, whose results it reproduces bit for bit.
 * Returns RTC_ERR_UNSUPPORTED outside the prefilter kernel's configurations (17 <= kmer_size <= 28 with half_subk = 6,
 * i.e. drlevel 3 (the default) or 4: at most 4 096 kept dimensions): callers then expand the batch with rtc_unpack_bases_dev and call rtc_sketch_kssd_dev. */
int rtc_sketch_kssd_packed_dev(rtc_ctx* ctx, const uint8_t* d_packed, uint64_t n_bases, const uint64_t* d_runs,
                               uint64_t n_runs, const uint64_t* h_off, uint32_t n, int kmer_size, int drlevel,
                               const int32_t* h_shuffled_dim, void* d_out, uint32_t stride, uint32_t* d_cnt,
                               int* width_out, uint32_t* h_need);

/* ---- all-pairs sorted-sketch intersection ----------------------------------------------- */
/* common[i][j] = |A_i ∩ A_j| for i in [row0,row1), j in [col0,col1): the integers that
 * compute_minhash_mst / compute_kssd_mst obtain through their inverted index
 * (src/MST.cpp:1408-1435, :428-487) and that modifyMST's distance()/jaccard() calls derive
 * (src/MST.cpp:851-866).  Sketches: `d_hashes` (u64 when width==8, u32 when width==4), genome g
 * occupies d_hashes[d_start[g] .. d_start[g]+d_len[g]) ascending and distinct.
 * d_common: (row1-row0) x ld u32, row-major.  lower_only != 0: only entries with j < i are
 * defined (others are left untouched).  algo: 0 = auto, 1 = per-pair merge (generic),
 * 2 = LDS mask-table tiles. */
int rtc_pair_common_dev(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start,
                        const uint32_t* d_len, uint32_t n, uint32_t row0, uint32_t row1,
                        uint32_t col0, uint32_t col1, uint32_t* d_common, uint64_t ld,
                        int lower_only, int algo);

/* The dense loop's estimator: what Sketch::MinHash::jaccard()/distance() hand to modifyMST
 * (src/MST.cpp:851-866) is Mash's union-truncated Jaccard, NOT the set-Jaccard of the index path: merge
 * the two ascending lists, stop after `sketch_size` elements of the union; d_common = shared elements
 * among them, d_denom = union elements seen (sketch_size unless both lists run out); distance on the host
 * = -ln(2j/(1+j))/k with j = common/denom.  RabbitSketch is absent from the reference tree: this restates
 * the published Mash algorithm and is parity-unpinned like the k-mer hash. */
int rtc_pair_mash_dev(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start,
                      const uint32_t* d_len, uint32_t n, uint32_t sketch_size, uint32_t row0, uint32_t row1,
                      uint32_t col0, uint32_t col1, uint32_t* d_common, uint32_t* d_denom, uint64_t ld);

/* ---- candidate edges ----------------------------------------------------------------------- */
typedef struct { uint32_t i, j, common; } rtc_cedge; /* i > j */
/* Scans the common matrix produced above and appends every pair the reference would turn into
 * an EdgeInfo: j < i, common > 0, both sketches non-empty, max(|A|,|B|) <= radio*min(|A|,|B|)
 * (src/MST.cpp:1468-1487; radio = floor(2*exp(threshold*(k-1))-1), :1292, saturated at INT32_MAX), the
 * product taken exactly in 64 bits (the reference's int product wraps: DESIGN 5).  d_count is a u64
 * counter the caller zeroes; edges beyond `cap` are counted but not stored. */
int rtc_extract_edges_dev(rtc_ctx* ctx, const uint32_t* d_common, uint64_t ld, uint32_t row0,
                          uint32_t row1, uint32_t col0, uint32_t col1, const uint32_t* d_len,
                          int radio, rtc_cedge* d_edges, uint64_t cap, uint64_t* d_count);

/* Fused form of the two calls above for the tile rows [row0,row1) x cols [col0,col1): the
 * surviving (i, j, common), j < i, of the same filters (src/MST.cpp:1468-1487) are appended
 * directly -- no dense matrix is written.  radio < 0 disables the size-ratio test (greedy
 * clustering filters on the host).  d_count as above.  Two device paths with identical results:
 * the inverted join (the reference's index, src/MST.cpp:1408-1435, as a device sort of
 * (hash, genome) + a count of every column's partner lists in on-chip tables; cost ~ hashes +
 * co-occurrences) where the tile is sparse enough for it to win, otherwise the tiled kernel
 * (cost ~ rows x cols x s / 64, independent of the data).  RTC_PAIR_JOIN=0 in the environment
 * disables the join, =2 takes it wherever its scratch fits.
 * Overflow protocol: a count beyond `cap` on return means the list was too short -- grow it to at least the count and call
 * again from the old count.  When the join's density sample says that a list is too short for the set before the tiled
 * kernel has run, the count comes back as an ESTIMATE above `cap` with nothing appended (one launch saved); the repeated
 * call always runs to the end and returns the exact count. */
int rtc_pair_edges_dev(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start,
                       const uint32_t* d_len, uint32_t n, uint32_t row0, uint32_t row1, uint32_t col0,
                       uint32_t col1, int radio, rtc_cedge* d_edges, uint64_t cap, uint64_t* d_count);
/* Which path the last rtc_pair_edges_dev of this context took: 0 none yet, 1 per-pair merge kernel,
 * 2 tiled kernel, 3 inverted join (measurement: bench.py names the kernels of the pair phase by it). */
int rtc_pair_last_path(const rtc_ctx* ctx);
/* Which paths this context has taken since it was created (tests and measurement): out[0] tiles the inverted join took,
 * out[1] tiles the tiled kernel took, out[2] tiles of the merge kernel, out[3] candidate lists contracted to their forest
 * between row chunks, out[4] greedy runs replayed from one global join, out[5] query blocks of greedy's block loop, out[6]
 * estimates rtc_pair_edges_dev handed back instead of a launch; out[7] query chunks rtc_rep_match measured. */
int rtc_diag_counters(const rtc_ctx* ctx, uint64_t out[8]);
/* Duration of this context's last tiled pair kernel launch (rtc_pair_last_path == 2), from HIP events recorded on the
 * stream it was launched on; waits for the launch to finish (measurement: bench.py's roofline_dist). */
int rtc_pair_last_kernel_ms(rtc_ctx* ctx, float* ms_out);

/* ---- minimum spanning forest over candidate edges (Boruvka, order-exact integer weights) -- */
/* One Boruvka round primitive for row-sharded multi-GPU use: for every current component c
 * (d_comp[v] = component label of vertex v) computes the minimum key over the local edges that
 * leave c.  Pass 1 (d_wkey): weight key = bit pattern of the exact rational similarity order
 * (see DESIGN.md); pass 2 (d_ekey): (i<<32|j) among edges attaining d_wkey.  Between the passes
 * the caller all-reduces (MIN) d_wkey across ranks; after pass 2 it all-reduces d_ekey. */
int rtc_boruvka_minweight_dev(rtc_ctx* ctx, const rtc_cedge* d_edges, uint64_t m,
                              const uint32_t* d_len, int is_containment, const uint32_t* d_comp,
                              uint32_t n, uint64_t* d_wkey);
int rtc_boruvka_minedge_dev(rtc_ctx* ctx, const rtc_cedge* d_edges, uint64_t m,
                            const uint32_t* d_len, int is_containment, const uint32_t* d_comp,
                            uint32_t n, const uint64_t* d_wkey, uint64_t* d_ekey);

/* After d_ekey is final (all-reduced), the rank owning each winning edge publishes its `common`
 * into d_ecommon[component] (others leave 0; all-reduce(MAX) across ranks). */
int rtc_boruvka_fetch_dev(rtc_ctx* ctx, const rtc_cedge* d_edges, uint64_t m, const uint32_t* d_comp,
                          uint32_t n, const uint64_t* d_ekey, uint32_t* d_ecommon);

/* Fixed-size mode (every sketch holds exactly s hashes -- the -s configs): the distance
 * (src/MST.cpp:1489-1503) is monotone in `common` alone, so ONE u64 key per component carries weight,
 * edge and count:  key = (s - common) << 2B | i << B | j,  B = rtc_boruvka_key_bits(n, s) (0 when the
 * key would not fit 63 bits -> use the three-pass form).  Across GPUs: one all-reduce(MIN) per round. */
int rtc_boruvka_key_bits(uint32_t n, uint32_t s_fixed);
int rtc_boruvka_minkey_dev(rtc_ctx* ctx, const rtc_cedge* d_edges, uint64_t m, const uint32_t* d_comp,
                           uint32_t n, uint32_t s_fixed, uint64_t* d_key);

/* Round state on the device: d_comp[v] = v, forest counter d_nsel[0] = 0 (d_nsel: two u64). */
int rtc_boruvka_init_dev(rtc_ctx* ctx, uint32_t n, uint32_t* d_comp, uint64_t* d_nsel);
/* Union step of a round on the device (kruskalAlgorithm's union-find work, src/MST.cpp:59-75):
 * every component hooks onto the one its (all-reduced) minimum edge leads to, chosen edges are
 * appended to d_sel (capacity n) and d_comp is relabelled.  s_fixed != 0: d_key holds fused keys;
 * s_fixed == 0: d_key holds edge ids (i<<32|j, the d_ekey of the three-pass form) and d_ecommon the
 * counts.  d_succ: n u32 of scratch.  *h_added = edges added this round (0: forest complete).
 * Synchronises the stream (reads one counter back). */
int rtc_boruvka_union_dev(rtc_ctx* ctx, uint32_t n, uint32_t s_fixed, const uint64_t* d_key,
                          const uint32_t* d_ecommon, uint32_t* d_comp, uint32_t* d_succ, rtc_cedge* d_sel,
                          uint64_t* d_nsel, uint32_t* h_added);

/* All rounds on ONE GPU behind one call: the minimum spanning forest (kruskalAlgorithm's result, src/MST.cpp:59-75) of
 * a device-resident candidate list.  d_sel: n entries; *h_n_sel edges are written; h_rounds may be NULL.  Synchronous.
 * The forest is the one the strict total order (weight key of the double common / denom, then i, then j) leaves, and d_sel
 * holds it in that order.  The call reads the smallest and the largest size and takes the round that fits, the forest being
 * the same in all three: equal sizes whose fused key fits 63 bits, one pass; sizes that vary, with two vertex indices and
 * the longest size's count in 63 bits, two passes (the edge id carries the count, as in rtc_mst and rtc_mst_sharded);
 * otherwise three.  Every pair (i, j) occurs once, i > j, and common <= min(size of i, size of j). */
int rtc_msf_dev(rtc_ctx* ctx, const rtc_cedge* d_edges, uint64_t m, const uint32_t* d_len, uint32_t n, int is_containment,
                rtc_cedge* d_sel, uint64_t* h_n_sel, int* h_rounds);

/* Host helper closing one Boruvka round: unions the components joined by the winning edges
 * (h_ekey[c] = i<<32|j or 0x7FFF...F for none), appends them to h_sel (capacity n) and relabels
 * h_comp[v] with the new root vertex ids.  *h_added == 0 means the forest is complete. */
int rtc_boruvka_merge_host(uint32_t n, const uint64_t* h_ekey, const uint32_t* h_ecommon, uint32_t* h_comp,
                           rtc_cedge* h_sel, uint64_t* h_n_sel, uint64_t* h_added);

/* EdgeInfo of the reference (src/MST.h:17-21); the on-disk edge.mst record (src/MST_IO.cpp:200-217) */
typedef struct { int32_t preNode, sufNode; double dist; } rtc_edge;

/* Host helper: selected forest edges (i, j, common) -> EdgeInfo records with the reference's
 * double arithmetic (src/MST.cpp:1295,1489-1515), sorted by (dist, preNode, sufNode). */
int rtc_edges_to_mst_host(const rtc_cedge* h_sel, uint64_t m, const uint32_t* h_len, int kmer_size,
                          int is_containment, rtc_edge* h_out);

/* Whole single-GPU MST step: compute_minhash_mst / compute_kssd_mst (src/MST.cpp:1290-1737,
 * :216-807) from device-resident sketches.  Distances are evaluated on the HOST with the
 * reference's expression order (src/MST.cpp:1295,1489-1515) so doubles are bit-identical.
 * h_edges_out must hold n entries; *h_n_edges receives the forest size.  Synchronous. */
int rtc_mst(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start,
            const uint32_t* d_len, uint32_t n, int kmer_size, int is_containment, double threshold,
            rtc_edge* h_edges_out, uint64_t* h_n_edges);

/* The start_index form of the same functions (src/MST.cpp:1375-1383, used by append_clust_mst,
 * src/sub_command.cpp:1532-1759): only rows i >= start_index of the pair space (all columns j < i)
 * are evaluated -- the pairs that involve an appended genome -- and the forest over those edges is
 * returned; the caller merges it with the stored MST (sort + kruskalAlgorithm, :1693-1700). */
int rtc_mst_append(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start,
                   const uint32_t* d_len, uint32_t n, uint32_t start_index, int kmer_size, int is_containment,
                   double threshold, rtc_edge* h_edges_out, uint64_t* h_n_edges);

/* The same with the --dense by-products (src/MST.cpp:1333-1352, :1517-1530, :1703-1713): for every
 * candidate pair (the pairs that become EdgeInfo records) with distance d, both genomes are counted
 * in every radius bucket t with t/dense_span >= d, and ANI bin (int)((1-d)*100) is incremented.
 * h_dense: dense_span x n int32 row-major (mst.dense layout, src/MST_IO.cpp:219-233), h_ani: 101 u64
 * (mst.ani).  dense_span = 0: plain rtc_mst_append.  Buckets use the host doubles of the edge weights. */
int rtc_mst_dense(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                  uint32_t n, uint32_t start_index, int kmer_size, int is_containment, double threshold,
                  rtc_edge* h_edges_out, uint64_t* h_n_edges, int dense_span, int32_t* h_dense, uint64_t* h_ani);

/* The dense loop modifyMST (src/MST.cpp:809-1018; reached when the index path is switched off, src/sub_command.cpp:2764,
 * :2995, :1680): EVERY pair i < j with j >= start_index is an edge -- no filters -- weighted by MinHash::distance()
 * (the union-truncated estimator of rtc_pair_mash_dev with `sketch_size`; is_containment != 0: containDistance(),
 * -ln(|A n B| / min(|A|, |B|)) / k) and the minimum spanning TREE over them is returned (pairs without a common hash
 * weigh 1), records {i, j, dist} with i < j as modifyMST builds them.  dense_span / h_dense / h_ani as rtc_mst_dense
 * (here every pair is counted, :868-879).  The estimator restates the published Mash algorithm: parity-unpinned like
 * the k-mer hash (RabbitSketch is absent from the reference tree). */
int rtc_mst_mash(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                 uint32_t n, uint32_t start_index, int kmer_size, int is_containment, uint32_t sketch_size,
                 rtc_edge* h_edges_out, uint64_t* h_n_edges, int dense_span, int32_t* h_dense, uint64_t* h_ani);

/* ---- multi-GPU: RCCL collectives over xGMI and the sharded clust-mst step ----------------- */
/* The reference is one shared-memory process (OpenMP over 8-row blocks of the pair space,
 * src/MST.cpp:1382, and over files, src/SketchInfo.cpp:878).  Here one rtc_comm per rtc_ctx (= per
 * GPU); ranks are processes (one per GPU, the id travels through the launcher's own channel) or
 * host threads of one process.  Every rank sketches its block of genomes; the sketches are gathered
 * into the canonical order (genome g of rank r at row r*n_local + g); the strict lower triangle of
 * the pair space is cut into contiguous row ranges of equal cost; each Boruvka round all-reduces
 * (MIN) one u64 key per component (fixed sketch sizes) or three small arrays (variable sizes). */
typedef struct rtc_comm rtc_comm;
#define RTC_COMM_ID_BYTES 128
int rtc_comm_unique_id(void* id_out /* RTC_COMM_ID_BYTES, created on one rank, passed to all */);
int rtc_comm_init_rank(rtc_ctx* ctx, int nranks, int rank, const void* id, rtc_comm** out); /* collective */
/* One process, one context per GPU, one host thread per context afterwards: communicators for
 * ctxs[0..n).  Contexts that share a device (RCCL rejects duplicate GPUs) get an in-process
 * exchange instead -- the way the protocol is exercised on a one-GPU box. */
int rtc_comm_init_all(rtc_ctx** ctxs, int n, rtc_comm** comms_out);
void rtc_comm_destroy(rtc_comm* comm);
int rtc_comm_rank(const rtc_comm* comm);
int rtc_comm_size(const rtc_comm* comm);
const char* rtc_comm_backend(const rtc_comm* comm); /* "rccl" | "in-process" | "single" */
/* in-place all-reduce on the context stream; dtype 0 = int64, 1 = uint32, 2 = uint64 (the Boruvka key arrays);
 * op 0 = MIN, 1 = MAX */
int rtc_comm_all_reduce(rtc_comm* comm, void* d_buf, size_t count, int dtype, int op);
/* the same for up to 64 host values (agreeing on strides, counts); synchronises */
int rtc_comm_all_reduce_host(rtc_comm* comm, int64_t* h_vals, size_t count, int op);
/* Rows [a,b) of every rank's block of a canonical global buffer (rank r owns rows
 * [r*n_local, (r+1)*n_local), row_bytes each) travel to all ranks, in place (grouped broadcasts).
 * async != 0: on the communicator's side stream, ordered after the work enqueued so far on the
 * context stream; rtc_comm_wait makes the context stream wait for it. */
int rtc_comm_gather_rows(rtc_comm* comm, void* d_global, size_t row_bytes, uint32_t n_local, uint32_t a,
                         uint32_t b, int async);
int rtc_comm_wait(rtc_comm* comm);
/* d_buf[0..bytes) of rank `root` replaces every other rank's copy (context stream) */
int rtc_comm_broadcast(rtc_comm* comm, void* d_buf, size_t bytes, int root);
/* h_bounds[world+1]: row ranges of the strict lower triangle of equal cost, row i costing
 * (i + fixed_cols) columns (fixed_cols: the per-row-block table build; rtc_mst_sharded uses the measured
 * 1.84 x mean sketch size). */
int rtc_triangle_rows(uint32_t n, int world, double fixed_cols, uint32_t* h_bounds);
/* sketchFiles' sketch loop (src/SketchInfo.cpp:878-976) for this rank's genomes, written into its
 * block of the global buffers (d_out_global: size*n_local*stride u64, d_cnt_global: size*n_local)
 * and gathered to all ranks; the gather of the first part overlaps the sketching of the rest. */
int rtc_sketch_minhash_sharded(rtc_ctx* ctx, rtc_comm* comm, const uint8_t* d_seq, const uint64_t* h_off,
                               uint32_t n_local, int k, uint32_t seed, const uint32_t* h_sizes, uint32_t size,
                               uint64_t* d_out_global, uint32_t stride, uint32_t* d_cnt_global);
/* The same phase for a rank whose genomes are resident as batches in the 2-bit staging format (layout: rtc_unpack_bases_dev;
 * what both command lines stage, src/SketchInfo.cpp:928-948 being the records they hold): one call per batch, in the order
 * of the rank's rows.  The batch's n_batch genomes become rows [row_first, row_first + n_batch) of this rank's block of
 * n_local rows; they are sketched straight from the packed bases (rtc_sketch_minhash_packed_dev) and their gather starts on
 * the communicator's side stream behind the sketch kernel, i.e. it travels beside the NEXT batch's kernel.  last != 0 marks
 * the rank's final batch: it is cut in two parts (as rtc_sketch_minhash_sharded cuts a rank's genomes) and the call returns
 * with the context stream waiting for every gather.  Every rank passes the same sequence of (row_first, n_batch) and the
 * same n_local / stride (checked on the first batch).  With one rank the calls sketch into the rows and nothing travels. */
int rtc_sketch_minhash_packed_sharded(rtc_ctx* ctx, rtc_comm* comm, const uint8_t* d_packed, uint64_t n_bases,
                                      const uint64_t* d_runs, uint64_t n_runs, const uint64_t* h_off, uint32_t n_batch,
                                      uint32_t row_first, uint32_t n_local, int last, int k, uint32_t seed,
                                      const uint32_t* h_sizes, uint32_t size, uint64_t* d_out_global, uint32_t stride,
                                      uint32_t* d_cnt_global);
/* --fast: sketchFileWithKssd (src/SketchInfo.cpp:994-1252) over the rank's packed batches, same protocol
 * (rtc_sketch_kssd_packed_dev per batch).  d_out_global: size * n_local * stride tuples of *width_out bytes (4 or 8,
 * src/SketchInfo.cpp:1021).  KSSD sketches vary in length and the rows travel at the caller's stride, so a tight one saves
 * link time.  A batch whose longest sketch exceeds the stride is still gathered -- the ranks' collectives stay matched --
 * and the call with last != 0 returns RTC_ERR_OVERFLOW on EVERY rank with *h_need = the longest sketch any rank produced;
 * the caller repeats the phase with wider rows. */
int rtc_sketch_kssd_packed_sharded(rtc_ctx* ctx, rtc_comm* comm, const uint8_t* d_packed, uint64_t n_bases,
                                   const uint64_t* d_runs, uint64_t n_runs, const uint64_t* h_off, uint32_t n_batch,
                                   uint32_t row_first, uint32_t n_local, int last, int kmer_size, int drlevel,
                                   const int32_t* h_shuffled_dim, void* d_out_global, uint32_t stride,
                                   uint32_t* d_cnt_global, int* width_out, uint32_t* h_need);
typedef struct {
  uint32_t row0, row1;  /* this rank's rows of the pair space */
  uint64_t cand_edges;  /* candidate edges it produced */
  uint32_t rounds, s_fixed, contractions, pad;
  float pair_ms, mst_ms;
} rtc_shard_stats;
/* rtc_mst across the ranks of `comm` (sketches: the complete canonical set, on every rank).  Every
 * rank receives the identical forest, identical to rtc_mst's on one GPU.  stats may be NULL. */
int rtc_mst_sharded(rtc_ctx* ctx, rtc_comm* comm, const void* d_hashes, int width, const uint64_t* d_start,
                    const uint32_t* d_len, uint32_t n, int kmer_size, int is_containment, double threshold,
                    rtc_edge* h_edges_out, uint64_t* h_n_edges, rtc_shard_stats* stats);

/* ---- greedy incremental clustering ------------------------------------------------------- */
/* MinHashGreedyClusterWithInvertedIndex at -t 1 (src/greedy.cpp:986-1399) and
 * KssdGreedyClusterWithInvertedIndex (:566-899; caller sorts by size first, :594-597).
 * Genomes are processed in the given order; the GPU computes query-batch x representative
 * intersections, the host applies the reference's filter / best-match / tie rules.
 * h_size_cfg[n]: what getSketchSize() returns for each genome (configured size, :1201); NULL for
 * KSSD.  h_rep_of[n] receives the representative of each genome (itself if it is one). */
int rtc_greedy(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start,
               const uint32_t* d_len, uint32_t n, const uint32_t* h_size_cfg, int kmer_size,
               int is_containment, int is_kssd, double threshold, int32_t* h_rep_of,
               uint32_t* h_n_clusters);

/* greedyCluster (src/greedy.cpp:285-351), the legacy loop without index and filters: every genome is measured
 * against every current representative with MinHash::distance() (Mash's union-truncated estimator over
 * `sketch_size`) or, for containment sketches, containDistance(); it joins the nearest one within the threshold
 * (earliest of equals) or opens a cluster.  Reached with the index path switched off and by `clust-greedy --append`
 * on MinHash sketches without a stored state (src/sub_command.cpp:91).  Estimator: parity-unpinned (RabbitSketch). */
int rtc_greedy_mash(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                    uint32_t n, int kmer_size, int is_containment, uint32_t sketch_size, double threshold,
                    int32_t* h_rep_of, uint32_t* h_n_clusters);

/* ---- clust-greedy --order degree: representatives that do not depend on the order of the genomes ----------------- */
/* rtc_greedy's clusters are a function of the order the genomes are walked in.  Here the order is a function of the
 * neighbour graph, so the clusters are a function of the set alone.  The reference has no counterpart: this is the definition.
 *
 * Neighbours.  N is symmetric, p != q.
 *   KSSD (is_minhash = 0): rtc_dbscan's predicate at eps = threshold with max_posting = 0 -- both orientations in double with the
 *     1e-12 term and the size bounds, on the count that predicate sees (u32 sketches: saturated at 65 535).  A pair whose
 *     orientations disagree fails the call with RTC_ERR_UNSUPPORTED and is named in the message; so do a threshold whose
 *     jaccard_min t is <= 1e-12 and, for u32 sketches, a size bound ceil(max |sketch| / t) past INT_MAX.
 *   MinHash (is_minhash = 1): rtc_mash_distance(common, denom, sketch_size, kmer_size) <= threshold on the union-truncated
 *     counts, decided through the table rtc_dbscan_mash_table gives -- the device forms no distance.  threshold < 0 or NaN:
 *     RTC_ERR_ARG; threshold >= 1 (pairs without a common hash would be neighbours): RTC_ERR_UNSUPPORTED.  sketch_size: 1 .. 2^28 - 1.
 *   An empty sketch has no neighbours at either width and is a cluster of its own.  This is the one place where N is not
 *   rtc_dbscan's relation: the u64 brute force there makes the empty sketches neighbours of each other.
 * Order.  degree(v) = |N(v)|.  v precedes w iff degree(v) > degree(w), or the degrees are equal and v < w (clust-greedy puts
 *   the larger genome at the lower index, so ties go to the larger genome).
 * Representatives.  Walking the order, v is a representative iff no earlier representative is in N(v): R is the
 *   lexicographically first maximal independent set of the graph under the order.
 * Members.  Every other v joins the representative r in N(v) & R with the largest j(v, r) -- KSSD: common / (|v| + |r| -
 *   common), MinHash: the truncated common / denom -- compared exactly by cross-multiplication in 64 bits; equal j goes to the
 *   r that comes earlier in the order.
 * h_out[v]: rep (v itself for a representative), degree, and the common and denom of the pair (v, rep), both 0 for a
 *   representative.  *h_n_clusters = |R|.  n = 0 is fine (h_out may be NULL).
 *
 * The pair phase is rtc_dbscan's: RTC_EDGE_BUDGET chunks the rows.  The kept pairs (16 bytes each) stay on the device;
 * RTC_ERR_NOMEM when they do not fit, no fallback.  The selection runs in rounds (mark, promote, demote: DESIGN 3.4s) until no
 * vertex is open, with no round cap -- a path of n genomes takes n / 2 rounds.  From RTC_DEGREE_TAIL open vertices down (0:
 * never; default 4 096, measured on one MI355X: DESIGN 3.4s), with at most four times as many edges between them, one workgroup
 * runs the remaining rounds in one launch.  A member's candidate
 * representatives are folded by one wave, by 256 lanes from 4 097 of them on; RTC_DEGREE_BLOCK=1 sends every row through the
 * latter.  Neither switch changes a result.  Synchronous. */
typedef struct { uint32_t rep, degree, common, denom; } rtc_degree_place;
int rtc_greedy_degree(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                      int is_minhash, uint32_t sketch_size, double threshold, int kmer_size, rtc_degree_place* h_out,
                      uint32_t* h_n_clusters);
/* The last rtc_greedy_degree: out[0] row chunks, out[1] candidate edges, out[2] MinHash candidates merged, out[3] pairs kept,
 * out[4] representatives, out[5] selection rounds in the low 32 bits and, of those, the rounds run inside the tail kernel in
 * the high 32, out[6] rows of the assignment on the wave path in the low 32 bits and on the 256-lane path in the high 32,
 * out[7] pair phase ns, out[8] predicate ns, out[9] selection ns (degrees included), out[10] assignment ns, out[11] whole call
 * ns (host clock, each ending in a synchronise). */
int rtc_greedy_degree_counters(const rtc_ctx* ctx, uint64_t out[12]);
/* the paths of the last rtc_greedy_degree: bit 0 the one-wave row path of the assignment, bit 1 the 256-lane path, bit 2 the
 * tail kernel ran */
int rtc_greedy_degree_last_path(const rtc_ctx* ctx);

/* ---- clust-mst post-processing ----------------------------------------------------------- */
/* The --dedup-dist representatives: build_dedup_candidates_per_cluster_core (src/cluster_postprocess.cpp:60-156).  The forest
 * edges with dist <= dedup_dist (h_edges[0..m), EdgeInfo records; those edges must form a forest over n nodes) are joined into
 * groups; every group's representative is its tree medoid, the member with the smallest sum of tree distances to the other
 * members -- ties to the longer sequence (h_seq_len[n], may be NULL), then to the smaller id.  h_node_to_rep[n] receives the
 * representative of every node (itself in a group of one; every node when dedup_dist <= 0, the reference's no-op).  The sums
 * carry the reference's rounding: each distance accumulated outward from the candidate, one add per edge, the members summed
 * in ascending id.  Groups below a measured size are done on the host (rtc_ctx_set_host_threads), the larger ones on the GPU,
 * one wave per candidate; RTC_DEDUP_GPU=0 keeps every group on the host, =2 sends every group of two or more to the GPU.
 * Synchronous. */
int rtc_tree_medoids(rtc_ctx* ctx, uint32_t n, const rtc_edge* h_edges, uint64_t m, double dedup_dist, const uint64_t* h_seq_len,
                     int32_t* h_node_to_rep);
/* Where the last rtc_tree_medoids of this context computed its sums: 0 nowhere (no group of two or more), 1 host only,
 * 2 GPU only, 3 both (tests and measurement). */
int rtc_dedup_last_path(const rtc_ctx* ctx);
/* Host threads of the context's host-side work (rtc_tree_medoids' small groups); default 1. */
int rtc_ctx_set_host_threads(rtc_ctx* ctx, int threads);

/* ---- clust-mst --append against a --save-rep state ------------------------------------- */
typedef struct { uint32_t query, slot, common, pad; double dist; } rtc_rep_pair;
/* The measuring half of MinHashMstAppendCluster / KssdMstAppendCluster (src/mst_state.cpp:681-1106).  The set holds
 * n_reps representatives (genomes [0, n_reps)) followed by n_queries new sketches (genome n_reps + q is query q).  Every
 * pair (query q, slot s) with s < n_reps + q -- an old representative, or an earlier query that may have become one -- that
 * shares a hash and passes the reference's filters is written: is_kssd: sizeQry / sizeRef within [1 / radio, radio],
 * radio = exp(threshold k); common >= (int)(jmin min(sizeQry, sizeRef)) (is_containment) or
 * (int)(jmin (sizeQry + sizeRef) / (1 + jmin)), jmin = e / (2 - e), e = exp(-threshold k); the distance -ln(2j / (1 + j)) / k
 * from the full-set common (j = common / min(sizes) or common / (sizeQry + sizeRef - common), capped at 1) is <= threshold,
 * neither NaN nor Inf.  dist is the host libm's value.  h_pairs[0 .. min(*n_pairs, cap)) sorted by (query, slot); *n_pairs
 * beyond cap: call again with a buffer that large.  query_chunk > 0 measures that many queries at a time (0: all at once);
 * a chunk whose scratch does not fit is halved and measured again.  Synchronous. */
int rtc_rep_match(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                  uint32_t n_reps, uint32_t n_queries, int kmer_size, int is_kssd, int is_containment, double threshold,
                  uint32_t query_chunk, rtc_rep_pair* h_pairs, uint64_t cap, uint64_t* n_pairs);

/* ---- clust-mst --db --query / --assign: the best representatives of every query ---------------- */
typedef struct { uint32_t query, slot, common, denom; } rtc_rep_hit;
/* The search of MinHashMstQueryTopK / KssdMstQueryTopK (src/mst_state.cpp:1211-1340).  The set holds n_reps representatives
 * (genomes [0, n_reps)) followed by n_queries queries (genome n_reps + q is query q).  A candidate of query q is every live
 * slot s < n_reps (h_live == NULL, or h_live[s] != 0) that shares a hash with it; queries never see each other.  (common,
 * denom) by wmode: 0 set Jaccard (denom = |A| + |B| - common), 1 containment (denom = min(|A|, |B|)), 2 | s << 2 Mash's
 * union-truncated estimator with sketch size s > 0 (common and denom recounted over the first s union elements, as
 * rtc_pair_mash_dev).  Every query keeps its best topk candidates (topk == 0: all of them): larger common / denom first,
 * compared exactly; equal keys by the lower slot.  h_hits[0 .. min(*n_hits, cap)) sorted by (query, rank); h_per_query
 * (n_queries entries, may be NULL) receives the number kept for each query; *n_hits beyond cap: call again with a buffer that
 * large.  query_chunk > 0 measures that many queries at a time (0: all at once); a chunk whose scratch does not fit is halved
 * and measured again.  The device forms no distance.  topk in [1, 256] selects on the device; topk == 0 and topk > 256 sort
 * every segment on the host.  Synchronous. */
int rtc_rep_topk(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                 uint32_t n_reps, uint32_t n_queries, const uint8_t* h_live, int wmode, uint32_t topk,
                 uint32_t query_chunk, rtc_rep_hit* h_hits, uint64_t cap, uint64_t* n_hits, uint32_t* h_per_query);
/* Which selection paths the last rtc_rep_topk call took: bit 0 the one-wave workgroup (segments of up to 4 096 candidates),
 * bit 1 the 256-lane workgroup (longer segments), bit 2 the full-segment host sort (topk == 0 or topk > 256). */
int rtc_rep_topk_last_path(const rtc_ctx* ctx);
/* What the last rtc_rep_topk call did: out[0] query chunks measured, out[1] / out[2] / out[3] queries selected by the wave /
 * workgroup / full-sort path, out[4] candidates, out[5] bytes read back, out[6] join ns, out[7] bucketing ns (count, scan,
 * scatter), out[8] selection ns (with the read-back), out[9] reserved. */
int rtc_rep_topk_counters(const rtc_ctx* ctx, uint64_t out[10]);

/* ---- clust-mst --db --screen: which representatives a sample contains --------------------------- */
typedef struct { uint32_t query, slot, common, size, unique, rank; } rtc_screen_hit;
typedef struct { uint32_t n_hashes, n_matched, n_explained, n_hits, n_picks, pad; } rtc_screen_sum;
/* Containment of every representative in every sample, and a winner-takes-all decomposition of the sample (what mash screen -w
 * and sourmash gather give), for KSSD sketches: a fixed subsample of k-mer space, so |X n P| / |P| is an unbiased containment
 * whatever the two sizes.  The set is laid out as for rtc_rep_topk: n_reps representatives, then n_queries samples, ascending
 * lists of distinct hashes, width 4 or 8, empty lists allowed.  For a sample X and a slot p with hash set P:
 *   eligible  h_live == NULL or h_live[p] != 0; |P| > 0; common = |X n P| >= max(1, min_common); and
 *             common * 2^20 >= min_cont_q20 * |P| in 64-bit integers (min_cont_q20 = llround(min_containment * 2^20), formed by
 *             the caller; 0: no containment test).  The device forms no quotient and no floating-point number.
 *   matched   the hashes of X that lie in at least one eligible slot.
 *   gather    R = matched.  In round t = 1, 2, ... every eligible slot not yet picked has u_p = |R n P|; the pick is the slot
 *             with the largest u_p, equal counts to the lower slot.  The rounds end when that u_p < min_unique (>= 1), when no
 *             unpicked slot is left, or when max_picks > 0 picks have been made; otherwise the pick gets rank = t and
 *             unique = u_p, and R <- R \ P.  A sample takes at most as many rounds as it has eligible slots.
 *   hits      every eligible slot, (query, slot, common, size = |P|, unique, rank): for a pick unique is its count when picked;
 *             for the others rank = 0 and unique is what was left of them when the rounds ended.  A query's picks come first,
 *             by rank; the rest follow by common / size, larger first, compared exactly by 64-bit cross-multiplication, equal
 *             ratios to the lower slot.
 *   summary   n_hashes = |X|, n_matched, n_explained = n_matched - |R| at the end (the sum of unique over the picks), n_hits,
 *             n_picks.
 * Queries never see each other and the database is not changed.  Everything is an integer: the result depends on no kernel
 * path, chunking or scheduling.  h_hits[0 .. min(*n_hits, cap)) is sorted by query, then in the order above; *n_hits beyond
 * cap: call again with a buffer that large (h_sum[n_queries] is complete either way).  query_chunk > 0 screens that many
 * samples at a time (0: all at once).  A chunk's match records and views are charged against RTC_SCREEN_BYTES (default: half
 * the free HBM; csrc/rtc_screen.h has the rates); a chunk that does not fit is halved and screened again, a single sample that
 * does not fit is RTC_ERR_NOMEM, as is one with 2^32 - 1 match records or more.  RTC_ERR_ARG: min_unique == 0, min_cont_q20 >
 * 2^20, h_sum == NULL with n_queries > 0, a width other than 4 or 8, n_reps + n_queries >= 2^31 - 1.  RTC_ERR_UNSUPPORTED: a
 * sketch of 2^31 hashes or more.  One workgroup runs all rounds of one sample, by its number of eligible slots on one of three
 * paths; RTC_SCREEN_GLOBAL=1 sends every sample through the last one.  Synchronous. */
int rtc_rep_screen(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                   uint32_t n_reps, uint32_t n_queries, const uint8_t* h_live, uint32_t min_common, uint32_t min_cont_q20,
                   uint32_t min_unique, uint32_t max_picks, uint32_t query_chunk, rtc_screen_hit* h_hits, uint64_t cap,
                   uint64_t* n_hits, rtc_screen_sum* h_sum);
/* What the last rtc_rep_screen call did: out[0] query chunks screened, out[1] match records, out[2] candidates (pairs that share
 * a hash), out[3] eligible candidates, out[4] picks, out[5] the most rounds any sample took, out[6] / out[7] / out[8] samples
 * gathered by the wave / workgroup / global path, out[9] expansion ns (index, join, candidates, views), out[10] gather ns (with
 * the read-back), out[11] the whole call's ns. */
int rtc_rep_screen_counters(const rtc_ctx* ctx, uint64_t out[12]);
/* Which gather paths the last rtc_rep_screen call took: bit 0 one wave (u in LDS), bit 1 a 256-lane workgroup (u in LDS),
 * bit 2 a 256-lane workgroup with u in global memory. */
int rtc_rep_screen_last_path(const rtc_ctx* ctx);
/* Mash's containment identity, host only: 1 if common == size, 0 if common == 0, else pow(common / size, 1 / kmer_size). */
double rtc_screen_identity(uint32_t common, uint32_t size, int kmer_size);

/* ---- clust-dbscan --fast: KSSD DBSCAN on one GPU ----------------------------------------------------- */
/* KssdDBSCAN (src/dbscan.cpp:725-985) without --knn.  Neighbours are findNeighborsKSSDWithIndex's (:366-612): p != q, both
 * non-empty, floor(t |p|) <= |q| <= ceil(|p| / t) and !(common (1 + t) + 1e-12 < t |p| + t |q|) in double, t = x / (2 - x),
 * x = exp(-eps kmer_size) on the host (:751-752).  width 4 (u32, the inverted index): common is the u16 count of MarkCnt,
 * min(common, 65535), and max_posting > 0 drops every hash held by more than max_posting sketches before counting (:95-130)
 * while |p| and |q| stay the unpruned sizes.  width 8 (u64, the brute force :383-445): no saturation, no pruning, and the
 * empty sketches are neighbours of each other.  A core point has |N(p)| + 1 >= min_pts.  h_labels[n]: the cluster of every
 * point, numbered in the order the reference's walk opens them (by smallest core index), -1 for noise; border points join the
 * lowest-numbered cluster among their core neighbours'.  h_core[n] (may be NULL): 1 for the core points.  Returns RTC_ERR_UNSUPPORTED where the reference's relation is not
 * symmetric or not defined: t <= 1e-12, ceil(max |p| / t) > INT_MAX for u32 sketches, or a candidate pair whose two
 * orientations disagree (the message names it).  RTC_EDGE_BUDGET bounds the candidate edges of one row chunk.  Synchronous. */
int rtc_dbscan(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
               double eps, int min_pts, int kmer_size, int max_posting, int32_t* h_labels, uint8_t* h_core,
               uint32_t* h_n_clusters, uint32_t* h_n_noise);
/* What the last rtc_dbscan call did: out[0] row chunks of the pair phase, out[1] candidate edges (pairs sharing a hash),
 * out[2] eps edges, out[3] core points, out[4] pairs whose orientations disagreed, out[5] hook rounds, out[6] pair phase ns,
 * out[7] eps filter ns, out[8] components and labels ns, out[9] whole call ns. */
int rtc_dbscan_counters(const rtc_ctx* ctx, uint64_t out[10]);

/* ---- clust-dbscan --knn: KssdDBSCAN over the reference's k-NN graph ------------------------------------ */
/* KssdDBSCAN with knn_k > 0 (src/dbscan.cpp:725-982): every point's neighbourhood is cut to its knn_k best-scoring candidates
 * before the eps test, which makes the relation DIRECTED.  t, the sizes, max_posting and the count `common` are rtc_dbscan's.
 * Per point p of a u32 set (buildKNNForPoint, :221-360):
 *   candidates: c != p sharing a kept hash with p, floor(t |p|) <= |c| <= ceil(|p| / t); an empty sketch has none;
 *   arrival order (the `touched` list, :271-300): ascending by (the smallest index in p's hash list of a kept hash that c
 *     holds too, c);
 *   passers (:333-338): the candidates with !(common (1 + t) + 1e-12 < t |p| + t |c|) in double, scored
 *     (float)common / (float)(|p| + |c| - common), one correctly rounded binary32 division (:341-342);
 *   selection (:344-349): the passers go in arrival order through a min-heap of (score, id) of capacity knn_k -- pushed while
 *     it holds fewer, otherwise replacing its minimum (lowest score, then lowest id) only when score > that minimum's score;
 *   N(p) (:444-454): the heap's members with (double)score >= t -- a second test, not the passers' one: a passer that fails it
 *     still took a heap slot.
 * p is a core point when |N(p)| + 1 >= min_pts, and the walk of :813-929 runs over these directed lists.  Both order-dependent
 * steps are computed by their closed forms, which give the walk's result exactly: with s* the knn_k-th largest
 * score of a row of more than knn_k passers and T the arrival of the knn_k-th passer at or above s*, the heap ends as every
 * passer above s* plus the passers at s* that arrive no later than T, without the h of them with the lowest ids, h = the
 * passers above s* arriving after T; and with edges p -> q for core p and q in N(p), m(v) = the smallest core index u with a
 * path u -> ... -> v whose vertices other than v are all core (v itself for an empty path), v is noise (-1) when there is no
 * such u and otherwise in the cluster numbered by the rank of m(v) among the distinct values of m -- core and border points
 * alike.  h_core[n] (may be NULL): 1 for the core points.
 * knn_k <= 0 (the reference builds no graph) and width 8 (its u64 brute force never reads the graph, :384-442) are rtc_dbscan's
 * call with the same arguments.  knn_k < min_pts - 1 is raised to min_pts - 1 (:754-757).  Returns RTC_ERR_UNSUPPORTED for
 * t <= 1e-12 and ceil(max |p| / t) > INT_MAX as rtc_dbscan does; a pair whose two orientations disagree is NO failure here:
 * each orientation is evaluated on its own, as the reference does.  RTC_EDGE_BUDGET bounds the candidate edges of one row chunk;
 * RTC_ERR_NOMEM past the device's memory, no fallback.  Synchronous. */
int rtc_dbscan_knn(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                   double eps, int min_pts, int kmer_size, int max_posting, int knn_k, int32_t* h_labels, uint8_t* h_core,
                   uint32_t* h_n_clusters, uint32_t* h_n_noise);
/* What the last rtc_dbscan_knn call did (all 0 where it was rtc_dbscan's call): out[0] row chunks, out[1] candidate edges,
 * out[2] directed passers, out[3] rows truncated (more than knn_k passers), out[4] rows that needed arrival keys (more than
 * knn_k passers at or above s*), out[5] directed neighbour edges kept, out[6] core points, out[7] propagation rounds, out[8]
 * selection ns (passers, sorts, arrival keys, neighbours), out[9] whole call ns. */
int rtc_dbscan_knn_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* The last rtc_dbscan_knn call's propagation and labelling, ns. */
uint64_t rtc_dbscan_knn_propagate_ns(const rtc_ctx* ctx);

/* ---- clust-dbscan --eps-sweep / --kdist: many eps values and the k-distance curve from one pair phase ---------- */
/* A point's k-th nearest candidate, k = min_pts - 1: j = common / (size_p + size_q - common).  neighbour = UINT32_MAX: the
 * point has fewer than k candidates (the other fields are 0 but size_p). */
typedef struct { uint32_t common, size_p, size_q, neighbour; } rtc_kdist;
/* rtc_dbscan for n_eps values of eps (1 .. 32, any order, duplicates allowed) with ONE pair phase.  Row e of h_labels
 * [n_eps x n] and h_core [n_eps x n, may be NULL] and entry e of h_n_clusters / h_n_noise [n_eps, may be NULL] are exactly what
 * rtc_dbscan returns for h_eps[e] with the same other arguments.  Whatever makes rtc_dbscan return RTC_ERR_UNSUPPORTED for one
 * of the values fails the whole call; the message names that eps.
 * h_kdist [n, may be NULL]: among the points sharing at least one (kept) hash with p, ranked by j compared exactly as integers
 * (larger first; common is the count the predicate sees, min(common, 65535) over the pruned sketches at width 4; the sizes
 * are the unpruned ones; equal j: the lower index first), the k-th.  k <= 0: {|p|, |p|, |p|, p} (j = 1).  At width 8 the
 * empty sketches see each other at j = 1, as rtc_dbscan's predicate accepts them at every eps; at width 4 an empty sketch has no
 * candidates.  The device forms no distance: the caller computes -ln(2 j / (1 + j)) / kmer_size with its libm.  The integer order
 * is exact for sketches of up to 2^31 - 1 hashes; a longer one returns RTC_ERR_UNSUPPORTED when the curve is asked for.
 * k <= 256 selects on the device chunk by chunk; a larger k reads every candidate chunk back and selects on the host.
 * n_eps == 0 with h_kdist computes the curve alone.  Synchronous. */
int rtc_dbscan_sweep(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                     const double* h_eps, uint32_t n_eps, int min_pts, int kmer_size, int max_posting, int32_t* h_labels,
                     uint8_t* h_core, uint32_t* h_n_clusters, uint32_t* h_n_noise, rtc_kdist* h_kdist);
/* What the last rtc_dbscan_sweep call did: out[0] row chunks and out[1] candidate edges of its one pair phase, out[2] pairs
 * kept (passing at some level), out[3] levels, out[4] hook rounds (the level that took longest), out[5] pair phase ns, out[6]
 * predicate ns, out[7] components and labels ns, out[8] k-distance ns, out[9] whole call ns. */
int rtc_dbscan_sweep_counters(const rtc_ctx* ctx, uint64_t out[10]);

/* ---- clust-dbscan --minhash: DBSCAN over MinHash sketches -------------------------------------- */
/* MinHashDBSCAN (src/dbscan.cpp:685-720, :987-1096; the reference's command line never reaches it) for the levels h_eps[0 ..
 * n_eps), 1 <= n_eps <= 32, any order, duplicates allowed, from ONE pair phase.  The sketches are ascending lists of distinct
 * hashes of at most sketch_size elements (shorter and empty ones allowed).  dist(p, q) is MinHash::distance() as
 * rtc_pair_mash_dev restates it: (common, denom) of the merge truncated after sketch_size union elements, j = common / denom
 * in double, 1 when j == 0, 0 when j == 1, otherwise min(1, -ln(2j / (1 + j)) / kmer_size) with the host's libm
 * (rtc_mash_distance) -- parity-unpinned against RabbitSketch like rtc_mst_mash.  q is a neighbour of p iff q != p and
 * dist(p, q) <= eps in double; the relation is symmetric.  p is a core point iff it has at least min_pts neighbours, ITSELF NOT
 * COUNTED (:1017, :1050; rtc_dbscan's rule counts it).  min_pts <= 0 makes every point a core point; a negative min_pts is
 * treated like 0 (the reference compares it against an unsigned size, which no caller can mean).  Labels, h_core, h_n_clusters
 * and h_n_noise exactly as rtc_dbscan_sweep's: clusters are the components of the core points over core-core eps edges,
 * numbered by their smallest core index; a non-core point with a core neighbour joins the lowest-numbered cluster among its
 * core neighbours'; every other point is -1.  The device forms no distance: the host turns every eps into the least common
 * that passes for every denom (rtc_dbscan_mash_table) and the device compares counts.
 * 0 <= eps < 1: eps < 0 or NaN returns RTC_ERR_ARG; eps >= 1 returns RTC_ERR_UNSUPPORTED (pairs without a common hash have
 * distance 1 and no candidate list holds them).  RTC_EDGE_BUDGET chunks the rows as in rtc_dbscan; RTC_ERR_NOMEM as there, no
 * fallback.  RTC_DBSCAN_MASH_SERIAL=1: the per-thread merge instead of the wave-cooperative one; RTC_DBSCAN_MASH_NOPREFILTER=1:
 * no candidate is dropped before the merge; results are identical either way.  Synchronous. */
int rtc_dbscan_mash(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                    uint32_t sketch_size, const double* h_eps, uint32_t n_eps, int min_pts, int kmer_size, int32_t* h_labels,
                    uint8_t* h_core, uint32_t* h_n_clusters, uint32_t* h_n_noise);
/* What the last rtc_dbscan_mash call did: out[0] row chunks, out[1] candidate edges, out[2] candidates merged (past the
 * prefilter), out[3] pairs kept (passing at some level), out[4] levels, out[5] hook rounds, out[6] pair phase ns, out[7]
 * predicate ns, out[8] components and labels ns, out[9] whole call ns. */
int rtc_dbscan_mash_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* The distance above for a given (common, denom <= sketch_size), and rtc_dbscan_mash's decision table for one eps in [0, 1):
 * out[d], d = 0 .. sketch_size, is the least common with rtc_mash_distance(common, d) <= eps, d + 1 where none passes.  Host
 * only, no context. */
double rtc_mash_distance(uint32_t common, uint32_t denom, uint32_t sketch_size, int kmer_size);
int rtc_dbscan_mash_table(uint32_t sketch_size, int kmer_size, double eps, uint32_t* out);
/* The recount of rtc_dbscan_mash on its own: d_common[e], d_denom[e] = the union-truncated counts of rtc_pair_mash_dev for the
 * pair (d_edges[e].i, d_edges[e].j), e < m, both below n (the edge's own count is ignored).  Context stream, asynchronous. */
int rtc_pair_mash_edges_dev(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                            uint32_t sketch_size, const rtc_cedge* d_edges, uint64_t m, uint32_t* d_common, uint32_t* d_denom);

/* ---- clust-dbscan --hierarchy: the density hierarchy (HDBSCAN*) of the neighbour graph at eps_max ------------- */
/* One edge of the hierarchy: its mutual-reachability similarity is m = common / (size_p + size_q - common), p < q
 * (size_p = size_q = common = 0: m = 1, two empty u64 sketches). */
typedef struct { uint32_t p, q, common, size_p, size_q; } rtc_hedge;
/* The maximum spanning forest of the mutual-reachability relation over the pairs rtc_dbscan keeps at eps_max (both
 * orientations of its predicate; the same common, sizes, max_posting and empty u64 sketches), from ONE pair phase.
 *   j(p, q) = common / (|p| + |q| - common), compared exactly by 64-bit cross-multiplication (sketches of up to 2^31 - 1 hashes;
 *             a longer one returns RTC_ERR_UNSUPPORTED);
 *   jcore(p) = the j of h_core[p], which is exactly rtc_dbscan_sweep's h_kdist[p] (k = min_pts - 1, ranked over all candidates);
 *             neighbour = UINT32_MAX: p has no core level, is never a core point, and its edges are not part of the forest;
 *   m(p, q) = min(j(p, q), jcore(p), jcore(q)); the edge carries the triple of the term that limits it: the pair's own
 *             (common, |p|, |q|) unless jcore(p) is strictly smaller, then h_core[p]'s, unless jcore(q) is strictly smaller
 *             than that, then h_core[q]'s (p < q).
 * The forest is the one Kruskal's algorithm builds under the total order (larger m first, then smaller p, then smaller q), and
 * h_forest [n - 1 slots] holds its *h_n_forest edges in that order.  The device forms no distance: an edge's distance is
 * -ln(2 m / (1 + m)) / kmer_size with the caller's libm (kmer_size only enters t(eps_max)).  Fails as rtc_dbscan_sweep fails
 * for the single level eps_max (RTC_ERR_UNSUPPORTED, RTC_ERR_NOMEM: no fallback).  Synchronous. */
int rtc_dbscan_hierarchy(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                         double eps_max, int min_pts, int kmer_size, int max_posting, rtc_hedge* h_forest, uint64_t* h_n_forest,
                         rtc_kdist* h_core);
/* rtc_dbscan_sweep and rtc_dbscan_hierarchy from ONE pair phase (what clust-dbscan --hierarchy --eps-sweep --kdist runs):
 * the arguments and results of both, each exactly as from its own call; both counter sets are filled.  n_eps may be 0. */
int rtc_dbscan_sweep_hierarchy(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                               const double* h_eps, uint32_t n_eps, int min_pts, int kmer_size, int max_posting, int32_t* h_labels,
                               uint8_t* h_core_flags, uint32_t* h_n_clusters, uint32_t* h_n_noise, rtc_kdist* h_kdist, double eps_max,
                               rtc_hedge* h_forest, uint64_t* h_n_forest, rtc_kdist* h_core);
/* What the last hierarchy call did: out[0] row chunks and out[1] candidate edges of its pair phase, out[2] pairs kept at
 * eps_max, out[3] forest edges, out[4] Boruvka rounds, out[5] pair phase ns, out[6] k-distance ns, out[7] filter, weights and
 * ranking ns, out[8] forest ns, out[9] whole call ns. */
int rtc_dbscan_hierarchy_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* DBSCAN*'s clusters at eps <= eps_max from a hierarchy (host only, O(n alpha)).  t = t(eps) as rtc_dbscan forms it.  p is a
 * core point iff h_core[p] has a neighbour and its triple passes rtc_dbscan's predicate at t in both orientations (in double,
 * with the 1e-12 term; the triple 0, 0, 0 passes, as two empty u64 sketches do).  A forest edge joins its ends iff both are core
 * points and its triple passes the same test.  h_labels[n]: clusters numbered by their smallest core index; every non-core
 * point is -1 -- there is NO border attachment (DBSCAN*), unlike rtc_dbscan, whose labels agree with these on the core points.
 * h_is_core[n] may be NULL.  eps > eps_max (the value the hierarchy was built with) or eps <= 0: RTC_ERR_ARG; t <= 1e-12:
 * RTC_ERR_UNSUPPORTED. */
int rtc_hierarchy_cut(uint32_t n, const rtc_hedge* h_forest, uint64_t n_forest, const rtc_kdist* h_core, double eps_max, double eps,
                      int kmer_size, int32_t* h_labels, uint8_t* h_is_core, uint32_t* n_clusters);
/* A flat clustering without eps (host only, O(n log n)): the condensed tree of the forest, selected by excess of mass.
 *   - distance(e) = -ln(2 m / (1 + m)) / kmer_size (0 at m = 1), lambda(e) = 1 / max(distance(e), 1e-12).
 *   - The forest's edges, taken in forest order, merge components into a binary dendrogram (left child: p's side, right: q's).
 *     Points without a core level are outside it.  Each tree with at least min_cluster_size (>= 2) points is a top-level cluster
 *     born at lambda 0; the points of a smaller tree are -1.
 *   - Walking down, a merge at lambda whose two sides both hold >= min_cluster_size points ends its cluster and starts two
 *     children born at lambda; a side with fewer points falls out of the cluster at lambda and its points stay attached to it.
 *     Each such event adds  points leaving x (lambda - lambda of the cluster's birth)  to the cluster's stability, one term per
 *     merge, the terms added in forest order.
 *   - Selection from the leaves up: a cluster is selected iff its stability is strictly greater than the sum (left + right) of
 *     its children's best -- on a tie the children win -- and its best is the larger of the two.  A top-level cluster that is
 *     the only one and has children is the root and is not selected.
 *   - h_labels[n]: a point takes the selected cluster it fell out of or the nearest selected ancestor of that, else -1; clusters are
 *     numbered by their smallest member.  h_stability [as many as clusters, at most n / min_cluster_size; may be NULL]. */
int rtc_hierarchy_flat(uint32_t n, const rtc_hedge* h_forest, uint64_t n_forest, const rtc_kdist* h_core, int kmer_size,
                       int min_cluster_size, int32_t* h_labels, double* h_stability, uint32_t* n_clusters);

/* ---- clust-dbscan --db --assign: new points placed into a clustered set ------------------------------- */
/* DBSCAN's border rule applied to a point that was not there.  The reference has nothing of the kind: this is the definition.
 * A model is a clustered sketch set: the rows [0, n_db) of the set with rtc_dbscan's (is_minhash = 0) or rtc_dbscan_mash's
 * (is_minhash = 1, sketch_size as there) labels h_labels[n_db] and core flags h_core[n_db] for ONE (eps, min_pts, kmer_size),
 * clustered WITHOUT max_posting.  The rows [n_db, n_db + n_queries) are the queries, the layout of rtc_rep_topk.  For a query q:
 *   - N(q): the model points p the model's own predicate accepts.  KSSD: rtc_dbscan's, both orientations in double with the
 *     1e-12 term and the size bounds, on the count that predicate sees (saturated at 65 535 at width 4); at width 8 an empty
 *     query is the neighbour of every empty model sketch and of nothing else, at width 4 of nothing.  A pair whose two
 *     orientations disagree fails the call with RTC_ERR_UNSUPPORTED, the message naming the pair.  MinHash:
 *     rtc_mash_distance(common, denom) <= eps, decided through rtc_dbscan_mash_table; the device forms no distance.
 *   - label / label_max: the lowest / highest cluster number among the CORE points of N(q), both -1 where there is none (noise;
 *     the command line prints "novel").  label != label_max: q would bridge clusters.
 *   - n_neighbours = |N(q)|, n_core = the core points among them.
 *   - flags bit 0: q would itself be a core point -- KSSD n_neighbours + 1 >= min_pts, MinHash n_neighbours >= max(min_pts, 0).
 *   - nearest, common, denom: over ALL model points sharing a hash with q, in N(q) or not, the one with the largest
 *     common / denom, compared exactly by 64-bit cross-multiplication (common_a * denom_b against common_b * denom_a) as
 *     rtc_rep_topk compares; equal keys go to the lower index.  KSSD: common as above, denom = |p| + |q| - common; MinHash: the
 *     union-truncated counts.  nearest = UINT32_MAX and zeros when q shares no hash with the model.  The caller forms the
 *     distance with its libm.
 *   - Queries never see each other, and the model is not changed.
 * Anchor: if adding q last to a set S changes no core flag of S and q is not a core point of S + {q}, DBSCAN on S + {q}
 * labels S as it labels S alone and gives q exactly `label`.
 * query_chunk: queries per join (0: all); a chunk whose candidates exceed RTC_EDGE_BUDGET or whose join scratch does not fit
 * is halved -- down to one join per query, each with its three host round trips -- and RTC_ERR_NOMEM past one query; no fallback.  Errors as rtc_dbscan / rtc_dbscan_mash for the kind: MinHash eps < 0
 * or NaN RTC_ERR_ARG, eps >= 1 RTC_ERR_UNSUPPORTED; KSSD jaccard_min <= 1e-12 and, at width 4, a size bound past INT_MAX
 * RTC_ERR_UNSUPPORTED; h_labels or h_core NULL with n_db > 0 RTC_ERR_ARG.  Containment sketches are out of scope.  Synchronous. */
typedef struct { int32_t label, label_max; uint32_t n_neighbours, n_core, nearest, common, denom, flags; } rtc_dbscan_place;
int rtc_dbscan_assign(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                      uint32_t n_db, uint32_t n_queries, const int32_t* h_labels, const uint8_t* h_core,
                      int is_minhash, uint32_t sketch_size, double eps, int min_pts, int kmer_size,
                      uint32_t query_chunk, rtc_dbscan_place* h_out);
/* What the last rtc_dbscan_assign call did: out[0] query chunks, out[1] candidates (pairs sharing a hash; a MinHash model merges
 * every one of them, a KSSD model none), out[2] neighbours found (the sum of n_neighbours), out[3] queries placed (label >= 0),
 * out[4] novel, out[5] bridging (among the placed), out[6] join ns, out[7] predicate and bucketing ns, out[8] fold ns, out[9]
 * whole call ns.  A call that fails after its argument checks leaves zeros. */
int rtc_dbscan_assign_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* The fold paths of the last rtc_dbscan_assign call: bit 0 one wave per query (segments of up to 4 096 candidates), bit 1 a
 * 256-lane workgroup (the longer ones). */
int rtc_dbscan_assign_last_path(const rtc_ctx* ctx);

/* ---- clust-dbscan --db --update: new points added to a clustered set, exactly ------------------------------ */
/* The layout is rtc_dbscan_assign's: rows [0, n_old) are the model, rows [n_old, n_old + n_new) the new points, n = their sum.
 * RESULT: h_labels[n], h_core[n] (may be NULL), *h_n_clusters, *h_n_noise equal those of rtc_dbscan (is_minhash = 0, max_posting 0)
 * or of rtc_dbscan_mash with this one eps (is_minhash = 1, sketch_size as there) on all n rows -- as long as h_labels_old[n_old]
 * and h_core_old[n_old] are that call's output on the first n_old rows for the same (eps, min_pts, kmer_size).  Only the rows
 * that can change anything are joined.  The neighbour relation is the kind's; a point is a core point iff
 *     KSSD:     |N(v)| + 1 >= min_pts   (the point counts itself; at width 8 the empty sketches are neighbours of each other)
 *     MinHash:  |N(v)| >= max(min_pts, 0), the point itself not counted (min_pts <= 0: every point is a core point).
 * The rule.  Neighbour counts only grow, so an old core point stays one.  Two old core points within eps of each other are in
 * one old cluster already, so every old core-core edge is implied by the old labels: each old core point starts under the
 * smallest core index of its old cluster.  An old non-core point can become a core point ("promoted") only by a new neighbour.
 * A non-core point takes the lowest-numbered cluster among its core neighbours', clusters are numbered by their smallest core
 * index, and a promoted point can renumber them: an old border point needs all of its core neighbours again.  So:
 *   stage 1: rows = the new points, columns = everything below the row: every new-old and new-new eps edge.  T = the old NOISE
 *            points with at least one new eps neighbour; B = all old BORDER points (not core, label >= 0).
 *   stage 2: rows = T u B, columns = the old points; each unordered pair with an end in T u B once.
 * The core flags are the old ones OR the count rule; the count is complete for the new points, T and B, and an old point
 * outside them has gained nothing.  Components over the seeds and the kept core-core edges; clusters numbered by their smallest
 * core index in the original numbering; a non-core point with a core neighbour among the kept edges joins the lowest-numbered
 * of their clusters; every other point is -1.  Old core points and untouched old noise points are never rows.
 * n_new = 0: the model unchanged.  n_old = 0: the kind's full call.
 * Errors.  RTC_ERR_ARG: h_labels_old or h_core_old NULL with n_old > 0, h_labels NULL with n > 0, n >= 2^31 - 1, an old label
 * below -1, an old core point with label -1, an old cluster among 0 .. max label without a core point; otherwise those of
 * the kind's full call (MinHash eps < 0 or NaN RTC_ERR_ARG, eps >= 1 RTC_ERR_UNSUPPORTED; KSSD jaccard_min <= 1e-12, a size
 * bound past INT_MAX at width 4, a pair whose orientations disagree: RTC_ERR_UNSUPPORTED).  Both stages run in row chunks under
 * RTC_EDGE_BUDGET; RTC_ERR_NOMEM means what it says, there is no fallback.  Old labels that are well-formed but not the full
 * call's output give labels that mean nothing.  Synchronous. */
int rtc_dbscan_update(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                      uint32_t n_old, uint32_t n_new, const int32_t* h_labels_old, const uint8_t* h_core_old,
                      int is_minhash, uint32_t sketch_size, double eps, int min_pts, int kmer_size,
                      int32_t* h_labels, uint8_t* h_core, uint32_t* h_n_clusters, uint32_t* h_n_noise);
/* What the last rtc_dbscan_update call did: out[0] stage-1 rows, out[1] stage-2 rows (|T u B|), out[2] row chunks and out[3]
 * candidate edges of both stages together, out[4] pairs kept, out[5] promoted points, out[6] old clusters merged away (old
 * clusters minus the final clusters that hold an old core point), out[7] hook rounds, out[8] join ns, out[9] filter ns, out[10]
 * components and labels ns, out[11] whole call ns.  Twelve words: the two stages' rows each have their own. */
int rtc_dbscan_update_counters(const rtc_ctx* ctx, uint64_t out[12]);

/* ---- clust-leiden: similarity graph, Louvain and Leiden ---------------------------------------------- */
/* The graph of the reference's KssdLeidenCluster (src/leiden.cpp:168-293).  A pair u < v is an edge iff both sketches are
 * non-empty and share a hash, the size ratio passes -- !(2 min(|u|, |v|) < max(|u|, |v|)), which is the reference's
 * (double)small / large < 0.5 skip -- and dist < threshold strictly, dist = 1 - rtc_graph_weight(common, |u|, |v|, kmer_size):
 * calculate_mash_distance_fast (:109-121) with the host's libm.  The device forms no distance: the host finds J*, the least
 * double whose distance through that very function is below threshold, and the device tests (double)common / (double)union >= J*.
 * The rounding of 2j / (1 + j) can turn the order of doubles a few ulps apart, so J* is moved past every failing double within
 * 64 ulps above the bisection's flip: a pair the host function fails is never an edge, and the graph equals the host
 * function's pair by pair whenever no two pairs' quotients lie within 64 ulps of each other around J* -- guaranteed for
 * unions below 2^22 hashes (distinct quotients are then more than 256 ulps apart), not beyond.
 * knn_k > 0: every node u keeps only its knn_k best edges among v > u, the reference's asymmetric rule (:199-221).  The rank is
 * common / union compared exactly by 64-bit cross-multiplication, larger first, equal ratios to the lower v; the reference ranks
 * by the rounded distance and leaves equal distances in the order of its heap, so this is one of its possible outcomes.
 * knn_k = 0: no such filter (the command line cannot ask for that, as the reference's cannot).
 * h_edges[cap] receives the edges in (u, v) order, *h_n_edges their number.  More than cap: RTC_ERR_OVERFLOW with the needed
 * count in *h_n_edges.  threshold <= 0 or NaN: RTC_ERR_ARG.  A sketch of 2^31 hashes or more: RTC_ERR_UNSUPPORTED.
 * RTC_EDGE_BUDGET chunks the rows as in rtc_dbscan; a kept list that does not fit: RTC_ERR_NOMEM, no fallback.  Synchronous. */
typedef struct { uint32_t u, v, common, pad; } rtc_gedge; /* u < v; pad: 0 from rtc_graph_build, the truncated denom from rtc_graph_build_mash */
int rtc_graph_build(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                    double threshold, int kmer_size, uint32_t knn_k, rtc_gedge* h_edges, uint64_t cap, uint64_t* h_n_edges);
/* host only: 1 - calculate_mash_distance_fast(common, size_u, size_v, kmer_size) */
double rtc_graph_weight(uint32_t common, uint32_t size_u, uint32_t size_v, int kmer_size);
/* clust-leiden --minhash: the same graph over MinHash sketches -- as for rtc_dbscan_mash, ascending lists of distinct hashes of
 * at most sketch_size elements, shorter and empty ones allowed, width 4 or 8.  A pair u < v is an edge iff both lists are
 * non-empty, they share a hash and rtc_mash_distance(common, denom, sketch_size, kmer_size) < threshold strictly, (common, denom)
 * the union-truncated counts of rtc_pair_mash_dev.  There is no size-ratio rule: the reference's skip belongs to KSSD sketches,
 * whose sizes scale with the genome; MinHash::distance() has none and MinHashDBSCAN applies none.  A pair that shares a hash
 * only beyond the truncation has common 0, distance 1, and is never an edge.  The device forms no distance: the host builds
 * cmin[d], d = 0 .. min(sketch_size, 2 * the longest list) -- the least common whose distance through that very host function
 * is < threshold, d + 1 where none is (rtc_graph_mash_table; rtc_dbscan_mash_table's bisection with < for <=) -- and its suffix
 * minima for the prefilter on the pair phase's full-set common; the device tests common >= cmin[denom].
 * knn_k > 0: every node u keeps its knn_k best edges among v > u, ranked by common / denom compared exactly by 64-bit
 * cross-multiplication (both counts are <= sketch_size < 2^32), larger first, equal ratios to the lower v; knn_k = 0: no filter.
 * h_edges[cap] receives the edges in (u, v) order with pad = the truncated denom, *h_n_edges their number.  More than cap:
 * RTC_ERR_OVERFLOW with the needed count in *h_n_edges.  0 < threshold <= 1: threshold <= 0 or NaN returns RTC_ERR_ARG,
 * threshold > 1 RTC_ERR_UNSUPPORTED (pairs without a shared hash have distance 1 and no candidate list holds them);
 * sketch_size == 0 or kmer_size < 1: RTC_ERR_ARG.  RTC_EDGE_BUDGET chunks the rows, RTC_ERR_NOMEM without fallback, as
 * rtc_graph_build.  RTC_DBSCAN_MASH_SERIAL=1 and RTC_DBSCAN_MASH_NOPREFILTER=1 as for rtc_dbscan_mash; results are identical
 * either way.  Synchronous. */
int rtc_graph_build_mash(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                         uint32_t sketch_size, double threshold, int kmer_size, uint32_t knn_k, rtc_gedge* h_edges, uint64_t cap,
                         uint64_t* h_n_edges);
/* host only: 1 - rtc_mash_distance(common, denom, sketch_size, kmer_size), the weight of a rtc_graph_build_mash edge (> 0) */
double rtc_graph_weight_mash(uint32_t common, uint32_t denom, uint32_t sketch_size, int kmer_size);
/* host only, no context: rtc_graph_build_mash's table for one threshold in (0, 1], out[d] for d = 0 .. sketch_size */
int rtc_graph_mash_table(uint32_t sketch_size, int kmer_size, double threshold, uint32_t* out);
/* The last rtc_graph_build or rtc_graph_build_mash: out[0] row chunks, out[1] candidates (pairs sharing a hash), out[2] pairs
 * passing the edge rule, out[3] edges after the k-NN filter, out[4] nodes the filter cut, out[5] pair ns, out[6] filter (MinHash:
 * prefilter and merge) ns, out[7] select and sort ns, out[8] candidates merged past the prefilter (MinHash; 0 after
 * rtc_graph_build), out[9] whole call ns. */
int rtc_graph_counters(const rtc_ctx* ctx, uint64_t out[10]);

/* Deterministic Louvain in exact integers.  The reference calls igraph_community_multilevel, which visits the nodes in a
 * shuffled order and is no reproducible target: this is the definition (tests/reflouvain.py restates it).
 *   - Input: n vertices, m records (u, v, q), q >= 1 the weight in units of 2^-20 -- callers form q = max(1, llround(weight *
 *     2^20)).  Duplicate (u, v) are summed; u == v adds 2q to the self entry; the adjacency is symmetric.  k_x is x's row sum,
 *     the self entry included; M2 is the sum of all k_x.  g = llround(resolution * 65536); resolution <= 0, NaN or g >= 2^32:
 *     RTC_ERR_ARG.  u or v >= n, or q = 0: RTC_ERR_ARG.  M2 >= 2^46: RTC_ERR_UNSUPPORTED (the scores fit 128 signed bits below).
 *   - A level starts from singletons, community x = {x}, tot_c = the sum of k over c's members.  Round r = 0, 1, ...: every
 *     vertex decides from the state at the start of the round.  For x in community c and a community d, e_d is the weight from
 *     x to the members of d other than x, and S(d) = e_d M2 65536 - g k_x (tot_d - [d == c] k_x).  Among the communities d != c
 *     that hold a neighbour of x, with d < c on even rounds and d > c on odd ones, and S(d) > S(c) strictly, x moves to the one
 *     with the largest S, equal scores to the smallest d; if there is none it stays.  All moves are applied together and tot is
 *     rebuilt from the memberships.  The level ends after two rounds in a row without a move, or after 64 rounds.
 *   - If the level moved nothing, the algorithm stops.  Otherwise the communities are numbered by their smallest member and
 *     become the vertices of the next level; the weight between two communities is summed, the weight inside one (every entry,
 *     both directions and the self entries) becomes its self entry.  At most 32 levels.
 *   - h_labels[n]: the final community of every vertex, communities numbered by their smallest original vertex;
 *     *h_n_clusters their number; *h_modularity (may be NULL) the sum over c of (in_c M2 65536 - g tot_c^2) divided by
 *     (M2^2 65536) on the host, for information.  m == 0: every vertex is its own cluster (:286-293).
 * Every sum is an integer (64-bit integer atomics: order-independent), every score a 128-bit signed integer, so the result does
 * not depend on the scheduling or on which kernel path a row takes.  Synchronous. */
typedef struct { uint32_t u, v, q; } rtc_wedge;
int rtc_louvain(rtc_ctx* ctx, uint32_t n, const rtc_wedge* h_edges, uint64_t m, double resolution, int32_t* h_labels,
                uint32_t* h_n_clusters, double* h_modularity);
/* The last rtc_louvain: out[0] levels, out[1] rounds (all levels), out[2] moves (all levels), out[3] vertices and out[4]
 * adjacency entries of the last level, out[5] rows the long paths took (workgroup and global table, all rounds), out[6] move ns,
 * out[7] aggregate ns, out[8] rows the global-table path took, out[9] whole call ns. */
int rtc_louvain_counters(const rtc_ctx* ctx, uint64_t out[10]);

/* Deterministic Leiden in exact integers: clust-leiden --leiden.  The reference calls igraph_community_leiden (src/leiden.cpp:
 * 337-383) without node weights -- the CPM objective with node weight 1 -- with beta 0.01 and 100 iterations.  igraph visits the
 * nodes in a random order and draws the refinement's merges at random (with probability ~ exp(gain / beta)); this definition
 * visits all vertices at once and takes the best merge, so it is no port of igraph's and igraph is no reproducible target:
 * this is the definition (tests/refleiden.py restates it).
 *   - Input, k_x, M2, g and the refusals are rtc_louvain's.  objective: RTC_LEIDEN_CPM, as the reference calls igraph, or
 *     RTC_LEIDEN_MODULARITY; anything else RTC_ERR_ARG.
 *   - The score.  Vertex x has node weight nu_x; N_d is the sum of nu over community d; e_d the weight from x to the members of
 *     d other than x.  For x in community c,  S(d) = e_d A - g B nu_x (N_d - [d == c] nu_x)  in 128-bit signed integers, with
 *         CPM:         nu of an input vertex 1,   A = 65536,      B = 2^20
 *         modularity:  nu of an input vertex k_x, A = M2 65536,   B = 1     (rtc_louvain's score)
 *     and nu summed when vertices are merged into one.
 *   - An iteration runs levels 0, 1, ... (at most 32).  The vertices of a level enter with a coarse community each, named by
 *     its smallest member at that level: at level 0 singletons in the first iteration, the previous iteration's result after.
 *     (a) Move phase: rtc_louvain's rounds with the score above, from the partition given instead of from singletons.  Every
 *         vertex decides from the state at the start of the round; candidates are the communities d != c that hold a
 *         neighbour, d < c on even rounds and d > c on odd ones, with S(d) > S(c) strictly; the largest S wins, equal scores
 *         go to the smallest d; all moves are applied together and N is rebuilt.  Two idle rounds in a row or 64 rounds end it.
 *         A vertex never moves to an empty community.  C(x) below is the coarse community it leaves x in.
 *     (b) Refinement.  Every vertex starts alone in the refined community R(x) = x.  With in_x the weight from x to C(x) minus
 *         itself, x is eligible iff in_x A >= g B nu_x (N_C - nu_x), tested once.  A refined community r inside C is an
 *         eligible target iff E_r A >= g B N_r (N_C - N_r), E_r the weight between r and C minus r, rebuilt every round.  In
 *         round r = 0, 1, ... every eligible vertex x that is still the only member of R(x) proposes: its candidates are the
 *         eligible targets d != R(x) that hold a neighbour y of x with C(y) = C(x), d < R(x) on even rounds and d > R(x) on
 *         odd ones, with S(d) >= 0 (a lone vertex stays at score 0; >= is igraph's rule here); it proposes the one with the
 *         largest S, equal scores to the smallest d.  A proposal is accepted iff no member of its target proposes in that
 *         round, so a community either gives up its vertex or receives vertices; accepted moves are applied together.  A
 *         refined community that has members holds the vertex it is named after, and only that vertex can propose for it.  The
 *         proposal with the smallest target (even rounds; the largest on odd ones) is always accepted, so a round with a
 *         proposal makes progress.  Every merge joins a vertex to a community that stays, over a positive edge, inside one
 *         coarse community: refined communities are connected by construction.  Two rounds in a row without an accepted
 *         proposal, or 64 rounds, end it.
 *     (c) If the refinement merged nothing, or this was the 32nd level, the iteration ends and its result is the coarse
 *         partition of (a) at the input's vertices.  Otherwise the refined communities, numbered by their smallest member,
 *         are the next level's vertices: nu and the adjacency summed as rtc_louvain aggregates (the weight inside one becomes
 *         its self entry), the coarse community of a new vertex that of its members.
 *   - Iterations repeat from the input's graph, each from the result before, until one returns the labels it was given or 100
 *     have run (:379); they are deterministic, so stopping at the first unchanged one equals running them all.
 *   - h_labels, *h_n_clusters: as rtc_louvain's.  *h_quality (may be NULL), on the host from the labels, for information:
 *     CPM the sum over c of (in_c 65536 - g 2^20 size_c^2) divided by (M2 65536), modularity rtc_louvain's.  m == 0: every
 *     vertex is its own cluster.
 *   - Under CPM every weight of at most one unit (q <= 2^20) gives e_d 65536 <= g 2^20 nu_x N_d at resolution >= 1: nothing
 *     moves and every vertex is its own cluster.
 * As for rtc_louvain, the result depends neither on the scheduling nor on the kernel path of a row.  Synchronous. */
#define RTC_LEIDEN_CPM 0
#define RTC_LEIDEN_MODULARITY 1
int rtc_leiden(rtc_ctx* ctx, uint32_t n, const rtc_wedge* h_edges, uint64_t m, double resolution, int objective, int32_t* h_labels,
               uint32_t* h_n_clusters, double* h_quality);
/* The last rtc_leiden: out[0] iterations, out[1] levels (all iterations), out[2] move rounds, out[3] moves, out[4] refinement
 * rounds, out[5] merges accepted, out[6] proposals rejected, out[7] move ns, out[8] refinement ns, out[9] whole call ns. */
int rtc_leiden_counters(const rtc_ctx* ctx, uint64_t out[10]);

/* Markov clustering (MCL, van Dongen's flow simulation) in exact integers: clust-leiden --mcl.  MCL is usually run in floating
 * point; this is a definition in fixed point, so that the result depends neither on the scheduling nor on the kernel path of a
 * column (tests/refmcl.py restates it).  ONE = 2^30.  h = inflation_x2 is twice the inflation, 3 <= h <= 16 (1.5, 2, 2.5 .. 8);
 * S = select, 1 <= S <= 4096; T = max_iter.  Every quantity is an unsigned 64-bit integer, / is floor division, and no step forms
 * a floating-point value.
 *   - Input: n vertices, m records (u, v, q) as rtc_louvain takes them.  Duplicates of an unordered pair are summed, records
 *     with u == v are ignored, A is the symmetric adjacency.  u or v >= n, or q == 0: RTC_ERR_ARG.  A summed entry >= 2^32:
 *     RTC_ERR_UNSUPPORTED.  h or S out of range: RTC_ERR_ARG.
 *   - select(column): of the column's entries (i, x) the S largest stay, in the order x descending, then i ascending (all, if
 *     there are no more than S).  With X the sum of the x that stay, each becomes p = x ONE / X; entries with p == 0 drop out.
 *     The keys (x, i) are distinct, so the selection is unique.
 *   - Start: column j is A's column j and the loop (j, L), L the largest entry of A's column j, or 1 if it is empty;
 *     M[j] = select(column j).
 *   - One iteration, for every column j:
 *       1. Expand: s_i = the sum over the k of column j of M[i,k] M[k,j] (at most 2^60; one integer sum, so order-free);
 *          e_i = s_i >> 30; rows with e_i == 0 drop out.
 *       2. Rescale: with E the largest e_i of the column, e'_i = e_i ONE / E -- the largest becomes ONE exactly, so inflation
 *          never empties a column.
 *       3. Inflate: y = e'; then h / 2 - 1 times y = (y e') >> 30; if h is odd once more y = (y isqrt(e' << 30)) >> 30, isqrt the
 *          floor of the exact square root.  Rows with y == 0 drop out.
 *       4. N[j] = select({(i, y_i)}).
 *   - Stop after the first iteration with N == M, columns compared as sets of (row, value): that iteration counts and
 *     *h_converged = 1.  Otherwise after T iterations, *h_converged = 0.  T == 0 returns the start matrix.
 *   - Clusters, on the host from the final matrix: a is an attractor iff M[a,a] > 0.  Every attractor is united with every
 *     attractor among the rows of its column.  Every other vertex j is united with one row of its column: the attractor row
 *     with the largest p, the lowest i among equals; if its column holds no attractor -- possible only without convergence --
 *     that row among all its rows.  h_labels[x] is the smallest member of x's cluster, so the clusters come in the order in
 *     which rtc_louvain numbers its communities; *h_n_clusters their number.  No record (or only u == v): every vertex is its own
 *     cluster, after one iteration.
 *   - h_matrix (may be NULL): the final matrix in (col, row) order, *h_nnz its entries; cap < *h_nnz: RTC_ERR_OVERFLOW with the
 *     count in *h_nnz (labels, iterations and converged are set).  h_iterations, h_converged, h_nnz may be NULL without h_matrix.
 * The device holds two matrices of n columns of min(S, n) slots, 16 n min(S, n) bytes, and the long path's tables; if they do
 * not fit the free memory: RTC_ERR_NOMEM with the bytes in the message, no fallback.  A column takes one of three kernel paths
 * by its work W, the number of products its expansion gathers (rabbittclust_amd/csrc/rtc_mcl.h: W <= 256 one wave, W <= 3072 a
 * 256-lane workgroup, both with the table in LDS; beyond, a table in global memory).  RTC_MCL_GLOBAL=1 sends every column
 * through the last; results are identical.  Synchronous. */
typedef struct { uint32_t col, row, value, pad; } rtc_mcl_entry;
int rtc_mcl(rtc_ctx* ctx, uint32_t n, const rtc_wedge* h_edges, uint64_t m, int inflation_x2, uint32_t select, uint32_t max_iter,
            int32_t* h_labels, uint32_t* h_n_clusters, uint32_t* h_iterations, int* h_converged, rtc_mcl_entry* h_matrix, uint64_t cap,
            uint64_t* h_nnz);
/* The last rtc_mcl: out[0] iterations, out[1] converged, out[2] entries of the final matrix, out[3] attractors, out[4] / out[5] /
 * out[6] columns x iterations on the wave / workgroup / long path, out[7] columns where select cut something (the start and all
 * iterations), out[8] ns between the first and the last column launch of the iterations (device clock), out[9] whole call ns. */
int rtc_mcl_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* the column paths of the last rtc_mcl: bit 0 one wave, bit 1 a 256-lane workgroup, bit 2 the table in global memory */
int rtc_mcl_last_path(const rtc_ctx* ctx);

/* Shared-nearest-neighbour (SNN) edge weights: clust-leiden --snn.  The weight of an edge becomes the Jaccard index of its two
 * ends' neighbourhoods (Jarvis-Patrick; the usual preparation of a k-NN graph for Louvain and Leiden).  The quantity is an integer
 * count per edge, so the result depends neither on the scheduling nor on the kernel path (tests/refsnn.py restates it).
 *   - Input: n vertices and m records (u, v, q) in any order; q is not read.  G is the simple undirected graph of the records:
 *     (u, v) and (v, u) are the same edge, equal edges collapse to one, a record with u == v is in no neighbourhood.  N(x) is the
 *     set of neighbours of x in G, deg x = |N(x)|.
 *   - For a record with u != v: shared = |N(u) & N(v)|, the triangles through the edge; deg_u, deg_v the two degrees; flags 0.
 *     With the closed neighbourhoods N[x] = N(x) + {x} the weight is
 *         w = |N[u] & N[v]| / |N[u] | N[v]| = (shared + 2) / (deg_u + deg_v - shared),
 *     so 0 < w <= 1 and the denominator is never below 2: an isolated edge and every edge of a clique weigh 1, an edge of a star
 *     with L leaves 2 / (L + 1), the bridge between two K40 2 / 80.  The device returns the integers; rtc_snn_weight forms the one
 *     double division on the host.
 *   - A record with u == v: shared 0, deg_u = deg_v = the degree of u in G, flags bit 0 set.
 *   - h_out[m], record for record.  u or v >= n, h_edges or h_out NULL with m > 0, n >= 2^31 - 1: RTC_ERR_ARG.  m == 0 or n == 0:
 *     RTC_OK, nothing is written.
 * The device holds the records, two buffers of 2m 64-bit keys, the rows and the result, about 76 m + 8 n bytes and the sort's
 * scratch; if they do not fit the free memory: RTC_ERR_NOMEM with the bytes in the message, no fallback.  A record is counted by
 * the end with the longer row (the lower index on equal lengths), on one of three kernel paths by that row's length
 * (rabbittclust_amd/csrc/rtc_snn.h: at most 768 entries one wave, at most 8192 a 256-lane workgroup, both with the row in LDS;
 * beyond, the row where it lies in global memory).  RTC_SNN_GLOBAL=1 sends every record through the last; counts are identical.
 * Synchronous. */
typedef struct { uint32_t shared, deg_u, deg_v, flags; } rtc_snn;   /* flags bit 0: u == v (shared = 0, the degrees still those of G) */
int rtc_graph_snn(rtc_ctx* ctx, uint32_t n, const rtc_wedge* h_edges, uint64_t m, rtc_snn* h_out);
/* host only: (double)(shared + 2) / (double)(deg_u + deg_v - shared) */
double rtc_snn_weight(uint32_t shared, uint32_t deg_u, uint32_t deg_v);
/* The last rtc_graph_snn: out[0] records, out[1] distinct edges of G, out[2] triangles of G (the sum of shared over distinct
 * edges, divided by 3), out[3] probes (elements of the shorter rows that were looked up), out[4] / out[5] / out[6] records counted
 * on the wave / workgroup / global path, out[7] adjacency ns (upload, sort, unique, rows), out[8] counting ns (owners, their sort
 * and the three launches), out[9] whole call ns (host clock, each ending in a synchronise). */
int rtc_graph_snn_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* the paths of the last rtc_graph_snn: bit 0 one wave, bit 1 a 256-lane workgroup, bit 2 the row in global memory */
int rtc_graph_snn_last_path(const rtc_ctx* ctx);

/* ---- clust-leiden --db --assign: new genomes placed into the communities of a finished run ------------------- */
/* The move phase's choice for a vertex that was not there.  The reference has nothing of the kind: this is the definition
 * (tests/refleiden_assign.py restates it).
 * A model is the result of one clust-leiden run over n_db KSSD sketches: the labels L[p], numbered as the run numbered its
 * clusters; the graph parameters threshold, kmer_size, knn_k; the objective (CPM or modularity; rtc_louvain is modularity);
 * g = llround(resolution 65536); the quantisation the run used -- under CPM the scale flag with lo and range of the host's
 * leiden_quantise, under modularity none; under CPM the community sizes N_d; under modularity tot_d, the sum over d's members
 * of the row sums k_p of the very records the run gave rtc_louvain or rtc_leiden (k_x as defined at rtc_louvain), and
 * M2 = the sum of all tot_d.
 * For a query x, a sketch that is not in the model:
 *   - C(x): the model genomes p that share a hash with x and pass rtc_graph_build's edge rule -- both sketches non-empty,
 *     !(2 min < max) on the sizes, (double)common / (double)union >= J* with rtc_graph_build's J* for (threshold, kmer_size) --
 *     on the count the pair phase reports, as rtc_graph_build sees it.
 *   - E(x): the knn_k best of C(x).  The rank is common / union, larger first, compared exactly by 64-bit cross-multiplication,
 *     equal ratios to the lower p; knn_k = 0 keeps all of C(x).  The build's "higher-numbered neighbours only" rule has no
 *     meaning for a vertex outside the numbering: a query ranks against all model genomes.
 *   - q(x, p): the weight rtc_graph_weight(common, |x|, |p|, kmer_size), formed on the host, quantised exactly as the model's
 *     run quantised its own.  Modularity: max(1, llround(w 2^20)).  CPM: w' = scale ? (w - lo) / range : w, q = llround(w' 2^20)
 *     capped at 0xffffffff; a record with q < 1 is dropped (w' may lie outside [0, 1] for a query; the same lines apply).
 *   - k_x = the sum of q over the kept records, e_d = the sum over those with L[p] = d.
 *   - The score, in 128-bit signed integers: the move phase's for x alone in a community of its own, S(own) = 0, in the model's
 *     graph with x and its edges added.
 *         CPM:         S(d) = e_d 65536 - g 2^20 N_d
 *         modularity:  S(d) = e_d (M2 + 2 k_x) 65536 - g k_x (tot_d + e_d);    M2 + 2 k_x >= 2^46: RTC_ERR_UNSUPPORTED
 *   - label: the d with e_d > 0 and the largest S(d) > 0 strictly, equal scores to the smallest d; -1 if there is none (the
 *     command line prints "novel").  runner_up: the next community in that order among those with S > 0, or -1.
 *   - Queries never see each other, and the model is not changed.  Under CPM with resolution >= 1 and weights of at most one
 *     unit no score is positive and every query is novel, as every vertex of the build is its own cluster there.
 * The two calls mirror the build: rtc_graph_build, the host's weights, rtc_louvain.  The device forms no distance.
 *
 * rtc_graph_query: E(x) for every query.  The rows [0, n_db) are the model, the rows [n_db, n_db + n_queries) the queries, the
 * layout of rtc_rep_topk.  h_edges[cap] receives the records in (q, p) order, *h_n_edges their number; more than cap:
 * RTC_ERR_OVERFLOW with the needed count in *h_n_edges (h_near is complete then).  h_near[q]: nearest, common, denom -- over ALL
 * candidates (model genomes sharing a hash with q, passing or not) the one with the largest common / (|x| + |p| - common),
 * compared exactly, equal keys to the lower p; UINT32_MAX and zeros when q shares no hash -- and n_candidates, n_passing = |C(x)|,
 * n_kept = |E(x)|.  query_chunk: queries per join (0: all); a chunk whose candidates exceed RTC_EDGE_BUDGET or whose join scratch
 * does not fit is halved, RTC_ERR_NOMEM past one query; no fallback.  Argument errors are rtc_graph_build's (threshold <= 0 or
 * NaN, kmer_size < 1, n_db + n_queries >= 2^31 - 1, no room: RTC_ERR_ARG; a sketch of 2^31 hashes: RTC_ERR_UNSUPPORTED), and
 * h_near NULL with n_queries > 0 is RTC_ERR_ARG.  Synchronous. */
typedef struct { uint32_t q, p, common, pad; } rtc_qedge; /* q: query index, p: model genome */
typedef struct { uint32_t nearest, common, denom, n_candidates, n_passing, n_kept; } rtc_graph_near;
int rtc_graph_query(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n_db,
                    uint32_t n_queries, double threshold, int kmer_size, uint32_t knn_k, uint32_t query_chunk, rtc_qedge* h_edges,
                    uint64_t cap, uint64_t* h_n_edges, rtc_graph_near* h_near);
/* The last rtc_graph_query: out[0] query chunks, out[1] candidates, out[2] passing the edge rule, out[3] kept, out[4] queries the
 * k-NN rule cut, out[5] queries without a candidate, out[6] join ns, out[7] filter and bucketing ns, out[8] select and sort ns,
 * out[9] whole call ns. */
int rtc_graph_query_counters(const rtc_ctx* ctx, uint64_t out[10]);

/* rtc_leiden_place: label and runner-up of every query from its quantised records (u: query index, v: model genome, q), in any
 * order; duplicate (u, v) are summed.  h_labels[n_db] in [0, n_clusters); h_tot[n_clusters] the model's tot_d under modularity,
 * NULL under CPM (the sizes N_d are counted from the labels); m2 the model's M2 (unused under CPM).  h_out[q]: label, runner_up,
 * n_edges (distinct model genomes among the records), n_comms (communities they touch), k_x, e_label, e_runner (0 where there
 * is none).  A query without a record is novel with zeros.
 * Errors: u >= n_queries, v >= n_db, q = 0, a label outside [0, n_clusters), an objective that is neither RTC_LEIDEN_CPM nor
 * RTC_LEIDEN_MODULARITY, h_tot NULL under modularity: RTC_ERR_ARG; resolution as rtc_louvain refuses it; M2 + 2 k_x >= 2^46 for
 * some query under modularity: RTC_ERR_UNSUPPORTED.  Everything is an integer, so the result depends neither on the order of
 * the records nor on the kernel path of a row.  Synchronous. */
typedef struct { int32_t label, runner_up; uint32_t n_edges, n_comms; uint64_t k_x, e_label, e_runner; } rtc_leiden_placement;
int rtc_leiden_place(rtc_ctx* ctx, uint32_t n_db, const int32_t* h_labels, uint32_t n_clusters, const uint64_t* h_tot, uint64_t m2,
                     double resolution, int objective, uint32_t n_queries, const rtc_wedge* h_edges, uint64_t m,
                     rtc_leiden_placement* h_out);
/* The last rtc_leiden_place: out[0] records, out[1] distinct (u, v), out[2] queries with a record, out[3] placed, out[4] novel,
 * out[5] rows of the wave path, out[6] of the workgroup path, out[7] of the global-table path, out[8] sort and kernel ns,
 * out[9] whole call ns. */
int rtc_leiden_place_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* The row paths of the last rtc_leiden_place: bit 0 one wave with the table in LDS (rows of up to 128 entries), bit 1 a 256-lane
 * workgroup (up to 2 048), bit 2 the table in global memory (longer rows). */
int rtc_leiden_place_last_path(const rtc_ctx* ctx);

/* ---- clust-mst --linkage complete: complete linkage inside the single-linkage clusters ------------------------- */
/* clust-mst is single linkage: a chain of close pairs ends in one cluster whose far ends may be far apart.  Complete linkage inside
 * each of its clusters gives a diameter instead: every two members of a result cluster are within the threshold.  The Mash
 * distance is monotone in the Jaccard quotient and complete linkage takes only minima and maxima, so the device works on exact
 * rationals and forms no distance; this is the definition (tests/reflinkage.py restates it).
 *
 * Key of a pair.  kappa(u, v) = common / denom, common as rtc_pair_common_dev reports it, denom = |u| + |v| - common: the
 *     set-Jaccard of the index path.  A record is rtc_lkey {common, denom}.  Keys are compared exactly, common_x denom_y against
 *     common_y denom_x in 64 bits; denom == 0 (two empty sketches) counts as kappa = 0.
 * Agglomeration of one set of m points, given its symmetric m x m key matrix (the diagonal is ignored).  Every point starts as a
 *     cluster named by its index.  K(X, Y) is the minimum key over the pairs between X and Y in the order kappa ascending, then
 *     denom ascending (the reported counts are unique).  Each step takes the active pair (a, b), a < b, with the largest
 *     kappa(K(a, b)), ties to the smallest a, then the smallest b.  If that kappa is 0 or below the stop bound kmin_num / kmin_den
 *     (cross-multiplied; 0 / 1: no bound) the agglomeration ends.  Otherwise the step emits rtc_lmerge {a, b, common, denom,
 *     size}, size the member count of the new cluster; K(a, c) = min(K(a, c), K(b, c)) for every other active c, b is retired
 *     and the cluster keeps the name a.  At most m - 1 merges, in step order.
 * The cut is the host's: rtc_linkage_distance gives a merge the distance of its key through the function that weighs the MST's
 *     edges (same expression order), and a component's merges apply in order up to, not including, the first whose distance is
 *     > threshold.  Minimum keys never grow from step to step, so the cut is where a bound at or below the true one stops.
 *
 * Two kernel paths, each a component's whole dendrogram in one launch: m <= 64 one wave with the matrix in LDS, m > 64 one
 * 256-lane workgroup with the matrix in global memory.  Nothing is summed: the merge list depends on neither. */
typedef struct { uint32_t common, denom; } rtc_lkey;
typedef struct { uint32_t a, b, common, denom, size; } rtc_lmerge;
/* One matrix that is already on the device: d_key[i * ld + j], 8-byte aligned, ld >= m; it is read and overwritten.
 * h_merges[m - 1], *h_n_merges their number.  kmin_den == 0, ld < m, m >= 2^31 - 1, NULLs: RTC_ERR_ARG.  Synchronous. */
int rtc_linkage_dev(rtc_ctx* ctx, uint32_t m, rtc_lkey* d_key, uint64_t ld, uint32_t kmin_num, uint32_t kmin_den,
                    rtc_lmerge* h_merges, uint32_t* h_n_merges);
/* Every component of a labelling of n sketches.  h_comp[g] is the component of genome g, any labelling; components are numbered
 * in order of their smallest member and their members taken in ascending genome order.  The key blocks of the components are
 * filled from rtc_pair_common_dev over row bands and agglomerated in batches under a byte budget (RTC_LINKAGE_BYTES, default half
 * the free HBM).  h_merges[cap]: the merges of component 0, then 1, ..., a and b as genome indices; *h_n_merges their number;
 * h_first[c] is where component c's merges start, h_first[n_comp] == *h_n_merges -- room for n_comp + 1 entries, n + 1 always
 * suffices.  Components of one member cost nothing.
 * A component whose 8 m^2 bytes and one band exceed the budget: RTC_ERR_NOMEM, the message naming m and the bytes; no fallback.
 * More merges than cap: RTC_ERR_OVERFLOW with the needed count in *h_n_merges (h_first is complete then).  width not 4 or 8,
 * NULLs, n >= 2^31 - 1, kmin_den == 0: RTC_ERR_ARG.  Synchronous. */
int rtc_linkage_complete(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                         const uint32_t* h_comp, uint32_t kmin_num, uint32_t kmin_den, rtc_lmerge* h_merges, uint64_t cap,
                         uint64_t* h_n_merges, uint64_t* h_first);
/* The last rtc_linkage_complete (or rtc_linkage_dev): out[0] components agglomerated (m >= 2), out[1] wave-path components,
 * out[2] workgroup-path components, out[3] merges, out[4] row rescans (rows whose best was looked for again after a merge),
 * out[5] batches, out[6] fill ns, out[7] agglomeration ns, out[8] largest m, out[9] whole call ns. */
int rtc_linkage_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* The distance of a key: 1 for kappa = 0, 0 for kappa = 1, otherwise -ln(2j / (1 + j)) / kmer_size, j = common / denom in double,
 * with the host's libm; denom up to 2^31 - 1, the range of the MST's own weights.  Host only. */
double rtc_linkage_distance(uint32_t common, uint32_t denom, int kmer_size);

/* ---- clust-mst --nj-tree / --nj-all: neighbour-joining trees ------------------------------------------------------ */
/* Neighbour joining (Saitou-Nei, with Studier-Keppler's Q) of one set of m points over a symmetric m x m matrix D of finite
 * doubles; the diagonal is ignored.  This is the definition (tests/refnj.py restates it).  Every operation is one IEEE-754 double
 * operation in the order written: no contraction into FMA, no reassociation.
 *
 * Start.  Every point is an active node named by its index, r = m.  R[i] is the sum of D[i][j] over j != i in ascending j, added
 *     one after the other starting from 0.0 -- the only ordered sum, and it happens once.
 * While r > 3.  Q(i, j) = ((double)(r - 2) * D[i][j] - R[i]) - R[j] for active i < j; the pair with the least Q is joined, equal
 *     Q going to the smallest i, then the smallest j (comparisons of doubles are exact, so the choice does not depend on how the
 *     search is split).  dij = D[i][j], delta = (R[i] - R[j]) / (double)(2 (r - 2)), len_i = 0.5 * dij + delta,
 *     len_j = dij - len_i.  For every other active k: duk = 0.5 * ((D[i][k] + D[j][k]) - dij),
 *     R[k] = ((R[k] - D[i][k]) - D[j][k]) + duk, D[i][k] = D[k][i] = duk.  Then R[i] = 0.5 * ((R[i] + R[j]) - (double)r * dij)
 *     with the r from before the join, j is retired, the new node keeps the name i and r drops by one.  The step emits
 *     rtc_njoin {a = i, b = j, c = UINT32_MAX, len_a = len_i, len_b = len_j, len_c = 0}.
 * At r == 3, active i < j < k: one record {i, j, k, 0.5 * ((D[i][j] + D[i][k]) - D[j][k]), 0.5 * ((D[i][j] + D[j][k]) - D[i][k]),
 *     0.5 * ((D[i][k] + D[j][k]) - D[i][j])}.
 * m >= 3 gives m - 2 records, m == 2 the one record {0, 1, UINT32_MAX, 0.5 * d, d - 0.5 * d, 0}, m <= 1 none.  Branch lengths
 *     are not clamped: negative ones come out as they are.  Non-finite input is undefined.
 *
 * Three kernel paths, chosen per component: m <= 64 one wave with D and R in LDS; larger ones a 256-lane workgroup with D in
 * global memory, the whole tree in one launch; from RTC_NJ_GRID_MIN points on (default 256; set, it holds down to 4) the whole
 * device, two launches a join, all of them enqueued without a read-back.  The records are the same on every path.  A grid-path
 * scan launch has one workgroup per four rows of the active list, at most RTC_NJ_SCAN_BLOCKS of them (1 .. 1024, default and
 * ceiling 1024); past that a workgroup takes further rows.  The switch is for tests: it brings that at any m. */
typedef struct { uint32_t a, b, c, pad; double len_a, len_b, len_c; } rtc_njoin;
/* One matrix that is already on the device: d_dist[i * ld + j], ld >= m; it is read and overwritten.  h_joins: room for
 * max(m - 2, 1) records, *h_n_joins their number.  ld < m, m >= 2^31 - 1, NULLs: RTC_ERR_ARG.  Synchronous. */
int rtc_nj_dev(rtc_ctx* ctx, uint32_t m, double* d_dist, uint64_t ld, rtc_njoin* h_joins, uint32_t* h_n_joins);
/* One tree per component of a labelling of n sketches: component numbering, member order, h_first and RTC_ERR_OVERFLOW as
 * rtc_linkage_complete has them; a component of m >= 3 has m - 2 records, one of two has one, a, b and c are genome indices.  The
 * key blocks are rtc_linkage_complete's; each batch is copied to the host, every entry becomes
 * rtc_linkage_distance(common, denom, kmer_size) -- 1 for common == 0 or denom == 0 -- with the host's libm on the context's host
 * threads (rtc_ctx_set_host_threads), the doubles go back into the same 8-byte cells and the device joins.  The byte budget of a
 * batch is RTC_NJ_BYTES (default half the free HBM); a component whose 8 m^2 bytes and one band exceed it: RTC_ERR_NOMEM, the
 * message naming m and the bytes; no fallback.  Argument errors as rtc_linkage_complete; kmer_size < 1: RTC_ERR_ARG. */
int rtc_nj_clusters(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                    const uint32_t* h_comp, int kmer_size, rtc_njoin* h_joins, uint64_t cap, uint64_t* h_n_joins, uint64_t* h_first);
/* The last rtc_nj_clusters (or rtc_nj_dev): out[0] components joined (m >= 2), out[1] on the wave path, out[2] on the workgroup
 * path, out[3] on the grid path, out[4] records, out[5] batches, out[6] fill ns, out[7] host distance ns (copies included),
 * out[8] joining ns, out[9] whole call ns. */
int rtc_nj_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* The paths of the last call: bit 0 the wave path, bit 1 the workgroup path, bit 2 the grid path. */
int rtc_nj_last_path(const rtc_ctx* ctx);
/* RTC_NJ_SCAN_BLOCKS as this context holds it: the most workgroups of a grid-path scan launch, 1 .. 1024 (unset: 1024). */
int rtc_nj_scan_blocks(const rtc_ctx* ctx);

/* ---- clust-mst --nj-support: jackknife support values for the neighbour-joining trees --------------------------------- */
/* How many of B delete-half jackknife replicates over the sketch hashes hold each inner branch of rtc_nj_clusters' trees.  This
 * is the definition (tests/refnjsupport.py restates it); everything is integer but the neighbour joining itself, which is
 * rtc_nj_dev's definition unchanged.
 *   Mask.  mix(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *     mix = z ^ (z >> 31), all modulo 2^64.  word(h, seed, w) = mix(h ^ mix(seed + w)), h the hash, zero-extended at width 4.
 *     Replicate r in [0, B) keeps hash h iff bit r % 64 of word(h, seed, r / 64) is set: the same hash is kept or dropped in every
 *     genome.  B lies in 1 .. 256 (a cap, not a measurement).
 *   Keys.  size_r(a) = |{h in a : kept in r}|, common_r(a, b) = |{h in a and b : kept in r}| over the full sorted lists (the sets
 *     rtc_pair_common_dev counts), denom_r = size_r(a) + size_r(b) - common_r, and
 *     D_r[a][b] = rtc_linkage_distance(common_r, denom_r, kmer_size), 1 for common_r == 0 or denom_r == 0.
 *   Trees.  rtc_nj_dev's definition on D_r, over the same components and the same member order as the main tree.
 *   Splits.  In a tree of m >= 4 members every record with c == UINT32_MAX names a node; S is the set of leaves below it (the
 *     leaves of the nodes it joined, and of theirs).  Its split is {S, complement}, compared as the side that does not hold the
 *     component's smallest member.  These are the m - 3 inner branches; the closing record and trees of m <= 3 have none.
 *   Support.  support(record) = |{r : the record's split is a split of replicate r's tree}|, splits compared exactly.
 * The counts depend on neither the path of the joining, nor on how the replicates are grouped under the byte budget, nor on
 * RTC_PAIR_FORCE_MERGE.
 *
 * h_joins, h_n_joins, h_first and the errors are rtc_nj_clusters' for the same arguments; h_support[cap] gets one count per
 * record, 0 for the records that name no split.  The main blocks are filled as rtc_nj_clusters fills them, but a batch leaves
 * room for one more copy of its blocks; the replicates are then taken in groups of as many as RTC_NJ_BYTES leaves room for beside
 * the main blocks (whole words of 64 where that is more than 64).  A counting kernel walks every pair of a component once per
 * word -- one wave, one replicate per lane -- and writes (common_r, denom_r) straight into the replicate's key block; the blocks
 * go to the host for distances and come back, and the replicate trees are joined as further components of rtc_nj_clusters' own
 * launches.  The host counts the splits, O(B m) nodes per tree.  A component that cannot hold its own block, one replicate block
 * and one band: RTC_ERR_NOMEM, the message naming m and the bytes; no fallback.  replicates outside 1 .. 256: RTC_ERR_ARG.
 * rtc_nj_counters describes the main trees as after rtc_nj_clusters.  Synchronous. */
int rtc_nj_support(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                   const uint32_t* h_comp, int kmer_size, uint32_t replicates, uint64_t seed, rtc_njoin* h_joins, uint64_t cap,
                   uint64_t* h_n_joins, uint64_t* h_first, uint32_t* h_support);
/* The last rtc_nj_support: out[0] replicates, out[1] replicate trees joined, out[2] counting ns, out[3] host distance ns (copies
 * included), out[4] joining ns, out[5] split ns, out[6] whole call ns, out[7] replicate groups, out[8] records that name a
 * split, out[9] the sum of their counts. */
int rtc_nj_support_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* word(hash, seed, word) above.  Host only, no context. */
uint64_t rtc_jackknife_word(uint64_t hash, uint64_t seed, uint32_t word);
/* The counting kernel's pair routine over an edge list: d_common[e * 64 + r] = common_r of the pair (d_edges[e].i, d_edges[e].j),
 * e < m, both below n, for the replicates r of the given word (the edge's own count is ignored); d_size, where it is not NULL,
 * gets d_size[g * 64 + r] = size_r(g) for every sketch.  One wave per pair: the shorter list is staged in LDS when it has at most
 * 1024 hashes (rtc_jackknife.h: JK_LDS_ELEMS) and searched in global memory otherwise.  Context stream, asynchronous. */
int rtc_jackknife_pairs_dev(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                            const rtc_cedge* d_edges, uint64_t m, uint64_t seed, uint32_t word, uint32_t* d_common, uint32_t* d_size);

/* ---- clust-mst --cluster-support: jackknife support of the clusters themselves ---------------------------------------- */
/* Which clusters of a partition survive resampling of the sketches' hashes: for every cluster, in how many of B delete-half
 * jackknife replicates it comes back whole and alone.  This is the definition (tests/refsupport.py restates it); everything is
 * integer, and the one double function is evaluated on the host, when the keep table is built.
 *   Input.  Sketches as everywhere (width 4 or 8, ascending, distinct), n, a labelling h_comp[n] (any labelling), kmer_size,
 *     threshold, replicates B in 1 .. 256 and seed.  Clusters are numbered by their smallest member, a cluster's members are taken
 *     ascending; f_c is cluster c's smallest member and m_c its size.
 *   Mask, size_r, common_r, denom_r.  rtc_nj_support's, through rtc_jackknife_word.
 *   Candidates.  The pairs rtc_pair_edges_dev lists for radio = floor(2 e^(threshold (kmer_size - 1)) - 1), saturated at INT32_MAX:
 *     they share a hash and pass the size-ratio rule on the full sketches -- the MST's own candidates.  Replicates do not re-apply
 *     the size rule.
 *   Replicate graph G_r.  Candidate (i, j) is an edge of G_r iff common_r > 0 and
 *     rtc_linkage_distance(common_r, denom_r, kmer_size) <= threshold: the function that weighs the MST's edges, cut as the forest
 *     is cut.
 *   Keep table.  need[d], d in 0 .. D, is the least c in 1 .. d with rtc_linkage_distance(c, d, kmer_size) <= threshold, or d + 1
 *     if there is none; the device keeps an edge iff common_r >= need[denom_r].  D is the largest |a| + |b| over the sketches; a
 *     table of more than 2^25 entries is RTC_ERR_UNSUPPORTED (a cap, not a measurement).  The rule is monotone in c: checked on
 *     the host for (k, d) = (21, 0.05), (21, 0.001), (16, 0.2), (31, 0.9), (21, 0) and every denom up to 3 000
 *     (tests/test_cpu_support.py).
 *   Inner and crossing edges.  An edge of G_r is inner if both ends carry the same label and crossing otherwise.  P_r(g) is the
 *     smallest member of g's component in the graph of the inner edges of G_r; it always lies in g's cluster.  piece_r(g) is the
 *     number of genomes x with P_r(x) = P_r(g).
 *   Per cluster and replicate.  whole iff P_r(g) = f_c for every member; pure iff no crossing edge of G_r has an end in c (that is:
 *     every component of G_r that meets c lies inside c); pieces_r(c) = |{g in c : P_r(g) = g}|.
 *   Records.  One rtc_csupport per cluster, in cluster order: size = m_c; recovered = |{r : whole and pure}|, split = pure only,
 *     merged = whole only, mixed = neither -- the four always sum to B; max_pieces = max_r pieces_r(c).
 *     h_together[g] = sum_r (piece_r(g) - 1).
 *   Consequences.  A singleton cluster is recovered unless a crossing edge reaches it; an empty sketch has no candidate.
 * threshold below 0 or NaN, replicates outside 1 .. 256, width not 4 or 8, NULLs, kmer_size < 1, n >= 2^31 - 1: RTC_ERR_ARG.
 * threshold >= 1: RTC_ERR_UNSUPPORTED (pairs without a common hash are at distance 1 and no list holds them); a sketch of 2^31
 * hashes or more likewise.  Memory that does not fit: RTC_ERR_NOMEM with the bytes in the message, no fallback.
 *
 * The call: the pair phase in row chunks under RTC_EDGE_BUDGET as in rtc_cluster_quality; a chunk's candidates are taken in
 * pieces of 2^20 and, per piece and word of 64 replicates, rtc_jackknife_pairs_dev counts common_r, a mask kernel (one wave a
 * candidate, a replicate a lane) forms the 64-bit keep mask of every candidate -- inner edges with a non-zero mask go to a
 * compacted list, a crossing edge ORs its mask into a word per cluster end -- and rtc_components64_dev hooks the list into the
 * word's labels; at the end one wave per cluster tallies the word.  A word's state is 512 bytes a sketch; as many words as
 * RTC_SUPPORT_BYTES allows (default: half the free HBM, at least one word) are held at once, and the pair phase runs once per
 * group of words held.  The records depend on none of: the row chunks, the words held at once, the pair routine's LDS or global
 * path, RTC_PAIR_FORCE_MERGE.  h_out[number of distinct labels], h_together[n].  Synchronous. */
typedef struct { uint32_t size, recovered, split, merged, mixed, max_pieces; } rtc_csupport; /* 24 bytes */
int rtc_cluster_support(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                        const uint32_t* h_comp, int kmer_size, double threshold, uint32_t replicates, uint64_t seed, rtc_csupport* h_out,
                        uint64_t* h_together);
/* The last rtc_cluster_support: out[0] row chunks (over every run of the pair phase), out[1] candidates, out[2] inner edges kept
 * (a candidate counts once per word in which some replicate keeps it), out[3] crossing edges kept (likewise), out[4] hooking
 * passes, out[5] pair ns, out[6] count ns (the pair routine and the mask kernel), out[7] components ns, out[8] tally ns, out[9]
 * whole call ns. */
int rtc_cluster_support_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* need[0 .. max_denom] above into out.  Host only, no context.  kmer_size < 1, threshold below 0 or NaN, out NULL: RTC_ERR_ARG;
 * more than 2^25 entries: RTC_ERR_UNSUPPORTED. */
int rtc_support_keep_table(int kmer_size, double threshold, uint32_t max_denom, uint32_t* out);
/* The connected components of 64 graphs over the same n vertices at once: graph r has the edges e < m whose d_mask[e] has bit r
 * set (d_edges[e].i and .j, both below n, in either order; the edge's count is ignored; duplicates and loops are allowed).
 * d_label[g * 64 + r] is state: on entry the smallest vertex of g's component under the edges given so far -- g itself for a
 * fresh start -- and on return the smallest vertex of g's component with these edges added, so chunks of edges may arrive one
 * after another, and a call on converged labels changes nothing.  One wave per edge, lane r graph r: every access to a vertex's
 * 64 labels is one 256-byte row.  Min-hooking on roots with pointer jumping, repeated until a device flag reports a pass
 * without change; the flag is read back once per pass.  Context stream, synchronous. */
int rtc_components64_dev(rtc_ctx* ctx, uint32_t n, const rtc_cedge* d_edges, const uint64_t* d_mask, uint64_t m, uint32_t* d_label);

/* ---- clust-mst --quality: silhouette and cluster separation of a finished partition ---------------------------------- */
/* The silhouette of every vertex of a labelled, weighted graph, and what a cluster's diameter and separation are read from, in
 * exact integers; this is the definition (tests/refquality.py restates it).  Q1 = 2^20 is distance 1.
 *   - Input: n vertices, m records (u, v, q): the pair u != v has distance q, 0 <= q <= Q1, in units of 2^-20.  Every pair that
 *     is not listed has distance Q1.  h_label[x] >= 0 is x's cluster, any number below n; a negative label means x is
 *     unclustered (noise): it is a member of nothing, it is nobody's neighbour, and its record is all zero with b_cluster =
 *     near_cluster = UINT32_MAX.  N_d is the number of vertices labelled d.
 *   - For a clustered x in cluster c and a cluster d: cnt(x, d) the listed neighbours of x labelled d, sum(x, d) the sum of
 *     their q, S(x, d) = sum(x, d) + (N_d - [d == c] - cnt(x, d)) Q1: the total distance from x to d's members other than x.
 *   - a_num = S(x, c), a_den = N_c - 1 (0 for a singleton).
 *   - b: among the clusters d != c that hold a listed neighbour of x, the one with the least mean S(x, d) / N_d, means compared
 *     exactly as S1 N2 against S2 N1 in 128 bits (S < 2^51, N < 2^31), equal means to the smaller d.  If that mean is strictly
 *     below Q1: b_num = S, b_den = N_d, b_cluster = d.  Otherwise every other cluster is at mean distance exactly 1 (a cluster
 *     without a listed neighbour always is): b_num = Q1, b_den = 1, b_cluster = UINT32_MAX.  If there is no other clustered
 *     vertex at all: b_num = 0, b_den = 0, b_cluster = UINT32_MAX.
 *   - far_q: the largest distance from x to a member of c: Q1 as soon as cnt(x, c) < N_c - 1, otherwise the largest listed q
 *     into c; 0 for a singleton.  A cluster's diameter is the largest far_q of its members.
 *   - near_q, near_cluster: the least q over the listed neighbours with a label >= 0 and != c, and that neighbour's cluster,
 *     equal q to the smaller cluster; Q1 and UINT32_MAX without such a neighbour.  A cluster's separation is the least near_q
 *     of its members.
 *   - rtc_silhouette_value (host only): 0 when a_den == 0 or b_den == 0; otherwise a = (double)a_num / ((double)a_den *
 *     1048576.0), b likewise, and the value is (b - a) / max(a, b), 0 when both are 0.  Every operation is one IEEE-754 double
 *     operation in that order.  This is Rousseeuw's s(x) with a singleton at 0.
 * Errors, RTC_ERR_ARG with a message naming the record: u == v, u or v >= n, q > Q1, a label >= n, a pair given twice in either
 * orientation (whatever the labels of its ends).  n >= 2^31 - 1: RTC_ERR_ARG.
 * Every sum is an integer (integer atomics: order-independent) and every comparison exact, so the records depend neither on the
 * scheduling nor on the kernel path of a row: a row of up to 128 entries takes one wave with the table in LDS, one of up to
 * 1 024 a 256-lane workgroup with a larger LDS table, a longer one a table of at least twice its entries in global memory
 * (rabbittclust_amd/csrc/rtc_quality.h).  RTC_SIL_GLOBAL=1 sends every row through the last; results are identical.  The device
 * holds the CSR of the 2 m directed entries and what builds it, about 124 bytes a record and 100 a vertex, and on top of that the
 * global tables: 16 bytes a slot, 2 to 4 slots an entry of every row past 1 024 entries (of every row, 64 slots at least, under
 * RTC_SIL_GLOBAL=1).  The call asks for the free memory twice, before the CSR and before the tables; if either does not fit:
 * RTC_ERR_NOMEM with the bytes in the message, no fallback.  Synchronous. */
typedef struct { uint64_t a_num, b_num; uint32_t a_den, b_den, b_cluster, far_q, near_q, near_cluster; } rtc_sil; /* 40 bytes */
int rtc_silhouette(rtc_ctx* ctx, uint32_t n, const rtc_wedge* h_edges, uint64_t m, const int32_t* h_label, rtc_sil* h_out /* [n] */);
/* The last rtc_silhouette (or the score of the last rtc_cluster_quality): out[0] records, out[1] directed entries of the CSR,
 * out[2] clustered vertices, out[3] clusters, out[4] / out[5] / out[6] rows on the wave / workgroup / global-table path (a vertex
 * without an entry, and every unclustered one, is on none), out[7] CSR ns, out[8] row kernels ns, out[9] whole call ns. */
int rtc_silhouette_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* the row paths of the last score: bit 0 one wave, bit 1 a 256-lane workgroup, bit 2 the table in global memory */
int rtc_silhouette_last_path(const rtc_ctx* ctx);
double rtc_silhouette_value(const rtc_sil* r);
/* The same over sketches (KSSD or MinHash hash sets, width 4 or 8): the score of any labelling of them -- clust-mst's cut,
 * rtc_dbscan's labels with -1 for noise, rtc_louvain's.  The listed pairs are all pairs that share a hash, from
 * rtc_pair_edges_dev with radio = -1 over row chunks under RTC_EDGE_BUDGET as in rtc_dbscan: there is no size-ratio rule, a pair
 * that the MST's filter drops has its true distance here.  Each chunk goes to the host, where every pair gets
 *   q = min(Q1, llround(rtc_linkage_distance(common, |u| + |v| - common, kmer_size) * 1048576.0))
 * with the host's libm on the context's host threads (rtc_ctx_set_host_threads): the set-Jaccard of the index path through the
 * function that weighs --linkage and --nj-tree.  An empty sketch shares nothing and is at distance 1 from everything.  The
 * records then go through rtc_silhouette's implementation.
 * Memory: the host holds every candidate at once, 12 bytes as it arrives and 12 as a record; the device holds one chunk of the
 * pair phase (12 bytes a candidate), and after it the score's 124 bytes a candidate and 100 a sketch, and its global tables.  RTC_ERR_NOMEM if that does
 * not fit, no fallback.  kmer_size < 1, width not 4 or 8, NULLs, a label >= n, n >= 2^31 - 1: RTC_ERR_ARG; a sketch of 2^31 hashes
 * or more: RTC_ERR_UNSUPPORTED.  Synchronous. */
int rtc_cluster_quality(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                        const int32_t* h_label, int kmer_size, rtc_sil* h_out /* [n] */);
/* The last rtc_cluster_quality: out[0] row chunks, out[1] candidates, out[2] / out[3] / out[4] rows on the wave / workgroup /
 * global-table path, out[5] pair ns, out[6] host distance ns (copies included), out[7] score ns, out[8] clusters, out[9] whole
 * call ns. */
int rtc_cluster_quality_counters(const rtc_ctx* ctx, uint64_t out[10]);

/* ---- clust-mst --upgma: average linkage (UPGMA) in exact integers ------------------------------------------------------ */
/* Average-linkage agglomeration of one set of m clusters-to-be; this is the definition (tests/refupgma.py restates it).
 * Q1 = 2^20 is distance 1.  All quantities are unsigned integers; no step on the device forms a floating-point value.
 *   - Input: a symmetric m x m matrix of uint64_t sums S[i][j], the diagonal ignored, and sizes w[i] >= 1 (NULL: all 1).
 *     S[i][j] is the sum of the quantised distances between the members of i and those of j; for single points it is the pair's
 *     q, 0 <= q <= Q1.  W is the sum of all w; W < 2^22 keeps every S below 2^62 and every cross product below 2^106.
 *   - Mean: D(a, b) = S(a, b) / (n_a n_b).  Two means are compared exactly, S1 (n_a2 n_b2) against S2 (n_a1 n_b1), in 128 bits.
 *   - Every index starts as an active cluster named by its index, n_i = w[i].  A step takes the active pair a < b with the least
 *     mean, ties to the smallest a, then the smallest b; emits rtc_umerge {a, b, size_a, size_b, sum}, sizes and sum those of the
 *     pair before the merge; sets S(a, c) = S(a, c) + S(b, c) for every other active c; sets n_a += n_b and retires b: the
 *     cluster keeps the name a.  Exactly m - 1 merges, in step order; there is no stop bound, the tree needs all of them.
 *   - Height and cut are the host's.  rtc_upgma_distance(sum, size_a, size_b) = (double)sum / (((double)size_a *
 *     (double)size_b) * 1048576.0), each operation one IEEE-754 double operation in that order.  The cut is in integers:
 *     qcut = llround(threshold * 1048576.0), and a component's merges apply in order up to, not including, the first with
 *     sum > qcut size_a size_b (128 bits).  Exact means never decrease from step to step -- the new D(a + b, c) is a weighted
 *     mean of D(a, c) and D(b, c), each >= D(a, b) -- so the cut is a prefix.
 * Three kernel paths, chosen per component: m <= 64 one wave with S and the sizes in LDS; larger ones a 256-lane workgroup with
 * S in global memory, the whole dendrogram in one launch; from RTC_UPGMA_GRID_MIN points on (default 128; set, it holds down to 4)
 * the whole device, two launches a merge, all of them enqueued without a read-back.  Every path scans all active pairs at every
 * step and compares on the triple (mean, a, b), so the records are the same on every path.  A grid-path scan launch has one
 * workgroup per four rows of the active list, at most RTC_UPGMA_SCAN_BLOCKS of them (1 .. 1024, default and ceiling 1024); past
 * that a workgroup takes further rows.  The switch is for tests: it brings that at any m. */
typedef struct { uint32_t a, b, size_a, size_b; uint64_t sum; } rtc_umerge; /* 24 bytes */
/* One matrix that is already on the device: d_sum[i * ld + j], 8-byte aligned, ld >= m; it is read and overwritten.  h_size[m]
 * on the host, or NULL.  h_merges: room for max(m - 1, 1) records; m - 1 are written, a and b as indices.  The sums are not
 * checked against Q1 w_i w_j: any are taken, and the records are the definition's, while every S the run forms stays below 2^62.
 * W >= 2^22, ld < m, NULLs, a size of 0: RTC_ERR_ARG.  Synchronous. */
int rtc_upgma_dev(rtc_ctx* ctx, uint32_t m, uint64_t* d_sum, uint64_t ld, const uint32_t* h_size /* may be NULL */, rtc_umerge* h_merges);
/* One dendrogram per component of a labelling of n sketches: arguments, component numbering, member order, h_first and
 * RTC_ERR_OVERFLOW (with the needed count) as rtc_nj_clusters has them; a component of m members has m - 1 records, a and b
 * genome indices, and one of one member costs nothing.  The key blocks are rtc_linkage_complete's; each batch is copied to the
 * host, every cell becomes q = min(Q1, llround(rtc_linkage_distance(common, denom, kmer_size) * 1048576.0)) -- Q1 for
 * common == 0 or denom == 0, rtc_cluster_quality's formula -- on the context's host threads, the q go back as uint64_t into the
 * same 8-byte cells and the device agglomerates.  The byte budget of a batch is RTC_UPGMA_BYTES (default half the free HBM); a
 * component whose 8 m^2 bytes and one band exceed it: RTC_ERR_NOMEM, the message naming m and the bytes; no fallback. */
int rtc_upgma_clusters(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                       const uint32_t* h_comp, int kmer_size, rtc_umerge* h_merges, uint64_t cap, uint64_t* h_n_merges, uint64_t* h_first);
/* The last rtc_upgma_clusters (or rtc_upgma_dev): out[0] components of two or more, out[1] on the wave path, out[2] on the
 * workgroup path, out[3] on the grid path, out[4] merges, out[5] row rescans (0: every step is a full scan), out[6] fill ns,
 * out[7] host distance ns (copies included), out[8] agglomeration ns, out[9] whole call ns. */
int rtc_upgma_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* The paths of the last call: bit 0 the wave path, bit 1 the workgroup path, bit 2 the grid path. */
int rtc_upgma_last_path(const rtc_ctx* ctx);
/* RTC_UPGMA_SCAN_BLOCKS as this context holds it: the most workgroups of a grid-path scan launch, 1 .. 1024 (unset: 1024). */
int rtc_upgma_scan_blocks(const rtc_ctx* ctx);
/* The height of a merge, as defined above.  Host only. */
double rtc_upgma_distance(uint64_t sum, uint32_t size_a, uint32_t size_b);

/* ---- clust-mst --pangenome: core and accessory hashes of the clusters ---------------------------------------------------- */
/* What the members of a cluster hold in common and what only a few of them hold: for every cluster the number of members that
 * hold each hash.  A KSSD sketch is a fixed subsample of k-mer space, so the answer for the sketches estimates the answer for
 * the k-mers.  This is the definition (tests/refpangenome.py restates it); everything on the device is an integer.
 *   Input.  Sketches as everywhere (width 4 or 8, ascending, distinct), n, h_label[n] as rtc_cluster_quality takes it (any number
 *     in [0, n); negative: unclustered), soft_pct and cloud_pct with 1 <= cloud_pct <= soft_pct <= 100.  Clusters are numbered by
 *     their smallest member; m_c is the size of cluster c.
 *   Occurrence.  occ_c(h) is the number of members of c whose sketch holds h; occ(g, h) = occ_c(h) for c = g's cluster.
 *   Classes of a hash in c, every compare in 64-bit integers.  Core: occ == m_c.  Soft: not core and 100 occ >= soft_pct m_c.
 *     Cloud: not core and 100 occ < cloud_pct m_c.  Shell: the rest.
 *   Per cluster, one rtc_pan in cluster order: size = m_c; total = the sum of the members' sketch lengths; pan = the number of
 *     distinct hashes; core, soft, shell, cloud (they sum to pan); single = the hashes with occ == 1.
 *   Histogram.  Cluster c owns h_hist[o_c .. o_c + m_c), o_c the sum of the sizes of the clusters before it; entry f - 1 is the
 *     number of distinct hashes with occ == f.  The caller gives n entries; those past the clustered genomes are zeroed.
 *   Per genome, rtc_pan_genome[n]: unique = its hashes with occ == 1; core, soft, shell, cloud = its hashes by class; occ_sum =
 *     the sum of occ over its hashes.  An unclustered genome gets an all-zero record and belongs to no cluster.  An empty sketch
 *     contributes nothing (and still counts in m_c).
 *   Consequences.  A singleton cluster has pan = core = single = len.  sum_f f hist[f] = total.  hist[m] = core.  The members'
 *     unique values sum to hist[1].  The members' occ_sum values sum to sum_f f^2 hist[f].
 * Percentages out of order, a label >= n, width not 4 or 8, NULLs, n >= 2^31 - 1: RTC_ERR_ARG.  A sketch of 2^31 hashes or more:
 * RTC_ERR_UNSUPPORTED.  Memory that does not fit: RTC_ERR_NOMEM with the bytes in the message, no fallback.
 *
 * The call.  One open-addressing table of (hash, count) slots per cluster, never more than half full; three steps over it: count
 * (insert with a 64-bit compare-and-swap, add 1), sweep (every slot into the histogram) and look-up (every member's hashes again,
 * for the genomes' records).  The members are reached through the clustered genomes ordered by cluster, a permutation and segment
 * offsets built once on the host.  A cluster of up to 512 records (the sum of its members' lengths) takes one wave with table
 * and histogram in LDS, one of up to 2 048 a 256-lane workgroup likewise, everything larger a table of 1 << ceil(log2(2 K)) slots
 * in one arena in global memory, where count, sweep and look-up are device-wide kernels over all arena clusters at once: a member
 * a wave, 256 slots a tile (rabbittclust_amd/csrc/rtc_pan.h).  RTC_PAN_GLOBAL=1 sends every cluster through the arena; results are
 * identical.  The all-ones 64-bit value marks an empty slot; a hash of that value is counted in a word of its own per cluster, and
 * 0 is a key like any other.  A cluster's class counts are sums over its histogram, formed on the host.  Clusters are taken in
 * groups, in cluster order, whose arena (12 bytes a slot) and views (56 bytes a member, 48 a cluster) fit RTC_PAN_BYTES (default:
 * half the free HBM); a cluster that does not fit alone: RTC_ERR_NOMEM.  The records depend on neither the grouping nor the path:
 * every sum is an integer and every compare exact.  h_clusters[number of distinct labels >= 0, at least 1], h_hist[n],
 * h_genomes[n].  Returns the number of clusters in *h_n_clusters.  Synchronous. */
typedef struct { uint64_t total, pan, core, soft, shell, cloud, single; uint32_t size, pad; } rtc_pan; /* 64 bytes */
typedef struct { uint64_t occ_sum; uint32_t unique, core, soft, shell, cloud, pad; } rtc_pan_genome; /* 32 bytes */
int rtc_pangenome(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                  const int32_t* h_label, uint32_t soft_pct, uint32_t cloud_pct, rtc_pan* h_clusters, uint64_t* h_hist,
                  rtc_pan_genome* h_genomes, uint32_t* h_n_clusters);
/* The last rtc_pangenome: out[0] clusters, out[1] clustered genomes, out[2] records (the clustered genomes' hashes), out[3]
 * distinct hashes (the sum of pan), out[4] / out[5] / out[6] clusters on the wave / workgroup / arena path, out[7] groups, out[8]
 * kernel ns, out[9] whole call ns. */
int rtc_pangenome_counters(const rtc_ctx* ctx, uint64_t out[10]);
/* The kernel ns of the last rtc_pangenome by step: out[0] count (the LDS kernels do all three steps in one launch and are counted
 * here), out[1] the arena's sweep, out[2] the arena's look-up. */
int rtc_pangenome_phases(const rtc_ctx* ctx, uint64_t out[3]);
/* the cluster paths of the last call: bit 0 one wave, bit 1 a 256-lane workgroup, bit 2 the arena in global memory */
int rtc_pangenome_last_path(const rtc_ctx* ctx);
/* The expected pangenome and core size after j of a cluster's m members, over all orders of the members, from the cluster's
 * histogram h_hist[0 .. m) (entry f - 1: the hashes held by f members).  The closed form; nothing is sampled.  Host only, no
 * context.
 *   Points: j = 1 .. m when m <= 256, else the 256 values 1 + floor(i (m - 1) / 255), i = 0 .. 255.
 *   For every f with hist[f] > 0 start u = v = 1.0 and for i = 0, 1, ..: u = u * (double)(m - f - i) / (double)(m - i), and 0 from
 *     the first zero factor on; v = v * (double)(f - i) / (double)(m - i), f - i a signed integer.  u_f(j), v_f(j) are the
 *     values after the factors i = 0 .. j - 1: the chance that none, and that every one, of j members holds a hash held by f.
 *   pan(j) is the sum over ascending f of (double)hist[f] * (1.0 - u_f(j)), core(j) that of (double)hist[f] * v_f(j), both
 *     starting from 0.0.  Every step is one IEEE-754 double operation in that order; nothing is contracted into an fma.
 *   It follows exactly that pan(m) = pan and core(m) = hist[m].
 * The f are spread over `threads` host threads (each u_f, v_f is independent; the final sums keep their order).  h_j, h_pan,
 * h_core: room for min(m, 256) entries each; *h_points gets the number of points, 0 for m == 0.  NULLs: RTC_ERR_ARG. */
int rtc_pan_growth(const uint64_t* h_hist, uint32_t m, int threads, uint32_t* h_j, double* h_pan, double* h_core, uint32_t* h_points);

#ifdef __cplusplus
}
#endif
#endif /* RTCLUST_H */
