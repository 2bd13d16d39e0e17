// rtc_nj_support.hip -- clust-mst --nj-support: jackknife support values for the neighbour-joining trees.
//
// The definition is in include/rtclust.h (tests/refnjsupport.py restates it).  A replicate keeps a hash iff its bit of the hash's
// mask word is set, so one pass over a pair's common hashes counts 64 replicates at once, one per lane (rtc_jackknife.h):
//   jk_size_kernel    size_r of every row of a batch (or of every sketch), one wave a list
//   jk_blocks_kernel  one wave per row a of a component: a's list staged in LDS once, then every partner b > a walked against it;
//                     lane r then holds common_r and writes (common_r, size_r(a) + size_r(b) - common_r) into cell (a, b) and
//                     (b, a) of replicate r's key block -- the counts never exist as a table
//   jk_edges_kernel   the same pair routine over an edge list, the counts written out (rtc_jackknife_pairs_dev)
// The replicate blocks have rtc_key_blocks' geometry, one copy of the batch's blocks per replicate of a group; they go to the host
// for distances as the main blocks do and are joined by rtc_nj's own paths as further components of one launch.  The host then
// counts, for every inner branch of the main tree, the replicate trees that hold its split -- Day's algorithm: the main tree's
// leaves numbered in depth-first order from the component's smallest member, every cluster an interval of that numbering, and a
// replicate's cluster is one of them iff its least and greatest number span exactly its size and the interval is in the table.
#include <algorithm>
#include <atomic>
#include <memory>
#include <thread>
#include <vector>

#include "rtc_jackknife.h"

namespace {

constexpr uint32_t NJ_NONE = 0xFFFFFFFFu;
constexpr uint32_t NJS_MAX_REPLICATES = 256;

// a row of a batch's permuted set: its genome, and its component's block and first row
struct jk_row { uint64_t key_off, ld; uint32_t first, m, g, pad; };

template <typename T>
__global__ __launch_bounds__(64) void jk_size_kernel(const T* __restrict__ hashes, const uint64_t* __restrict__ start, const uint32_t* __restrict__ len,
                                                     const jk_row* __restrict__ rows, uint32_t n, uint64_t key, uint32_t* __restrict__ size) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t x = blockIdx.x; x < n; x += gridDim.x) {  // uniform
    const uint32_t g = rows ? rows[x].g : x;
    size[(uint64_t)x * 64 + lane] = jk_size_wave(hashes + start[g], len[g], key, lane);
  }
}

// grid (rows of the batch, partner slices).  Replicates [r0, r1) of word w = r0 / 64 .. are written: lane r of the word is
// replicate 64 w + r, block 64 w + r - r0 of rep (n_keys cells each).
template <typename T>
__global__ __launch_bounds__(64) void jk_blocks_kernel(const T* __restrict__ hashes, const uint64_t* __restrict__ start, const uint32_t* __restrict__ len,
                                                       const jk_row* __restrict__ rows, uint64_t key, const uint32_t* __restrict__ size, uint32_t w,
                                                       uint32_t r0, uint32_t r1, uint64_t n_keys, uint64_t* __restrict__ rep) {
  __shared__ T sb[JK_LDS_ELEMS];
  const uint32_t lane = threadIdx.x, x = blockIdx.x;
  const jk_row ra = rows[x];
  const uint32_t a = x - ra.first;
  if (ra.m < 4 || a + 1 + blockIdx.y >= ra.m) return;  // uniform: a tree without inner branches, or no partner in this slice
  const T* la = hashes + start[ra.g];
  const uint32_t na = len[ra.g];
  const bool staged = jk_stage(sb, la, na, lane);
  const uint32_t r = w * 64 + lane;
  const bool mine = r >= r0 && r < r1;
  const uint32_t sa = size[(uint64_t)x * 64 + lane];
  uint64_t* blk = rep + (uint64_t)(mine ? r - r0 : 0) * n_keys + ra.key_off;
  for (uint32_t b = a + 1 + blockIdx.y; b < ra.m; b += gridDim.y) {  // uniform
    const uint32_t xb = ra.first + b, gb = rows[xb].g;
    const uint32_t common = jk_pair_wave(la, na, sb, staged, hashes + start[gb], len[gb], key, lane);
    if (mine) {
      const uint32_t denom = sa + size[(uint64_t)xb * 64 + lane] - common;
      const uint64_t cell = (uint64_t)common | (uint64_t)denom << 32;  // rtc_lkey {common, denom}
      blk[(uint64_t)a * ra.ld + b] = cell;
      blk[(uint64_t)b * ra.ld + a] = cell;
    }
  }
}

// one wave per edge: the shorter list staged, the longer one walked
template <typename T>
__global__ __launch_bounds__(64) void jk_edges_kernel(const T* __restrict__ hashes, const uint64_t* __restrict__ start, const uint32_t* __restrict__ len,
                                                      const rtc_cedge* __restrict__ edges, uint64_t m, uint64_t key, uint32_t* __restrict__ common) {
  __shared__ T sb[JK_LDS_ELEMS];
  const uint32_t lane = threadIdx.x;
  for (uint64_t e = blockIdx.x; e < m; e += gridDim.x) {  // uniform
    uint32_t i = edges[e].i, j = edges[e].j;
    if (len[i] > len[j]) { const uint32_t t = i; i = j; j = t; }
    const T* s = hashes + start[i];
    const uint32_t ns = len[i];
    const bool staged = jk_stage(sb, s, ns, lane);
    common[e * 64 + lane] = jk_pair_wave(s, ns, sb, staged, hashes + start[j], len[j], key, lane);
  }
}

// ---- distances ----------------------------------------------------------------------------------------------------------------
// rtc_linkage_distance per (common, denom), kept in a triangle over denom <= D where that is at most NJS_MEMO_DENOM: the same
// function, called once per key instead of once per cell, and the same bits.  A replicate's keys repeat heavily -- B copies of
// every pair, all near half of the main key.  Threads race only to store the same value.
constexpr uint32_t NJS_MEMO_DENOM = 4096;  // (D + 1) (D + 2) / 2 doubles: 64 MiB at the cap
struct njs_memo {
  uint32_t D = 0;
  int kmer_size = 0;
  std::unique_ptr<std::atomic<uint64_t>[]> t;
  void init(uint32_t max_denom, int k) {
    kmer_size = k;
    D = std::min(max_denom, NJS_MEMO_DENOM);
    const size_t cells = ((size_t)D + 1) * ((size_t)D + 2) / 2;
    t.reset(new std::atomic<uint64_t>[cells]);
    for (size_t i = 0; i < cells; i++) t[i].store(~0ull, std::memory_order_relaxed);  // no distance has these bits
  }
  double at(uint32_t common, uint32_t denom) const {
    if (common == 0 || denom == 0) return 1.0;
    if (denom > D || common > denom) return rtc_linkage_distance(common, denom, kmer_size);
    std::atomic<uint64_t>& slot = t[(size_t)denom * (denom + 1) / 2 + common];
    uint64_t bits = slot.load(std::memory_order_relaxed);
    double d;
    if (bits == ~0ull) {
      d = rtc_linkage_distance(common, denom, kmer_size);
      memcpy(&bits, &d, 8);
      slot.store(bits, std::memory_order_relaxed);
    } else {
      memcpy(&d, &bits, 8);
    }
    return d;
  }
};

// keys -> distances in place as rtc_nj_clusters forms them (the diagonal 0), a pair once: the fill wrote the same key on both sides of the diagonal
void njs_distances(uint64_t* cells, const std::vector<rtc_kb_comp>& comps, const njs_memo& memo, int threads) {
  struct unit { const rtc_kb_comp* c; uint32_t r0, r1; };
  std::vector<unit> units;
  for (const rtc_kb_comp& c : comps) {
    const uint32_t rows = (uint32_t)std::max<uint64_t>(1, 32768 / c.m);
    for (uint32_t r = 0; r < c.m; r += rows) units.push_back(unit{&c, r, std::min(c.m, r + rows)});
  }
  auto work = [&](size_t u0, size_t stride) {
    for (size_t u = u0; u < units.size(); u += stride) {
      const rtc_kb_comp& c = *units[u].c;
      uint64_t* blk = cells + c.key_off;
      for (uint32_t i = units[u].r0; i < units[u].r1; i++) {
        uint64_t* row = blk + (uint64_t)i * c.ld;
        const double zero = 0.0;
        memcpy(&row[i], &zero, 8);
        for (uint32_t j = i + 1; j < c.m; j++) {
          const double d = memo.at((uint32_t)row[j], (uint32_t)(row[j] >> 32));  // rtc_lkey {common, denom}, little endian
          memcpy(&row[j], &d, 8);
          memcpy(&blk[(uint64_t)j * c.ld + i], &d, 8);
        }
      }
    }
  };
  const size_t T = std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), units.size()));
  if (T == 1) { work(0, 1); return; }
  std::vector<std::thread> pool;
  for (size_t t = 0; t < T; t++) pool.emplace_back(work, t, T);
  for (std::thread& th : pool) th.join();
}

// ---- splits -----------------------------------------------------------------------------------------------------------------
// A tree of m >= 4 leaves from its m - 2 records (local indices): leaves 0 .. m - 1, record e's node m + e.  The walk starts at
// leaf 0, the component's smallest member, so the leaves below a node are the side of its upper branch that does not hold it.
struct njs_tree {
  uint32_t m = 0;
  std::vector<uint32_t> nb;      // three neighbours of node m + e at 3 e
  std::vector<uint32_t> up;      // the record-order parent of every node (NJ_NONE: the closing node)
  std::vector<uint32_t> order;   // nodes in depth-first preorder from leaf 0's neighbour
  std::vector<uint32_t> parent;  // the walk's parent
  void build(const rtc_njoin* rec, uint32_t m_) {
    m = m_;
    const uint32_t nn = 2 * m - 2;
    nb.assign((size_t)3 * (m - 2), NJ_NONE);
    up.assign(nn, NJ_NONE);
    std::vector<uint32_t> cur(m);
    for (uint32_t i = 0; i < m; i++) cur[i] = i;
    std::vector<uint32_t> deg(m - 2, 0), leaf_nb(m, NJ_NONE);
    auto link = [&](uint32_t node, uint32_t child) {
      nb[(size_t)3 * (node - m) + deg[node - m]++] = child;
      up[child] = node;
      if (child < m) leaf_nb[child] = node; else nb[(size_t)3 * (child - m) + deg[child - m]++] = node;
    };
    for (uint32_t e = 0; e + 2 < m; e++) {
      const uint32_t node = m + e;
      link(node, cur[rec[e].a]);
      link(node, cur[rec[e].b]);
      if (rec[e].c != NJ_NONE) link(node, cur[rec[e].c]);
      cur[rec[e].a] = node;
    }
    order.clear();
    parent.assign(nn, NJ_NONE);
    std::vector<uint32_t> stack;
    parent[leaf_nb[0]] = 0;
    stack.push_back(leaf_nb[0]);
    while (!stack.empty()) {
      const uint32_t v = stack.back();
      stack.pop_back();
      order.push_back(v);
      if (v < m) continue;
      for (int t = 2; t >= 0; t--) {
        const uint32_t c = nb[(size_t)3 * (v - m) + t];
        if (c != parent[v]) { parent[c] = v; stack.push_back(c); }
      }
    }
  }
};

// the main tree's table: leaf numbers, and the interval of every inner branch with the record that names it
struct njs_table {
  std::vector<uint32_t> number;                          // leaf -> its place in the walk (leaf 0 has none)
  std::vector<std::pair<uint64_t, uint32_t>> interval;  // (lo << 32 | hi, record), ascending
};

// lo, hi, count of the leaves below every node of t in num's numbering, children before parents
void njs_spans(const njs_tree& t, const std::vector<uint32_t>& num, std::vector<uint32_t>& lo, std::vector<uint32_t>& hi, std::vector<uint32_t>& cnt) {
  const uint32_t nn = 2 * t.m - 2;
  lo.assign(nn, NJ_NONE); hi.assign(nn, 0); cnt.assign(nn, 0);
  for (size_t s = t.order.size(); s-- > 0;) {
    const uint32_t v = t.order[s];
    if (v < t.m) { lo[v] = hi[v] = num[v]; cnt[v] = 1; }
    const uint32_t p = t.parent[v];
    if (p >= t.m) { lo[p] = std::min(lo[p], lo[v]); hi[p] = std::max(hi[p], hi[v]); cnt[p] += cnt[v]; }
  }
}

void njs_main_table(const njs_tree& t, njs_table* T) {
  T->number.assign(t.m, NJ_NONE);
  uint32_t k = 0;
  for (uint32_t v : t.order) if (v < t.m) T->number[v] = k++;
  std::vector<uint32_t> lo, hi, cnt;
  njs_spans(t, T->number, lo, hi, cnt);
  T->interval.clear();
  for (uint32_t v : t.order) {
    const uint32_t p = t.parent[v];
    if (v < t.m || p < t.m) continue;  // a leaf's branch, or the branch of leaf 0
    // the branch v - p is named by the record of whichever end is the other's child in record order
    const uint32_t rec = t.up[v] == p ? v - t.m : p - t.m;
    T->interval.emplace_back((uint64_t)lo[v] << 32 | hi[v], rec);
  }
  std::sort(T->interval.begin(), T->interval.end());
}

// adds one to support[record] for every inner branch of the main tree whose split the replicate tree holds
void njs_count(const njs_table& T, const njs_tree& rep, uint32_t* support, uint64_t* found) {
  std::vector<uint32_t> lo, hi, cnt;
  njs_spans(rep, T.number, lo, hi, cnt);
  for (uint32_t v : rep.order) {
    if (v < rep.m || rep.parent[v] < rep.m) continue;
    if (hi[v] - lo[v] + 1 != cnt[v]) continue;
    const uint64_t key = (uint64_t)lo[v] << 32 | hi[v];
    auto it = std::lower_bound(T.interval.begin(), T.interval.end(), std::make_pair(key, 0u));
    if (it != T.interval.end() && it->first == key) { support[it->second]++; (*found)++; }
  }
}

template <typename T>
void njs_launch_size(rtc_ctx* ctx, const void* d_hashes, const uint64_t* d_start, const uint32_t* d_len, const jk_row* d_rows, uint32_t n, uint64_t key,
                     uint32_t* d_size) {
  const uint32_t g = std::max<uint32_t>(1, std::min<uint32_t>(n, (uint32_t)ctx->num_cu * 64));
  hipLaunchKernelGGL(jk_size_kernel<T>, dim3(g), dim3(64), 0, ctx->stream, (const T*)d_hashes, d_start, d_len, d_rows, n, key, d_size);
}

}  // namespace

extern "C" uint64_t rtc_jackknife_word(uint64_t hash, uint64_t seed, uint32_t word) { return rtc_jk_word(hash, rtc_jk_mix(seed + word)); }

extern "C" int rtc_nj_support_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->nj_support[i];
  return RTC_OK;
}

extern "C" int rtc_jackknife_pairs_dev(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                       const rtc_cedge* d_edges, uint64_t m, uint64_t seed, uint32_t word, uint32_t* d_common, uint32_t* d_size) {
  if (!ctx) return RTC_ERR_ARG;
  if (width != 4 && width != 8) return rtc_fail(ctx, RTC_ERR_ARG, "width must be 4 or 8");
  if ((m && (!d_edges || !d_common)) || ((m || (n && d_size)) && (!d_start || !d_len))) return RTC_ERR_ARG;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t key = rtc_jk_mix(seed + word);
  if (m) {
    const dim3 g((uint32_t)std::min<uint64_t>(m, (uint64_t)ctx->num_cu * 64)), b(64);
    if (width == 8)
      hipLaunchKernelGGL(jk_edges_kernel<uint64_t>, g, b, 0, ctx->stream, (const uint64_t*)d_hashes, d_start, d_len, d_edges, m, key, d_common);
    else
      hipLaunchKernelGGL(jk_edges_kernel<uint32_t>, g, b, 0, ctx->stream, (const uint32_t*)d_hashes, d_start, d_len, d_edges, m, key, d_common);
    RTC_CHECK_LAUNCH(ctx);
  }
  if (d_size && n) {
    if (width == 8) njs_launch_size<uint64_t>(ctx, d_hashes, d_start, d_len, nullptr, n, key, d_size);
    else njs_launch_size<uint32_t>(ctx, d_hashes, d_start, d_len, nullptr, n, key, d_size);
    RTC_CHECK_LAUNCH(ctx);
  }
  return RTC_OK;
}

extern "C" int rtc_nj_support(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                              const uint32_t* h_comp, int kmer_size, uint32_t replicates, uint64_t seed, rtc_njoin* h_joins, uint64_t cap,
                              uint64_t* h_n_joins, uint64_t* h_first, uint32_t* h_support) {
  if (!ctx) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) ctx->nj_support[i] = 0;
  if (replicates < 1 || replicates > NJS_MAX_REPLICATES)
    return rtc_fail(ctx, RTC_ERR_ARG, "rtc_nj_support: replicates must lie in 1 .. %u", NJS_MAX_REPLICATES);
  if (cap && !h_support) return RTC_ERR_ARG;
  for (uint64_t i = 0; i < cap; i++) h_support[i] = 0;
  const uint64_t t0 = rtc_now_ns();
  uint64_t* S = ctx->nj_support;
  S[0] = replicates;
  const uint32_t B = replicates;
  std::vector<uint32_t> h_len;  // the sketch sizes, for the distance table's extent
  if (n && n < 0x7fffffffu && d_len && (width == 4 || width == 8)) {
    h_len.resize(n);
    RTC_HIP(ctx, hipSetDevice(ctx->device));
    RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }

  const rtc_nj_hook hook = [&](const rtc_kb_batch& b, const std::vector<rtc_kb_comp>& comps, const std::vector<rtc_njoin>& main_rec,
                               uint64_t total) -> int {
    const std::vector<uint32_t>&csize = *b.csize, &cfirst = *b.cfirst, &perm = *b.perm;
    const size_t nc = comps.size();
    bool any = false;
    for (const rtc_kb_comp& c : comps) any |= c.m >= 4;
    if (!any) return RTC_OK;  // no tree of the batch has an inner branch
    hipStream_t s = ctx->stream;
    // ---- the rows of the batch ----
    std::vector<jk_row> rows;
    {
      size_t i = 0;
      for (size_t q = b.c; q < b.ce; q++) {
        if (csize[q] < 2) continue;
        const rtc_kb_comp& c = comps[i++];
        const uint32_t first = (uint32_t)rows.size();
        for (uint32_t a = 0; a < c.m; a++) rows.push_back(jk_row{c.key_off, c.ld, first, c.m, perm[cfirst[q] + a], 0});
      }
    }
    const uint32_t n_rows = (uint32_t)rows.size();
    uint32_t m_max = 0;
    for (const rtc_kb_comp& c : comps) m_max = std::max(m_max, c.m);
    // the longest denominator a replicate of this batch can have: the two longest lists together
    uint32_t len1 = 0, len2 = 0;
    for (const jk_row& r : rows) { const uint32_t l = h_len[r.g]; if (l > len1) { len2 = len1; len1 = l; } else if (l > len2) len2 = l; }
    njs_memo memo;
    memo.init((uint32_t)std::min<uint64_t>((uint64_t)len1 + len2, 0xFFFFFFFFu), kmer_size);
    // ---- groups of as many replicates as the budget leaves room for beside the main blocks; whole words where that is many ----
    const uint64_t kb = b.n_keys * 8;
    uint64_t G = std::max<uint64_t>(1, (b.budget > kb ? b.budget - kb : 0) / kb);
    G = std::min<uint64_t>(G, B);
    if (G >= 64 && G < B) G -= G % 64;
    DevBuf bufs;
    jk_row* d_rows = nullptr;
    uint32_t* d_size = nullptr;
    uint64_t* d_rep = nullptr;
    RTC_TRY(bufs.get(ctx, n_rows, &d_rows));
    RTC_TRY(bufs.get(ctx, (size_t)n_rows * 64, &d_size));
    RTC_TRY(bufs.get(ctx, (size_t)(G * b.n_keys), &d_rep));
    RTC_HIP(ctx, hipMemcpyAsync(d_rows, rows.data(), (size_t)n_rows * sizeof(jk_row), hipMemcpyHostToDevice, s));
    // ---- the main trees' tables ----
    const uint64_t ts0 = rtc_now_ns();
    std::vector<njs_table> tables(nc);
    std::vector<uint64_t> rec_at(nc);  // where component i's records start in the call's output
    {
      njs_tree t;
      uint64_t at = total;
      for (size_t i = 0; i < nc; i++) {
        rec_at[i] = at;
        at += rtc_nj_records_of(comps[i].m);
        if (comps[i].m < 4) continue;
        t.build(main_rec.data() + comps[i].merge_off, comps[i].m);
        njs_main_table(t, &tables[i]);
      }
    }
    S[5] += rtc_now_ns() - ts0;
    // partner slices: enough waves for the device where the rows alone are few
    const uint32_t want = (uint32_t)ctx->num_cu * 8;
    const uint32_t gy = std::max<uint32_t>(1, std::min<uint32_t>(std::min<uint32_t>(m_max - 1, 1024), (want + n_rows - 1) / n_rows));
    std::vector<uint64_t> cells;
    std::vector<rtc_kb_comp> rcomps;
    std::vector<rtc_njoin> rrec;
    for (uint32_t r0 = 0; r0 < B; r0 += (uint32_t)G) {
      const uint32_t r1 = (uint32_t)std::min<uint64_t>(B, r0 + G), ng = r1 - r0;
      S[7]++;
      // ---- counting: the keys of replicates [r0, r1), word after word ----
      const uint64_t tc0 = rtc_now_ns();
      for (uint32_t w = r0 / 64; w <= (r1 - 1) / 64; w++) {
        const uint64_t key = rtc_jk_mix(seed + w);
        if (width == 8) {
          njs_launch_size<uint64_t>(ctx, d_hashes, d_start, d_len, d_rows, n_rows, key, d_size);
          RTC_CHECK_LAUNCH(ctx);
          hipLaunchKernelGGL(jk_blocks_kernel<uint64_t>, dim3(n_rows, gy), dim3(64), 0, s, (const uint64_t*)d_hashes, d_start, d_len, (const jk_row*)d_rows, key,
                             (const uint32_t*)d_size, w, r0, r1, b.n_keys, d_rep);
        } else {
          njs_launch_size<uint32_t>(ctx, d_hashes, d_start, d_len, d_rows, n_rows, key, d_size);
          RTC_CHECK_LAUNCH(ctx);
          hipLaunchKernelGGL(jk_blocks_kernel<uint32_t>, dim3(n_rows, gy), dim3(64), 0, s, (const uint32_t*)d_hashes, d_start, d_len, (const jk_row*)d_rows, key,
                             (const uint32_t*)d_size, w, r0, r1, b.n_keys, d_rep);
        }
        RTC_CHECK_LAUNCH(ctx);
      }
      RTC_HIP(ctx, hipStreamSynchronize(s));
      const uint64_t tc1 = rtc_now_ns();
      S[2] += tc1 - tc0;
      // ---- distances on the host, as the main blocks get them ----
      rcomps.clear();
      for (uint32_t g = 0; g < ng; g++)
        for (size_t i = 0; i < nc; i++) {
          if (comps[i].m < 4) continue;
          rtc_kb_comp c = comps[i];
          c.key_off += (uint64_t)g * b.n_keys;
          c.merge_off = c.scratch_off = 0;
          c.pad = (uint32_t)i;
          rcomps.push_back(c);
        }
      try { cells.resize((size_t)ng * b.n_keys); }
      catch (const std::bad_alloc&) {
        return rtc_fail(ctx, RTC_ERR_NOMEM, "rtc_nj_support: no host memory for %u replicate blocks of %llu bytes (a smaller RTC_NJ_BYTES makes smaller groups)", ng,
                        (unsigned long long)kb);
      }
      RTC_HIP(ctx, hipMemcpyAsync(cells.data(), d_rep, (size_t)ng * kb, hipMemcpyDeviceToHost, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
      njs_distances(cells.data(), rcomps, memo, ctx->host_threads);
      RTC_HIP(ctx, hipMemcpyAsync(d_rep, cells.data(), (size_t)ng * kb, hipMemcpyHostToDevice, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
      const uint64_t td1 = rtc_now_ns();
      S[3] += td1 - tc1;
      // ---- the replicate trees: further components of rtc_nj's launches ----
      uint64_t n_path[3];
      RTC_TRY(rtc_nj_join(ctx, (double*)d_rep, rcomps, rrec, n_path));
      const uint64_t tj1 = rtc_now_ns();
      S[4] += tj1 - td1;
      S[1] += rcomps.size();
      // ---- splits ----
      // a host thread takes the main trees i = t, t + T, ... with all their replicates: no two threads count into one record
      const size_t T = std::max<size_t>(1, std::min<size_t>((size_t)std::max(ctx->host_threads, 1), rcomps.size() / ng));
      std::vector<uint64_t> found(T, 0);
      auto work = [&](size_t t) {
        njs_tree rt;
        for (const rtc_kb_comp& c : rcomps) {
          const size_t i = c.pad;
          if (i % T != t || rec_at[i] + rtc_nj_records_of(c.m) > cap) continue;  // past cap: the call ends in RTC_ERR_OVERFLOW
          rt.build(rrec.data() + c.merge_off, c.m);
          njs_count(tables[i], rt, h_support + rec_at[i], &found[t]);
        }
      };
      if (T == 1) work(0);
      else {
        std::vector<std::thread> pool;
        for (size_t t = 0; t < T; t++) pool.emplace_back(work, t);
        for (std::thread& th : pool) th.join();
      }
      for (uint64_t f : found) S[9] += f;
      S[5] += rtc_now_ns() - tj1;
    }
    for (size_t i = 0; i < nc; i++) if (comps[i].m >= 4) S[8] += comps[i].m - 3;
    return RTC_OK;
  };
  const int st = rtc_nj_clusters_impl(ctx, "rtc_nj_support", d_hashes, width, d_start, d_len, n, h_comp, kmer_size, h_joins, cap, h_n_joins, h_first, 1, &hook);
  S[6] = rtc_now_ns() - t0;
  return st;
}
