// rtc_community.h -- what rtc_louvain (rtc_louvain.hip) and rtc_leiden (rtc_leiden.hip) share: a level's graph as a CSR built
// by one sort and one reduce_by_key, and the rules of the row kernel (rtc_rowtable.h) that score the communities next to a
// vertex: move_rule for both, place_rule for rtc_leiden_place.  The comment at the head of rtc_louvain.hip describes the three
// paths.
#ifndef RTC_COMMUNITY_H
#define RTC_COMMUNITY_H
#include "rtc_dbscan_common.h"
#include "rtc_rowtable.h"

namespace {

typedef __int128 i128;
constexpr uint32_t LV_WAVE_ROW = 128, LV_WAVE_SLOTS = 256, LV_BLOCK_ROW = 2048, LV_BLOCK_SLOTS = 4096;
constexpr uint32_t LV_NONE = RT_NONE;
constexpr uint32_t LV_WAVE_WGS_PER_CU = 32, LV_BLOCK_WGS_PER_CU = 3, LV_GLOBAL_WGS_PER_CU = 8;
// 12-byte slots (the community, the weight into it); a global table has 1 << 13 slots or more: above 2 * LV_BLOCK_ROW
struct lv_shape {
  static constexpr uint32_t WAVE_ROW = LV_WAVE_ROW, WAVE_SLOTS = LV_WAVE_SLOTS, BLOCK_ROW = LV_BLOCK_ROW, BLOCK_SLOTS = LV_BLOCK_SLOTS;
  static constexpr uint32_t GLOBAL_LOG2_MIN = 13;
  static constexpr uint32_t WGS_PER_CU[3] = {LV_WAVE_WGS_PER_CU, LV_BLOCK_WGS_PER_CU, LV_GLOBAL_WGS_PER_CU};
  static constexpr bool CNT = false;
};
constexpr uint32_t LV_MAX_ROUNDS = 64, LV_MAX_LEVELS = 32;

struct LevelView {
  const uint64_t* row_off;  // [n + 1]
  const uint64_t* key;      // row << 32 | column, ascending
  const uint64_t* w;
  const uint64_t* nu;       // node weights: the row sums (Louvain and Leiden's modularity) or the vertices a node stands for (CPM)
  const uint64_t* tot;      // the sum of nu by community
  const uint32_t* comm;
  // PROPOSE (Leiden's refinement) only: comm and tot are the refined communities'
  const uint32_t* coarse;   // the coarse community of a vertex: only neighbours inside it count
  const uint32_t* elig;     // the vertex passed the eligibility test
  const uint32_t* members;  // of a refined community
  const uint32_t* target;   // the refined community is an eligible target in this round
};

// the order of (score, community): larger score, then smaller community
__device__ __forceinline__ bool lv_better(i128 sc, uint32_t d, i128 best, uint32_t best_d) { return sc > best || (sc == best && d < best_d); }

// row_kernel's rule for a move or a refinement round; the table holds the weight into each neighbouring community.  The score
// of community d is e_d A - gB nu_x (tot_d - [d == c] nu_x) (include/rtclust.h: rtc_leiden's table of A and B; rtc_louvain is
// its modularity row).  A < 2^62 and gB < 2^52.
// PROPOSE false, a move round: out holds comm on entry; count counts the rows that change community.
// PROPOSE true, a refinement round: only an eligible vertex alone in its refined community decides, over the eligible targets
// that hold a neighbour of its coarse community, and a score of 0 or more is enough; out (all LV_NONE on entry) receives the
// proposal, count counts the proposals.
struct MoveArgs : LevelView { uint64_t A, gB; int odd; uint32_t* out; unsigned long long* count; };
// (score, community) under lv_better.  LV_NONE stands for staying, at S(c): a candidate needs a score strictly above it, so
// none ever ties with it.
struct __attribute__((packed, aligned(4))) LvBest { i128 s; uint32_t d; };
template <bool PROPOSE>
struct move_rule {
  typedef lv_shape shape;
  typedef RowTable<lv_shape::CNT, /* AGENT_READS */ false> Table;
  typedef MoveArgs Args;
  typedef LvBest Best;
  struct Lds { Best best[4]; };
  uint32_t cx, c;
  i128 gk, stay;

  __device__ __forceinline__ bool enter(const Args& G, uint32_t x) {
    cx = 0;
    if (PROPOSE) {
      if (!G.elig[x] || G.members[x] != 1) return false;
      cx = G.coarse[x];
    }
    return true;
  }
  __device__ __forceinline__ void gather(const Args& G, const Table& tab, uint32_t x, uint64_t e) {
    const uint32_t y = (uint32_t)G.key[e];
    if (y == x) return;  // the self entry is no neighbour
    if (PROPOSE && G.coarse[y] != cx) return;
    const uint32_t h = tab.claim(G.comm[y]);
    atomicAdd(&tab.sum[h], (unsigned long long)G.w[e]);
  }
  template <int BLOCK>
  __device__ __forceinline__ void gathered(Lds&) {}
  template <int BLOCK>
  __device__ __forceinline__ Best begin(const Args& G, const Table& tab, uint32_t x, const Lds&) {
    c = G.comm[x];
    const uint64_t kx = G.nu[x];
    uint64_t e_c = 0;
    if (!PROPOSE) {
      const uint32_t h = tab.find(c);
      if (h != RT_NONE) e_c = tab.read(&tab.sum[h]);
    }
    gk = (i128)G.gB * (i128)kx;
    // a lone vertex of the refinement stays at score 0 and takes a candidate at 0 or more: above -1
    stay = PROPOSE ? (i128)-1 : (i128)e_c * (i128)G.A - gk * (i128)(G.tot[c] - kx);
    return Best{stay, LV_NONE};
  }
  __device__ __forceinline__ void sweep(const Args& G, const Table& tab, uint32_t s, Best& best) {
    const uint32_t d = tab.read(&tab.keys[s]);
    if (d == LV_NONE || d == c || (G.odd ? d < c : d > c)) return;
    if (PROPOSE && !G.target[d]) return;
    const i128 sc = (i128)tab.read(&tab.sum[s]) * (i128)G.A - gk * (i128)G.tot[d];
    if (!(sc > stay)) return;
    if (lv_better(sc, d, best.s, best.d)) best = Best{sc, d};
  }
  static __device__ __forceinline__ void fold(Best& best, const Best& o) {
    if (lv_better(o.s, o.d, best.s, best.d)) best = o;
  }
  __device__ __forceinline__ void finish(const Args& G, const Table&, uint32_t x, uint64_t, const Best& best) {
    if (best.d == LV_NONE) return;
    G.out[x] = best.d;
    atomicAdd(G.count, 1ull);
  }
};

// ---- placement (rtc_leiden_place, rtc_leiden_assign.hip): a vertex that is not in the graph ----
// Query x's row holds its records (key: query << 32 | model genome, equal keys summed).  The table is the move rule's, keyed by
// the model genome's community; tot[d] is N_d (CPM) or tot_d (modularity).  The score is the one of a vertex alone in a
// community of its own in the model's graph with the query added (include/rtclust.h: rtc_leiden_place):
//   CPM         S(d) = e_d 65536 - g 2^20 N_d
//   modularity  S(d) = e_d (M2 + 2 k_x) 65536 - g k_x (tot_d + e_d),   M2 + 2 k_x < 2^46 (the host refuses more)
// Lane 0 writes the query's record; nothing else touches it.
struct PlaceArgs {
  const uint64_t *row_off, *key, *w, *tot;
  const int32_t* labels;
  int modularity;
  uint64_t g, m2;
  rtc_leiden_placement* out;
};
// The two best communities of a row under lv_better, with the weight into each, and how many communities the lane saw.
// d == LV_NONE at score 0: none -- a candidate needs a score above 0, so it beats every such entry and no such entry beats
// anything.
struct __attribute__((packed, aligned(4))) LvTop2 { i128 s[2]; uint64_t e[2]; uint32_t d[2]; uint32_t nc; };
__device__ __forceinline__ void lv_top2_insert(LvTop2& t, i128 sc, uint32_t d, uint64_t e) {
  if (lv_better(sc, d, t.s[0], t.d[0])) {
    t.s[1] = t.s[0]; t.d[1] = t.d[0]; t.e[1] = t.e[0];
    t.s[0] = sc; t.d[0] = d; t.e[0] = e;
  } else if (lv_better(sc, d, t.s[1], t.d[1])) {
    t.s[1] = sc; t.d[1] = d; t.e[1] = e;
  }
}
struct place_rule {
  typedef lv_shape shape;
  typedef RowTable<lv_shape::CNT, /* AGENT_READS */ false> Table;
  typedef PlaceArgs Args;
  typedef LvTop2 Best;
  struct Lds { Best best[4]; unsigned long long k[4]; };
  unsigned long long kx;
  i128 A, gB;

  static __device__ __forceinline__ void add(unsigned long long& k, unsigned long long o) { k += o; }
  __device__ __forceinline__ bool enter(const Args&, uint32_t) { kx = 0; return true; }
  __device__ __forceinline__ void gather(const Args& P, const Table& tab, uint32_t, uint64_t e) {
    const uint64_t we = P.w[e];
    const uint32_t h = tab.claim((uint32_t)P.labels[(uint32_t)P.key[e]]);
    atomicAdd(&tab.sum[h], (unsigned long long)we);
    kx += we;
  }
  template <int BLOCK>
  __device__ __forceinline__ void gathered(Lds& lds) { kx = row_reduce_wave<BLOCK>(kx, add, lds.k); }
  template <int BLOCK>
  __device__ __forceinline__ Best begin(const Args& P, const Table&, uint32_t, const Lds& lds) {
    kx = row_reduce_all<BLOCK>(kx, add, lds.k);
    A = P.modularity ? (i128)(P.m2 + 2 * kx) * 65536 : (i128)65536;
    gB = P.modularity ? (i128)P.g * (i128)kx : (i128)P.g * 1048576;
    return Best{{0, 0}, {0, 0}, {LV_NONE, LV_NONE}, 0};
  }
  __device__ __forceinline__ void sweep(const Args& P, const Table& tab, uint32_t s, Best& t) {
    const uint32_t d = tab.read(&tab.keys[s]);
    if (d == LV_NONE) return;
    t.nc++;
    const uint64_t ed = tab.read(&tab.sum[s]);
    const i128 sc = (i128)ed * A - gB * (i128)(P.tot[d] + (P.modularity ? ed : 0ull));
    if (sc > 0) lv_top2_insert(t, sc, d, ed);
  }
  static __device__ __forceinline__ void fold(Best& t, const Best& o) {
    lv_top2_insert(t, o.s[0], o.d[0], o.e[0]);
    lv_top2_insert(t, o.s[1], o.d[1], o.e[1]);
    t.nc += o.nc;
  }
  __device__ __forceinline__ void finish(const Args& P, const Table&, uint32_t x, uint64_t len, const Best& t) {
    rtc_leiden_placement r;
    r.label = t.d[0] == LV_NONE ? -1 : (int32_t)t.d[0];
    r.runner_up = t.d[1] == LV_NONE ? -1 : (int32_t)t.d[1];
    r.n_edges = (uint32_t)len;
    r.n_comms = t.nc;
    r.k_x = kx;
    r.e_label = t.e[0];
    r.e_runner = t.e[1];
    P.out[x] = r;
  }
};

// level 0: record e as two directed entries (u == v: twice the self entry, 2q in all)
__global__ __launch_bounds__(256) void louvain_entries_kernel(const rtc_wedge* __restrict__ edges, uint64_t m, uint64_t* __restrict__ key,
                                                              uint64_t* __restrict__ w) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_wedge r = edges[e];
    key[2 * e] = ((uint64_t)r.u << 32) | r.v;
    key[2 * e + 1] = ((uint64_t)r.v << 32) | r.u;
    w[2 * e] = w[2 * e + 1] = r.q;
  }
}
// the entries of the next level: both ends renamed
__global__ __launch_bounds__(256) void louvain_rekey_kernel(const uint64_t* __restrict__ key, uint64_t E, const uint32_t* __restrict__ newc,
                                                            uint64_t* __restrict__ out) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (uint64_t)gridDim.x * blockDim.x)
    out[e] = ((uint64_t)newc[key[e] >> 32] << 32) | newc[(uint32_t)key[e]];
}
// row_off[x], x = 0 .. n: the first entry whose key is not below x << 32
__global__ __launch_bounds__(256) void louvain_rows_kernel(const uint64_t* __restrict__ key, uint64_t E, uint32_t n, uint64_t* __restrict__ row_off) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x <= n; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t want = x << 32;
    uint64_t lo = 0, hi = E;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (key[mid] < want) lo = mid + 1; else hi = mid;
    }
    row_off[x] = lo;
  }
}
__global__ __launch_bounds__(256) void louvain_rowsum_kernel(const uint64_t* __restrict__ key, const uint64_t* __restrict__ w, uint64_t E,
                                                             unsigned long long* __restrict__ k) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (uint64_t)gridDim.x * blockDim.x)
    atomicAdd(&k[key[e] >> 32], (unsigned long long)w[e]);
}
__global__ __launch_bounds__(256) void louvain_iota_kernel(uint32_t n, uint32_t* __restrict__ out) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) out[x] = x;
}
// tot (zeroed) from the memberships
__global__ __launch_bounds__(256) void louvain_totals_kernel(const uint32_t* __restrict__ comm, const uint64_t* __restrict__ k, uint32_t n,
                                                             unsigned long long* __restrict__ tot) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x)
    atomicAdd(&tot[comm[x]], (unsigned long long)k[x]);
}
// smallest (all ones on entry) [c] = the smallest member of community c
__global__ __launch_bounds__(256) void louvain_smallest_kernel(const uint32_t* __restrict__ comm, uint32_t n, uint32_t* __restrict__ smallest) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) atomicMin(&smallest[comm[x]], x);
}
__global__ __launch_bounds__(256) void louvain_heads_kernel(const uint32_t* __restrict__ comm, const uint32_t* __restrict__ smallest, uint32_t n,
                                                            uint32_t* __restrict__ head) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) head[x] = smallest[comm[x]] == x ? 1u : 0u;
}
// newc[x] = how many communities have a smaller smallest member than x's (rank: the exclusive scan of head)
__global__ __launch_bounds__(256) void louvain_newc_kernel(const uint32_t* __restrict__ comm, const uint32_t* __restrict__ smallest,
                                                           const uint32_t* __restrict__ rank, uint32_t n, uint32_t* __restrict__ newc) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) newc[x] = rank[smallest[comm[x]]];
}
__global__ __launch_bounds__(256) void louvain_compose_kernel(const uint32_t* __restrict__ newc, uint32_t n0, uint32_t* __restrict__ label) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n0; x += gridDim.x * blockDim.x) label[x] = newc[label[x]];
}

struct Louvain {
  rtc_ctx* ctx;
  DevBuf db;
  uint64_t *key = nullptr, *key_in = nullptr, *key_sorted = nullptr, *w = nullptr, *w_sorted = nullptr;  // [E0]
  uint64_t *row_off = nullptr, *k = nullptr, *tot = nullptr;  // [n + 1], [n], [n]
  uint32_t *comm = nullptr, *comm_new = nullptr, *label = nullptr, *smallest = nullptr, *head = nullptr, *rank = nullptr, *newc = nullptr;
  unsigned long long* d_cnt = nullptr;  // [0] reduce_by_key's count, [1] moves
  char* tmp = nullptr;
  size_t tmp_bytes = 0;

  int alloc(uint32_t n, uint64_t E0) {
    for (uint64_t** p : {&key, &key_in, &key_sorted, &w, &w_sorted}) RTC_TRY(db.get(ctx, E0, p));
    RTC_TRY(db.get(ctx, (size_t)n + 1, &row_off));
    RTC_TRY(db.get(ctx, n, &k));
    RTC_TRY(db.get(ctx, n, &tot));
    for (uint32_t** p : {&comm, &comm_new, &label, &smallest, &head, &rank, &newc}) RTC_TRY(db.get(ctx, n, p));
    RTC_TRY(db.get(ctx, 2, &d_cnt));
    size_t a = 0, b = 0, c = 0;
    RTC_HIP(ctx, rocprim::radix_sort_pairs(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                           (size_t)E0, 0u, 64u, ctx->stream));
    RTC_HIP(ctx, rocprim::reduce_by_key(nullptr, b, (const uint64_t*)nullptr, (const uint64_t*)nullptr, (size_t)E0, (uint64_t*)nullptr,
                                        (uint64_t*)nullptr, (unsigned long long*)nullptr, rocprim::plus<uint64_t>(),
                                        rocprim::equal_to<uint64_t>(), ctx->stream));
    RTC_HIP(ctx, rocprim::exclusive_scan(nullptr, c, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(),
                                         ctx->stream));
    tmp_bytes = std::max(a, std::max(b, c)) + 256;
    return db.get(ctx, tmp_bytes, &tmp);
  }

  // The CSR of n vertices from E directed entries, keys in key_in and weights in w: sorted, equal keys summed, then the row
  // offsets and the row sums.  *E_out: the entries left.
  int build(uint32_t n, uint64_t E, uint64_t* E_out) {
    hipStream_t s = ctx->stream;
    size_t tb = tmp_bytes;
    RTC_HIP(ctx, rocprim::radix_sort_pairs(tmp, tb, (const uint64_t*)key_in, key_sorted, (const uint64_t*)w, w_sorted, (size_t)E, 0u, 64u, s));
    tb = tmp_bytes;
    RTC_HIP(ctx, rocprim::reduce_by_key(tmp, tb, (const uint64_t*)key_sorted, (const uint64_t*)w_sorted, (size_t)E, key, w, d_cnt,
                                        rocprim::plus<uint64_t>(), rocprim::equal_to<uint64_t>(), s));
    unsigned long long cnt = 0;
    RTC_HIP(ctx, hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    *E_out = cnt;
    hipLaunchKernelGGL(louvain_rows_kernel, dim3(blocks_for((uint64_t)n + 1, ctx->num_cu)), dim3(256), 0, s, (const uint64_t*)key, (uint64_t)cnt, n,
                       row_off);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemsetAsync(k, 0, (size_t)n * 8, s));
    hipLaunchKernelGGL(louvain_rowsum_kernel, dim3(blocks_for(cnt, ctx->num_cu)), dim3(256), 0, s, (const uint64_t*)key, (const uint64_t*)w,
                       (uint64_t)cnt, (unsigned long long*)k);
    RTC_CHECK_LAUNCH(ctx);
    return RTC_OK;
  }
};

}  // namespace

#endif  // RTC_COMMUNITY_H
