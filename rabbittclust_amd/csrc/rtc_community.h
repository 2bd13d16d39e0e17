// rtc_community.h -- what rtc_louvain (rtc_louvain.hip) and rtc_leiden (rtc_leiden.hip) share: a level's graph as a CSR built
// by one sort and one reduce_by_key, the row kernel that scores the communities next to a vertex, and the rows sorted by kernel
// path.  The comment at the head of rtc_louvain.hip describes the three paths.
#ifndef RTC_COMMUNITY_H
#define RTC_COMMUNITY_H
#include "rtc_dbscan_common.h"

namespace {

typedef __int128 i128;
constexpr uint32_t LV_WAVE_ROW = 128, LV_WAVE_SLOTS = 256, LV_BLOCK_ROW = 2048, LV_BLOCK_SLOTS = 4096;
constexpr uint32_t LV_NONE = 0xffffffffu;
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

// Row list[it] decides.  SLOTS > 0: the table lies in LDS; SLOTS == 0: in global memory, 1 << tab_log2[it] slots from
// tab_off[it] on.  The score of community d is e_d A - gB nu_x (tot_d - [d == c] nu_x) (include/rtclust.h: rtc_leiden's table
// of A and B; rtc_louvain is its modularity row).  A < 2^62 and gB < 2^52.
// PROPOSE false, a move round: comm_new holds comm on entry; moves counts the rows that change community.
// PROPOSE true, a refinement round: only an eligible vertex alone in its refined community decides, over the eligible targets
// that hold a neighbour of its coarse community, and a score of 0 or more is enough; comm_new (all LV_NONE on entry) receives
// the proposal, moves counts the proposals.
template <int BLOCK, uint32_t SLOTS, bool PROPOSE>
__global__ __launch_bounds__(BLOCK) void louvain_move_kernel(const uint32_t* __restrict__ list, uint32_t n_list, LevelView G, uint64_t A, uint64_t gB,
                                                             int odd, const uint64_t* __restrict__ tab_off, const uint32_t* __restrict__ tab_log2,
                                                             uint32_t* gkeys, unsigned long long* gvals, uint32_t* __restrict__ comm_new,
                                                             unsigned long long* __restrict__ moves) {
  __shared__ uint32_t s_keys[SLOTS ? SLOTS : 1];
  __shared__ unsigned long long s_vals[SLOTS ? SLOTS : 1];
  __shared__ unsigned long long s_hi[4], s_lo[4];
  __shared__ uint32_t s_d[4];
  const i128 m2s = (i128)A;
  for (uint32_t it = blockIdx.x; it < n_list; it += gridDim.x) {  // uniform over the workgroup: the barriers below are reached by all
    const uint32_t x = list[it];
    uint32_t cx = 0;
    if (PROPOSE) {
      if (!G.elig[x] || G.members[x] != 1) continue;  // uniform too: x is
      cx = G.coarse[x];
    }
    uint32_t* keys = s_keys;
    unsigned long long* vals = s_vals;
    uint32_t log2_slots = 31 - __builtin_clz(SLOTS ? SLOTS : 1u);
    if (!SLOTS) {
      keys = gkeys + tab_off[it];
      vals = gvals + tab_off[it];
      log2_slots = tab_log2[it];
    }
    const uint32_t slots = 1u << log2_slots, mask = slots - 1, shift = 32 - log2_slots;
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) { keys[s] = LV_NONE; vals[s] = 0ull; }
    __syncthreads();
    const uint64_t r0 = G.row_off[x], r1 = G.row_off[x + 1];
    for (uint64_t e = r0 + threadIdx.x; e < r1; e += BLOCK) {
      const uint32_t y = (uint32_t)G.key[e];
      if (y == x) continue;  // the self entry is no neighbour
      if (PROPOSE && G.coarse[y] != cx) continue;
      const uint32_t d = G.comm[y];
      uint32_t h = (d * 2654435761u) >> shift;
      for (;;) {
        const uint32_t old = atomicCAS(&keys[h], LV_NONE, d);
        if (old == LV_NONE || old == d) break;
        h = (h + 1) & mask;
      }
      atomicAdd(&vals[h], (unsigned long long)G.w[e]);
    }
    __syncthreads();
    const uint32_t c = G.comm[x];
    const uint64_t kx = G.nu[x];
    uint64_t e_c = 0;
    if (!PROPOSE)
      for (uint32_t h = (c * 2654435761u) >> shift;; h = (h + 1) & mask) {
        const uint32_t key = keys[h];
        if (key == c) e_c = vals[h];
        if (key == c || key == LV_NONE) break;
      }
    const i128 gk = (i128)gB * (i128)kx;
    // a lone vertex of the refinement stays at score 0 and takes a candidate at 0 or more: above -1
    const i128 stay = PROPOSE ? (i128)-1 : (i128)e_c * m2s - gk * (i128)(G.tot[c] - kx);
    // (score, community) in the order: larger score, then smaller community.  LV_NONE stands for staying, at S(c): a
    // candidate needs a score strictly above it, so none ever ties with it.
    i128 best = stay;
    uint32_t best_d = LV_NONE;
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) {
      const uint32_t d = keys[s];
      if (d == LV_NONE || d == c || (odd ? d < c : d > c)) continue;
      if (PROPOSE && !G.target[d]) continue;
      const i128 sc = (i128)vals[s] * m2s - gk * (i128)G.tot[d];
      if (!(sc > stay)) continue;
      if (sc > best || (sc == best && d < best_d)) { best = sc; best_d = d; }
    }
    for (int off = 32; off; off >>= 1) {
      const unsigned long long ohi = __shfl_xor((unsigned long long)((unsigned __int128)best >> 64), off);
      const unsigned long long olo = __shfl_xor((unsigned long long)best, off);
      const uint32_t od = __shfl_xor(best_d, off);
      const i128 o = (i128)(((unsigned __int128)ohi << 64) | olo);
      if (o > best || (o == best && od < best_d)) { best = o; best_d = od; }
    }
    if (BLOCK > 64) {
      const uint32_t wave = threadIdx.x / 64;
      if ((threadIdx.x & 63) == 0) {
        s_hi[wave] = (unsigned long long)((unsigned __int128)best >> 64);
        s_lo[wave] = (unsigned long long)best;
        s_d[wave] = best_d;
      }
      __syncthreads();
      if (threadIdx.x == 0)
        for (uint32_t wv = 1; wv < BLOCK / 64; wv++) {
          const i128 o = (i128)(((unsigned __int128)s_hi[wv] << 64) | s_lo[wv]);
          if (o > best || (o == best && s_d[wv] < best_d)) { best = o; best_d = s_d[wv]; }
        }
    }
    if (threadIdx.x == 0 && best_d != LV_NONE) {
      comm_new[x] = best_d;
      atomicAdd(moves, 1ull);
    }
    __syncthreads();  // the table and the wave slots are written again in the next turn
  }
}

// ---- placement (rtc_leiden_place, rtc_leiden_assign.hip): the move kernel's sibling for a vertex that is not in the graph ----
// The move kernel's table and order, as functions: open addressing over 1 << (32 - shift) slots with its hash, keys all LV_NONE
// on entry.  Returns community d's slot, claimed if it had none; the caller adds the weight to vals[slot].  (louvain_move_kernel
// keeps its own lines: written through these functions its instruction stream comes out differently.)
__device__ __forceinline__ uint32_t lv_table_slot(uint32_t* keys, uint32_t d, uint32_t shift, uint32_t mask) {
  uint32_t h = (d * 2654435761u) >> shift;
  for (;;) {
    const uint32_t old = atomicCAS(&keys[h], LV_NONE, d);
    if (old == LV_NONE || old == d) break;
    h = (h + 1) & mask;
  }
  return h;
}
// the move kernel's order of (score, community): larger score, then smaller community
__device__ __forceinline__ bool lv_better(i128 sc, uint32_t d, i128 best, uint32_t best_d) { return sc > best || (sc == best && d < best_d); }
// The two best communities of a row under lv_better, with the weight into each.  d == LV_NONE at score 0: none -- a candidate
// needs a score above 0, so it beats every such entry and no such entry beats anything.
struct LvTop2 { i128 s[2]; uint64_t e[2]; uint32_t d[2]; };
__device__ __forceinline__ void lv_top2_insert(LvTop2& t, i128 sc, uint32_t d, uint64_t e) {
  if (lv_better(sc, d, t.s[0], t.d[0])) {
    t.s[1] = t.s[0]; t.d[1] = t.d[0]; t.e[1] = t.e[0];
    t.s[0] = sc; t.d[0] = d; t.e[0] = e;
  } else if (lv_better(sc, d, t.s[1], t.d[1])) {
    t.s[1] = sc; t.d[1] = d; t.e[1] = e;
  }
}
__device__ __forceinline__ i128 lv_shfl_xor(i128 v, int off) {
  const unsigned long long hi = __shfl_xor((unsigned long long)((unsigned __int128)v >> 64), off);
  const unsigned long long lo = __shfl_xor((unsigned long long)v, off);
  return (i128)(((unsigned __int128)hi << 64) | lo);
}

// Query list[it]'s row holds its records (key: query << 32 | model genome, equal keys summed).  The table is the move kernel's,
// keyed by the model genome's community; tot[d] is N_d (CPM) or tot_d (modularity).  The score is the one of a vertex alone in
// a community of its own in the model's graph with the query added (include/rtclust.h: rtc_leiden_place):
//   CPM         S(d) = e_d 65536 - g 2^20 N_d
//   modularity  S(d) = e_d (M2 + 2 k_x) 65536 - g k_x (tot_d + e_d),   M2 + 2 k_x < 2^46 (the host refuses more)
// Lane 0 writes the query's record; nothing else touches it.
template <int BLOCK, uint32_t SLOTS>
__global__ __launch_bounds__(BLOCK) void leiden_place_kernel(const uint32_t* __restrict__ list, uint32_t n_list, const uint64_t* __restrict__ row_off,
                                                             const uint64_t* __restrict__ key, const uint64_t* __restrict__ w,
                                                             const int32_t* __restrict__ labels, const uint64_t* __restrict__ tot, int modularity,
                                                             uint64_t g, uint64_t m2, const uint64_t* __restrict__ tab_off,
                                                             const uint32_t* __restrict__ tab_log2, uint32_t* gkeys, unsigned long long* gvals,
                                                             rtc_leiden_placement* __restrict__ out) {
  __shared__ uint32_t s_keys[SLOTS ? SLOTS : 1];
  __shared__ unsigned long long s_vals[SLOTS ? SLOTS : 1];
  __shared__ unsigned long long s_k[4];
  __shared__ uint32_t s_n[4];
  __shared__ LvTop2 s_top[4];
  for (uint32_t it = blockIdx.x; it < n_list; it += gridDim.x) {  // uniform over the workgroup
    const uint32_t x = list[it];
    uint32_t* keys = s_keys;
    unsigned long long* vals = s_vals;
    uint32_t log2_slots = 31 - __builtin_clz(SLOTS ? SLOTS : 1u);
    if (!SLOTS) {
      keys = gkeys + tab_off[it];
      vals = gvals + tab_off[it];
      log2_slots = tab_log2[it];
    }
    const uint32_t slots = 1u << log2_slots, mask = slots - 1, shift = 32 - log2_slots;
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) { keys[s] = LV_NONE; vals[s] = 0ull; }
    __syncthreads();
    const uint64_t r0 = row_off[x], r1 = row_off[x + 1];
    unsigned long long kx = 0;
    for (uint64_t e = r0 + threadIdx.x; e < r1; e += BLOCK) {
      const uint64_t we = w[e];
      const uint32_t h = lv_table_slot(keys, (uint32_t)labels[(uint32_t)key[e]], shift, mask);
      atomicAdd(&vals[h], (unsigned long long)we);
      kx += we;
    }
    for (int off = 32; off; off >>= 1) kx += __shfl_xor(kx, off);
    if (BLOCK > 64) {
      if ((threadIdx.x & 63) == 0) s_k[threadIdx.x / 64] = kx;
    }
    __syncthreads();  // the table is complete, and so are the waves' sums
    if (BLOCK > 64) {
      kx = 0;
      for (uint32_t wv = 0; wv < BLOCK / 64; wv++) kx += s_k[wv];
    }
    const i128 A = modularity ? (i128)(m2 + 2 * kx) * 65536 : (i128)65536;
    const i128 gB = modularity ? (i128)g * (i128)kx : (i128)g * 1048576;
    LvTop2 t;
    t.s[0] = t.s[1] = 0; t.d[0] = t.d[1] = LV_NONE; t.e[0] = t.e[1] = 0;
    uint32_t nc = 0;
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) {
      const uint32_t d = keys[s];
      if (d == LV_NONE) continue;
      nc++;
      const uint64_t ed = vals[s];
      const i128 sc = (i128)ed * A - gB * (i128)(tot[d] + (modularity ? ed : 0ull));
      if (sc > 0) lv_top2_insert(t, sc, d, ed);
    }
    for (int off = 32; off; off >>= 1) {
      nc += __shfl_xor(nc, off);
      LvTop2 o;
      for (int j = 0; j < 2; j++) {
        o.s[j] = lv_shfl_xor(t.s[j], off);
        o.d[j] = __shfl_xor(t.d[j], off);
        o.e[j] = __shfl_xor((unsigned long long)t.e[j], off);
      }
      lv_top2_insert(t, o.s[0], o.d[0], o.e[0]);
      lv_top2_insert(t, o.s[1], o.d[1], o.e[1]);
    }
    if (BLOCK > 64) {
      if ((threadIdx.x & 63) == 0) { s_top[threadIdx.x / 64] = t; s_n[threadIdx.x / 64] = nc; }
      __syncthreads();
      if (threadIdx.x == 0)
        for (uint32_t wv = 1; wv < BLOCK / 64; wv++) {
          const LvTop2 o = s_top[wv];
          lv_top2_insert(t, o.s[0], o.d[0], o.e[0]);
          lv_top2_insert(t, o.s[1], o.d[1], o.e[1]);
          nc += s_n[wv];
        }
    }
    if (threadIdx.x == 0) {
      rtc_leiden_placement r;
      r.label = t.d[0] == LV_NONE ? -1 : (int32_t)t.d[0];
      r.runner_up = t.d[1] == LV_NONE ? -1 : (int32_t)t.d[1];
      r.n_edges = (uint32_t)(r1 - r0);
      r.n_comms = nc;
      r.k_x = kx;
      r.e_label = t.e[0];
      r.e_runner = t.e[1];
      out[x] = r;
    }
    __syncthreads();  // the table and the wave slots are written again in the next turn
  }
}

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


// The rows of a level by kernel path (which one a row takes depends on its length alone) and the tables of the long ones.
struct RowPaths {
  std::vector<uint64_t> h_row, h_off;
  std::vector<uint32_t> lists[3], h_log2;
  uint32_t* d_list[3] = {nullptr, nullptr, nullptr};
  uint32_t *d_log2 = nullptr, *d_gkeys = nullptr;
  uint64_t* d_off = nullptr;
  unsigned long long* d_gvals = nullptr;

  // synchronises the stream: the host lists are rewritten at the next level
  int prepare(Louvain& L, uint32_t nl, const char* who) {
    rtc_ctx* ctx = L.ctx;
    hipStream_t s = ctx->stream;
    h_row.resize((size_t)nl + 1);
    RTC_HIP(ctx, hipMemcpyAsync(h_row.data(), L.row_off, ((size_t)nl + 1) * 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    for (auto& l : lists) l.clear();
    h_log2.clear();
    h_off.clear();
    uint64_t table_slots = 0;
    for (uint32_t x = 0; x < nl; x++) {
      const uint64_t len = h_row[x + 1] - h_row[x];
      if (len == 0) continue;  // no neighbour: it stays
      if (len <= LV_WAVE_ROW) lists[0].push_back(x);
      else if (len <= LV_BLOCK_ROW) lists[1].push_back(x);
      else {
        uint32_t lg = 13;  // above 2 * LV_BLOCK_ROW
        while ((1ull << lg) < 2 * len) lg++;
        if (lg > 31) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: a row of %llu entries", who, (unsigned long long)len);
        lists[2].push_back(x);
        h_log2.push_back(lg);
        h_off.push_back(table_slots);
        table_slots += 1ull << lg;
      }
    }
    for (int p = 0; p < 3; p++)
      if (!lists[p].empty()) {
        RTC_TRY(L.db.get(ctx, lists[p].size(), &d_list[p]));
        RTC_HIP(ctx, hipMemcpyAsync(d_list[p], lists[p].data(), lists[p].size() * 4, hipMemcpyHostToDevice, s));
      }
    if (!lists[2].empty()) {
      RTC_TRY(L.db.get(ctx, h_log2.size(), &d_log2));
      RTC_TRY(L.db.get(ctx, h_off.size(), &d_off));
      RTC_TRY(L.db.get(ctx, table_slots, &d_gkeys));
      RTC_TRY(L.db.get(ctx, table_slots, &d_gvals));
      RTC_HIP(ctx, hipMemcpyAsync(d_log2, h_log2.data(), h_log2.size() * 4, hipMemcpyHostToDevice, s));
      RTC_HIP(ctx, hipMemcpyAsync(d_off, h_off.data(), h_off.size() * 8, hipMemcpyHostToDevice, s));
    }
    RTC_HIP(ctx, hipStreamSynchronize(s));
    return RTC_OK;
  }

  // one round over every row: the three launches
  template <bool PROPOSE>
  int launch(rtc_ctx* ctx, const LevelView& G, uint64_t A, uint64_t gB, int odd, uint32_t* out, unsigned long long* count) {
    hipStream_t s = ctx->stream;
    if (!lists[0].empty()) {
      const uint32_t nb = (uint32_t)std::min<uint64_t>(lists[0].size(), (uint64_t)ctx->num_cu * 32);
      hipLaunchKernelGGL((louvain_move_kernel<64, LV_WAVE_SLOTS, PROPOSE>), dim3(nb), dim3(64), 0, s, (const uint32_t*)d_list[0],
                         (uint32_t)lists[0].size(), G, A, gB, odd, (const uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                         (unsigned long long*)nullptr, out, count);
      RTC_CHECK_LAUNCH(ctx);
    }
    if (!lists[1].empty()) {
      const uint32_t nb = (uint32_t)std::min<uint64_t>(lists[1].size(), (uint64_t)ctx->num_cu * 3);
      hipLaunchKernelGGL((louvain_move_kernel<256, LV_BLOCK_SLOTS, PROPOSE>), dim3(nb), dim3(256), 0, s, (const uint32_t*)d_list[1],
                         (uint32_t)lists[1].size(), G, A, gB, odd, (const uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                         (unsigned long long*)nullptr, out, count);
      RTC_CHECK_LAUNCH(ctx);
    }
    if (!lists[2].empty()) {
      const uint32_t nb = (uint32_t)std::min<uint64_t>(lists[2].size(), (uint64_t)ctx->num_cu * 8);
      hipLaunchKernelGGL((louvain_move_kernel<256, 0, PROPOSE>), dim3(nb), dim3(256), 0, s, (const uint32_t*)d_list[2], (uint32_t)lists[2].size(),
                         G, A, gB, odd, (const uint64_t*)d_off, (const uint32_t*)d_log2, d_gkeys, d_gvals, out, count);
      RTC_CHECK_LAUNCH(ctx);
    }
    return RTC_OK;
  }

  void release(Louvain& L) {
    for (void** q : {(void**)&d_list[0], (void**)&d_list[1], (void**)&d_list[2], (void**)&d_log2, (void**)&d_off, (void**)&d_gkeys, (void**)&d_gvals})
      if (*q) { L.db.release(*q); *q = nullptr; }
  }
};

}  // namespace

#endif  // RTC_COMMUNITY_H
