// rtc_mcl.hip -- rtc_mcl: the Markov clustering of clust-leiden --mcl in exact integers (include/rtclust.h holds the definition,
// tests/refmcl.py restates it).
//   * The matrix lies in slotted columns: select bounds a column at S entries, so column j is stride = min(S, n) slots of
//     (row u32, value u32) from j * stride on, and a length.  Two of them, the old and the new one: 16 n stride bytes.  The order
//     of the entries inside a column means nothing: every sum below is an integer sum and every selection is by a unique key.
//   * The start matrix comes from the CSR that rtc_louvain builds of its records (rtc_community.h: one sort, one reduce_by_key);
//     mcl_start_kernel adds the loop and selects.
//   * mcl_column_kernel is the hot path: one column per workgroup.  It gathers the columns k that column j names and adds
//     M[i,k] M[k,j] into a hash table over the rows i (64-bit integer atomics), then rescales, inflates and selects slot by slot
//     in that table, writes the new column and compares it with the old one through the same table.  Three launches share the
//     code, by the column's work W (rtc_mcl.h):
//       - W <= MCL_WAVE_WORK: a workgroup of ONE wave, MCL_WAVE_SLOTS slots in LDS;
//       - W <= MCL_BLOCK_WORK: 256 lanes, MCL_BLOCK_SLOTS slots in LDS;
//       - beyond: 256 lanes, a table in global memory that the workgroup keeps for all its columns.
//     A table has more slots than its column has products, so a probe ends at a free slot.
//   * select: when more than S rows survive, the S-th largest key (y << 32 | ~row) is found bit by bit from the top, one count
//     over the table per bit; the keys are distinct, so the kept set is the definition's.
//   * mcl_work_kernel computes W of every column before an iteration and appends the column to the list of its path; the
//     column launches read the lists' lengths on the device, so an iteration costs the host one read-back: the word that says a
//     column changed, with the path and cut counts beside it.
#include "rtc_community.h"
#include "rtc_mcl.h"

namespace {

constexpr uint64_t MCL_ONE = 1ull << 30;
// the state words of a call on the device
enum { MCL_CHANGED = 0, MCL_LIST0 = 1, MCL_CUT = 4, MCL_TOO_LARGE = 5, MCL_STATE_WORDS = 8 };

struct MclMat {
  uint32_t* row;  // [n * stride]
  uint32_t* val;  // [n * stride]
  uint32_t* len;  // [n]
};

// The table of a column.  In LDS it is read and written plainly.  In global memory a workgroup uses its table for one column
// after another, so a line that a plain load left in the vector cache could be read again after the atomics of the next column
// have changed it in L2: every access there is an atomic one at device scope, which goes to L2.
template <bool GLOBAL>
struct MclTable {
  uint32_t* keys;
  unsigned long long* vals;
  uint32_t mask, shift;
  __device__ __forceinline__ uint32_t key(uint32_t s) const {
    return GLOBAL ? __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : keys[s];
  }
  __device__ __forceinline__ unsigned long long val(uint32_t s) const {
    return GLOBAL ? __hip_atomic_load(&vals[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : vals[s];
  }
  __device__ __forceinline__ void set_key(uint32_t s, uint32_t k) const {
    if (GLOBAL) __hip_atomic_store(&keys[s], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else keys[s] = k;
  }
  __device__ __forceinline__ void set_val(uint32_t s, unsigned long long v) const {
    if (GLOBAL) __hip_atomic_store(&vals[s], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else vals[s] = v;
  }
  // row i's slot, claimed if it had none
  __device__ __forceinline__ uint32_t claim(uint32_t i) const {
    uint32_t h = (i * MCL_GOLDEN) >> shift;
    for (;;) {
      const uint32_t old = atomicCAS(&keys[h], LV_NONE, i);
      if (old == LV_NONE || old == i) break;
      h = (h + 1) & mask;
    }
    return h;
  }
  // row i's slot, or LV_NONE if it has none
  __device__ __forceinline__ uint32_t find(uint32_t i) const {
    for (uint32_t h = (i * MCL_GOLDEN) >> shift;; h = (h + 1) & mask) {
      const uint32_t k = key(h);
      if (k == i) return h;
      if (k == LV_NONE) return LV_NONE;
    }
  }
};

template <bool GLOBAL>
__device__ __forceinline__ void mcl_sync() {
  if (GLOBAL) __threadfence();
  __syncthreads();
}

// the sum / the maximum over the workgroup, in every lane; red: four words of LDS
template <int BLOCK>
__device__ __forceinline__ unsigned long long mcl_sum(unsigned long long v, unsigned long long* red) {
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  if (BLOCK > 64) {
    __syncthreads();  // the last reduction's readers are through
    if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = v;
    __syncthreads();
    v = 0;
    for (int w = 0; w < BLOCK / 64; w++) v += red[w];
  }
  return v;
}
template <int BLOCK>
__device__ __forceinline__ unsigned long long mcl_max(unsigned long long v, unsigned long long* red) {
  for (int off = 32; off; off >>= 1) { const unsigned long long o = __shfl_xor(v, off); v = o > v ? o : v; }
  if (BLOCK > 64) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = v;
    __syncthreads();
    v = 0;
    for (int w = 0; w < BLOCK / 64; w++) v = red[w] > v ? red[w] : v;
  }
  return v;
}

// floor(sqrt(x)), x <= 2^60: the double root, corrected in integers
__device__ __forceinline__ uint64_t mcl_isqrt(uint64_t x) {
  uint64_t r = (uint64_t)sqrt((double)x);
  while (r * r > x) r--;
  while ((r + 1) * (r + 1) <= x) r++;
  return r;
}
// the definition's step 3 on a rescaled entry e1 <= ONE: e1 to the power h / 2 in units of ONE
__device__ __forceinline__ uint64_t mcl_inflate(uint64_t e1, int h) {
  uint64_t y = e1;
  for (int c = 1; c < h / 2; c++) y = (y * e1) >> 30;
  if (h & 1) y = (y * mcl_isqrt(e1 << 30)) >> 30;
  return y;
}

// the key of select: larger value first, then the lower row
__device__ __forceinline__ uint64_t mcl_key(uint64_t x, uint32_t i) { return (x << 32) | (uint32_t)~i; }

// ---- the start matrix: column j of the CSR plus the loop (j, largest entry or 1), selected ----
__global__ __launch_bounds__(256) void mcl_start_kernel(const uint64_t* __restrict__ row_off, const uint64_t* __restrict__ key,
                                                        const uint64_t* __restrict__ w, uint32_t n, uint32_t stride, uint32_t S, MclMat N,
                                                        uint32_t* __restrict__ state) {
  __shared__ unsigned long long red[4];
  __shared__ uint32_t s_cnt;
  for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {  // uniform over the workgroup
    const uint64_t r0 = row_off[j], r1 = row_off[j + 1];
    unsigned long long big = 0, sum = 0;
    for (uint64_t e = r0 + threadIdx.x; e < r1; e += 256) { const uint64_t x = w[e]; big = x > big ? x : big; sum += x; }
    big = mcl_max<256>(big, red);
    if (big >> 32) {  // an entry of 2^32 or more: the host refuses the call
      if (threadIdx.x == 0) atomicOr(&state[MCL_TOO_LARGE], 1u);
      continue;
    }
    const uint64_t loop = big ? big : 1;
    const uint64_t cnt = r1 - r0 + 1;
    uint64_t T = 0;  // keys below T drop out
    if (cnt > S) {
      for (int bit = 63; bit >= 0; bit--) {
        const uint64_t cand = T | (1ull << bit);
        unsigned long long c = 0;
        for (uint64_t e = r0 + threadIdx.x; e < r1; e += 256) c += mcl_key(w[e], (uint32_t)key[e]) >= cand;
        if (threadIdx.x == 0) c += mcl_key(loop, j) >= cand;
        c = mcl_sum<256>(c, red);
        if (c >= S) T = cand;
        if (c == S) break;
      }
      sum = 0;
      for (uint64_t e = r0 + threadIdx.x; e < r1; e += 256) sum += mcl_key(w[e], (uint32_t)key[e]) >= T ? w[e] : 0;
      if (threadIdx.x == 0) atomicAdd(&state[MCL_CUT], 1u);
    }
    const bool loop_kept = mcl_key(loop, j) >= T;
    const uint64_t X = mcl_sum<256>(sum, red) + (loop_kept ? loop : 0);
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)j * stride;
    for (uint64_t e = r0 + threadIdx.x; e <= r1; e += 256) {  // e == r1: the loop
      const uint32_t i = e < r1 ? (uint32_t)key[e] : j;
      const uint64_t x = e < r1 ? w[e] : loop;
      if (mcl_key(x, i) < T) continue;
      const uint64_t p = x * MCL_ONE / X;
      if (!p) continue;
      const uint32_t at = atomicAdd(&s_cnt, 1u);
      if (at < stride) { N.row[base + at] = i; N.val[base + at] = (uint32_t)p; }
    }
    __syncthreads();
    if (threadIdx.x == 0) N.len[j] = s_cnt < stride ? s_cnt : stride;
    __syncthreads();
  }
}

// ---- W of every column (a wave each), the column appended to the list of its path ----
__global__ __launch_bounds__(256) void mcl_work_kernel(MclMat M, uint32_t n, uint32_t stride, int all_global, uint32_t* __restrict__ work,
                                                       uint32_t* __restrict__ list0, uint32_t* __restrict__ list1, uint32_t* __restrict__ list2,
                                                       uint32_t* __restrict__ state) {
  const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * 4;
  for (uint32_t j = blockIdx.x * 4 + threadIdx.x / 64; j < n; j += waves) {
    const uint32_t len = M.len[j];
    const uint64_t base = (uint64_t)j * stride;
    uint32_t wsum = 0;
    for (uint32_t t = lane; t < len; t += 64) wsum += M.len[M.row[base + t]];
    for (int off = 32; off; off >>= 1) wsum += __shfl_xor(wsum, off);
    if (lane == 0) {
      work[j] = wsum;
      const int p = all_global ? 2 : wsum <= MCL_WAVE_WORK ? 0 : wsum <= MCL_BLOCK_WORK ? 1 : 2;
      const uint32_t at = atomicAdd(&state[MCL_LIST0 + p], 1u);
      (p == 0 ? list0 : p == 1 ? list1 : list2)[at] = j;
    }
  }
}

// ---- one iteration of the columns list[0 .. *n_list): expand, rescale, inflate, select, write, compare ----
// SLOTS > 0: the table lies in LDS.  SLOTS == 0: in global memory, workgroup b's from b << gtab_log2 on, of which a column uses
// the first power of two that is at least 2 min(W, n), MCL_GLOBAL_LOG2_MIN at the least.
template <int BLOCK, uint32_t SLOTS>
__global__ __launch_bounds__(BLOCK) void mcl_column_kernel(const uint32_t* __restrict__ list, const uint32_t* __restrict__ n_list, MclMat M, MclMat N,
                                                           uint32_t n, uint32_t stride, uint32_t S, int h, const uint32_t* __restrict__ work,
                                                           uint32_t* gkeys, unsigned long long* gvals, uint32_t gtab_log2,
                                                           uint32_t* __restrict__ state) {
  constexpr bool GLOBAL = SLOTS == 0;
  __shared__ uint32_t s_keys[SLOTS ? SLOTS : 1];
  __shared__ unsigned long long s_vals[SLOTS ? SLOTS : 1];
  __shared__ unsigned long long red[4];
  __shared__ uint32_t s_cnt, s_diff;
  const uint32_t count = *n_list;
  for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {  // uniform over the workgroup: the barriers below are reached by all
    const uint32_t j = list[it];
    MclTable<GLOBAL> tab;
    uint32_t log2_slots = 31 - __builtin_clz(SLOTS ? SLOTS : 1u);
    tab.keys = s_keys;
    tab.vals = s_vals;
    if (GLOBAL) {
      tab.keys = gkeys + ((uint64_t)blockIdx.x << gtab_log2);
      tab.vals = gvals + ((uint64_t)blockIdx.x << gtab_log2);
      const uint32_t rows = work[j] < n ? work[j] : n;
      log2_slots = MCL_GLOBAL_LOG2_MIN;
      while (log2_slots < gtab_log2 && (1u << log2_slots) < 2 * rows) log2_slots++;
    }
    const uint32_t slots = 1u << log2_slots;
    tab.mask = slots - 1;
    tab.shift = 32 - log2_slots;
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) { tab.set_key(s, LV_NONE); tab.set_val(s, 0ull); }
    if (threadIdx.x == 0) { s_cnt = 0; s_diff = 0; }
    mcl_sync<GLOBAL>();

    // 1. expand: sixteen lanes per named column k
    const uint32_t len_j = M.len[j];
    const uint64_t base_j = (uint64_t)j * stride;
    for (uint32_t t = threadIdx.x / 16; t < len_j; t += BLOCK / 16) {
      const uint32_t k = M.row[base_j + t];
      const uint64_t p_kj = M.val[base_j + t];
      const uint32_t len_k = M.len[k];
      const uint64_t base_k = (uint64_t)k * stride;
      for (uint32_t e = threadIdx.x & 15; e < len_k; e += 16) {
        const uint32_t slot = tab.claim(M.row[base_k + e]);
        atomicAdd(&tab.vals[slot], (unsigned long long)((uint64_t)M.val[base_k + e] * p_kj));
      }
    }
    mcl_sync<GLOBAL>();

    // 2. rescale by the column's largest entry, 3. inflate: a slot's sum becomes its y (a lane keeps to its own slots from here on)
    unsigned long long big = 0;
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) {
      const unsigned long long e = tab.val(s) >> 30;
      big = e > big ? e : big;
    }
    const uint64_t E = mcl_max<BLOCK>(big, red);
    unsigned long long alive = 0, sum = 0;
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) {
      const uint64_t e = tab.val(s) >> 30;
      const uint64_t y = e ? mcl_inflate(e * MCL_ONE / E, h) : 0;
      tab.set_val(s, y);
      alive += y != 0;
      sum += y;
    }
    alive = mcl_sum<BLOCK>(alive, red);

    // 4. select: past S survivors, the S-th largest key bit by bit; y is at most ONE, so bit 62 is the first that can be set
    if (alive > S) {
      uint64_t T = 0;
      for (int bit = 62; bit >= 0; bit--) {
        const uint64_t cand = T | (1ull << bit);
        unsigned long long c = 0;
        for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) {
          const uint64_t y = tab.val(s);
          c += y && mcl_key(y, tab.key(s)) >= cand;
        }
        c = mcl_sum<BLOCK>(c, red);
        if (c >= S) T = cand;
        if (c == S) break;
      }
      sum = 0;
      for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) {
        const uint64_t y = tab.val(s);
        if (!y) continue;
        if (mcl_key(y, tab.key(s)) >= T) sum += y; else tab.set_val(s, 0ull);
      }
      if (threadIdx.x == 0) atomicAdd(&state[MCL_CUT], 1u);
    }
    const uint64_t X = mcl_sum<BLOCK>(sum, red);
    const uint64_t base_n = base_j;
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) {
      const uint64_t y = tab.val(s);
      if (!y) continue;
      const uint64_t p = y * MCL_ONE / X;
      tab.set_val(s, p);
      if (!p) continue;
      const uint32_t at = atomicAdd(&s_cnt, 1u);
      if (at < stride) { N.row[base_n + at] = tab.key(s); N.val[base_n + at] = (uint32_t)p; }
    }
    mcl_sync<GLOBAL>();

    // the new column against the old one: as many entries, and every old entry found with its value
    const uint32_t len_n = s_cnt < stride ? s_cnt : stride;
    uint32_t diff = len_n != len_j;
    for (uint32_t t = threadIdx.x; t < len_j && !diff; t += BLOCK) {
      const uint32_t slot = tab.find(M.row[base_j + t]);
      diff = slot == LV_NONE || tab.val(slot) != M.val[base_j + t];
    }
    if (diff) s_diff = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
      N.len[j] = len_n;
      if (s_diff) atomicOr(&state[MCL_CHANGED], 1u);
    }
    mcl_sync<GLOBAL>();  // the table and the counters are written again in the next turn
  }
}

// the final matrix as records, column j's from off[j] on (in the order of the column's slots)
__global__ __launch_bounds__(256) void mcl_entries_kernel(MclMat M, uint32_t n, uint32_t stride, const uint64_t* __restrict__ off,
                                                          rtc_mcl_entry* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * 4;
  for (uint32_t j = blockIdx.x * 4 + threadIdx.x / 64; j < n; j += waves) {
    const uint32_t len = M.len[j];
    const uint64_t base = (uint64_t)j * stride;
    for (uint32_t t = lane; t < len; t += 64) out[off[j] + t] = rtc_mcl_entry{j, M.row[base + t], M.val[base + t], 0u};
  }
}

struct MclEvents {
  hipEvent_t a = nullptr, b = nullptr;
  ~MclEvents() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// the clusters of a matrix in (col, row) order (include/rtclust.h: Clusters): every vertex labelled by its cluster's smallest member
void mcl_clusters(const std::vector<rtc_mcl_entry>& mat, const std::vector<uint64_t>& off, uint32_t n, int32_t* labels, uint32_t* n_clusters,
                  uint64_t* attractors) {
  std::vector<uint32_t> parent(n);
  std::vector<char> attractor(n, 0);
  for (uint32_t x = 0; x < n; x++) parent[x] = x;
  auto find = [&](uint32_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
  };
  auto unite = [&](uint32_t a, uint32_t b) {
    a = find(a); b = find(b);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
  };
  uint64_t na = 0;
  for (uint32_t j = 0; j < n; j++)
    for (uint64_t e = off[j]; e < off[j + 1]; e++)
      if (mat[e].row == j && mat[e].value > 0) { attractor[j] = 1; na++; }
  for (uint32_t j = 0; j < n; j++) {
    if (attractor[j]) {
      for (uint64_t e = off[j]; e < off[j + 1]; e++)
        if (attractor[mat[e].row]) unite(j, mat[e].row);
      continue;
    }
    // the rows come in ascending order: a later one wins only by a larger value
    int64_t best = -1, best_any = -1;
    for (uint64_t e = off[j]; e < off[j + 1]; e++) {
      if (best_any < 0 || mat[e].value > mat[best_any].value) best_any = (int64_t)e;
      if (attractor[mat[e].row] && (best < 0 || mat[e].value > mat[best].value)) best = (int64_t)e;
    }
    if (best < 0) best = best_any;
    if (best >= 0) unite(j, mat[best].row);
  }
  uint32_t ncl = 0;
  for (uint32_t x = 0; x < n; x++) {
    const uint32_t r = find(x);  // the smallest member: unite keeps the smaller root
    labels[x] = (int32_t)r;
    ncl += r == x;
  }
  *n_clusters = ncl;
  *attractors = na;
}

}  // namespace

extern "C" int rtc_mcl(rtc_ctx* ctx, uint32_t n, const rtc_wedge* h_edges, uint64_t m, int inflation_x2, uint32_t select, uint32_t max_iter,
                       int32_t* h_labels, uint32_t* h_n_clusters, uint32_t* h_iterations, int* h_converged, rtc_mcl_entry* h_matrix, uint64_t cap,
                       uint64_t* h_nnz) {
  const char* who = "rtc_mcl";
  if (!ctx || !h_n_clusters || (n && !h_labels) || (m && !h_edges) || (h_matrix && !h_nnz)) return RTC_ERR_ARG;
  if (inflation_x2 < 3 || inflation_x2 > 16) return rtc_fail(ctx, RTC_ERR_ARG, "%s: inflation_x2 %d, not in 3 .. 16", who, inflation_x2);
  if (select < 1 || select > 4096) return rtc_fail(ctx, RTC_ERR_ARG, "%s: select %u, not in 1 .. 4096", who, select);
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u vertices", who, n);
  std::vector<rtc_wedge> rec;  // the records without those of a vertex with itself
  rec.reserve(m);
  for (uint64_t e = 0; e < m; e++) {
    if (h_edges[e].u >= n || h_edges[e].v >= n || h_edges[e].q == 0)
      return rtc_fail(ctx, RTC_ERR_ARG, "%s: record %llu is (%u, %u, %u) with %u vertices", who, (unsigned long long)e, h_edges[e].u, h_edges[e].v,
                      h_edges[e].q, n);
    if (h_edges[e].u != h_edges[e].v) rec.push_back(h_edges[e]);
  }
  memset(ctx->mcl, 0, sizeof ctx->mcl);
  ctx->mcl_path = 0;
  uint64_t* C = ctx->mcl;
  const uint64_t t_begin = now_ns();
  std::vector<rtc_mcl_entry> mat;
  std::vector<uint64_t> off((size_t)n + 1, 0);
  uint32_t iterations = 0;
  int converged = 0;

  if (rec.empty() || n == 0) {
    // no edge: every column is its loop at ONE, which the first iteration reproduces -- nothing for a device to do, as in
    // rtc_louvain (the path counters stay 0)
    mat.resize(n);
    for (uint32_t j = 0; j < n; j++) { mat[j] = rtc_mcl_entry{j, j, (uint32_t)MCL_ONE, 0u}; off[j + 1] = (uint64_t)j + 1; }
    if (max_iter) { iterations = 1; converged = 1; }
  } else {
    RTC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t stride = std::min(select, n);
    const int all_global = ctx->opt.mcl_global;
    // the global tables: one per workgroup of the long launch, for the largest column there can be
    const uint32_t long_wgs = (uint32_t)std::min<uint64_t>(n, (uint64_t)ctx->num_cu * MCL_GLOBAL_WGS_PER_CU);
    uint32_t gtab_log2 = MCL_GLOBAL_LOG2_MIN;
    while (gtab_log2 < 31 && (1ull << gtab_log2) < 2 * std::min<uint64_t>((uint64_t)stride * stride, n)) gtab_log2++;
    const uint64_t mat_bytes = 16ull * n * stride, tab_bytes = 12ull * long_wgs << gtab_log2, small_bytes = 28ull * n + 4096;
    const uint64_t free_bytes = rtc_free_hbm(ctx);
    if (mat_bytes + tab_bytes + small_bytes > free_bytes)
      return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: %llu bytes for the two matrices of %u columns of %u slots and %llu for the long path's tables, %llu free",
                      who, (unsigned long long)mat_bytes, n, stride, (unsigned long long)tab_bytes, (unsigned long long)free_bytes);
    DevBuf db;
    MclMat A{}, B{};
    for (MclMat* q : {&A, &B}) {
      RTC_TRY(db.get(ctx, (size_t)n * stride, &q->row));
      RTC_TRY(db.get(ctx, (size_t)n * stride, &q->val));
      RTC_TRY(db.get(ctx, n, &q->len));
    }
    uint32_t *d_work = nullptr, *d_list[3] = {nullptr, nullptr, nullptr}, *d_state = nullptr, *d_gkeys = nullptr;
    unsigned long long* d_gvals = nullptr;
    RTC_TRY(db.get(ctx, n, &d_work));
    for (auto& l : d_list) RTC_TRY(db.get(ctx, n, &l));
    RTC_TRY(db.get(ctx, MCL_STATE_WORDS, &d_state));
    RTC_TRY(db.get(ctx, (size_t)long_wgs << gtab_log2, &d_gkeys));
    RTC_TRY(db.get(ctx, (size_t)long_wgs << gtab_log2, &d_gvals));
    MclEvents ev;
    RTC_HIP(ctx, hipEventCreate(&ev.a));
    RTC_HIP(ctx, hipEventCreate(&ev.b));
    uint32_t state[MCL_STATE_WORDS];

    // ---- the start matrix, from the summed symmetric adjacency ----
    {
      Louvain L{ctx};
      const uint64_t m1 = rec.size(), E0 = 2 * m1;
      uint64_t E = 0;
      RTC_TRY(L.alloc(n, E0));
      rtc_wedge* d_edges = nullptr;
      RTC_TRY(L.db.get(ctx, m1, &d_edges));
      RTC_HIP(ctx, hipMemcpyAsync(d_edges, rec.data(), m1 * sizeof(rtc_wedge), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(louvain_entries_kernel, dim3(blocks_for(m1, ctx->num_cu)), dim3(256), 0, s, (const rtc_wedge*)d_edges, m1, L.key_in, L.w);
      RTC_CHECK_LAUNCH(ctx);
      RTC_TRY(L.build(n, E0, &E));
      RTC_HIP(ctx, hipMemsetAsync(d_state, 0, sizeof state, s));
      hipLaunchKernelGGL(mcl_start_kernel, dim3(std::min<uint32_t>(n, (uint32_t)ctx->num_cu * MCL_START_WGS_PER_CU)), dim3(256), 0, s, (const uint64_t*)L.row_off,
                         (const uint64_t*)L.key, (const uint64_t*)L.w, n, stride, select, A, d_state);
      RTC_CHECK_LAUNCH(ctx);
      RTC_HIP(ctx, hipMemcpyAsync(state, d_state, sizeof state, hipMemcpyDeviceToHost, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
      if (state[MCL_TOO_LARGE]) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: the records of a pair sum to 2^32 units or more", who);
      C[7] += state[MCL_CUT];
    }

    // ---- the iterations ----
    MclMat *M = &A, *N = &B;
    while (iterations < max_iter) {
      RTC_HIP(ctx, hipMemsetAsync(d_state, 0, sizeof state, s));
      hipLaunchKernelGGL(mcl_work_kernel, dim3(blocks_for((uint64_t)n * 64, ctx->num_cu)), dim3(256), 0, s, *M, n, stride, all_global, d_work,
                         d_list[0], d_list[1], d_list[2], d_state);
      RTC_CHECK_LAUNCH(ctx);
      RTC_HIP(ctx, hipEventRecord(ev.a, s));
      hipLaunchKernelGGL((mcl_column_kernel<64, MCL_WAVE_SLOTS>), dim3(std::min<uint32_t>(n, (uint32_t)ctx->num_cu * MCL_WAVE_WGS_PER_CU)), dim3(64), 0, s,
                         (const uint32_t*)d_list[0], (const uint32_t*)(d_state + MCL_LIST0), *M, *N, n, stride, select, inflation_x2,
                         (const uint32_t*)d_work, (uint32_t*)nullptr, (unsigned long long*)nullptr, 0u, d_state);
      RTC_CHECK_LAUNCH(ctx);
      hipLaunchKernelGGL((mcl_column_kernel<256, MCL_BLOCK_SLOTS>), dim3(std::min<uint32_t>(n, (uint32_t)ctx->num_cu * MCL_BLOCK_WGS_PER_CU)), dim3(256), 0, s,
                         (const uint32_t*)d_list[1], (const uint32_t*)(d_state + MCL_LIST0 + 1), *M, *N, n, stride, select, inflation_x2,
                         (const uint32_t*)d_work, (uint32_t*)nullptr, (unsigned long long*)nullptr, 0u, d_state);
      RTC_CHECK_LAUNCH(ctx);
      hipLaunchKernelGGL((mcl_column_kernel<256, 0>), dim3(long_wgs), dim3(256), 0, s, (const uint32_t*)d_list[2],
                         (const uint32_t*)(d_state + MCL_LIST0 + 2), *M, *N, n, stride, select, inflation_x2, (const uint32_t*)d_work, d_gkeys,
                         d_gvals, gtab_log2, d_state);
      RTC_CHECK_LAUNCH(ctx);
      RTC_HIP(ctx, hipEventRecord(ev.b, s));
      RTC_HIP(ctx, hipMemcpyAsync(state, d_state, sizeof state, hipMemcpyDeviceToHost, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));  // the one read-back of an iteration
      float ms = 0.f;
      RTC_HIP(ctx, hipEventElapsedTime(&ms, ev.a, ev.b));
      C[8] += (uint64_t)((double)ms * 1e6);
      iterations++;
      for (int p = 0; p < 3; p++) {
        C[4 + p] += state[MCL_LIST0 + p];
        if (state[MCL_LIST0 + p]) ctx->mcl_path |= 1 << p;
      }
      C[7] += state[MCL_CUT];
      std::swap(M, N);
      if (!state[MCL_CHANGED]) { converged = 1; break; }
    }

    // ---- the final matrix to the host, every column in row order ----
    std::vector<uint32_t> len(n);
    RTC_HIP(ctx, hipMemcpyAsync(len.data(), M->len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    for (uint32_t j = 0; j < n; j++) off[j + 1] = off[j] + len[j];
    mat.resize(off[n]);
    if (off[n]) {
      uint64_t* d_off = nullptr;
      rtc_mcl_entry* d_mat = nullptr;
      RTC_TRY(db.get(ctx, (size_t)n + 1, &d_off));
      RTC_TRY(db.get(ctx, (size_t)off[n], &d_mat));
      RTC_HIP(ctx, hipMemcpyAsync(d_off, off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(mcl_entries_kernel, dim3(blocks_for((uint64_t)n * 64, ctx->num_cu)), dim3(256), 0, s, *M, n, stride, (const uint64_t*)d_off,
                         d_mat);
      RTC_CHECK_LAUNCH(ctx);
      RTC_HIP(ctx, hipMemcpyAsync(mat.data(), d_mat, (size_t)off[n] * sizeof(rtc_mcl_entry), hipMemcpyDeviceToHost, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
    }
    for (uint32_t j = 0; j < n; j++)
      std::sort(mat.begin() + off[j], mat.begin() + off[j + 1], [](const rtc_mcl_entry& a, const rtc_mcl_entry& b) { return a.row < b.row; });
  }

  uint64_t attractors = 0;
  mcl_clusters(mat, off, n, h_labels, h_n_clusters, &attractors);
  if (h_iterations) *h_iterations = iterations;
  if (h_converged) *h_converged = converged;
  if (h_nnz) *h_nnz = mat.size();
  C[0] = iterations; C[1] = (uint64_t)converged; C[2] = mat.size(); C[3] = attractors;
  C[9] = now_ns() - t_begin;
  if (h_matrix) {
    if (mat.size() > cap)
      return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: the matrix has %llu entries, room for %llu", who, (unsigned long long)mat.size(), (unsigned long long)cap);
    if (!mat.empty()) memcpy(h_matrix, mat.data(), mat.size() * sizeof(rtc_mcl_entry));
  }
  return RTC_OK;
}

extern "C" int rtc_mcl_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->mcl[i];
  return RTC_OK;
}

extern "C" int rtc_mcl_last_path(const rtc_ctx* ctx) { return ctx ? ctx->mcl_path : 0; }
