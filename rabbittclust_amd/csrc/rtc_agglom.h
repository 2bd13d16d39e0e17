// rtc_agglom.h -- the agglomeration skeleton of rtc_nj.hip and rtc_upgma.hip: a method is a Rule, everything else is here once.
//
// A component is an m x m matrix of 8-byte cells and one state per cluster.  A step finds the least candidate over the active
// pairs (a, b), a < b, updates row and column a and every survivor's state, retires b and appends a record; the cluster keeps
// the name a.  The candidates are totally ordered, so neither the path nor the way the search is split over lanes, waves or
// workgroups changes a record.
//
//   wave path       m <= 64: one wave per component, the cells and the states in LDS, lane x owns cluster x and scans the pairs
//                   (x, y), y > x
//   workgroup path  one 256-lane workgroup per component, the cells in global memory, the states and the active list in a global
//                   scratch; the whole component in one launch
//   grid path       m >= Rule::grid_min: one component on the whole device; a scan launch leaves one minimum per workgroup, a step
//                   launch reduces them, updates, retires b and appends the record.  The two launches a step (and the closing
//                   one) are enqueued back to back; the launch boundary is the only device-wide barrier
// The workgroup and grid paths keep the active clusters as an ascending list, rewritten (one entry dropped) into its twin at
// every step, so a scan touches live rows and columns only and (a < b) is (position of a < position of b).
//
// A Rule is a struct of statics; no kernel branches on which one it runs.
//   cell, state, cand, record         the 8-byte cell, a cluster's state, a candidate {..., uint32_t a, b}, the output record
//   held                              what a scan carries a loaded state as (a size is widened once, not once a pair)
//   END, CLOSING                      the live clusters that end the loop; whether a closing record follows them
//   none(), better(x, y), shfl(v, o)  behind every candidate; the total order; v of lane ^ o
//   init(col, stride, m, x, St, w)    St[x] from column x of the matrix, col[y * stride] for y < m (w: the call's sizes or NULL)
//   step(r)                           what a scan of r live clusters computes once
//   consider(v, k, sa, d, sb, a, b)   v = the better of v and the candidate of the pair (a, b): states sa, sb, cell d, step value k.
//                                     A lane meets its pairs in ascending (a, b); a rule may lean on that
//   pivot(D, ld, v)                   the cell of the chosen pair, read before the update
//   update(D, ld, St, k, v, pv)       row and column v.a at the survivor k, and St[k]
//   emit(St, v, pv, r, out)           one lane: the record, and the state of v.a
//   close(D, ld, i, j, k, m, out)     one lane: the closing record of the live i < j < k (m == 2: of i and j)
//   (D, ld: the matrix and its row stride -- LDS and 32-bit indices on the wave path, global memory and 64-bit ones on the
//   others, so the statics that take them are templates over the index type)
//   host: WAVE_MAX, SCAN_BLOCKS, records_of(m), grid_min(ctx), scan_blocks(ctx), counters(ctx), path(ctx), budget(ctx),
//         batch(ctx, comps) -- what a batch owes the method before its cells are formed
#pragma once
#include <numeric>
#include <thread>
#include <vector>

#include "rtc_internal.h"

namespace {

constexpr uint32_t AGG_NONE = 0xFFFFFFFFu;

template <class Rule>
__device__ __forceinline__ typename Rule::cand agg_wave_best(typename Rule::cand v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const typename Rule::cand o = Rule::shfl(v, off);
    if (Rule::better(o, v)) v = o;
  }
  return v;
}
// the best of a 256-lane workgroup, the same in every lane; s_best is free again after the caller's next barrier
template <class Rule>
__device__ __forceinline__ typename Rule::cand agg_block_best(typename Rule::cand v, typename Rule::cand* s_best, uint32_t lane, uint32_t wave) {
  v = agg_wave_best<Rule>(v);
  if (lane == 0) s_best[wave] = v;
  __syncthreads();
  v = s_best[0];
  for (int w = 1; w < 4; w++) { const typename Rule::cand o = s_best[w]; if (Rule::better(o, v)) v = o; }
  return v;
}

// ---- wave path --------------------------------------------------------------------------------------------------------------
// LDS: K[y * lds + x], lds = m | 1, then the states St[m].  The active set is a 64-bit mask, the same in every lane.
template <class Rule>
__global__ __launch_bounds__(64) void agg_wave_kernel(const typename Rule::cell* __restrict__ cells, const rtc_kb_comp* __restrict__ comps,
                                                      const uint32_t* __restrict__ w, typename Rule::record* __restrict__ recs) {
  using cell = typename Rule::cell;
  using state = typename Rule::state;
  using cand = typename Rule::cand;
  extern __shared__ uint64_t agg_lds[];  // one type for every rule: a dependent one would be declared anew, and differently, per instantiation
  const rtc_kb_comp cp = comps[blockIdx.x];
  const uint32_t m = cp.m, x = threadIdx.x, lds = m | 1;
  cell* K = (cell*)agg_lds;
  state* St = (state*)(agg_lds + (size_t)m * lds);
  const cell* g = cells + cp.key_off;
  typename Rule::record* out = recs + cp.merge_off;
  if (x < m)
    for (uint32_t y = 0; y < m; y++) K[y * lds + x] = g[(uint64_t)y * cp.ld + x];
  __syncthreads();
  if (x < m) Rule::init(K + x * lds, 1u, m, x, St, w);  // row x: the matrix is symmetric
  __syncthreads();
  unsigned long long mask = m == 64 ? ~0ull : (1ull << m) - 1;
  uint32_t r = m;
  for (; r > Rule::END; r--) {
    const auto k = Rule::step(r);
    const bool active = (mask >> x) & 1;
    cand v = Rule::none();
    if (active) {
      const typename Rule::held sx = St[x];
      for (unsigned long long mm = mask & ~((2ull << x) - 1); mm; mm &= mm - 1) {  // the live y above x, ascending
        const uint32_t y = (uint32_t)__ffsll((long long)mm) - 1;
        Rule::consider(v, k, sx, K[x * lds + y], St[y], x, y);
      }
    }
    v = agg_wave_best<Rule>(v);
    if (v.a == AGG_NONE) return;  // no pair: cannot happen on valid input, and nothing may be indexed by it (every lane sees the same)
    const cell pv = Rule::pivot(K, lds, v);
    if (active && x != v.a && x != v.b) Rule::update(K, lds, St, x, v, pv);
    if (x == 0) Rule::emit(St, v, pv, r, out + (m - r));
    __syncthreads();
    mask &= ~(1ull << v.b);
  }
  if constexpr (Rule::CLOSING)
    if (x == 0) {
      const uint32_t i = (uint32_t)__ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const uint32_t j = (uint32_t)__ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const uint32_t k = (uint32_t)__ffsll((long long)mask) - 1;  // m == 2: none, and close does not look at it
      Rule::close(K, lds, i, j, k, m, out + (m - r));
    }
}

// ---- workgroup and grid paths -----------------------------------------------------------------------------------------------
// The least candidate over the rows row0, row0 + step, ... of the active list act[0 .. r), one wave a row, lanes striding its
// columns above the row's own position.  Four loads in flight a lane.
template <class Rule>
__device__ __forceinline__ typename Rule::cand agg_scan(const typename Rule::cell* D, uint64_t ld, const uint32_t* act, const typename Rule::state* St,
                                                        uint32_t r, uint32_t row0, uint32_t step, uint32_t lane) {
  typename Rule::cand v = Rule::none();
  const auto k = Rule::step(r);
  for (uint32_t p = row0; p + 1 < r; p += step) {
    const uint32_t a = act[p];
    const typename Rule::held sa = St[a];
    const typename Rule::cell* row = D + (uint64_t)a * ld;
    for (uint32_t q0 = p + 1 + lane; q0 < r; q0 += 256) {
      uint32_t b[4];
      typename Rule::cell d[4];
      typename Rule::held sb[4];
#pragma unroll
      for (int u = 0; u < 4; u++) b[u] = q0 + 64 * u < r ? act[q0 + 64 * u] : AGG_NONE;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        d[u] = b[u] != AGG_NONE ? row[b[u]] : typename Rule::cell(0);
        sb[u] = b[u] != AGG_NONE ? St[b[u]] : typename Rule::held(0);
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (b[u] != AGG_NONE) Rule::consider(v, k, sa, d[u], sb[u], a, b[u]);
    }
  }
  return v;
}

// the cluster at position p of the active list: its place in the next list (ascending: those above v.b move down one), and the
// rule's update where it survives
template <class Rule>
__device__ __forceinline__ void agg_update_point(typename Rule::cell* D, uint64_t ld, const uint32_t* cur, uint32_t* nxt, typename Rule::state* St,
                                                 uint32_t p, const typename Rule::cand& v, typename Rule::cell pv) {
  const uint32_t k = cur[p];
  if (k == v.b) return;
  nxt[p - (k > v.b ? 1u : 0u)] = k;
  if (k == v.a) return;
  Rule::update(D, ld, St, k, v, pv);
}

// scratch of a component, in 8-byte words from scratch_off: the states, then the two active lists (m u32 each, m rounded up to
// even), then -- grid path -- the scan's minima
__device__ __host__ __forceinline__ uint64_t agg_list_words(uint32_t m) { return ((uint64_t)m + 1) / 2; }
template <class Rule>
__device__ __host__ __forceinline__ uint64_t agg_state_words(uint32_t m) { return ((uint64_t)m * sizeof(typename Rule::state) + 7) / 8; }

template <class Rule>
__global__ __launch_bounds__(256) void agg_wg_kernel(typename Rule::cell* cells, const rtc_kb_comp* __restrict__ comps, const uint32_t* __restrict__ w,
                                                     typename Rule::record* __restrict__ recs, uint64_t* scratch) {
  using cand = typename Rule::cand;
  __shared__ cand s_best[4];
  const rtc_kb_comp cp = comps[blockIdx.x];
  const uint32_t m = cp.m, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t ld = cp.ld;
  typename Rule::cell* D = cells + cp.key_off;
  typename Rule::state* St = (typename Rule::state*)(scratch + cp.scratch_off);
  uint32_t* cur = (uint32_t*)(scratch + cp.scratch_off + agg_state_words<Rule>(m));
  uint32_t* nxt = (uint32_t*)(scratch + cp.scratch_off + agg_state_words<Rule>(m) + agg_list_words(m));
  typename Rule::record* out = recs + cp.merge_off;
  for (uint32_t x = tid; x < m; x += 256) { Rule::init(D + x, ld, m, x, St, w); cur[x] = x; }
  __syncthreads();
  for (uint32_t r = m; r > Rule::END; r--) {
    const cand v = agg_block_best<Rule>(agg_scan<Rule>(D, ld, cur, St, r, wave, 4, lane), s_best, lane, wave);
    if (v.a == AGG_NONE) return;  // no pair: cannot happen on valid input, and nothing may be indexed by it (every lane sees the same)
    const typename Rule::cell pv = Rule::pivot(D, ld, v);
    for (uint32_t p = tid; p < r; p += 256) agg_update_point<Rule>(D, ld, cur, nxt, St, p, v, pv);
    if (tid == 0) Rule::emit(St, v, pv, r, out + (m - r));
    __syncthreads();
    uint32_t* t = cur; cur = nxt; nxt = t;
  }
  if constexpr (Rule::CLOSING)
    if (tid == 0) Rule::close(D, ld, cur[0], cur[1], cur[2], m, out + (m - Rule::END));
}

// column x of the matrix: consecutive lanes read consecutive addresses.  The active list starts as 0, 1, ..., m - 1
template <class Rule>
__global__ __launch_bounds__(256) void agg_grid_init_kernel(const typename Rule::cell* __restrict__ D, uint64_t ld, uint32_t m,
                                                            const uint32_t* __restrict__ w, typename Rule::state* __restrict__ St,
                                                            uint32_t* __restrict__ act) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x < m) { Rule::init(D + x, ld, m, x, St, w); act[x] = x; }
}

template <class Rule>
__global__ __launch_bounds__(256) void agg_grid_scan_kernel(const typename Rule::cell* __restrict__ D, uint64_t ld, const uint32_t* __restrict__ act,
                                                            const typename Rule::state* __restrict__ St, uint32_t r,
                                                            typename Rule::cand* __restrict__ minima) {
  using cand = typename Rule::cand;
  __shared__ cand s_best[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const cand v = agg_block_best<Rule>(agg_scan<Rule>(D, ld, act, St, r, blockIdx.x * 4 + wave, gridDim.x * 4, lane), s_best, lane, wave);
  if (tid == 0) minima[blockIdx.x] = v;
}

// Every workgroup reduces the scan's minima for itself and updates the 256 clusters at its positions of the list; the first one
// also writes the record and the state of v.a.  No workgroup reads what another writes: the cells (a, k) and (k, a) and St[k]
// belong to the lane that holds k, the cell (a, b) is not written, St[a] and St[b] are the first workgroup's alone, and the
// next scan starts at the launch boundary.
template <class Rule>
__global__ __launch_bounds__(256) void agg_grid_step_kernel(typename Rule::cell* D, uint64_t ld, const uint32_t* __restrict__ cur, uint32_t* __restrict__ nxt,
                                                            typename Rule::state* St, uint32_t r, const typename Rule::cand* __restrict__ minima,
                                                            uint32_t n_minima, typename Rule::record* __restrict__ out) {
  using cand = typename Rule::cand;
  __shared__ cand s_best[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  cand v = Rule::none();
  for (uint32_t b = tid; b < n_minima; b += 256) { const cand o = minima[b]; if (Rule::better(o, v)) v = o; }
  v = agg_block_best<Rule>(v, s_best, lane, wave);
  if (v.a == AGG_NONE) return;  // no pair: cannot happen on valid input, and nothing may be indexed by it
  const typename Rule::cell pv = Rule::pivot(D, ld, v);
  const uint32_t p = blockIdx.x * 256 + tid;
  if (p < r) agg_update_point<Rule>(D, ld, cur, nxt, St, p, v, pv);
  if (blockIdx.x == 0 && tid == 0) Rule::emit(St, v, pv, r, out);
}

template <class Rule>
__global__ void agg_grid_close_kernel(const typename Rule::cell* __restrict__ D, uint64_t ld, const uint32_t* __restrict__ act, uint32_t m,
                                      typename Rule::record* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) Rule::close(D, ld, act[0], act[1], act[2], m, out);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// 0 wave, 1 workgroup, 2 grid
template <class Rule>
inline int agg_path_of(const rtc_ctx* ctx, uint32_t m) { return m >= Rule::grid_min(ctx) ? 2 : m <= Rule::WAVE_MAX ? 0 : 1; }

// Agglomerates comps[0 .. nc) (each m >= 2) over the matrices in d_cells: one launch for the wave-path components, one for the
// workgroup-path ones, the launch chain of every grid-path one; then the records come back, laid out by merge_off (set here).
// d_w: the sizes of the one component of a call that has them, or NULL.  n_path[3]: the components of each path.
template <class Rule>
int agg_run(rtc_ctx* ctx, typename Rule::cell* d_cells, std::vector<rtc_kb_comp>& comps, const uint32_t* d_w, std::vector<typename Rule::record>& h_out,
            uint64_t n_path[3]) {
  using cell = typename Rule::cell;
  using state = typename Rule::state;
  using cand = typename Rule::cand;
  using record = typename Rule::record;
  static_assert(sizeof(cell) == 8 && sizeof(cand) % 8 == 0, "cells and candidates are whole 8-byte words");
  const size_t nc = comps.size();
  h_out.clear();
  n_path[0] = n_path[1] = n_path[2] = 0;
  if (!nc) return RTC_OK;
  std::vector<uint32_t> order(nc);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return agg_path_of<Rule>(ctx, comps[x].m) < agg_path_of<Rule>(ctx, comps[y].m); });
  uint64_t n_rec = 0, n_scratch = 0;
  uint32_t m_wave = 0;
  std::vector<rtc_kb_comp> sorted(nc);
  for (size_t s = 0; s < nc; s++) {
    rtc_kb_comp& c = comps[order[s]];
    const int path = agg_path_of<Rule>(ctx, c.m);
    n_path[path]++;
    c.merge_off = n_rec;
    n_rec += Rule::records_of(c.m);
    if (path == 0) m_wave = std::max(m_wave, c.m);
    else {
      c.scratch_off = n_scratch;
      n_scratch += agg_state_words<Rule>(c.m) + 2 * agg_list_words(c.m) + (path == 2 ? (uint64_t)Rule::SCAN_BLOCKS * (sizeof(cand) / 8) : 0);
    }
    sorted[s] = c;
  }
  DevBuf B;
  rtc_kb_comp* d_comps = nullptr;
  record* d_recs = nullptr;
  uint64_t* d_scratch = nullptr;
  RTC_TRY(B.get(ctx, nc, &d_comps));
  RTC_TRY(B.get(ctx, n_rec, &d_recs));
  RTC_TRY(B.get(ctx, n_scratch, &d_scratch));
  RTC_HIP(ctx, hipMemcpyAsync(d_comps, sorted.data(), nc * sizeof(rtc_kb_comp), hipMemcpyHostToDevice, ctx->stream));
  if (n_path[0]) {
    const size_t lds = (size_t)m_wave * (m_wave | 1) * 8 + (size_t)m_wave * sizeof(state);
    hipLaunchKernelGGL(agg_wave_kernel<Rule>, dim3((uint32_t)n_path[0]), dim3(64), lds, ctx->stream, (const cell*)d_cells, (const rtc_kb_comp*)d_comps, d_w,
                       d_recs);
    RTC_CHECK_LAUNCH(ctx);
  }
  if (n_path[1]) {
    hipLaunchKernelGGL(agg_wg_kernel<Rule>, dim3((uint32_t)n_path[1]), dim3(256), 0, ctx->stream, d_cells, (const rtc_kb_comp*)(d_comps + n_path[0]), d_w,
                       d_recs, d_scratch);
    RTC_CHECK_LAUNCH(ctx);
  }
  for (size_t s = n_path[0] + n_path[1]; s < nc; s++) {
    const rtc_kb_comp& c = sorted[s];
    const uint32_t m = c.m;  // >= 4
    const uint64_t sw = agg_state_words<Rule>(m), lw = agg_list_words(m);
    cell* D = d_cells + c.key_off;
    state* St = (state*)(d_scratch + c.scratch_off);
    uint32_t* act[2] = {(uint32_t*)(d_scratch + c.scratch_off + sw), (uint32_t*)(d_scratch + c.scratch_off + sw + lw)};
    cand* minima = (cand*)(d_scratch + c.scratch_off + sw + 2 * lw);
    record* out = d_recs + c.merge_off;
    hipLaunchKernelGGL(agg_grid_init_kernel<Rule>, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, (const cell*)D, c.ld, m, d_w, St, act[0]);
    RTC_CHECK_LAUNCH(ctx);
    int t = 0;
    const uint32_t cap = Rule::scan_blocks(ctx);
    for (uint32_t r = m; r > Rule::END; r--, t ^= 1) {
      const uint32_t nb = std::min<uint32_t>((r - 1 + 3) / 4, cap);
      hipLaunchKernelGGL(agg_grid_scan_kernel<Rule>, dim3(nb), dim3(256), 0, ctx->stream, (const cell*)D, c.ld, (const uint32_t*)act[t], (const state*)St, r,
                         minima);
      RTC_CHECK_LAUNCH(ctx);
      hipLaunchKernelGGL(agg_grid_step_kernel<Rule>, dim3((r + 255) / 256), dim3(256), 0, ctx->stream, D, c.ld, (const uint32_t*)act[t], act[t ^ 1], St, r,
                         (const cand*)minima, nb, out + (m - r));
      RTC_CHECK_LAUNCH(ctx);
    }
    if constexpr (Rule::CLOSING) {
      hipLaunchKernelGGL(agg_grid_close_kernel<Rule>, dim3(1), dim3(64), 0, ctx->stream, (const cell*)D, c.ld, (const uint32_t*)act[t], m, out + (m - Rule::END));
      RTC_CHECK_LAUNCH(ctx);
    }
  }
  h_out.resize(n_rec);
  if (n_rec) RTC_HIP(ctx, hipMemcpyAsync(h_out.data(), d_recs, n_rec * sizeof(record), hipMemcpyDeviceToHost, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RTC_OK;
}

// keys -> cells in place, rows [r0, r1) of every block on one thread: cell(on the diagonal, common, denom) gives the 8 bytes.
// The fill leaves the diagonal alone, so its keys mean nothing.
template <class CellOf>
void agg_cells(uint64_t* cells, const std::vector<rtc_kb_comp>& comps, int threads, CellOf cell) {
  struct unit { const rtc_kb_comp* c; uint32_t r0, r1; };
  std::vector<unit> units;
  for (const rtc_kb_comp& c : comps) {
    const uint32_t rows = (uint32_t)std::max<uint64_t>(1, 65536 / c.m);
    for (uint32_t r = 0; r < c.m; r += rows) units.push_back(unit{&c, r, std::min(c.m, r + rows)});
  }
  auto work = [&](size_t u0, size_t stride) {
    for (size_t u = u0; u < units.size(); u += stride) {
      const rtc_kb_comp& c = *units[u].c;
      for (uint32_t i = units[u].r0; i < units[u].r1; i++) {
        uint64_t* row = cells + c.key_off + (uint64_t)i * c.ld;
        for (uint32_t j = 0; j < c.m; j++) row[j] = cell(i == j, (uint32_t)row[j], (uint32_t)(row[j] >> 32));  // rtc_lkey {common, denom}, little endian
      }
    }
  };
  const size_t T = std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), units.size()));
  if (T == 1) { work(0, 1); return; }
  std::vector<std::thread> pool;
  for (size_t t = 0; t < T; t++) pool.emplace_back(work, t, T);
  for (std::thread& th : pool) th.join();
}

// a hook sees every batch of two or more after its components are agglomerated: the batch (blocks overwritten), the
// components, their records with local indices, the records before the batch
template <class Rule>
using agg_hook = std::function<int(const rtc_kb_batch&, const std::vector<rtc_kb_comp>&, const std::vector<typename Rule::record>&, uint64_t)>;

// One dendrogram per component of a labelling: the argument checks of rtc_nj_clusters and rtc_upgma_clusters, then batch after
// batch of rtc_key_blocks -- the keys to the host, the cells back into the same 8 bytes, the agglomeration, the records handed
// over.  Counters 0 to 4 and 6 to 9 and the path bits are kept here; who starts the messages.
template <class Rule, class CellOf>
int agg_clusters(rtc_ctx* ctx, const char* who, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                 const uint32_t* h_comp, int kmer_size, typename Rule::record* h_recs, uint64_t cap, uint64_t* h_n_recs, uint64_t* h_first,
                 uint32_t spare_copies, const agg_hook<Rule>* hook, CellOf cell) {
  if (!ctx || !h_n_recs || !h_first) return RTC_ERR_ARG;
  *h_n_recs = 0;
  h_first[0] = 0;
  if (width != 4 && width != 8) return rtc_fail(ctx, RTC_ERR_ARG, "width must be 4 or 8");
  if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: kmer_size must be at least 1", who);
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: n must be below 2^31 - 1", who);
  if (cap && !h_recs) return RTC_ERR_ARG;
  uint64_t* C = Rule::counters(ctx);
  for (int i = 0; i < 10; i++) C[i] = 0;
  *Rule::path(ctx) = 0;
  if (n == 0) return RTC_OK;
  if (!d_start || !d_len || !h_comp) return RTC_ERR_ARG;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t t0 = rtc_now_ns();
  uint64_t total = 0;
  bool overflow = false;
  std::vector<uint64_t> cells;
  RTC_TRY(rtc_key_blocks(ctx, who, Rule::budget(ctx), d_hashes, width, d_start, d_len, n, h_comp, h_first, [&](const rtc_kb_batch& b) -> int {
    std::vector<rtc_kb_comp>& comps = *b.comps;
    std::vector<typename Rule::record> out;
    if (b.d_keys) {
      C[6] += b.fill_ns;
      RTC_TRY(Rule::batch(ctx, comps));
      // the keys to the host, the cells back into the same 8 bytes
      const uint64_t td0 = rtc_now_ns();
      cells.resize(b.n_keys);
      RTC_HIP(ctx, hipMemcpyAsync(cells.data(), b.d_keys, b.n_keys * 8, hipMemcpyDeviceToHost, ctx->stream));
      RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
      agg_cells(cells.data(), comps, ctx->host_threads, cell);
      RTC_HIP(ctx, hipMemcpyAsync(b.d_keys, cells.data(), b.n_keys * 8, hipMemcpyHostToDevice, ctx->stream));
      RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
      const uint64_t td1 = rtc_now_ns();
      C[7] += td1 - td0;
      uint64_t n_path[3];
      RTC_TRY(agg_run<Rule>(ctx, (typename Rule::cell*)b.d_keys, comps, nullptr, out, n_path));
      C[8] += rtc_now_ns() - td1;
      for (int p = 0; p < 3; p++) { C[1 + p] += n_path[p]; if (n_path[p]) *Rule::path(ctx) |= 1 << p; }
      if (hook) RTC_TRY((*hook)(b, comps, out, total));
    }
    rtc_kb_remap(b, out, [&](size_t, const rtc_kb_comp& cp) { const uint64_t nr = Rule::records_of(cp.m); C[0]++; C[4] += nr; return nr; }, h_recs, cap, h_first,
                 &total, &overflow);
    return RTC_OK;
  }, spare_copies));
  *h_n_recs = total;
  C[9] = rtc_now_ns() - t0;
  if (overflow) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu records, room for %llu", who, (unsigned long long)total, (unsigned long long)cap);
  return RTC_OK;
}

// what a call over one matrix leaves in the counters: one component, its path, its records, the whole call as the agglomeration
template <class Rule>
void agg_count_one(rtc_ctx* ctx, const uint64_t n_path[3], uint64_t n_rec, uint64_t ns) {
  uint64_t* C = Rule::counters(ctx);
  C[0] = 1; C[1] = n_path[0]; C[2] = n_path[1]; C[3] = n_path[2]; C[4] = n_rec; C[8] = ns; C[9] = ns;
  *Rule::path(ctx) = (n_path[0] ? 1 : 0) | (n_path[1] ? 2 : 0) | (n_path[2] ? 4 : 0);
}

}  // namespace
