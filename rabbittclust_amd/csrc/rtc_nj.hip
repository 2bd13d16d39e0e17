// rtc_nj.hip -- clust-mst --nj-tree / --nj-all: neighbour joining of the clusters on the device.
//
// The definition is in include/rtclust.h (tests/refnj.py restates it).  Every value a join forms is one double operation in the
// written order (the unit is built with -ffp-contract=off), and the only sum whose order matters -- the initial R -- is one
// thread's loop over ascending j.  The least Q is found on the triple (Q, i, j) with exact comparisons, so neither the path nor
// the way the search is split over lanes, waves or workgroups changes a record.
//
//   wave path       m <= 64: one wave per component, D and R in LDS, lane x owns point x and scans the pairs (x, y), y > x
//   workgroup path  one 256-lane workgroup per component, D in global memory, R and the active list in a global scratch; the
//                   whole tree in one launch
//   grid path       m >= RTC_NJ_GRID_MIN: one component on the whole device; a scan launch leaves one minimum per workgroup, a
//                   join launch reduces them, updates row i, column i and R, retires j and appends the record.  The 2 (m - 3)
//                   launches and the last one are enqueued back to back; the launch boundary is the only device-wide barrier
// The workgroup and grid paths keep the active nodes as an ascending list, rewritten (one entry dropped) into its twin at every
// join, so a scan touches live rows and columns only and (i < j) is (position of i < position of j).
#include <time.h>

#include <algorithm>
#include <numeric>
#include <thread>
#include <vector>

#include "rtc_internal.h"

namespace {

constexpr uint32_t NJ_NONE = 0xFFFFFFFFu;
constexpr uint32_t NJ_WAVE_MAX = 64;        // the wave path's largest m
constexpr uint32_t NJ_GRID_MIN = 256;       // the grid path's default first m (RTC_NJ_GRID_MIN; measured)
constexpr uint32_t NJ_SCAN_BLOCKS = 1024;   // the most workgroups of a scan launch: their minima are read again by every join workgroup

struct nj_cand { double q; uint32_t i, j; };

// the order of a step's choice: Q ascending, then i ascending, then j ascending
__device__ __forceinline__ bool nj_better(const nj_cand& x, const nj_cand& y) {
  return x.q < y.q || (x.q == y.q && (x.i < y.i || (x.i == y.i && x.j < y.j)));
}
__device__ __forceinline__ nj_cand nj_none() { return nj_cand{__longlong_as_double(0x7FF0000000000000ll), NJ_NONE, NJ_NONE}; }
__device__ __forceinline__ nj_cand nj_wave_best(nj_cand v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    nj_cand o;
    o.q = __shfl_xor(v.q, off); o.i = __shfl_xor(v.i, off); o.j = __shfl_xor(v.j, off);
    if (nj_better(o, v)) v = o;
  }
  return v;
}
// the best of a 256-lane workgroup, the same in every lane; s_best is free again after the caller's next barrier
__device__ __forceinline__ nj_cand nj_block_best(nj_cand v, nj_cand* s_best, uint32_t lane, uint32_t wave) {
  v = nj_wave_best(v);
  if (lane == 0) s_best[wave] = v;
  __syncthreads();
  v = s_best[0];
  for (int w = 1; w < 4; w++) { const nj_cand o = s_best[w]; if (nj_better(o, v)) v = o; }
  return v;
}

// what a join does to its two nodes (steps 4 and 6) -- one lane
__device__ __forceinline__ void nj_emit_join(double* R, uint32_t i, uint32_t j, double dij, uint32_t r, rtc_njoin* out) {
  const double ri = R[i], rj = R[j];
  const double delta = (ri - rj) / (double)(2 * (uint64_t)(r - 2));
  const double len_i = 0.5 * dij + delta;
  const double len_j = dij - len_i;
  R[i] = 0.5 * ((ri + rj) - (double)r * dij);
  *out = rtc_njoin{i, j, NJ_NONE, 0u, len_i, len_j, 0.0};
}
__device__ __forceinline__ void nj_emit_last(double dij, double dik, double djk, uint32_t i, uint32_t j, uint32_t k, rtc_njoin* out) {
  *out = rtc_njoin{i, j, k, 0u, 0.5 * ((dij + dik) - djk), 0.5 * ((dij + djk) - dik), 0.5 * ((dik + djk) - dij)};
}

// ---- wave path --------------------------------------------------------------------------------------------------------------
// LDS: K[y * lds + x], lds = m | 1, then R[m].  The active set is a 64-bit mask, the same in every lane.
__global__ __launch_bounds__(64) void nj_wave_kernel(const double* __restrict__ dist, const rtc_kb_comp* __restrict__ comps,
                                                     rtc_njoin* __restrict__ joins) {
  extern __shared__ double nj_lds[];
  const rtc_kb_comp cp = comps[blockIdx.x];
  const uint32_t m = cp.m, x = threadIdx.x, lds = m | 1;
  double* K = nj_lds;
  double* R = nj_lds + (size_t)m * lds;
  const double* g = dist + cp.key_off;
  rtc_njoin* out = joins + cp.merge_off;
  if (x < m)
    for (uint32_t y = 0; y < m; y++) K[y * lds + x] = g[(uint64_t)y * cp.ld + x];
  __syncthreads();
  if (m == 2) {
    if (x == 0) { const double d = K[1], la = 0.5 * d; out[0] = rtc_njoin{0u, 1u, NJ_NONE, 0u, la, d - la, 0.0}; }
    return;
  }
  if (x < m) {
    double s = 0.0;
    for (uint32_t y = 0; y < m; y++) if (y != x) s = s + K[x * lds + y];
    R[x] = s;
  }
  __syncthreads();
  unsigned long long mask = m == 64 ? ~0ull : (1ull << m) - 1;
  uint32_t r = m, nrec = 0;
  while (r > 3) {
    const double rm2 = (double)(r - 2);
    const bool active = (mask >> x) & 1;
    nj_cand v = nj_none();
    if (active) {
      const double rx = R[x];
      for (unsigned long long mm = mask & ~((2ull << x) - 1); mm; mm &= mm - 1) {  // the live y above x, ascending
        const uint32_t y = (uint32_t)__ffsll((long long)mm) - 1;
        const double q = (rm2 * K[x * lds + y] - rx) - R[y];
        if (q < v.q) v = nj_cand{q, x, y};
      }
    }
    v = nj_wave_best(v);
    const uint32_t i = v.i, j = v.j;
    if (i == NJ_NONE) return;  // no pair: cannot happen on finite input, and nothing may be indexed by it (every lane sees the same)
    const double dij = K[i * lds + j];
    if (active && x != i && x != j) {
      const double dik = K[i * lds + x], djk = K[j * lds + x];
      const double duk = 0.5 * ((dik + djk) - dij);
      R[x] = ((R[x] - dik) - djk) + duk;
      K[i * lds + x] = duk;
      K[x * lds + i] = duk;
    }
    if (x == 0) nj_emit_join(R, i, j, dij, r, out + nrec);
    __syncthreads();
    mask &= ~(1ull << j);
    r--;
    nrec++;
  }
  if (x == 0) {
    const uint32_t i = (uint32_t)__ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const uint32_t j = (uint32_t)__ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const uint32_t k = (uint32_t)__ffsll((long long)mask) - 1;
    nj_emit_last(K[i * lds + j], K[i * lds + k], K[j * lds + k], i, j, k, out + nrec);
  }
}

// ---- workgroup and grid paths -----------------------------------------------------------------------------------------------
// R[x] over column x -- the matrix is symmetric, and consecutive lanes read consecutive addresses -- in ascending y; the active list
// starts as 0, 1, ..., m - 1
__device__ __forceinline__ void nj_init_point(const double* D, uint64_t ld, uint32_t m, uint32_t x, double* R, uint32_t* act) {
  double s = 0.0;
  for (uint32_t y = 0; y < m; y++) {
    const double d = D[(uint64_t)y * ld + x];
    if (y != x) s = s + d;
  }
  R[x] = s;
  act[x] = x;
}

// The least Q over the rows row0, row0 + step, ... of the active list act[0 .. r), one wave a row, lanes striding its columns above
// the row's own position.  A lane meets its pairs in ascending (i, j), so the first of equal Q stays.  Four loads in flight a lane.
__device__ __forceinline__ nj_cand nj_scan(const double* D, uint64_t ld, const uint32_t* act, const double* R, uint32_t r, uint32_t row0,
                                           uint32_t step, uint32_t lane) {
  nj_cand v = nj_none();
  const double rm2 = (double)(r - 2);
  for (uint32_t p = row0; p + 1 < r; p += step) {
    const uint32_t a = act[p];
    const double ra = R[a];
    const double* row = D + (uint64_t)a * ld;
    for (uint32_t q0 = p + 1 + lane; q0 < r; q0 += 256) {
      uint32_t b[4];
      double d[4], rb[4];
#pragma unroll
      for (int u = 0; u < 4; u++) b[u] = q0 + 64 * u < r ? act[q0 + 64 * u] : NJ_NONE;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        d[u] = b[u] != NJ_NONE ? row[b[u]] : 0.0;
        rb[u] = b[u] != NJ_NONE ? R[b[u]] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (b[u] != NJ_NONE) {
          const double q = (rm2 * d[u] - ra) - rb[u];
          if (q < v.q) v = nj_cand{q, a, b[u]};
        }
    }
  }
  return v;
}

// step 5 for the node at position p of the active list, and its place in the next list (ascending: the nodes above j move down one)
__device__ __forceinline__ void nj_update_point(double* D, uint64_t ld, const uint32_t* cur, uint32_t* nxt, double* R, uint32_t p, uint32_t i,
                                                uint32_t j, double dij) {
  const uint32_t k = cur[p];
  if (k == j) return;
  nxt[p - (k > j ? 1u : 0u)] = k;
  if (k == i) return;
  const double dik = D[(uint64_t)i * ld + k], djk = D[(uint64_t)j * ld + k];
  const double duk = 0.5 * ((dik + djk) - dij);
  R[k] = ((R[k] - dik) - djk) + duk;
  D[(uint64_t)i * ld + k] = duk;
  D[(uint64_t)k * ld + i] = duk;
}

__device__ __forceinline__ void nj_last_three(const double* D, uint64_t ld, const uint32_t* act, rtc_njoin* out) {
  const uint32_t i = act[0], j = act[1], k = act[2];
  nj_emit_last(D[(uint64_t)i * ld + j], D[(uint64_t)i * ld + k], D[(uint64_t)j * ld + k], i, j, k, out);
}

// scratch of a component, in 8-byte words from scratch_off: R[m], then the two active lists (m u32 each, m rounded up to even),
// then -- grid path -- the scan's minima
__device__ __host__ __forceinline__ uint64_t nj_list_words(uint32_t m) { return ((uint64_t)m + 1) / 2; }

__global__ __launch_bounds__(256) void nj_wg_kernel(double* dist, const rtc_kb_comp* __restrict__ comps, rtc_njoin* __restrict__ joins,
                                                    uint64_t* scratch) {
  __shared__ nj_cand s_best[4];
  const rtc_kb_comp cp = comps[blockIdx.x];
  const uint32_t m = cp.m, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t ld = cp.ld;
  double* D = dist + cp.key_off;
  double* R = (double*)(scratch + cp.scratch_off);
  uint32_t* cur = (uint32_t*)(scratch + cp.scratch_off + m);
  uint32_t* nxt = (uint32_t*)(scratch + cp.scratch_off + m + nj_list_words(m));
  rtc_njoin* out = joins + cp.merge_off;
  for (uint32_t x = tid; x < m; x += 256) nj_init_point(D, ld, m, x, R, cur);
  __syncthreads();
  uint32_t r = m, nrec = 0;
  while (r > 3) {
    const nj_cand v = nj_block_best(nj_scan(D, ld, cur, R, r, wave, 4, lane), s_best, lane, wave);
    const uint32_t i = v.i, j = v.j;
    if (i == NJ_NONE) return;  // no pair: cannot happen on finite input, and nothing may be indexed by it (every lane sees the same)
    const double dij = D[(uint64_t)i * ld + j];
    for (uint32_t p = tid; p < r; p += 256) nj_update_point(D, ld, cur, nxt, R, p, i, j, dij);
    if (tid == 0) nj_emit_join(R, i, j, dij, r, out + nrec);
    __syncthreads();
    uint32_t* t = cur; cur = nxt; nxt = t;
    r--;
    nrec++;
  }
  if (tid == 0) nj_last_three(D, ld, cur, out + nrec);
}

__global__ __launch_bounds__(256) void nj_grid_init_kernel(const double* __restrict__ D, uint64_t ld, uint32_t m, double* __restrict__ R,
                                                           uint32_t* __restrict__ act) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x < m) nj_init_point(D, ld, m, x, R, act);
}

__global__ __launch_bounds__(256) void nj_grid_scan_kernel(const double* __restrict__ D, uint64_t ld, const uint32_t* __restrict__ act,
                                                           const double* __restrict__ R, uint32_t r, nj_cand* __restrict__ minima) {
  __shared__ nj_cand s_best[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const nj_cand v = nj_block_best(nj_scan(D, ld, act, R, r, blockIdx.x * 4 + wave, gridDim.x * 4, lane), s_best, lane, wave);
  if (tid == 0) minima[blockIdx.x] = v;
}

// Every workgroup reduces the scan's minima for itself and updates the 256 nodes at its positions of the list; the first one also
// does the join's own two nodes and the record.  No workgroup reads what another writes: R[i] and R[j] are the first one's alone,
// D[i][j] is not written, and the next scan starts at the launch boundary.
__global__ __launch_bounds__(256) void nj_grid_join_kernel(double* D, uint64_t ld, const uint32_t* __restrict__ cur, uint32_t* __restrict__ nxt,
                                                           double* R, uint32_t r, const nj_cand* __restrict__ minima, uint32_t n_minima,
                                                           rtc_njoin* __restrict__ out) {
  __shared__ nj_cand s_best[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  nj_cand v = nj_none();
  for (uint32_t b = tid; b < n_minima; b += 256) { const nj_cand o = minima[b]; if (nj_better(o, v)) v = o; }
  v = nj_block_best(v, s_best, lane, wave);
  const uint32_t i = v.i, j = v.j;
  if (i == NJ_NONE) return;  // no pair: cannot happen on finite input, and nothing may be indexed by it
  const double dij = D[(uint64_t)i * ld + j];
  const uint32_t p = blockIdx.x * 256 + tid;
  if (p < r) nj_update_point(D, ld, cur, nxt, R, p, i, j, dij);
  if (blockIdx.x == 0 && tid == 0) nj_emit_join(R, i, j, dij, r, out);
}

__global__ void nj_grid_last_kernel(const double* __restrict__ D, uint64_t ld, const uint32_t* __restrict__ act, rtc_njoin* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) nj_last_three(D, ld, act, out);
}

uint64_t nj_now_ns() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

// device buffers of one call, released on every way out
struct nj_bufs {
  std::vector<void*> p;
  ~nj_bufs() { for (void* q : p) (void)hipFree(q); }
  int get(rtc_ctx* ctx, size_t bytes, void** out) {
    ctx->free_hbm_at = -1.0;
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e != hipSuccess) { (void)hipGetLastError(); return rtc_fail(ctx, RTC_ERR_NOMEM, "rtc_nj: hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
    p.push_back(*out);
    return RTC_OK;
  }
};

inline uint64_t nj_records_of(uint32_t m) { return m >= 3 ? m - 2 : m == 2 ? 1 : 0; }
inline uint32_t nj_grid_min(const rtc_ctx* ctx) { return ctx->opt.nj_grid_min ? std::max<uint32_t>(ctx->opt.nj_grid_min, 4) : NJ_GRID_MIN; }
// the most workgroups of a scan launch: RTC_NJ_SCAN_BLOCKS below the ceiling the scratch reserves (tests reach a second row per workgroup with it)
inline uint32_t nj_scan_blocks(const rtc_ctx* ctx) { return ctx->opt.nj_scan_blocks ? std::min<uint32_t>(ctx->opt.nj_scan_blocks, NJ_SCAN_BLOCKS) : NJ_SCAN_BLOCKS; }
// 0 wave, 1 workgroup, 2 grid
inline int nj_path_of(const rtc_ctx* ctx, uint32_t m) { return m >= nj_grid_min(ctx) ? 2 : m <= NJ_WAVE_MAX ? 0 : 1; }

// Joins comps[0 .. nc) (each m >= 2) over the matrices in d_dist: one launch for the wave-path components, one for the
// workgroup-path ones, the launch chain of every grid-path one; then the records come back, laid out by merge_off (set here).
// n_path[3]: the components of each path.
int nj_join(rtc_ctx* ctx, double* d_dist, std::vector<rtc_kb_comp>& comps, std::vector<rtc_njoin>& h_out, uint64_t n_path[3]) {
  const size_t nc = comps.size();
  h_out.clear();
  n_path[0] = n_path[1] = n_path[2] = 0;
  if (!nc) return RTC_OK;
  std::vector<uint32_t> order(nc);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return nj_path_of(ctx, comps[x].m) < nj_path_of(ctx, comps[y].m); });
  uint64_t n_rec = 0, n_scratch = 0;
  uint32_t m_wave = 0;
  std::vector<rtc_kb_comp> sorted(nc);
  for (size_t s = 0; s < nc; s++) {
    rtc_kb_comp& c = comps[order[s]];
    const int path = nj_path_of(ctx, c.m);
    n_path[path]++;
    c.merge_off = n_rec;
    n_rec += nj_records_of(c.m);
    if (path == 0) m_wave = std::max(m_wave, c.m);
    else {
      c.scratch_off = n_scratch;
      n_scratch += (uint64_t)c.m + 2 * nj_list_words(c.m) + (path == 2 ? (uint64_t)NJ_SCAN_BLOCKS * (sizeof(nj_cand) / 8) : 0);
    }
    sorted[s] = c;
  }
  static_assert(sizeof(nj_cand) == 16, "nj_cand is two 8-byte words");
  nj_bufs B;
  rtc_kb_comp* d_comps = nullptr;
  rtc_njoin* d_joins = nullptr;
  uint64_t* d_scratch = nullptr;
  RTC_TRY(B.get(ctx, nc * sizeof(rtc_kb_comp), (void**)&d_comps));
  RTC_TRY(B.get(ctx, n_rec * sizeof(rtc_njoin), (void**)&d_joins));
  RTC_TRY(B.get(ctx, n_scratch * 8, (void**)&d_scratch));
  RTC_HIP(ctx, hipMemcpyAsync(d_comps, sorted.data(), nc * sizeof(rtc_kb_comp), hipMemcpyHostToDevice, ctx->stream));
  if (n_path[0]) {
    const size_t lds = ((size_t)m_wave * (m_wave | 1) + m_wave) * 8;
    hipLaunchKernelGGL(nj_wave_kernel, dim3((uint32_t)n_path[0]), dim3(64), lds, ctx->stream, (const double*)d_dist, (const rtc_kb_comp*)d_comps, d_joins);
    RTC_CHECK_LAUNCH(ctx);
  }
  if (n_path[1]) {
    hipLaunchKernelGGL(nj_wg_kernel, dim3((uint32_t)n_path[1]), dim3(256), 0, ctx->stream, d_dist, (const rtc_kb_comp*)(d_comps + n_path[0]), d_joins,
                       d_scratch);
    RTC_CHECK_LAUNCH(ctx);
  }
  for (size_t s = n_path[0] + n_path[1]; s < nc; s++) {
    const rtc_kb_comp& c = sorted[s];
    const uint32_t m = c.m;  // >= 4
    double* D = d_dist + c.key_off;
    double* R = (double*)(d_scratch + c.scratch_off);
    uint32_t* act[2] = {(uint32_t*)(d_scratch + c.scratch_off + m), (uint32_t*)(d_scratch + c.scratch_off + m + nj_list_words(m))};
    nj_cand* minima = (nj_cand*)(d_scratch + c.scratch_off + m + 2 * nj_list_words(m));
    rtc_njoin* out = d_joins + c.merge_off;
    hipLaunchKernelGGL(nj_grid_init_kernel, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, (const double*)D, c.ld, m, R, act[0]);
    RTC_CHECK_LAUNCH(ctx);
    int w = 0;
    const uint32_t cap = nj_scan_blocks(ctx);
    for (uint32_t r = m; r > 3; r--, w ^= 1) {
      const uint32_t nb = std::min<uint32_t>((r - 1 + 3) / 4, cap);
      hipLaunchKernelGGL(nj_grid_scan_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const double*)D, c.ld, (const uint32_t*)act[w], (const double*)R, r, minima);
      RTC_CHECK_LAUNCH(ctx);
      hipLaunchKernelGGL(nj_grid_join_kernel, dim3((r + 255) / 256), dim3(256), 0, ctx->stream, D, c.ld, (const uint32_t*)act[w], act[w ^ 1], R, r,
                         (const nj_cand*)minima, nb, out + (m - r));
      RTC_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL(nj_grid_last_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double*)D, c.ld, (const uint32_t*)act[w], out + (m - 3));
    RTC_CHECK_LAUNCH(ctx);
  }
  h_out.resize(n_rec);
  if (n_rec) RTC_HIP(ctx, hipMemcpyAsync(h_out.data(), d_joins, n_rec * sizeof(rtc_njoin), hipMemcpyDeviceToHost, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RTC_OK;
}

// keys -> distances in place, rows [r0, r1) of every block on one thread; the diagonal, which the fill leaves alone, becomes 0
void nj_distances(uint64_t* cells, const std::vector<rtc_kb_comp>& comps, int kmer_size, int threads) {
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
        for (uint32_t j = 0; j < c.m; j++) {
          const uint32_t common = (uint32_t)row[j], denom = (uint32_t)(row[j] >> 32);  // rtc_lkey {common, denom}, little endian
          const double d = i == j ? 0.0 : (common == 0 || denom == 0) ? 1.0 : rtc_linkage_distance(common, denom, kmer_size);
          memcpy(&row[j], &d, 8);
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

}  // namespace

extern "C" int rtc_nj_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->nj[i];
  return RTC_OK;
}

extern "C" int rtc_nj_last_path(const rtc_ctx* ctx) { return ctx ? ctx->nj_path : 0; }

extern "C" int rtc_nj_scan_blocks(const rtc_ctx* ctx) { return ctx ? (int)nj_scan_blocks(ctx) : 0; }

extern "C" int rtc_nj_dev(rtc_ctx* ctx, uint32_t m, double* d_dist, uint64_t ld, rtc_njoin* h_joins, uint32_t* h_n_joins) {
  if (!ctx || !h_n_joins) return RTC_ERR_ARG;
  *h_n_joins = 0;
  if (m >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_nj_dev: m must be below 2^31 - 1");
  for (int i = 0; i < 10; i++) ctx->nj[i] = 0;
  ctx->nj_path = 0;
  if (!d_dist || !h_joins) return RTC_ERR_ARG;
  if (((uintptr_t)d_dist & 7) != 0) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_nj_dev: d_dist must be 8-byte aligned");
  if (ld < m) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_nj_dev: ld smaller than m");
  if (m < 2) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t t0 = nj_now_ns();
  std::vector<rtc_kb_comp> comps(1);
  comps[0] = rtc_kb_comp{0, ld, 0, 0, m, 0};
  std::vector<rtc_njoin> out;
  uint64_t n_path[3];
  RTC_TRY(nj_join(ctx, d_dist, comps, out, n_path));
  memcpy(h_joins, out.data(), out.size() * sizeof(rtc_njoin));
  *h_n_joins = (uint32_t)out.size();
  const uint64_t t1 = nj_now_ns();
  uint64_t* C = ctx->nj;
  C[0] = 1; C[1] = n_path[0]; C[2] = n_path[1]; C[3] = n_path[2]; C[4] = out.size(); C[5] = 1; C[8] = t1 - t0; C[9] = t1 - t0;
  ctx->nj_path = (n_path[0] ? 1 : 0) | (n_path[1] ? 2 : 0) | (n_path[2] ? 4 : 0);
  return RTC_OK;
}

int rtc_nj_join(rtc_ctx* ctx, double* d_dist, std::vector<rtc_kb_comp>& comps, std::vector<rtc_njoin>& h_out, uint64_t n_path[3]) {
  return nj_join(ctx, d_dist, comps, h_out, n_path);
}

extern "C" int rtc_nj_clusters(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                               const uint32_t* h_comp, int kmer_size, rtc_njoin* h_joins, uint64_t cap, uint64_t* h_n_joins, uint64_t* h_first) {
  return rtc_nj_clusters_impl(ctx, "rtc_nj_clusters", d_hashes, width, d_start, d_len, n, h_comp, kmer_size, h_joins, cap, h_n_joins, h_first, 0, nullptr);
}

int rtc_nj_clusters_impl(rtc_ctx* ctx, const char* who, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len,
                         uint32_t n, const uint32_t* h_comp, int kmer_size, rtc_njoin* h_joins, uint64_t cap, uint64_t* h_n_joins,
                         uint64_t* h_first, uint32_t spare_copies, const rtc_nj_hook* hook) {
  if (!ctx || !h_n_joins || !h_first) return RTC_ERR_ARG;
  *h_n_joins = 0;
  h_first[0] = 0;
  if (width != 4 && width != 8) return rtc_fail(ctx, RTC_ERR_ARG, "width must be 4 or 8");
  if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: kmer_size must be at least 1", who);
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: n must be below 2^31 - 1", who);
  if (cap && !h_joins) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) ctx->nj[i] = 0;
  ctx->nj_path = 0;
  if (n == 0) return RTC_OK;
  if (!d_start || !d_len || !h_comp) return RTC_ERR_ARG;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t t0 = nj_now_ns();
  uint64_t* C = ctx->nj;
  uint64_t total = 0;
  bool overflow = false;
  std::vector<uint64_t> cells;
  RTC_TRY(rtc_key_blocks(ctx, who, ctx->opt.nj_bytes, d_hashes, width, d_start, d_len, n, h_comp, h_first, [&](const rtc_kb_batch& b) -> int {
    std::vector<rtc_kb_comp>& comps = *b.comps;
    std::vector<rtc_njoin> out;
    if (b.d_keys) {
      C[5]++;
      C[6] += b.fill_ns;
      // the keys to the host, the distances back into the same cells
      const uint64_t td0 = nj_now_ns();
      cells.resize(b.n_keys);
      RTC_HIP(ctx, hipMemcpyAsync(cells.data(), b.d_keys, b.n_keys * 8, hipMemcpyDeviceToHost, ctx->stream));
      RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
      nj_distances(cells.data(), comps, kmer_size, ctx->host_threads);
      RTC_HIP(ctx, hipMemcpyAsync(b.d_keys, cells.data(), b.n_keys * 8, hipMemcpyHostToDevice, ctx->stream));
      RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
      const uint64_t td1 = nj_now_ns();
      C[7] += td1 - td0;
      uint64_t n_path[3];
      RTC_TRY(nj_join(ctx, (double*)b.d_keys, comps, out, n_path));
      C[8] += nj_now_ns() - td1;
      for (int p = 0; p < 3; p++) { C[1 + p] += n_path[p]; if (n_path[p]) ctx->nj_path |= 1 << p; }
      if (hook) RTC_TRY((*hook)(b, comps, out, total));
    }
    // the records in component order, local indices turned into genome indices
    const std::vector<uint32_t>&csize = *b.csize, &cfirst = *b.cfirst, &perm = *b.perm;
    size_t i = 0;
    for (size_t q = b.c; q < b.ce; q++) {
      if (csize[q] >= 2) {
        const rtc_kb_comp& cp = comps[i];
        const uint64_t nr = nj_records_of(cp.m);
        C[0]++;
        C[4] += nr;
        if (total + nr > cap) overflow = true;
        if (!overflow)
          for (uint64_t e = 0; e < nr; e++) {
            rtc_njoin r = out[cp.merge_off + e];
            r.a = perm[cfirst[q] + r.a];
            r.b = perm[cfirst[q] + r.b];
            if (r.c != NJ_NONE) r.c = perm[cfirst[q] + r.c];
            h_joins[total + e] = r;
          }
        total += nr;
        i++;
      }
      h_first[q + 1] = total;
    }
    return RTC_OK;
  }, spare_copies));
  *h_n_joins = total;
  C[9] = nj_now_ns() - t0;
  if (overflow) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "%s: %llu records, room for %llu", who, (unsigned long long)total, (unsigned long long)cap);
  return RTC_OK;
}
