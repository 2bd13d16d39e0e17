// rtc_upgma.hip -- clust-mst --upgma: average linkage (UPGMA) of the clusters on the device, in exact integers.
//
// The definition is in include/rtclust.h (tests/refupgma.py restates it).  A candidate is (S, n_a n_b, a, b); two candidates are
// ordered by the mean S / (n_a n_b), compared as 128-bit cross products, then by a, then by b.  That order is total, so neither
// the path nor the way the search is split over lanes, waves or workgroups changes a record.  Every step scans all active pairs:
// there is no cached best partner to keep right under ties, and nothing to rescan.
//
//   wave path       m <= 64: one wave per component, S and the sizes in LDS, lane x owns cluster x and scans the pairs (x, y), y > x
//   workgroup path  one 256-lane workgroup per component, S in global memory, sizes and the active list in a global scratch; the
//                   whole dendrogram in one launch
//   grid path       m >= RTC_UPGMA_GRID_MIN: one component on the whole device; a scan launch leaves one minimum per workgroup, a
//                   merge launch reduces them, adds row b into row a and column a, retires b and appends the record.  The 2 (m - 1)
//                   launches are enqueued back to back; the launch boundary is the only device-wide barrier
// The workgroup and grid paths keep the active clusters as an ascending list, rewritten (one entry dropped) into its twin at
// every merge, as rtc_nj.hip does.  Both triangles of S are kept in step.  No sums from different lanes meet: every cell has one
// writer a step, so there is no atomic.
#include <time.h>

#include <algorithm>
#include <numeric>
#include <thread>
#include <vector>

#include "rtc_internal.h"
#include "rtc_upgma.h"

namespace {

typedef unsigned __int128 u128;
constexpr uint32_t UP_NONE = 0xFFFFFFFFu;

struct up_cand { uint64_t s, p; uint32_t a, b; };  // sum, n_a n_b, the pair

// the order of a step's choice: mean ascending (s_x p_y against s_y p_x; s < 2^62, p < 2^44), then a ascending, then b ascending
__device__ __forceinline__ bool up_better(const up_cand& x, const up_cand& y) {
  const u128 l = (u128)x.s * y.p, r = (u128)y.s * x.p;
  return l < r || (l == r && (x.a < y.a || (x.a == y.a && x.b < y.b)));
}
// behind every real candidate: a real s is below 2^62
__device__ __forceinline__ up_cand up_none() { return up_cand{~0ull, 1ull, UP_NONE, UP_NONE}; }
__device__ __forceinline__ up_cand up_wave_best(up_cand v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    up_cand o;
    o.s = (uint64_t)__shfl_xor((unsigned long long)v.s, off); o.p = (uint64_t)__shfl_xor((unsigned long long)v.p, off);
    o.a = __shfl_xor(v.a, off); o.b = __shfl_xor(v.b, off);
    if (up_better(o, v)) v = o;
  }
  return v;
}
// the best of a 256-lane workgroup, the same in every lane; s_best is free again after the caller's next barrier
__device__ __forceinline__ up_cand up_block_best(up_cand v, up_cand* s_best, uint32_t lane, uint32_t wave) {
  v = up_wave_best(v);
  if (lane == 0) s_best[wave] = v;
  __syncthreads();
  v = s_best[0];
  for (int w = 1; w < 4; w++) { const up_cand o = s_best[w]; if (up_better(o, v)) v = o; }
  return v;
}

// steps 2 and 4 -- one lane; N[v.a] and N[v.b] are read by nobody else between the scan and the next barrier
__device__ __forceinline__ void up_emit(uint32_t* N, const up_cand& v, rtc_umerge* out) {
  const uint32_t na = N[v.a], nb = N[v.b];
  *out = rtc_umerge{v.a, v.b, na, nb, v.s};
  N[v.a] = na + nb;
}

// ---- wave path --------------------------------------------------------------------------------------------------------------
// LDS: K[y * lds + x], lds = m | 1, then the sizes N[m].  The active set is a 64-bit mask, the same in every lane.
__global__ __launch_bounds__(64) void upgma_wave_kernel(const uint64_t* __restrict__ sums, const rtc_kb_comp* __restrict__ comps,
                                                        const uint32_t* __restrict__ w, rtc_umerge* __restrict__ merges) {
  extern __shared__ uint64_t up_lds[];
  const rtc_kb_comp cp = comps[blockIdx.x];
  const uint32_t m = cp.m, x = threadIdx.x, lds = m | 1;
  uint64_t* K = up_lds;
  uint32_t* N = (uint32_t*)(up_lds + (size_t)m * lds);
  const uint64_t* g = sums + cp.key_off;
  rtc_umerge* out = merges + cp.merge_off;
  if (x < m) {
    for (uint32_t y = 0; y < m; y++) K[y * lds + x] = g[(uint64_t)y * cp.ld + x];
    N[x] = w ? w[x] : 1u;
  }
  __syncthreads();
  unsigned long long mask = m == 64 ? ~0ull : (1ull << m) - 1;
  for (uint32_t nrec = 0; nrec + 1 < m; nrec++) {
    const bool active = (mask >> x) & 1;
    up_cand v = up_none();
    if (active) {
      const uint64_t nx = N[x];
      for (unsigned long long mm = mask & ~((2ull << x) - 1); mm; mm &= mm - 1) {  // the live y above x, ascending
        const uint32_t y = (uint32_t)__ffsll((long long)mm) - 1;
        const up_cand c{K[x * lds + y], nx * N[y], x, y};
        if (up_better(c, v)) v = c;
      }
    }
    v = up_wave_best(v);
    const uint32_t a = v.a, b = v.b;
    if (a == UP_NONE) return;  // no pair: cannot happen while two clusters are active, and nothing may be indexed by it (every lane sees the same)
    if (active && x != a && x != b) {
      const uint64_t s = K[a * lds + x] + K[b * lds + x];
      K[a * lds + x] = s;
      K[x * lds + a] = s;
    }
    if (x == 0) up_emit(N, v, out + nrec);
    __syncthreads();
    mask &= ~(1ull << b);
  }
}

// ---- workgroup and grid paths -----------------------------------------------------------------------------------------------
// The least candidate over the rows row0, row0 + step, ... of the active list act[0 .. r), one wave a row, lanes striding its
// columns above the row's own position.  Four loads in flight a lane.
__device__ __forceinline__ up_cand up_scan(const uint64_t* S, uint64_t ld, const uint32_t* act, const uint32_t* N, uint32_t r, uint32_t row0,
                                           uint32_t step, uint32_t lane) {
  up_cand v = up_none();
  for (uint32_t p = row0; p + 1 < r; p += step) {
    const uint32_t a = act[p];
    const uint64_t na = N[a];
    const uint64_t* row = S + (uint64_t)a * ld;
    for (uint32_t q0 = p + 1 + lane; q0 < r; q0 += 256) {
      uint32_t b[4];
      uint64_t s[4], nb[4];
#pragma unroll
      for (int u = 0; u < 4; u++) b[u] = q0 + 64 * u < r ? act[q0 + 64 * u] : UP_NONE;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        s[u] = b[u] != UP_NONE ? row[b[u]] : 0;
        nb[u] = b[u] != UP_NONE ? N[b[u]] : 1;
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (b[u] != UP_NONE) {
          const up_cand c{s[u], na * nb[u], a, b[u]};
          if (up_better(c, v)) v = c;
        }
    }
  }
  return v;
}

// step 3 for the cluster at position p of the active list, and its place in the next list (ascending: those above b move down one)
__device__ __forceinline__ void up_update_point(uint64_t* S, uint64_t ld, const uint32_t* cur, uint32_t* nxt, uint32_t p, uint32_t a, uint32_t b) {
  const uint32_t k = cur[p];
  if (k == b) return;
  nxt[p - (k > b ? 1u : 0u)] = k;
  if (k == a) return;
  const uint64_t s = S[(uint64_t)a * ld + k] + S[(uint64_t)b * ld + k];
  S[(uint64_t)a * ld + k] = s;
  S[(uint64_t)k * ld + a] = s;
}

// scratch of a component, in 8-byte words from scratch_off: the sizes and the two active lists (m u32 each, m rounded up to
// even), then -- grid path -- the scan's minima
__device__ __host__ __forceinline__ uint64_t up_list_words(uint32_t m) { return ((uint64_t)m + 1) / 2; }
constexpr uint64_t UP_CAND_WORDS = sizeof(up_cand) / 8;
static_assert(sizeof(up_cand) == 24, "up_cand is three 8-byte words");

__global__ __launch_bounds__(256) void upgma_wg_kernel(uint64_t* sums, const rtc_kb_comp* __restrict__ comps, const uint32_t* __restrict__ w,
                                                       rtc_umerge* __restrict__ merges, uint64_t* scratch) {
  __shared__ up_cand s_best[4];
  const rtc_kb_comp cp = comps[blockIdx.x];
  const uint32_t m = cp.m, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t ld = cp.ld, lw = up_list_words(m);
  uint64_t* S = sums + cp.key_off;
  uint32_t* N = (uint32_t*)(scratch + cp.scratch_off);
  uint32_t* cur = (uint32_t*)(scratch + cp.scratch_off + lw);
  uint32_t* nxt = (uint32_t*)(scratch + cp.scratch_off + 2 * lw);
  rtc_umerge* out = merges + cp.merge_off;
  for (uint32_t x = tid; x < m; x += 256) { N[x] = w ? w[x] : 1u; cur[x] = x; }
  __syncthreads();
  for (uint32_t r = m; r > 1; r--) {
    const up_cand v = up_block_best(up_scan(S, ld, cur, N, r, wave, 4, lane), s_best, lane, wave);
    if (v.a == UP_NONE) return;  // no pair: cannot happen while two clusters are active, and nothing may be indexed by it (every lane sees the same)
    for (uint32_t p = tid; p < r; p += 256) up_update_point(S, ld, cur, nxt, p, v.a, v.b);
    if (tid == 0) up_emit(N, v, out + (m - r));
    __syncthreads();
    uint32_t* t = cur; cur = nxt; nxt = t;
  }
}

__global__ __launch_bounds__(256) void upgma_grid_init_kernel(uint32_t m, const uint32_t* __restrict__ w, uint32_t* __restrict__ N,
                                                              uint32_t* __restrict__ act) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x < m) { N[x] = w ? w[x] : 1u; act[x] = x; }
}

__global__ __launch_bounds__(256) void upgma_grid_scan_kernel(const uint64_t* __restrict__ S, uint64_t ld, const uint32_t* __restrict__ act,
                                                              const uint32_t* __restrict__ N, uint32_t r, up_cand* __restrict__ minima) {
  __shared__ up_cand s_best[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const up_cand v = up_block_best(up_scan(S, ld, act, N, r, blockIdx.x * 4 + wave, gridDim.x * 4, lane), s_best, lane, wave);
  if (tid == 0) minima[blockIdx.x] = v;
}

// Every workgroup reduces the scan's minima for itself and updates the 256 clusters at its positions of the list; the first one
// also writes the record and the new size.  No workgroup reads what another writes: a cell S[a][k], S[k][a] belongs to the lane
// that holds k, the sizes are the first workgroup's alone, and the next scan starts at the launch boundary.
__global__ __launch_bounds__(256) void upgma_grid_merge_kernel(uint64_t* S, uint64_t ld, const uint32_t* __restrict__ cur, uint32_t* __restrict__ nxt,
                                                               uint32_t* N, uint32_t r, const up_cand* __restrict__ minima, uint32_t n_minima,
                                                               rtc_umerge* __restrict__ out) {
  __shared__ up_cand s_best[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  up_cand v = up_none();
  for (uint32_t b = tid; b < n_minima; b += 256) { const up_cand o = minima[b]; if (up_better(o, v)) v = o; }
  v = up_block_best(v, s_best, lane, wave);
  if (v.a == UP_NONE) return;  // no pair: cannot happen while two clusters are active, and nothing may be indexed by it
  const uint32_t p = blockIdx.x * 256 + tid;
  if (p < r) up_update_point(S, ld, cur, nxt, p, v.a, v.b);
  if (blockIdx.x == 0 && tid == 0) up_emit(N, v, out);
}

uint64_t up_now_ns() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

// device buffers of one call, released on every way out
struct up_bufs {
  std::vector<void*> p;
  ~up_bufs() { for (void* q : p) (void)hipFree(q); }
  int get(rtc_ctx* ctx, size_t bytes, void** out) {
    ctx->free_hbm_at = -1.0;
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e != hipSuccess) { (void)hipGetLastError(); return rtc_fail(ctx, RTC_ERR_NOMEM, "rtc_upgma: hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
    p.push_back(*out);
    return RTC_OK;
  }
};

inline uint32_t up_grid_min(const rtc_ctx* ctx) { return ctx->opt.upgma_grid_min ? std::max<uint32_t>(ctx->opt.upgma_grid_min, 4) : UPGMA_GRID_MIN; }
// the most workgroups of a scan launch: RTC_UPGMA_SCAN_BLOCKS below the ceiling the scratch reserves (tests reach a second row per workgroup with it)
inline uint32_t up_scan_blocks(const rtc_ctx* ctx) { return ctx->opt.upgma_scan_blocks ? std::min<uint32_t>(ctx->opt.upgma_scan_blocks, UPGMA_SCAN_BLOCKS) : UPGMA_SCAN_BLOCKS; }
// 0 wave, 1 workgroup, 2 grid
inline int up_path_of(const rtc_ctx* ctx, uint32_t m) { return m >= up_grid_min(ctx) ? 2 : m <= UPGMA_WAVE_MAX ? 0 : 1; }

// Agglomerates comps[0 .. nc) (each m >= 2) over the matrices in d_sum: one launch for the wave-path components, one for the
// workgroup-path ones, the launch chain of every grid-path one; then the records come back, laid out by merge_off (set here).
// d_w: the sizes of the one component of rtc_upgma_dev, or NULL (all 1).  n_path[3]: the components of each path.
int up_agglomerate(rtc_ctx* ctx, uint64_t* d_sum, std::vector<rtc_kb_comp>& comps, const uint32_t* d_w, std::vector<rtc_umerge>& h_out,
                   uint64_t n_path[3]) {
  const size_t nc = comps.size();
  h_out.clear();
  n_path[0] = n_path[1] = n_path[2] = 0;
  if (!nc) return RTC_OK;
  std::vector<uint32_t> order(nc);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return up_path_of(ctx, comps[x].m) < up_path_of(ctx, comps[y].m); });
  uint64_t n_rec = 0, n_scratch = 0;
  uint32_t m_wave = 0;
  std::vector<rtc_kb_comp> sorted(nc);
  for (size_t s = 0; s < nc; s++) {
    rtc_kb_comp& c = comps[order[s]];
    const int path = up_path_of(ctx, c.m);
    n_path[path]++;
    c.merge_off = n_rec;
    n_rec += c.m - 1;
    if (path == 0) m_wave = std::max(m_wave, c.m);
    else {
      c.scratch_off = n_scratch;
      n_scratch += 3 * up_list_words(c.m) + (path == 2 ? (uint64_t)UPGMA_SCAN_BLOCKS * UP_CAND_WORDS : 0);
    }
    sorted[s] = c;
  }
  up_bufs B;
  rtc_kb_comp* d_comps = nullptr;
  rtc_umerge* d_merges = nullptr;
  uint64_t* d_scratch = nullptr;
  RTC_TRY(B.get(ctx, nc * sizeof(rtc_kb_comp), (void**)&d_comps));
  RTC_TRY(B.get(ctx, n_rec * sizeof(rtc_umerge), (void**)&d_merges));
  RTC_TRY(B.get(ctx, n_scratch * 8, (void**)&d_scratch));
  RTC_HIP(ctx, hipMemcpyAsync(d_comps, sorted.data(), nc * sizeof(rtc_kb_comp), hipMemcpyHostToDevice, ctx->stream));
  if (n_path[0]) {
    const size_t lds = (size_t)m_wave * (m_wave | 1) * 8 + (size_t)m_wave * 4;
    hipLaunchKernelGGL(upgma_wave_kernel, dim3((uint32_t)n_path[0]), dim3(64), lds, ctx->stream, (const uint64_t*)d_sum, (const rtc_kb_comp*)d_comps, d_w,
                       d_merges);
    RTC_CHECK_LAUNCH(ctx);
  }
  if (n_path[1]) {
    hipLaunchKernelGGL(upgma_wg_kernel, dim3((uint32_t)n_path[1]), dim3(256), 0, ctx->stream, d_sum, (const rtc_kb_comp*)(d_comps + n_path[0]), d_w,
                       d_merges, d_scratch);
    RTC_CHECK_LAUNCH(ctx);
  }
  for (size_t s = n_path[0] + n_path[1]; s < nc; s++) {
    const rtc_kb_comp& c = sorted[s];
    const uint32_t m = c.m;  // >= 4
    const uint64_t lw = up_list_words(m);
    uint64_t* S = d_sum + c.key_off;
    uint32_t* N = (uint32_t*)(d_scratch + c.scratch_off);
    uint32_t* act[2] = {(uint32_t*)(d_scratch + c.scratch_off + lw), (uint32_t*)(d_scratch + c.scratch_off + 2 * lw)};
    up_cand* minima = (up_cand*)(d_scratch + c.scratch_off + 3 * lw);
    rtc_umerge* out = d_merges + c.merge_off;
    hipLaunchKernelGGL(upgma_grid_init_kernel, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, m, d_w, N, act[0]);
    RTC_CHECK_LAUNCH(ctx);
    int t = 0;
    const uint32_t cap = up_scan_blocks(ctx);
    for (uint32_t r = m; r > 1; r--, t ^= 1) {
      const uint32_t nb = std::min<uint32_t>((r - 1 + 3) / 4, cap);
      hipLaunchKernelGGL(upgma_grid_scan_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const uint64_t*)S, c.ld, (const uint32_t*)act[t], (const uint32_t*)N, r,
                         minima);
      RTC_CHECK_LAUNCH(ctx);
      hipLaunchKernelGGL(upgma_grid_merge_kernel, dim3((r + 255) / 256), dim3(256), 0, ctx->stream, S, c.ld, (const uint32_t*)act[t], act[t ^ 1], N, r,
                         (const up_cand*)minima, nb, out + (m - r));
      RTC_CHECK_LAUNCH(ctx);
    }
  }
  h_out.resize(n_rec);
  if (n_rec) RTC_HIP(ctx, hipMemcpyAsync(h_out.data(), d_merges, n_rec * sizeof(rtc_umerge), hipMemcpyDeviceToHost, ctx->stream));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RTC_OK;
}

// keys -> q in place, rows [r0, r1) of every block on one thread; the diagonal, which the fill leaves alone, becomes 0
void up_distances(uint64_t* cells, const std::vector<rtc_kb_comp>& comps, int kmer_size, int threads) {
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
          long long q = 0;
          if (i != j) {
            q = (common == 0 || denom == 0) ? (long long)UPGMA_Q1 : llround(rtc_linkage_distance(common, denom, kmer_size) * 1048576.0);
            q = std::min<long long>((long long)UPGMA_Q1, std::max<long long>(q, 0));
          }
          row[j] = (uint64_t)q;
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

extern "C" int rtc_upgma_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->upgma[i];
  return RTC_OK;
}

extern "C" int rtc_upgma_last_path(const rtc_ctx* ctx) { return ctx ? ctx->upgma_path : 0; }

extern "C" int rtc_upgma_scan_blocks(const rtc_ctx* ctx) { return ctx ? (int)up_scan_blocks(ctx) : 0; }

extern "C" double rtc_upgma_distance(uint64_t sum, uint32_t size_a, uint32_t size_b) {
  const double pairs = (double)size_a * (double)size_b;
  const double scale = pairs * 1048576.0;
  return (double)sum / scale;
}

extern "C" int rtc_upgma_dev(rtc_ctx* ctx, uint32_t m, uint64_t* d_sum, uint64_t ld, const uint32_t* h_size, rtc_umerge* h_merges) {
  if (!ctx) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) ctx->upgma[i] = 0;
  ctx->upgma_path = 0;
  if (!d_sum || !h_merges) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_dev: d_sum and h_merges must not be NULL");
  if (((uintptr_t)d_sum & 7) != 0) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_dev: d_sum must be 8-byte aligned");
  if (ld < m) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_dev: ld smaller than m");
  uint64_t W = m;
  if (h_size) {
    W = 0;
    for (uint32_t i = 0; i < m; i++) {
      if (h_size[i] == 0) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_dev: h_size[%u] is 0", i);
      W += h_size[i];
    }
  }
  if (W >= UPGMA_W_MAX) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_dev: the sizes sum to %llu, must be below 2^22", (unsigned long long)W);
  if (m < 2) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t t0 = up_now_ns();
  up_bufs B;
  uint32_t* d_w = nullptr;
  if (h_size) {
    RTC_TRY(B.get(ctx, (size_t)m * 4, (void**)&d_w));
    RTC_HIP(ctx, hipMemcpyAsync(d_w, h_size, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  std::vector<rtc_kb_comp> comps(1);
  comps[0] = rtc_kb_comp{0, ld, 0, 0, m, 0};
  std::vector<rtc_umerge> out;
  uint64_t n_path[3];
  RTC_TRY(up_agglomerate(ctx, d_sum, comps, d_w, out, n_path));
  memcpy(h_merges, out.data(), out.size() * sizeof(rtc_umerge));
  const uint64_t t1 = up_now_ns();
  uint64_t* C = ctx->upgma;
  C[0] = 1; C[1] = n_path[0]; C[2] = n_path[1]; C[3] = n_path[2]; C[4] = out.size(); C[8] = t1 - t0; C[9] = t1 - t0;
  ctx->upgma_path = (n_path[0] ? 1 : 0) | (n_path[1] ? 2 : 0) | (n_path[2] ? 4 : 0);
  return RTC_OK;
}

extern "C" int rtc_upgma_clusters(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                  const uint32_t* h_comp, int kmer_size, rtc_umerge* h_merges, uint64_t cap, uint64_t* h_n_merges, uint64_t* h_first) {
  if (!ctx || !h_n_merges || !h_first) return RTC_ERR_ARG;
  *h_n_merges = 0;
  h_first[0] = 0;
  if (width != 4 && width != 8) return rtc_fail(ctx, RTC_ERR_ARG, "width must be 4 or 8");
  if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_clusters: kmer_size must be at least 1");
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_clusters: n must be below 2^31 - 1");
  if (cap && !h_merges) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) ctx->upgma[i] = 0;
  ctx->upgma_path = 0;
  if (n == 0) return RTC_OK;
  if (!d_start || !d_len || !h_comp) return RTC_ERR_ARG;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t t0 = up_now_ns();
  uint64_t* C = ctx->upgma;
  uint64_t total = 0;
  bool overflow = false;
  std::vector<uint64_t> cells;
  RTC_TRY(rtc_key_blocks(ctx, "rtc_upgma_clusters", ctx->opt.upgma_bytes, d_hashes, width, d_start, d_len, n, h_comp, h_first, [&](const rtc_kb_batch& b) -> int {
    std::vector<rtc_kb_comp>& comps = *b.comps;
    std::vector<rtc_umerge> out;
    if (b.d_keys) {
      C[6] += b.fill_ns;
      for (const rtc_kb_comp& c : comps)  // all sizes are 1: W is m.  8 m^2 bytes run out long before, so this does not happen
        if (c.m >= UPGMA_W_MAX) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_upgma_clusters: a component of %u members, must be below 2^22", c.m);
      // the keys to the host, the q back into the same cells
      const uint64_t td0 = up_now_ns();
      cells.resize(b.n_keys);
      RTC_HIP(ctx, hipMemcpyAsync(cells.data(), b.d_keys, b.n_keys * 8, hipMemcpyDeviceToHost, ctx->stream));
      RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
      up_distances(cells.data(), comps, kmer_size, ctx->host_threads);
      RTC_HIP(ctx, hipMemcpyAsync(b.d_keys, cells.data(), b.n_keys * 8, hipMemcpyHostToDevice, ctx->stream));
      RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
      const uint64_t td1 = up_now_ns();
      C[7] += td1 - td0;
      uint64_t n_path[3];
      RTC_TRY(up_agglomerate(ctx, (uint64_t*)b.d_keys, comps, nullptr, out, n_path));
      C[8] += up_now_ns() - td1;
      for (int p = 0; p < 3; p++) { C[1 + p] += n_path[p]; if (n_path[p]) ctx->upgma_path |= 1 << p; }
    }
    // the records in component order, local indices turned into genome indices
    const std::vector<uint32_t>&csize = *b.csize, &cfirst = *b.cfirst, &perm = *b.perm;
    size_t i = 0;
    for (size_t q = b.c; q < b.ce; q++) {
      if (csize[q] >= 2) {
        const rtc_kb_comp& cp = comps[i];
        const uint64_t nr = cp.m - 1;
        C[0]++;
        C[4] += nr;
        if (total + nr > cap) overflow = true;
        if (!overflow)
          for (uint64_t e = 0; e < nr; e++) {
            rtc_umerge r = out[cp.merge_off + e];
            r.a = perm[cfirst[q] + r.a];
            r.b = perm[cfirst[q] + r.b];
            h_merges[total + e] = r;
          }
        total += nr;
        i++;
      }
      h_first[q + 1] = total;
    }
    return RTC_OK;
  }));
  *h_n_merges = total;
  C[9] = up_now_ns() - t0;
  if (overflow) return rtc_fail(ctx, RTC_ERR_OVERFLOW, "rtc_upgma_clusters: %llu records, room for %llu", (unsigned long long)total, (unsigned long long)cap);
  return RTC_OK;
}
