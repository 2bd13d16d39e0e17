// rtc_snn.hip -- rtc_graph_snn: the shared-neighbour counts of clust-leiden --snn (include/rtclust.h holds the definition,
// tests/refsnn.py restates it).
//   * The adjacency: every record with u != v gives the keys u << 32 | v and v << 32 | u (a record with u == v two keys of all
//     ones, which sort behind every row and are never read); one radix sort, one unique pass, the row offsets as
//     louvain_rows_kernel finds them, then the low words alone as the rows: ascending lists of distinct neighbours.
//   * snn_owner_kernel gives every record its owner -- the end with the longer row, the lower index on equal lengths, so a
//     record, its reverse and its duplicates have one owner -- and the path of the owner's row (rtc_snn.h).  One radix sort by
//     (path, owner) groups the records: the paths lie one behind the other, and inside a path the records of an owner are a run.
//   * snn_count_kernel is the hot path.  A workgroup takes a slice of as many sorted records as it has lanes; lane t reads
//     record t's ends and the other end's row bounds, so the dependent loads of a slice run side by side.  Then run by run: the
//     owner's row is staged into LDS once for the whole run, and every record of the run goes to one wave, whose lanes stride
//     over the other end's row (the shorter one), look each element up in the owner's row by binary search and count the hits
//     with __ballot and __popcll.  A record's count is formed in one wave's registers: no atomics on it.  Three launches share
//     the code:
//       - the owner's row of at most SNN_WAVE_ROW entries: a workgroup of ONE wave, the row in LDS;
//       - of at most SNN_BLOCK_ROW entries: 256 lanes, the row in LDS, a run's records dealt to the four waves;
//       - beyond: 256 lanes, the row searched where it lies in global memory.
//     A hub that owns more records than a slice holds is spread over as many workgroups as its records fill slices, each of
//     which stages the row again: a row is at most 32 KiB, read from L2 after the first, against 64 or 256 records' probes.
//   * The triangles are the sum of shared over DISTINCT edges: the wave that counts a record finds the other end's place in the
//     owner's row (one more search) and raises that entry's flag with an atomic exchange; the record that finds it down adds its
//     count.  The owner is a function of the edge, so every duplicate meets the same flag.
#include "rtc_community.h"
#include "rtc_snn.h"

namespace {

// the state words of a call on the device
enum { SNN_PATH0 = 0, SNN_PROBES = 3, SNN_SHARED_SUM = 4, SNN_UNIQUE = 5, SNN_STATE_WORDS = 8 };
constexpr uint64_t SNN_NO_KEY = ~0ull;
constexpr uint32_t SNN_OWNER_IS_U = 0x80000000u;  // beside the other end's row length, which is below 2^31

static_assert(SNN_WAVE_ROW * 4 + 64 * SNN_SLICE_BYTES + 8 <= 160 * 1024 / SNN_WAVE_WGS_PER_CU, "the wave path's LDS for its residency");
static_assert(SNN_BLOCK_ROW * 4 + 256 * SNN_SLICE_BYTES + 32 <= 160 * 1024 / SNN_BLOCK_WGS_PER_CU, "the workgroup path's LDS for its residency");

__global__ __launch_bounds__(256) void snn_keys_kernel(const rtc_wedge* __restrict__ edges, uint64_t m, uint64_t* __restrict__ key) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_wedge r = edges[e];
    const bool loop = r.u == r.v;
    key[2 * e] = loop ? SNN_NO_KEY : ((uint64_t)r.u << 32) | r.v;
    key[2 * e + 1] = loop ? SNN_NO_KEY : ((uint64_t)r.v << 32) | r.u;
  }
}
__global__ __launch_bounds__(256) void snn_adj_kernel(const uint64_t* __restrict__ key, uint64_t E, uint32_t* __restrict__ adj) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (uint64_t)gridDim.x * blockDim.x) adj[e] = (uint32_t)key[e];
}

// Record e's sort key path << 32 | owner and its index as the value; a record with u == v is written here (path 3: behind
// the three lists).  state: the records of each path and the probes, one atomic per workgroup and word.
__global__ __launch_bounds__(256) void snn_owner_kernel(const rtc_wedge* __restrict__ edges, uint64_t m, const uint64_t* __restrict__ row_off,
                                                        int all_global, uint64_t* __restrict__ okey, uint64_t* __restrict__ oval,
                                                        rtc_snn* __restrict__ out, unsigned long long* __restrict__ state) {
  unsigned long long c[3] = {0, 0, 0}, probes = 0;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_wedge r = edges[e];
    const uint32_t du = (uint32_t)(row_off[r.u + 1] - row_off[r.u]), dv = (uint32_t)(row_off[r.v + 1] - row_off[r.v]);
    oval[e] = e;
    if (r.u == r.v) {
      okey[e] = (3ull << 32) | r.u;
      out[e] = rtc_snn{0u, du, dv, 1u};
      continue;
    }
    const bool u_owns = du > dv || (du == dv && r.u < r.v);
    const uint32_t longer = u_owns ? du : dv;
    const uint32_t p = all_global ? 2u : longer <= SNN_WAVE_ROW ? 0u : longer <= SNN_BLOCK_ROW ? 1u : 2u;
    okey[e] = ((uint64_t)p << 32) | (u_owns ? r.u : r.v);
    c[0] += p == 0; c[1] += p == 1; c[2] += p == 2;
    probes += u_owns ? dv : du;
  }
  // the four sums over the workgroup, then one atomic a word: every workgroup adds to the same four words
  __shared__ unsigned long long s_red[4][4];
  for (int off = 32; off; off >>= 1) {
    for (int p = 0; p < 3; p++) c[p] += __shfl_xor(c[p], off);
    probes += __shfl_xor(probes, off);
  }
  if ((threadIdx.x & 63) == 0) {
    for (int p = 0; p < 3; p++) s_red[threadIdx.x / 64][p] = c[p];
    s_red[threadIdx.x / 64][3] = probes;
  }
  __syncthreads();
  if (threadIdx.x < 4) {  // SNN_PATH0 + 0 .. 2 and SNN_PROBES are the words 0 .. 3
    const unsigned long long v = s_red[0][threadIdx.x] + s_red[1][threadIdx.x] + s_red[2][threadIdx.x] + s_red[3][threadIdx.x];
    if (v) atomicAdd(&state[threadIdx.x], v);
  }
}

// the first entry of t[0 .. len) that is not below x, len >= 1: as many steps in every lane, whatever x is
__device__ __forceinline__ uint32_t snn_lower_bound(const uint32_t* t, uint32_t len, uint32_t x) {
  uint32_t base = 0;
  while (len > 1) {
    const uint32_t half = len >> 1;
    base += t[base + half - 1] < x ? half : 0u;
    len -= half;
  }
  return base + (t[base] < x ? 1u : 0u);
}

// the first run head at or behind `from` in a slice of cnt records, or cnt
template <int BLOCK>
__device__ __forceinline__ uint32_t snn_next_head(const unsigned long long* heads, uint32_t from, uint32_t cnt) {
  for (uint32_t w = from >> 6; w < BLOCK / 64; w++) {
    unsigned long long mk = heads[w];
    if (w == from >> 6) mk &= ~0ull << (from & 63);
    if (mk) return w * 64 + (uint32_t)__builtin_ctzll(mk);
  }
  return cnt;
}

// The records skey / sidx[base .. base + count) of path `path`, base and count read from state.  ROW > 0: the owner's row is
// staged in LDS, ROW entries at the most (the path's rule); ROW == 0: it is searched in adj.
template <int BLOCK, uint32_t ROW>
__global__ __launch_bounds__(BLOCK) void snn_count_kernel(const uint64_t* __restrict__ skey, const uint64_t* __restrict__ sidx,
                                                          const unsigned long long* __restrict__ state, int path,
                                                          const rtc_wedge* __restrict__ edges, const uint64_t* __restrict__ row_off,
                                                          const uint32_t* __restrict__ adj, uint32_t* __restrict__ seen,
                                                          rtc_snn* __restrict__ out, unsigned long long* __restrict__ shared_sum) {
  __shared__ uint32_t s_row[ROW ? ROW : 1];
  __shared__ uint64_t s_idx[BLOCK], s_ostart[BLOCK];
  __shared__ uint32_t s_owner[BLOCK], s_other[BLOCK], s_olen[BLOCK];
  __shared__ unsigned long long s_head[BLOCK / 64];
  uint64_t base = 0;
  for (int p = 0; p < path; p++) base += state[SNN_PATH0 + p];
  const uint64_t count = state[SNN_PATH0 + path];
  const uint64_t n_slices = (count + BLOCK - 1) / BLOCK;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  unsigned long long sum = 0;  // lane 0's: the counts of the records that were the first of their edge
  for (uint64_t slice = blockIdx.x; slice < n_slices; slice += gridDim.x) {  // uniform over the workgroup: the barriers below are reached by all
    const uint64_t s0 = base + slice * BLOCK;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(BLOCK, count - slice * BLOCK);
    bool head = false;
    if (threadIdx.x < cnt) {
      const uint32_t o = (uint32_t)skey[s0 + threadIdx.x];
      const uint64_t idx = sidx[s0 + threadIdx.x];
      const rtc_wedge r = edges[idx];
      const bool owner_is_u = r.u == o;
      const uint32_t other = owner_is_u ? r.v : r.u;
      const uint64_t a0 = row_off[other];
      s_owner[threadIdx.x] = o;
      s_other[threadIdx.x] = other;
      s_idx[threadIdx.x] = idx;
      s_ostart[threadIdx.x] = a0;
      s_olen[threadIdx.x] = (uint32_t)(row_off[other + 1] - a0) | (owner_is_u ? SNN_OWNER_IS_U : 0u);
      head = threadIdx.x == 0 || (uint32_t)skey[s0 + threadIdx.x - 1] != o;
    }
    const unsigned long long heads = __ballot(head);
    if (lane == 0) s_head[wave] = heads;
    __syncthreads();
    for (uint32_t a = 0; a < cnt;) {  // a run: the records [a, b) of one owner
      const uint32_t b = snn_next_head<BLOCK>(s_head, a + 1, cnt);
      const uint32_t o = s_owner[a];
      const uint64_t r0 = row_off[o];
      const uint32_t len = (uint32_t)(row_off[o + 1] - r0);
      const uint32_t* target = adj + r0;
      if (ROW) {
        for (uint32_t i = threadIdx.x; i < len; i += BLOCK) s_row[i] = adj[r0 + i];
        __syncthreads();
        target = s_row;
      }
      for (uint32_t r = a + wave; r < b; r += BLOCK / 64) {  // uniform over the wave
        const uint32_t other = s_other[r], olen = s_olen[r] & ~SNN_OWNER_IS_U;
        const bool owner_is_u = (s_olen[r] & SNN_OWNER_IS_U) != 0;
        const uint64_t a0 = s_ostart[r];
        uint32_t hits = 0;
        for (uint32_t i0 = 0; i0 < olen; i0 += 64) {
          bool hit = false;
          if (i0 + lane < olen) {
            const uint32_t x = adj[a0 + i0 + lane];
            const uint32_t at = snn_lower_bound(target, len, x);
            hit = at < len && target[at] == x;
          }
          hits += (uint32_t)__popcll(__ballot(hit));
        }
        const uint32_t at = snn_lower_bound(target, len, other);  // the edge's entry in the owner's row: it is there
        if (lane == 0) {
          out[s_idx[r]] = owner_is_u ? rtc_snn{hits, len, olen, 0u} : rtc_snn{hits, olen, len, 0u};
          if (at < len && atomicExch(&seen[r0 + at], 1u) == 0u) sum += hits;
        }
      }
      if (ROW) __syncthreads();  // the row is written again for the next run
      a = b;
    }
    __syncthreads();  // the slice's words are written again in the next turn
  }
  if (lane == 0 && sum) atomicAdd(shared_sum, sum);
}

}  // namespace

extern "C" double rtc_snn_weight(uint32_t shared, uint32_t deg_u, uint32_t deg_v) {
  return (double)((uint64_t)shared + 2) / (double)((uint64_t)deg_u + (uint64_t)deg_v - (uint64_t)shared);
}

extern "C" int rtc_graph_snn(rtc_ctx* ctx, uint32_t n, const rtc_wedge* h_edges, uint64_t m, rtc_snn* h_out) {
  const char* who = "rtc_graph_snn";
  if (!ctx) return RTC_ERR_ARG;
  if (m && (!h_edges || !h_out)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %llu records without %s", who, (unsigned long long)m, h_edges ? "a place for the result" : "the records");
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u vertices", who, n);
  memset(ctx->snn, 0, sizeof ctx->snn);
  ctx->snn_path = 0;
  if (m == 0 || n == 0) return RTC_OK;
  for (uint64_t e = 0; e < m; e++)
    if (h_edges[e].u >= n || h_edges[e].v >= n)
      return rtc_fail(ctx, RTC_ERR_ARG, "%s: record %llu is (%u, %u) with %u vertices", who, (unsigned long long)e, h_edges[e].u, h_edges[e].v, n);
  uint64_t* C = ctx->snn;
  const uint64_t t_begin = now_ns();
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;

  size_t ta = 0, tb = 0, tc = 0;
  RTC_HIP(ctx, rocprim::radix_sort_keys(nullptr, ta, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)(2 * m), 0u, 64u, s));
  RTC_HIP(ctx, rocprim::unique(nullptr, tb, (const uint64_t*)nullptr, (uint64_t*)nullptr, (unsigned long long*)nullptr, (size_t)(2 * m),
                               rocprim::equal_to<uint64_t>(), s));
  RTC_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tc, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                         (size_t)m, 0u, 34u, s));
  const size_t tmp_bytes = std::max(ta, std::max(tb, tc)) + 256;
  // two key buffers of 2m words (the sort's in and out, then the records' (key, index) pairs and their sorted copy), the rows and
  // their flags, the records, the result, the offsets
  const uint64_t need = 32ull * m + 16ull * m + 12ull * m + 16ull * m + 8ull * ((uint64_t)n + 1) + tmp_bytes + 4096;
  const uint64_t free_bytes = rtc_free_hbm(ctx);
  if (need > free_bytes)
    return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: %llu bytes for the adjacency of %llu records and the sort's scratch, %llu free", who,
                    (unsigned long long)need, (unsigned long long)m, (unsigned long long)free_bytes);
  DevBuf db;
  rtc_wedge* d_edges = nullptr;
  uint64_t *d_a = nullptr, *d_b = nullptr, *d_row = nullptr;
  uint32_t *d_adj = nullptr, *d_seen = nullptr;
  rtc_snn* d_out = nullptr;
  unsigned long long* d_state = nullptr;
  char* d_tmp = nullptr;
  RTC_TRY(db.get(ctx, m, &d_edges));
  RTC_TRY(db.get(ctx, 2 * m, &d_a));
  RTC_TRY(db.get(ctx, 2 * m, &d_b));
  RTC_TRY(db.get(ctx, 2 * m, &d_adj));
  RTC_TRY(db.get(ctx, 2 * m, &d_seen));
  RTC_TRY(db.get(ctx, (size_t)n + 1, &d_row));
  RTC_TRY(db.get(ctx, m, &d_out));
  RTC_TRY(db.get(ctx, SNN_STATE_WORDS, &d_state));
  RTC_TRY(db.get(ctx, tmp_bytes, &d_tmp));

  // ---- the adjacency ----
  RTC_HIP(ctx, hipMemcpyAsync(d_edges, h_edges, m * sizeof(rtc_wedge), hipMemcpyHostToDevice, s));
  RTC_HIP(ctx, hipMemsetAsync(d_state, 0, SNN_STATE_WORDS * 8, s));
  hipLaunchKernelGGL(snn_keys_kernel, dim3(blocks_for(m, ctx->num_cu)), dim3(256), 0, s, (const rtc_wedge*)d_edges, m, d_a);
  RTC_CHECK_LAUNCH(ctx);
  size_t bytes = tmp_bytes;
  RTC_HIP(ctx, rocprim::radix_sort_keys(d_tmp, bytes, (const uint64_t*)d_a, d_b, (size_t)(2 * m), 0u, 64u, s));
  bytes = tmp_bytes;
  RTC_HIP(ctx, rocprim::unique(d_tmp, bytes, (const uint64_t*)d_b, d_a, d_state + SNN_UNIQUE, (size_t)(2 * m), rocprim::equal_to<uint64_t>(), s));
  unsigned long long uniq = 0;
  RTC_HIP(ctx, hipMemcpyAsync(&uniq, d_state + SNN_UNIQUE, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  // the key of all ones, if there is one, lies behind row n - 1: no offset reaches it
  hipLaunchKernelGGL(louvain_rows_kernel, dim3(blocks_for((uint64_t)n + 1, ctx->num_cu)), dim3(256), 0, s, (const uint64_t*)d_a, (uint64_t)uniq, n, d_row);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(snn_adj_kernel, dim3(blocks_for(uniq, ctx->num_cu)), dim3(256), 0, s, (const uint64_t*)d_a, (uint64_t)uniq, d_adj);
  RTC_CHECK_LAUNCH(ctx);
  RTC_HIP(ctx, hipMemsetAsync(d_seen, 0, std::max<size_t>((size_t)uniq * 4, 4), s));
  uint64_t entries = 0;
  RTC_HIP(ctx, hipMemcpyAsync(&entries, d_row + n, 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint64_t t_adj = now_ns();
  C[7] = t_adj - t_begin;

  // ---- the counting: d_b takes the records' keys and indices, d_a their sorted copies ----
  uint64_t *okey = d_b, *oval = d_b + m, *skey = d_a, *sidx = d_a + m;
  hipLaunchKernelGGL(snn_owner_kernel, dim3(std::min<uint32_t>(blocks_for(m, ctx->num_cu), (uint32_t)ctx->num_cu * SNN_OWNER_WGS_PER_CU)), dim3(256), 0, s, (const rtc_wedge*)d_edges, m, (const uint64_t*)d_row,
                     ctx->opt.snn_global, okey, oval, d_out, d_state);
  RTC_CHECK_LAUNCH(ctx);
  bytes = tmp_bytes;
  RTC_HIP(ctx, rocprim::radix_sort_pairs(d_tmp, bytes, (const uint64_t*)okey, skey, (const uint64_t*)oval, sidx, (size_t)m, 0u, 34u, s));
  const uint32_t g0 = (uint32_t)std::min<uint64_t>((m + 63) / 64, (uint64_t)ctx->num_cu * SNN_WAVE_WGS_PER_CU);
  const uint32_t g1 = (uint32_t)std::min<uint64_t>((m + 255) / 256, (uint64_t)ctx->num_cu * SNN_BLOCK_WGS_PER_CU);
  const uint32_t g2 = (uint32_t)std::min<uint64_t>((m + 255) / 256, (uint64_t)ctx->num_cu * SNN_GLOBAL_WGS_PER_CU);
  hipLaunchKernelGGL((snn_count_kernel<64, SNN_WAVE_ROW>), dim3(g0), dim3(64), 0, s, (const uint64_t*)skey, (const uint64_t*)sidx,
                     (const unsigned long long*)d_state, 0, (const rtc_wedge*)d_edges, (const uint64_t*)d_row, (const uint32_t*)d_adj, d_seen, d_out,
                     d_state + SNN_SHARED_SUM);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL((snn_count_kernel<256, SNN_BLOCK_ROW>), dim3(g1), dim3(256), 0, s, (const uint64_t*)skey, (const uint64_t*)sidx,
                     (const unsigned long long*)d_state, 1, (const rtc_wedge*)d_edges, (const uint64_t*)d_row, (const uint32_t*)d_adj, d_seen, d_out,
                     d_state + SNN_SHARED_SUM);
  RTC_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL((snn_count_kernel<256, 0>), dim3(g2), dim3(256), 0, s, (const uint64_t*)skey, (const uint64_t*)sidx,
                     (const unsigned long long*)d_state, 2, (const rtc_wedge*)d_edges, (const uint64_t*)d_row, (const uint32_t*)d_adj, d_seen, d_out,
                     d_state + SNN_SHARED_SUM);
  RTC_CHECK_LAUNCH(ctx);
  unsigned long long state[SNN_STATE_WORDS];
  RTC_HIP(ctx, hipMemcpyAsync(state, d_state, sizeof state, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  C[8] = now_ns() - t_adj;
  RTC_HIP(ctx, hipMemcpyAsync(h_out, d_out, m * sizeof(rtc_snn), hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));

  C[0] = m;
  C[1] = entries / 2;
  C[2] = state[SNN_SHARED_SUM] / 3;
  C[3] = state[SNN_PROBES];
  for (int p = 0; p < 3; p++) {
    C[4 + p] = state[SNN_PATH0 + p];
    if (state[SNN_PATH0 + p]) ctx->snn_path |= 1 << p;
  }
  C[9] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_graph_snn_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->snn[i];
  return RTC_OK;
}

extern "C" int rtc_graph_snn_last_path(const rtc_ctx* ctx) { return ctx ? ctx->snn_path : 0; }
