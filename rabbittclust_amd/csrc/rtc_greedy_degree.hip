// rtc_greedy_degree.hip -- clust-greedy --order degree (include/rtclust.h has the definition): representatives
// that do not depend on the order the genomes came in.  The neighbour relation N is rtc_dbscan's (KSSD) or rtc_dbscan_mash's
// (MinHash) at the threshold, kept as a list of pairs by the pair phase those calls use (dbscan_pair_chunks, hier_filter_kernel,
// mash_edges_kernel with the rtc_medge record).  Then, all on the device:
//   * degrees: one edge-parallel pass, atomics that return nothing.  key(v) = degree(v) << 32 | ~v: "earlier in the order" is
//     one unsigned compare, and no two keys are equal;
//   * selection: the lexicographically first maximal independent set under that order, in rounds.  A vertex is open, a
//     representative or a member.  dg_mark_kernel (edges) marks every open vertex with an open neighbour of larger key,
//     dg_promote_kernel (vertices) makes the unmarked open vertices representatives, dg_demote_kernel (edges) makes the open
//     neighbours of representatives members.  The open vertex with the largest key is never marked, so a round decides at least
//     one vertex; an unmarked open vertex has no earlier open neighbour and no representative neighbour (it would be a member),
//     so the sequential walk makes it a representative too.  No round cap: the loop ends when nothing is open;
//   * the tail: from RTC_DEGREE_TAIL open vertices down the open vertices and the edges between them are compacted and, where
//     those edges are few as well, ONE workgroup runs the remaining rounds in one launch (dg_tail_kernel), barriers in the place
//     of launches and read-backs;
//   * assignment: the pairs with exactly one representative end, bucketed by the member (count, tk_scan_kernel, scatter, as the
//     k-distance buckets of rtc_dbscan_sweep.hip), each row folded to the best representative under the exact order
//     (common_a denom_b against common_b denom_a in 64 bits, ties to the representative's key) by one wave, or by 256 lanes
//     for a row of more than TK_LONG records.
// Every unit that evaluates eps_pred is built with -ffp-contract=off.
#include "rtc_dbscan_hier.h"
#include "rtc_dbscan_mash.h"
#include "rtc_topk_select.h"

namespace {

constexpr uint32_t DG_OPEN = 0, DG_REP = 1, DG_MEMBER = 2;
constexpr uint32_t DG_TAIL_THREADS = 1024;
// The open vertices from which the one-workgroup kernel takes over, where the edges between them are at most
// DG_TAIL_EDGES_PER_VERTEX times that number.  Measured with tools/run_greedy_degree.py --crossover on one MI355X:
// a round launched from the host takes 35 us, a round inside the kernel 4 to 8 us over up to 4 096 listed vertices of a path,
// 24 us over 16 384, 30 us over 20 000 -- it walks the lists it was given in every round -- and 0.6 ms over 245 000 pairs.
constexpr uint32_t DG_TAIL_DEFAULT = 4096;
constexpr uint64_t DG_TAIL_EDGES_PER_VERTEX = 4;

using DgEdge = rtc_medge;  // (i, j, common, denom): MinHash's kept record as it is, KSSD's with denom = |i| + |j| - common

__device__ __forceinline__ uint64_t dg_key(const uint32_t* __restrict__ deg, uint32_t v) { return ((uint64_t)deg[v] << 32) | (uint32_t)~v; }

__global__ __launch_bounds__(256) void dg_kssd_edges_kernel(const rtc_cedge* __restrict__ kept, uint64_t m, const uint32_t* __restrict__ len,
                                                            DgEdge* __restrict__ out) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const rtc_cedge c = kept[e];
    out[e] = DgEdge{c.i, c.j, c.common, len[c.i] + len[c.j] - c.common};
  }
}

__global__ __launch_bounds__(256) void dg_degree_kernel(const DgEdge* __restrict__ e, uint64_t m, uint32_t* __restrict__ deg) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < m; x += (uint64_t)gridDim.x * blockDim.x) {
    atomicAdd(&deg[e[x].i], 1u);  // the value is not used: no return
    atomicAdd(&deg[e[x].j], 1u);
  }
}

// of two open ends the later one is marked; many lanes may store the same 1
__global__ __launch_bounds__(256) void dg_mark_kernel(const DgEdge* __restrict__ e, uint64_t m, const uint32_t* __restrict__ deg,
                                                      const uint32_t* __restrict__ state, uint32_t* __restrict__ marked) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < m; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = e[x].i, b = e[x].j;
    if (state[a] != DG_OPEN || state[b] != DG_OPEN) continue;
    marked[dg_key(deg, a) < dg_key(deg, b) ? a : b] = 1u;
  }
}

// cnt[0] += the open vertices met, cnt[1] += those that became representatives (one atomic a wave, nothing returned); the marks are cleared
__global__ __launch_bounds__(256) void dg_promote_kernel(uint32_t n, uint32_t* __restrict__ state, uint32_t* __restrict__ marked,
                                                         unsigned long long* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t v0 = blockIdx.x * blockDim.x; v0 < n; v0 += gridDim.x * blockDim.x) {  // whole waves stay together
    const uint32_t v = v0 + threadIdx.x;
    bool open = false, rep = false;
    if (v < n && state[v] == DG_OPEN) {
      open = true;
      if (marked[v]) marked[v] = 0u;
      else { state[v] = DG_REP; rep = true; }
    }
    const uint64_t bo = __ballot(open), br = __ballot(rep);
    if (lane == 0 && bo) atomicAdd(&cnt[0], (unsigned long long)__popcll(bo));
    if (lane == 0 && br) atomicAdd(&cnt[1], (unsigned long long)__popcll(br));
  }
}

// No two representatives are neighbours, and only open vertices change: every store is the same DG_MEMBER, whoever wins.
// state is read and written here by different lanes: no __restrict__.
__global__ __launch_bounds__(256) void dg_demote_kernel(const DgEdge* __restrict__ e, uint64_t m, uint32_t* state) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < m; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = e[x].i, b = e[x].j;
    const uint32_t sa = state[a], sb = state[b];
    if (sa == DG_REP && sb == DG_OPEN) state[b] = DG_MEMBER;
    else if (sb == DG_REP && sa == DG_OPEN) state[a] = DG_MEMBER;
  }
}

// ---- the tail ----
// the open vertices (vl, cnt[4]) and the edges with two open ends (cl, cnt[5]); the lists have n and m slots
__global__ __launch_bounds__(256) void dg_compact_vertices_kernel(uint32_t n, const uint32_t* __restrict__ state, uint32_t* __restrict__ vl,
                                                                  unsigned long long* __restrict__ cnt) {
  for (uint32_t v0 = blockIdx.x * blockDim.x; v0 < n; v0 += gridDim.x * blockDim.x) {  // uniform per wave
    const uint32_t v = v0 + threadIdx.x;
    wave_append(v < n && state[v] == DG_OPEN, v, vl, (uint64_t)n, &cnt[4]);
  }
}
__global__ __launch_bounds__(256) void dg_compact_edges_kernel(const DgEdge* __restrict__ e, uint64_t m, const uint32_t* __restrict__ state,
                                                               uint2* __restrict__ cl, unsigned long long* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += stride) {  // uniform per wave
    const uint64_t x = base + threadIdx.x;
    bool keep = false;
    uint2 p = make_uint2(0u, 0u);
    if (x < m) {
      p = make_uint2(e[x].i, e[x].j);
      keep = state[p.x] == DG_OPEN && state[p.y] == DG_OPEN;
    }
    wave_append(keep, p, cl, m, &cnt[5]);
  }
}

// One workgroup runs the rounds that are left over the compacted lists: the three passes of a round with a barrier between them
// (the workgroup's lanes share one CU, whose vector cache they all read and write through).  Every round with an open vertex
// decides one, so nv + 1 rounds always suffice: the loop has that bound and reports in cnt[3] if it was not enough.
// cnt[1] += the representatives made, cnt[2] = the rounds run.  state and marked are shared between the lanes: no __restrict__.
__global__ __launch_bounds__(DG_TAIL_THREADS) void dg_tail_kernel(const uint2* __restrict__ cl, const uint32_t* __restrict__ vl,
                                                                  const uint32_t* __restrict__ deg, uint32_t* state, uint32_t* marked,
                                                                  unsigned long long* cnt) {
  __shared__ uint32_t s_open, s_rep;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t nv = (uint32_t)cnt[4];
  const uint64_t ne = cnt[5];
  uint32_t rounds = 0, reps = 0;
  bool done = false;
  for (uint32_t r = 0; r <= nv; r++) {  // uniform: nv, s_open and s_rep are the same for every lane
    if (tid == 0) { s_open = 0; s_rep = 0; }
    for (uint64_t x = tid; x < ne; x += DG_TAIL_THREADS) {
      const uint2 p = cl[x];
      if (state[p.x] == DG_OPEN && state[p.y] == DG_OPEN) marked[dg_key(deg, p.x) < dg_key(deg, p.y) ? p.x : p.y] = 1u;
    }
    __syncthreads();
    for (uint32_t x0 = 0; x0 < nv; x0 += DG_TAIL_THREADS) {  // whole waves stay together
      const uint32_t x = x0 + tid;
      bool open = false, rep = false;
      if (x < nv) {
        const uint32_t v = vl[x];
        if (state[v] == DG_OPEN) {
          open = true;
          if (marked[v]) marked[v] = 0u;
          else { state[v] = DG_REP; rep = true; }
        }
      }
      const uint64_t bo = __ballot(open), br = __ballot(rep);
      if (lane == 0 && bo) atomicAdd(&s_open, (uint32_t)__popcll(bo));
      if (lane == 0 && br) atomicAdd(&s_rep, (uint32_t)__popcll(br));
    }
    __syncthreads();
    const uint32_t n_open = s_open, n_rep = s_rep;
    if (n_open == 0) { done = true; break; }
    reps += n_rep;
    rounds++;
    for (uint64_t x = tid; x < ne; x += DG_TAIL_THREADS) {
      const uint2 p = cl[x];
      const uint32_t sa = state[p.x], sb = state[p.y];
      if (sa == DG_REP && sb == DG_OPEN) state[p.y] = DG_MEMBER;
      else if (sb == DG_REP && sa == DG_OPEN) state[p.x] = DG_MEMBER;
    }
    __syncthreads();  // the members are in, and every lane has read s_open / s_rep before lane 0 clears them
  }
  if (tid == 0) {
    cnt[1] += reps;
    cnt[2] = rounds;
    cnt[3] = done ? 0ull : 1ull;
  }
}

// ---- the assignment ----
__global__ __launch_bounds__(256) void dg_out_init_kernel(uint32_t n, const uint32_t* __restrict__ deg, rtc_degree_place* __restrict__ out) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) out[v] = rtc_degree_place{v, deg[v], 0u, 0u};
}
// an edge with exactly one representative end is a record of the other end's row
__global__ __launch_bounds__(256) void dg_row_count_kernel(const DgEdge* __restrict__ e, uint64_t m, const uint32_t* __restrict__ state,
                                                           uint32_t* __restrict__ cnt) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < m; x += (uint64_t)gridDim.x * blockDim.x) {
    const bool ra = state[e[x].i] == DG_REP, rb = state[e[x].j] == DG_REP;
    if (ra != rb) atomicAdd(&cnt[ra ? e[x].j : e[x].i], 1u);
  }
}
// the record: (representative, common, denom, the representative's degree -- with the index, its key)
__global__ __launch_bounds__(256) void dg_row_scatter_kernel(const DgEdge* __restrict__ e, uint64_t m, const uint32_t* __restrict__ state,
                                                             const uint32_t* __restrict__ deg, const uint64_t* __restrict__ off,
                                                             uint32_t* __restrict__ cursor, TkRec* __restrict__ seg) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < m; x += (uint64_t)gridDim.x * blockDim.x) {
    const DgEdge c = e[x];
    const bool ra = state[c.i] == DG_REP, rb = state[c.j] == DG_REP;
    if (ra == rb) continue;
    const uint32_t mem = ra ? c.j : c.i, rep = ra ? c.i : c.j;
    const uint32_t at = atomicAdd(&cursor[mem], 1u);
    if (off[mem] + at < off[mem + 1]) seg[off[mem] + at] = TkRec{rep, c.common, c.denom, deg[rep]};
  }
}
// a is the better representative: the larger common / denom, exactly; then the earlier in the order (larger degree, lower index).
// A total order on the records of a row (the representatives differ), so the fold does not depend on the order they lie in.
// denom 0 marks "none yet", which every record beats (a kept pair has common >= 1 and denom >= 1).
__device__ __forceinline__ bool dg_better(const TkRec& a, const TkRec& b) {
  if (a.denom == 0) return false;
  if (b.denom == 0) return true;
  const uint64_t l = (uint64_t)a.common * b.denom, r = (uint64_t)b.common * a.denom;  // common < 2^31, denom < 2^32
  if (l != r) return l > r;
  if (a.pad != b.pad) return a.pad > b.pad;
  return a.slot < b.slot;
}
// a workgroup of B lanes per row whose length lies in [lo, hi] (B = 64: one wave, no barrier)
template <int B>
__global__ __launch_bounds__(B) void dg_assign_kernel(const TkRec* __restrict__ seg, const uint64_t* __restrict__ off, uint32_t n, uint64_t lo,
                                                      uint64_t hi, rtc_degree_place* __restrict__ out) {
  __shared__ TkRec part[B / 64];
  const uint32_t v = blockIdx.x;
  if (v >= n) return;
  const uint64_t s0 = off[v], s1 = off[v + 1];
  if (s1 - s0 < lo || s1 - s0 > hi) return;  // uniform across the workgroup
  TkRec best{0xffffffffu, 0u, 0u, 0u};
  for (uint64_t x = s0 + threadIdx.x; x < s1; x += B) {
    const TkRec r = seg[x];
    if (dg_better(r, best)) best = r;
  }
  for (int d = 32; d; d >>= 1) {  // every lane of the wave takes part
    TkRec o;
    o.slot = __shfl_xor(best.slot, d); o.common = __shfl_xor(best.common, d); o.denom = __shfl_xor(best.denom, d); o.pad = __shfl_xor(best.pad, d);
    if (dg_better(o, best)) best = o;
  }
  if (B > 64) {
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < B / 64; w++)
        if (dg_better(part[w], best)) best = part[w];
  }
  if (threadIdx.x == 0 && best.denom) { out[v].rep = best.slot; out[v].common = best.common; out[v].denom = best.denom; }
}

}  // namespace

extern "C" int rtc_greedy_degree(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                 int is_minhash, uint32_t sketch_size, double threshold, int kmer_size, rtc_degree_place* h_out,
                                 uint32_t* h_n_clusters) {
  const char* who = "rtc_greedy_degree";
  if (!ctx || !h_n_clusters || (n && (!d_hashes || !d_start || !d_len || !h_out)) || (width != 4 && width != 8)) return RTC_ERR_ARG;
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u genomes", who, n);
  if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: k-mer size %d", who, kmer_size);
  EpsLevels lv;
  memset(&lv, 0, sizeof lv);
  if (is_minhash) {
    if (sketch_size == 0 || sketch_size >= (1u << 28)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: sketch size %u", who, sketch_size);
    if (!(threshold >= 0.0)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: threshold %g is not in [0, 1)", who, threshold);
    if (threshold >= 1.0)  // pairs without a common hash (distance 1) would be neighbours, and no candidate list holds them
      return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: threshold %g: from 1 on, pairs without a common hash are neighbours", who, threshold);
  } else if (!eps_to_t(threshold, kmer_size, &lv.t[0], &lv.one_plus_t[0])) {
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: threshold %g with k %d gives jaccard_min %g <= 1e-12", who, threshold, kmer_size, lv.t[0]);
  }
  *h_n_clusters = 0;
  memset(ctx->greedy_degree, 0, sizeof ctx->greedy_degree);
  ctx->greedy_degree_path = 0;
  if (n == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t t_begin = now_ns();
  uint64_t* g = ctx->greedy_degree;
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t max_len = *std::max_element(h_len.begin(), h_len.end());
  if (!is_minhash && width == 4 && !u32_size_bound_fits(max_len, lv.t[0]))
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: size bound ceil(%u / %g) past INT_MAX", who, max_len, lv.t[0]);
  const uint32_t sat = width == 4 ? 65535u : 0xffffffffu;

  // ---- the pair phase: N as a list of pairs, every pair once ----
  DevBuf db;
  unsigned long long* d_cnt = nullptr;  // [0] pair count, [1..4] the counters of the filter in flight
  RTC_TRY(db.get(ctx, 8, &d_cnt));
  KeptList kept;                   // KSSD: (p < q, the count the predicate saw)
  KeptListOf<rtc_medge> mkept;     // MinHash: (i, j, common, denom) on the union-truncated counts
  kept.cap = mkept.cap = std::max<uint64_t>((uint64_t)1 << 16, (uint64_t)n * 16);
  MashTables mt;
  uint64_t merged = 0;
  if (is_minhash) {
    RTC_TRY(db.get(ctx, mkept.cap, &mkept.d));
    RTC_TRY(mash_tables(ctx, db, sketch_size, max_len, kmer_size, &threshold, 1, &mt));
  } else {
    RTC_TRY(db.get(ctx, kept.cap, &kept.d));
  }
  PairPhase pp;
  auto on_chunk = [&](const rtc_cedge* d_cand, uint64_t cnt) -> int {
    if (!cnt) return RTC_OK;
    if (is_minhash) return mash_filter_chunk(ctx, db, who, d_hashes, width, d_start, d_len, sketch_size, d_cand, cnt, mt, 1, d_cnt + 1, &mkept, &merged);
    return filter_chunk(ctx, db, who, hier_filter_kernel, d_cand, cnt, d_len, lv, 1, sat, d_cnt + 1, &kept);
  };
  if (n > 1) RTC_TRY(dbscan_pair_chunks(ctx, db, d_hashes, width, d_start, d_len, n, 1, d_cnt, &pp, on_chunk));
  const uint64_t m = is_minhash ? mkept.used : kept.used;
  g[0] = pp.chunks; g[1] = pp.cand_total; g[2] = merged; g[3] = m;
  g[7] = pp.pair_ns; g[8] = is_minhash ? mkept.ns : kept.ns;
  if (kept.asym) {
    g[11] = now_ns() - t_begin;
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: %llu pairs whose threshold test depends on the orientation, e.g. (%u, %u)", who,
                    (unsigned long long)kept.asym, (uint32_t)(kept.first_asym >> 32), (uint32_t)kept.first_asym);
  }
  const dim3 b(256), gv(blocks_for(n, ctx->num_cu)), ge(blocks_for(std::max<uint64_t>(m, 1), ctx->num_cu));
  DgEdge* d_e = mkept.d;
  if (!is_minhash && m) {
    RTC_TRY(db.get(ctx, m, &d_e));
    hipLaunchKernelGGL(dg_kssd_edges_kernel, ge, b, 0, s, (const rtc_cedge*)kept.d, m, d_len, d_e);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipStreamSynchronize(s));
    db.release(kept.d);
  }

  // ---- degrees and selection ----
  const uint64_t t_sel = now_ns();
  uint32_t *d_deg = nullptr, *d_state = nullptr, *d_marked = nullptr;
  unsigned long long* d_sc = nullptr;  // [0] open, [1] representatives (running), [2] tail rounds, [3] tail gave up, [4] / [5] compacted vertices / edges
  RTC_TRY(db.get(ctx, n, &d_deg));
  RTC_TRY(db.get(ctx, n, &d_state));
  RTC_TRY(db.get(ctx, n, &d_marked));
  RTC_TRY(db.get(ctx, 8, &d_sc));
  RTC_HIP(ctx, hipMemsetAsync(d_deg, 0, (size_t)n * 4, s));
  RTC_HIP(ctx, hipMemsetAsync(d_state, 0, (size_t)n * 4, s));  // DG_OPEN
  RTC_HIP(ctx, hipMemsetAsync(d_marked, 0, (size_t)n * 4, s));
  RTC_HIP(ctx, hipMemsetAsync(d_sc, 0, 64, s));
  if (m) {
    hipLaunchKernelGGL(dg_degree_kernel, ge, b, 0, s, (const DgEdge*)d_e, m, d_deg);
    RTC_CHECK_LAUNCH(ctx);
  }
  const uint32_t tail = ctx->opt.has_degree_tail ? ctx->opt.degree_tail : DG_TAIL_DEFAULT;
  // open: the vertices without a decision, from above -- those open before the last round less its representatives (its new
  // members are not counted, so the tail may start a round later than it could; the result does not depend on when it starts)
  uint64_t open = n, rounds = 0, tail_rounds = 0, reps = 0, tail_below = ~0ull;
  uint32_t* d_vl = nullptr;
  uint2* d_cl = nullptr;
  for (;;) {
    if (open == 0) break;
    if (tail && open <= tail && open <= tail_below) {
      if (!d_vl) {
        RTC_TRY(db.get(ctx, n, &d_vl));
        RTC_TRY(db.get(ctx, std::max<uint64_t>(m, 1), &d_cl));
      }
      RTC_HIP(ctx, hipMemsetAsync(d_sc + 4, 0, 16, s));
      hipLaunchKernelGGL(dg_compact_vertices_kernel, gv, b, 0, s, n, (const uint32_t*)d_state, d_vl, d_sc);
      RTC_CHECK_LAUNCH(ctx);
      if (m) {
        hipLaunchKernelGGL(dg_compact_edges_kernel, ge, b, 0, s, (const DgEdge*)d_e, m, (const uint32_t*)d_state, d_cl, d_sc);
        RTC_CHECK_LAUNCH(ctx);
      }
      unsigned long long sc[6];
      RTC_HIP(ctx, hipMemcpyAsync(sc, d_sc, sizeof sc, hipMemcpyDeviceToHost, s));
      RTC_HIP(ctx, hipStreamSynchronize(s));
      if (sc[4] > n || sc[5] > m) return rtc_fail(ctx, RTC_ERR_HIP, "%s: %llu open vertices and %llu edges between them compacted", who, sc[4], sc[5]);
      if (sc[4] == 0) break;
      // one workgroup walks every compacted edge twice a round: it takes over where those are few as well, and otherwise the
      // host's rounds go on until half as many vertices are open
      if (sc[5] <= DG_TAIL_EDGES_PER_VERTEX * (uint64_t)tail) {
        hipLaunchKernelGGL(dg_tail_kernel, dim3(1), dim3(DG_TAIL_THREADS), 0, s, (const uint2*)d_cl, (const uint32_t*)d_vl, (const uint32_t*)d_deg,
                           d_state, d_marked, d_sc);
        RTC_CHECK_LAUNCH(ctx);
        RTC_HIP(ctx, hipMemcpyAsync(sc, d_sc, sizeof sc, hipMemcpyDeviceToHost, s));
        RTC_HIP(ctx, hipStreamSynchronize(s));
        if (sc[3]) return rtc_fail(ctx, RTC_ERR_HIP, "%s: the tail kernel left vertices open (%llu vertices, %llu edges, %llu rounds)", who, sc[4], sc[5], sc[2]);
        tail_rounds = sc[2];
        rounds += tail_rounds;
        reps = sc[1];
        ctx->greedy_degree_path |= 4;
        break;
      }
      tail_below = sc[4] / 2;
    }
    RTC_HIP(ctx, hipMemsetAsync(d_sc, 0, 8, s));  // the open count of this round; the representatives run on
    if (m) {
      hipLaunchKernelGGL(dg_mark_kernel, ge, b, 0, s, (const DgEdge*)d_e, m, (const uint32_t*)d_deg, (const uint32_t*)d_state, d_marked);
      RTC_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL(dg_promote_kernel, gv, b, 0, s, n, d_state, d_marked, d_sc);
    RTC_CHECK_LAUNCH(ctx);
    unsigned long long sc[2];
    RTC_HIP(ctx, hipMemcpyAsync(sc, d_sc, sizeof sc, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    if (sc[0] == 0) break;  // the bound was not tight: the last round's members were the rest
    const uint64_t made = sc[1] - reps;
    if (made == 0 || made > sc[0]) return rtc_fail(ctx, RTC_ERR_HIP, "%s: a round over %llu open vertices made %llu representatives", who, sc[0], (unsigned long long)made);
    reps = sc[1];
    rounds++;
    if (m) {
      hipLaunchKernelGGL(dg_demote_kernel, ge, b, 0, s, (const DgEdge*)d_e, m, d_state);
      RTC_CHECK_LAUNCH(ctx);
    }
    open = sc[0] - made;
  }
  RTC_HIP(ctx, hipStreamSynchronize(s));
  if (d_vl) { db.release(d_vl); db.release(d_cl); }
  g[4] = reps; g[5] = rounds | (tail_rounds << 32);
  const uint64_t t_asg = now_ns();
  g[9] = t_asg - t_sel;

  // ---- assignment ----
  rtc_degree_place* d_out = nullptr;
  uint32_t *d_rc = nullptr, *d_cur = nullptr;
  uint64_t *d_off = nullptr, *d_koff = nullptr;
  RTC_TRY(db.get(ctx, n, &d_out));
  hipLaunchKernelGGL(dg_out_init_kernel, gv, b, 0, s, n, (const uint32_t*)d_deg, d_out);
  RTC_CHECK_LAUNCH(ctx);
  uint64_t rows_wave = 0, rows_block = 0;
  if (m) {
    RTC_TRY(db.get(ctx, n, &d_rc));
    RTC_TRY(db.get(ctx, n, &d_cur));
    RTC_TRY(db.get(ctx, (size_t)n + 1, &d_off));
    RTC_TRY(db.get(ctx, (size_t)n + 1, &d_koff));
    RTC_HIP(ctx, hipMemsetAsync(d_rc, 0, (size_t)n * 4, s));
    RTC_HIP(ctx, hipMemsetAsync(d_cur, 0, (size_t)n * 4, s));
    hipLaunchKernelGGL(dg_row_count_kernel, ge, b, 0, s, (const DgEdge*)d_e, m, (const uint32_t*)d_state, d_rc);
    RTC_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(tk_scan_kernel, dim3(1), dim3(TK_SCAN_THREADS), 0, s, (const uint32_t*)d_rc, n, 0u, d_off, d_koff);
    RTC_CHECK_LAUNCH(ctx);
    std::vector<uint32_t> h_rc(n);
    uint64_t total = 0;
    RTC_HIP(ctx, hipMemcpyAsync(h_rc.data(), d_rc, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipMemcpyAsync(&total, d_off + n, 8, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    uint64_t sum = 0;
    const uint64_t wave_max = ctx->opt.degree_block ? 0 : TK_LONG;
    for (uint32_t v = 0; v < n; v++) {
      sum += h_rc[v];
      if (h_rc[v] == 0) continue;
      if (h_rc[v] <= wave_max) rows_wave++; else rows_block++;
    }
    if (sum != total || total > m) return rtc_fail(ctx, RTC_ERR_HIP, "%s: the rows hold %llu records, the scan %llu, of %llu pairs", who,
                                                  (unsigned long long)sum, (unsigned long long)total, (unsigned long long)m);
    if (rows_wave + rows_block != (uint64_t)n - reps)
      return rtc_fail(ctx, RTC_ERR_HIP, "%s: %llu members have a representative next to them, %llu genomes are no representatives", who,
                      (unsigned long long)(rows_wave + rows_block), (unsigned long long)((uint64_t)n - reps));
    if (total) {
      TkRec* d_seg = nullptr;
      RTC_TRY(db.get(ctx, total, &d_seg));
      hipLaunchKernelGGL(dg_row_scatter_kernel, ge, b, 0, s, (const DgEdge*)d_e, m, (const uint32_t*)d_state, (const uint32_t*)d_deg,
                         (const uint64_t*)d_off, d_cur, d_seg);
      RTC_CHECK_LAUNCH(ctx);
      if (rows_wave) {
        hipLaunchKernelGGL(dg_assign_kernel<64>, dim3(n), dim3(64), 0, s, (const TkRec*)d_seg, (const uint64_t*)d_off, n, (uint64_t)1, wave_max, d_out);
        RTC_CHECK_LAUNCH(ctx);
        ctx->greedy_degree_path |= 1;
      }
      if (rows_block) {
        hipLaunchKernelGGL(dg_assign_kernel<256>, dim3(n), dim3(256), 0, s, (const TkRec*)d_seg, (const uint64_t*)d_off, n, wave_max + 1, ~0ull, d_out);
        RTC_CHECK_LAUNCH(ctx);
        ctx->greedy_degree_path |= 2;
      }
    }
  } else if (reps != n) {
    return rtc_fail(ctx, RTC_ERR_HIP, "%s: %llu representatives among %u genomes without a pair", who, (unsigned long long)reps, n);
  }
  RTC_HIP(ctx, hipMemcpyAsync(h_out, d_out, (size_t)n * sizeof(rtc_degree_place), hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  *h_n_clusters = (uint32_t)reps;
  g[6] = rows_wave | (rows_block << 32);
  g[10] = now_ns() - t_asg;
  g[11] = now_ns() - t_begin;
  return RTC_OK;
}

extern "C" int rtc_greedy_degree_counters(const rtc_ctx* ctx, uint64_t out[12]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 12; i++) out[i] = ctx->greedy_degree[i];
  return RTC_OK;
}

extern "C" int rtc_greedy_degree_last_path(const rtc_ctx* ctx) { return ctx ? ctx->greedy_degree_path : 0; }
