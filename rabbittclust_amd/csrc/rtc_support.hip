// rtc_support.hip -- clust-mst --cluster-support: jackknife support of the clusters themselves.
//
// The definition is in include/rtclust.h (tests/refsupport.py restates it).  rtc_jackknife_pairs_dev (rtc_nj_support.hip) counts
// common_r and size_r of 64 replicates at once, a replicate a lane; everything after the counts is here, in the same shape -- one
// wave per item, lane r replicate r, so every access to the 64 values of a candidate, a vertex or a cluster is one 256-byte row:
//   csup_mask_kernel      a wave takes 64 candidates, one after the other: denom_r from the counts, the keep table, a ballot -- the
//                         candidate's 64-bit keep mask.  Lane k keeps the mask of the tile's k-th candidate, so the inner edges with
//                         a non-zero mask leave in one append per wave and a crossing edge ORs its mask into its two clusters' words.
//   csup_hook_kernel      rtc_components64_dev's pass: one wave per edge, lane r hooks the larger root under the smaller one in graph
//                         r (atomicMin on the root's slot, followed up where the slot was no root any more)
//   csup_jump_kernel      every label to its root
//   csup_tally_kernel     one wave per cluster walks its members: whole, pieces, the class from whole and the crossing word, and
//                         integer atomic adds of the piece sizes into row P_r(g)
//   csup_together_kernel  one wave per genome: the sum over the word's replicates of piece_r(g) - 1
// Integer atomics only (min, or, add): nothing depends on the order.
#include <math.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "rtc_dbscan_common.h"
#include "rtc_support.h"

namespace {

// The root of v in graph `lane`.  A label never exceeds its vertex, so the walk descends and ends; a value that does not descend
// is taken as a root, which also keeps every access inside [0, v].  The loads are coherent at the device's L2, where the hooks'
// atomics land.
__device__ __forceinline__ uint32_t csup_find(const uint32_t* label, uint32_t v, uint32_t lane) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&label[(uint64_t)v * 64 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= v) return v;
    v = p;
  }
}

__global__ __launch_bounds__(256) void csup_identity_kernel(uint32_t* __restrict__ label, uint64_t total) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) label[i] = (uint32_t)(i >> 6);
}

// One wave per edge.  Lane r, where the mask has bit r: the roots of both ends; the larger one goes under the smaller one by an
// atomicMin on its slot.  Where the slot was no root any more (another edge hooked it first), its old parent and the smaller root
// still have to meet: the lane goes on with that pair, whose larger member lies below the slot, so the loop ends.  Every attempt
// raises the flag, so the pass that leaves it down has found every edge inside one tree and has written nothing.
__global__ __launch_bounds__(256) void csup_hook_kernel(const rtc_cedge* __restrict__ edges, const uint64_t* __restrict__ mask, uint64_t m, uint32_t n,
                                                        uint32_t* label, uint32_t* __restrict__ flag) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64);
  for (uint64_t e = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; e < m; e += waves) {  // uniform per wave
    const uint32_t u = edges[e].i, v = edges[e].j;
    const uint64_t mk = mask[e];
    if (u >= n || v >= n || u == v) continue;  // uniform
    bool tried = false;
    if ((mk >> lane) & 1) {
      uint32_t a = u, b = v;
      for (;;) {
        const uint32_t ra = csup_find(label, a, lane), rb = csup_find(label, b, lane);
        if (ra == rb) break;
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        tried = true;
        const uint32_t old = atomicMin(&label[(uint64_t)hi * 64 + lane], lo);
        if (old >= hi) break;  // hi was a root and now hangs under lo
        a = old;
        b = lo;
      }
    }
    if (__ballot(tried) && lane == 0) *flag = 1u;
  }
}

// every label to its root; roots do not move here, and whatever a walk reads on the way is an ancestor
__global__ __launch_bounds__(256) void csup_jump_kernel(uint32_t* label, uint64_t total) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = (uint32_t)(i >> 6), lane = (uint32_t)(i & 63);
    const uint32_t r = csup_find(label, v, lane);
    if (r != v) label[i] = r;
  }
}

// cnt[0]: inner edges kept of this launch (the list's counter), cnt[1] / cnt[2]: inner / crossing edges kept, summed over launches
__global__ __launch_bounds__(256) void csup_mask_kernel(const rtc_cedge* __restrict__ edges, uint64_t m, const uint32_t* __restrict__ common,
                                                        const uint32_t* __restrict__ size, const uint32_t* __restrict__ need, uint32_t max_denom,
                                                        const uint32_t* __restrict__ cl, uint32_t lanes, rtc_cedge* __restrict__ kept,
                                                        uint64_t* __restrict__ kept_mask, uint64_t cap, unsigned long long* __restrict__ list_count,
                                                        unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ cross) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64);
  const uint64_t live = lanes >= 64 ? ~0ull : (1ull << lanes) - 1ull;  // the lanes at or past B in the last word are cleared
  const uint64_t tiles = (m + CSUP_TILE - 1) / CSUP_TILE;
  for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; t < tiles; t += waves) {  // uniform per wave
    const uint64_t base = t * CSUP_TILE;
    const uint32_t nt = (uint32_t)(m - base < CSUP_TILE ? m - base : CSUP_TILE);
    const bool have = lane < nt;
    uint32_t i = 0, j = 0;
    if (have) { i = edges[base + lane].i; j = edges[base + lane].j; }
    uint64_t mine = 0;
    for (uint32_t k = 0; k < nt; k++) {  // uniform
      const uint32_t ik = __shfl(i, k), jk = __shfl(j, k);
      const uint32_t c = common[(base + k) * 64 + lane];
      const uint32_t denom = size[(uint64_t)ik * 64 + lane] + size[(uint64_t)jk * 64 + lane] - c;
      const bool keep = c > 0 && denom <= max_denom && c >= need[denom];
      const uint64_t bal = __ballot(keep) & live;
      if (lane == k) mine = bal;
    }
    uint32_t ci = 0, cj = 0;
    if (have) { ci = cl[i]; cj = cl[j]; }
    const bool inner = have && mine != 0 && ci == cj, crossing = have && mine != 0 && ci != cj;
    const uint64_t bi = __ballot(inner), bc = __ballot(crossing);
    if (bi) {
      unsigned long long at = 0;
      if (lane == 0) { at = atomicAdd(list_count, (unsigned long long)__popcll(bi)); atomicAdd(&cnt[1], (unsigned long long)__popcll(bi)); }
      at = __shfl(at, 0);
      const uint64_t idx = at + (uint64_t)__popcll(bi & ((1ull << lane) - 1ull));
      if (inner && idx < cap) { kept[idx] = rtc_cedge{i, j, 0}; kept_mask[idx] = mine; }
    }
    if (crossing) { atomicOr(&cross[ci], (unsigned long long)mine); atomicOr(&cross[cj], (unsigned long long)mine); }
    if (bc && lane == 0) atomicAdd(&cnt[2], (unsigned long long)__popcll(bc));
  }
}

// One wave per cluster, lane r a replicate of the word.  psize[P * 64 + r] counts the genomes whose piece starts at P: in a
// recovered replicate a wave's adds go to one contiguous row.  Only this wave touches out[c].
__global__ __launch_bounds__(256) void csup_tally_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ cfirst, uint32_t n_cl,
                                                         const uint32_t* __restrict__ label, const unsigned long long* __restrict__ cross, uint32_t lanes,
                                                         uint32_t* __restrict__ psize, rtc_csupport* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  const bool live = lane < lanes;
  for (uint32_t c = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; c < n_cl; c += waves) {  // uniform per wave
    const uint32_t m0 = cfirst[c], m1 = cfirst[c + 1];
    const uint32_t f = perm[m0];
    bool whole = true;
    uint32_t pieces = 0;
    for (uint32_t x = m0; x < m1; x++) {  // uniform
      const uint32_t g = perm[x];
      const uint32_t P = label[(uint64_t)g * 64 + lane];
      whole &= P == f;
      pieces += P == g;
      if (live) atomicAdd(&psize[(uint64_t)P * 64 + lane], 1u);
    }
    const bool pure = ((cross[c] >> lane) & 1ull) == 0;
    const uint32_t rec = (uint32_t)__popcll(__ballot(live && whole && pure)), spl = (uint32_t)__popcll(__ballot(live && !whole && pure));
    const uint32_t mer = (uint32_t)__popcll(__ballot(live && whole && !pure)), mix = (uint32_t)__popcll(__ballot(live && !whole && !pure));
    uint32_t mx = live ? pieces : 0;
    for (int o = 32; o > 0; o >>= 1) { const uint32_t y = __shfl_xor(mx, o); mx = y > mx ? y : mx; }
    if (lane == 0) {
      rtc_csupport r = out[c];
      r.size = m1 - m0;
      r.recovered += rec; r.split += spl; r.merged += mer; r.mixed += mix;
      r.max_pieces = mx > r.max_pieces ? mx : r.max_pieces;
      out[c] = r;
    }
  }
}

// one wave per genome: together[g] += the sum over the word's replicates of piece_r(g) - 1
__global__ __launch_bounds__(256) void csup_together_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ psize, uint32_t n, uint32_t lanes,
                                                            unsigned long long* __restrict__ together) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t g = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; g < n; g += waves) {  // uniform per wave
    const uint32_t P = label[(uint64_t)g * 64 + lane];
    uint32_t s = lane < lanes ? psize[(uint64_t)P * 64 + lane] - 1u : 0u;  // a piece holds its own genome: at least 1
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) together[g] += s;
  }
}

uint32_t csup_grid(uint64_t waves_wanted, int num_cu) {  // 256-lane workgroups of four waves
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((waves_wanted + 3) / 4, (uint64_t)num_cu * 16));
}

// rtc_components64_dev with the flag's word given: passes until one leaves the flag down
int csup_components(rtc_ctx* ctx, uint32_t n, const rtc_cedge* d_edges, const uint64_t* d_mask, uint64_t m, uint32_t* d_label, uint32_t* d_flag,
                    uint64_t* passes) {
  if (m == 0 || n == 0) return RTC_OK;
  hipStream_t s = ctx->stream;
  void* hp = nullptr;
  RTC_TRY(rtc_pinned(ctx, 64, &hp));
  const uint64_t total = (uint64_t)n * 64;
  for (;;) {
    RTC_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, s));
    hipLaunchKernelGGL(csup_hook_kernel, dim3(csup_grid(m, ctx->num_cu)), dim3(256), 0, s, d_edges, d_mask, m, n, d_label, d_flag);
    RTC_CHECK_LAUNCH(ctx);
    RTC_HIP(ctx, hipMemcpyAsync(hp, d_flag, 4, hipMemcpyDeviceToHost, s));
    RTC_HIP(ctx, hipStreamSynchronize(s));
    if (passes) (*passes)++;
    if (*(const uint32_t*)hp == 0) return RTC_OK;
    hipLaunchKernelGGL(csup_jump_kernel, dim3(blocks_for(total, ctx->num_cu)), dim3(256), 0, s, d_label, total);
    RTC_CHECK_LAUNCH(ctx);
  }
}

bool csup_passes(uint32_t c, uint32_t d, int kmer_size, double threshold) { return rtc_linkage_distance(c, d, kmer_size) <= threshold; }

// need[d] for d = 0 .. max_denom.  The rule is monotone in c, so the least c is found by walking from the row before's answer:
// down while the count below still passes, else up to the first that does -- two or three distances a row.
void csup_keep_table(int kmer_size, double threshold, uint32_t max_denom, uint32_t* out) {
  out[0] = 1;
  uint32_t c = 1;
  for (uint32_t d = 1; d <= max_denom; d++) {
    c = std::min(std::max<uint32_t>(c, 1), d);
    if (csup_passes(c, d, kmer_size, threshold)) {
      while (c > 1 && csup_passes(c - 1, d, kmer_size, threshold)) c--;
    } else {
      do c++; while (c <= d && !csup_passes(c, d, kmer_size, threshold));
    }
    out[d] = c;  // d + 1: none
  }
}

}  // namespace

extern "C" int rtc_support_keep_table(int kmer_size, double threshold, uint32_t max_denom, uint32_t* out) {
  if (!out || kmer_size < 1 || !(threshold >= 0.0)) return RTC_ERR_ARG;
  if ((uint64_t)max_denom + 1 > CSUP_TABLE_MAX) return RTC_ERR_UNSUPPORTED;
  csup_keep_table(kmer_size, threshold, max_denom, out);
  return RTC_OK;
}

extern "C" int rtc_cluster_support_counters(const rtc_ctx* ctx, uint64_t out[10]) {
  if (!ctx || !out) return RTC_ERR_ARG;
  for (int i = 0; i < 10; i++) out[i] = ctx->csupport[i];
  return RTC_OK;
}

extern "C" int rtc_components64_dev(rtc_ctx* ctx, uint32_t n, const rtc_cedge* d_edges, const uint64_t* d_mask, uint64_t m, uint32_t* d_label) {
  if (!ctx) return RTC_ERR_ARG;
  if ((m && (!d_edges || !d_mask)) || (n && !d_label)) return RTC_ERR_ARG;
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "rtc_components64_dev: n must be below 2^31 - 1");
  if (m == 0 || n == 0) return RTC_OK;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  DevBuf db;
  uint32_t* d_flag = nullptr;
  RTC_TRY(db.get(ctx, 1, &d_flag));
  return csup_components(ctx, n, d_edges, d_mask, m, d_label, d_flag, nullptr);
}

extern "C" int rtc_cluster_support(rtc_ctx* ctx, const void* d_hashes, int width, const uint64_t* d_start, const uint32_t* d_len, uint32_t n,
                                   const uint32_t* h_comp, int kmer_size, double threshold, uint32_t replicates, uint64_t seed, rtc_csupport* h_out,
                                   uint64_t* h_together) {
  const char* who = "rtc_cluster_support";
  if (!ctx || (n && (!d_hashes || !d_start || !d_len || !h_comp || !h_out || !h_together)) || (width != 4 && width != 8)) return RTC_ERR_ARG;
  memset(ctx->csupport, 0, sizeof ctx->csupport);
  if (kmer_size < 1) return rtc_fail(ctx, RTC_ERR_ARG, "%s: k-mer size %d", who, kmer_size);
  if (n >= 0x7fffffffu) return rtc_fail(ctx, RTC_ERR_ARG, "%s: %u sketches", who, n);
  if (replicates < 1 || replicates > CSUP_MAX_REPLICATES) return rtc_fail(ctx, RTC_ERR_ARG, "%s: replicates must lie in 1 .. %u", who, CSUP_MAX_REPLICATES);
  if (!(threshold >= 0.0)) return rtc_fail(ctx, RTC_ERR_ARG, "%s: the threshold must be at least 0", who);
  if (threshold >= 1.0)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: threshold %g: pairs without a common hash are at distance 1 and no list holds them", who, threshold);
  uint64_t* S = ctx->csupport;
  const uint64_t t_begin = now_ns();
  if (n == 0) return RTC_OK;
  const uint32_t B = replicates, W = (B + 63) / 64;
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;

  // ---- the keep table over every denominator a pair can have: the two longest sketches together ----
  std::vector<uint32_t> h_len(n);
  RTC_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  uint64_t len1 = 0, len2 = 0;
  for (uint32_t l : h_len) { if (l > len1) { len2 = len1; len1 = l; } else if (l > len2) len2 = l; }
  if (len1 >= 0x80000000ull) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: a sketch of %llu hashes, the distance is defined below 2^31", who, (unsigned long long)len1);
  const uint64_t D = len1 + len2;
  if (D + 1 > CSUP_TABLE_MAX)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: the keep table would have %llu entries (the two longest sketches together, and one), the cap is %llu", who,
                    (unsigned long long)(D + 1), (unsigned long long)CSUP_TABLE_MAX);
  std::vector<uint32_t> need(D + 1);
  csup_keep_table(kmer_size, threshold, (uint32_t)D, need.data());

  // ---- clusters in order of their smallest member, members ascending ----
  std::vector<uint32_t> cl(n), csize, perm(n);
  {
    std::unordered_map<uint32_t, uint32_t> number;
    number.reserve(n);
    for (uint32_t g = 0; g < n; g++) {
      auto it = number.find(h_comp[g]);
      if (it == number.end()) { it = number.emplace(h_comp[g], (uint32_t)csize.size()).first; csize.push_back(0); }
      cl[g] = it->second;
      csize[it->second]++;
    }
  }
  const uint32_t n_cl = (uint32_t)csize.size();
  std::vector<uint32_t> cfirst(n_cl + 1, 0);
  for (uint32_t c = 0; c < n_cl; c++) cfirst[c + 1] = cfirst[c] + csize[c];
  {
    std::vector<uint32_t> at(cfirst.begin(), cfirst.end() - 1);
    for (uint32_t g = 0; g < n; g++) perm[at[cl[g]]++] = g;
  }

  // ---- device state ----
  const uint64_t total = (uint64_t)n * 64;
  const uint64_t pairs_all = (uint64_t)n * (n - 1) / 2;
  const uint64_t piece_cap = std::max<uint64_t>(64, std::min<uint64_t>(CSUP_PIECE_EDGES, pairs_all));
  const uint64_t word_bytes = total * 8 + (uint64_t)n_cl * 8 + piece_cap * (sizeof(rtc_cedge) + 8);  // labels, sizes, crossing words, kept edges
  const uint64_t budget = ctx->opt.support_bytes ? ctx->opt.support_bytes : rtc_free_hbm(ctx) / 2;
  const uint32_t held = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(W, budget / word_bytes));
  DevBuf db;
  auto nomem = [&](int st, uint64_t bytes) -> int {
    if (st != RTC_ERR_NOMEM) return st;
    const std::string why = ctx->err;
    return rtc_fail(ctx, RTC_ERR_NOMEM, "%s: %llu bytes (%u word(s) of 64 replicates at %llu bytes, the counts of %llu candidates and the tables): %s", who,
                    (unsigned long long)bytes, held, (unsigned long long)word_bytes, (unsigned long long)piece_cap, why.c_str());
  };
  const uint64_t all_bytes = (uint64_t)held * word_bytes + piece_cap * 256 + (D + 1) * 4 + (uint64_t)n * 16 + (uint64_t)n_cl * (4 + sizeof(rtc_csupport));
  uint32_t *d_need = nullptr, *d_cl = nullptr, *d_perm = nullptr, *d_cfirst = nullptr, *d_common = nullptr, *d_flag = nullptr;
  rtc_csupport* d_out = nullptr;
  unsigned long long *d_together = nullptr, *d_cnt = nullptr, *d_paircnt = nullptr;
  std::vector<uint32_t*> d_label(held, nullptr), d_size(held, nullptr);
  std::vector<unsigned long long*> d_cross(held, nullptr);
  std::vector<rtc_cedge*> d_kept(held, nullptr);
  std::vector<uint64_t*> d_kmask(held, nullptr);
#define CSUP_GET(count, ptr) do { const int st__ = db.get(ctx, (size_t)(count), ptr); if (st__ != RTC_OK) return nomem(st__, all_bytes); } while (0)
  CSUP_GET(D + 1, &d_need);
  CSUP_GET(n, &d_cl);
  CSUP_GET(n, &d_perm);
  CSUP_GET(n_cl + 1, &d_cfirst);
  CSUP_GET(n_cl, &d_out);
  CSUP_GET(n, &d_together);
  CSUP_GET(8 + held, &d_cnt);  // [1] inner kept, [2] crossing kept, [8 + h] the kept list of held word h
  CSUP_GET(1, &d_paircnt);
  CSUP_GET(1, &d_flag);
  CSUP_GET(piece_cap * 64, &d_common);
  for (uint32_t h = 0; h < held; h++) {
    CSUP_GET(total, &d_label[h]);
    CSUP_GET(total, &d_size[h]);
    CSUP_GET(n_cl, &d_cross[h]);
    CSUP_GET(piece_cap, &d_kept[h]);
    CSUP_GET(piece_cap, &d_kmask[h]);
  }
#undef CSUP_GET
  RTC_HIP(ctx, hipMemcpyAsync(d_need, need.data(), (D + 1) * 4, hipMemcpyHostToDevice, s));
  RTC_HIP(ctx, hipMemcpyAsync(d_cl, cl.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  RTC_HIP(ctx, hipMemcpyAsync(d_perm, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  RTC_HIP(ctx, hipMemcpyAsync(d_cfirst, cfirst.data(), ((size_t)n_cl + 1) * 4, hipMemcpyHostToDevice, s));
  RTC_HIP(ctx, hipMemsetAsync(d_out, 0, (size_t)n_cl * sizeof(rtc_csupport), s));
  RTC_HIP(ctx, hipMemsetAsync(d_together, 0, (size_t)n * 8, s));
  RTC_HIP(ctx, hipMemsetAsync(d_cnt, 0, (8 + (size_t)held) * 8, s));
  const int radio = rtc_size_radio(threshold, kmer_size);

  for (uint32_t w0 = 0; w0 < W; w0 += held) {
    const uint32_t nh = std::min(held, W - w0);
    auto lanes_of = [&](uint32_t h) { return std::min<uint32_t>(64, B - 64 * (w0 + h)); };
    // ---- a fresh state per word: every genome its own piece, no crossing edge seen, size_r of every sketch ----
    const uint64_t tc0 = now_ns();
    for (uint32_t h = 0; h < nh; h++) {
      hipLaunchKernelGGL(csup_identity_kernel, dim3(blocks_for(total, ctx->num_cu)), dim3(256), 0, s, d_label[h], total);
      RTC_CHECK_LAUNCH(ctx);
      RTC_HIP(ctx, hipMemsetAsync(d_cross[h], 0, (size_t)n_cl * 8, s));
      RTC_TRY(rtc_jackknife_pairs_dev(ctx, d_hashes, width, d_start, d_len, n, nullptr, 0, seed, w0 + h, nullptr, d_size[h]));
    }
    RTC_HIP(ctx, hipStreamSynchronize(s));
    S[6] += now_ns() - tc0;
    if (n >= 2) {
      PairPhase pp;
      auto on_chunk = [&](const rtc_cedge* d_cand, uint64_t cnt) -> int {
        for (uint64_t p0 = 0; p0 < cnt; p0 += piece_cap) {
          const uint64_t mp = std::min<uint64_t>(piece_cap, cnt - p0);
          // ---- the counts and the masks of the piece, word after word through one count buffer ----
          const uint64_t t0 = now_ns();
          RTC_HIP(ctx, hipMemsetAsync(d_cnt + 8, 0, (size_t)held * 8, s));
          for (uint32_t h = 0; h < nh; h++) {
            RTC_TRY(rtc_jackknife_pairs_dev(ctx, d_hashes, width, d_start, d_len, n, d_cand + p0, mp, seed, w0 + h, d_common, nullptr));
            hipLaunchKernelGGL(csup_mask_kernel, dim3(csup_grid((mp + CSUP_TILE - 1) / CSUP_TILE, ctx->num_cu)), dim3(256), 0, s, d_cand + p0, mp,
                               (const uint32_t*)d_common, (const uint32_t*)d_size[h], (const uint32_t*)d_need, (uint32_t)D, (const uint32_t*)d_cl, lanes_of(h),
                               d_kept[h], d_kmask[h], piece_cap, d_cnt + 8 + h, d_cnt, d_cross[h]);
            RTC_CHECK_LAUNCH(ctx);
          }
          void* hp = nullptr;  // the context's staging is shared: the passes below read their flag through it
          RTC_TRY(rtc_pinned(ctx, 64 + 8 * (size_t)held, &hp));
          RTC_HIP(ctx, hipMemcpyAsync(hp, d_cnt + 8, (size_t)held * 8, hipMemcpyDeviceToHost, s));
          RTC_HIP(ctx, hipStreamSynchronize(s));
          uint64_t mk[4] = {0, 0, 0, 0};  // at most mp each: a candidate is appended once
          for (uint32_t h = 0; h < nh; h++) mk[h] = ((const unsigned long long*)hp)[h];
          const uint64_t t1 = now_ns();
          S[6] += t1 - t0;
          // ---- the kept inner edges into the words' labels ----
          for (uint32_t h = 0; h < nh; h++)
            RTC_TRY(csup_components(ctx, n, d_kept[h], d_kmask[h], std::min<uint64_t>(mk[h], piece_cap), d_label[h], d_flag, &S[4]));
          S[7] += now_ns() - t1;
        }
        return RTC_OK;
      };
      const int st = dbscan_pair_chunks(ctx, db, d_hashes, width, d_start, d_len, n, 1, d_paircnt, &pp, on_chunk, radio);
      if (st != RTC_OK) {  // the chunk loop names rtc_dbscan, whose loop it is
        if (st == RTC_ERR_HIP) return st;
        const std::string why = ctx->err;
        return rtc_fail(ctx, st, "%s: in the pair phase: %s", who, why.c_str());
      }
      S[0] += pp.chunks;
      if (w0 == 0) S[1] = pp.cand_total;
      S[5] += pp.pair_ns;
    }
    // ---- the tally of the words held ----
    const uint64_t tt0 = now_ns();
    for (uint32_t h = 0; h < nh; h++) {
      uint32_t* d_psize = d_size[h];  // the sizes are done with
      RTC_HIP(ctx, hipMemsetAsync(d_psize, 0, total * 4, s));
      hipLaunchKernelGGL(csup_tally_kernel, dim3(csup_grid(n_cl, ctx->num_cu)), dim3(256), 0, s, (const uint32_t*)d_perm, (const uint32_t*)d_cfirst, n_cl,
                         (const uint32_t*)d_label[h], (const unsigned long long*)d_cross[h], lanes_of(h), d_psize, d_out);
      RTC_CHECK_LAUNCH(ctx);
      hipLaunchKernelGGL(csup_together_kernel, dim3(csup_grid(n, ctx->num_cu)), dim3(256), 0, s, (const uint32_t*)d_label[h], (const uint32_t*)d_psize, n,
                         lanes_of(h), d_together);
      RTC_CHECK_LAUNCH(ctx);
    }
    RTC_HIP(ctx, hipStreamSynchronize(s));
    S[8] += now_ns() - tt0;
  }
  void* hp = nullptr;
  RTC_TRY(rtc_pinned(ctx, 64, &hp));
  RTC_HIP(ctx, hipMemcpyAsync(hp, d_cnt, 64, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(h_out, d_out, (size_t)n_cl * sizeof(rtc_csupport), hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipMemcpyAsync(h_together, d_together, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  RTC_HIP(ctx, hipStreamSynchronize(s));
  S[2] = ((const unsigned long long*)hp)[1];
  S[3] = ((const unsigned long long*)hp)[2];
  S[9] = now_ns() - t_begin;
  return RTC_OK;
}
