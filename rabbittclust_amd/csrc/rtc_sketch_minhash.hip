// rtc_sketch_minhash.hip -- bottom-s MinHash sketching on gfx950.
//
// Replaces Sketch::MinHash::{update,storeMinHashes} driven from src/SketchInfo.cpp:918-942,969
// (reference tree paths).  One workgroup (512 lanes = 8 wave64) walks one *segment* of a genome:
//   * every lane owns 76 consecutive k-mer end positions of a 38 KiB tile and reads its 96 bases
//     (20 warm-up + 76 owned; 112 = 36 + 76 for k > 21) straight from global memory as 16-byte loads, decoding four
//     bases at once and rolling the 2-bit forward / reverse-complement words;
//   * MurmurHash3_x64_128 of the canonical k-mer's ASCII bytes is evaluated from the 2-bit word:
//     the first multiplication of every input word comes out of LDS product tables (linearity of
//     multiplication mod 2^64), leaving seven 64x64 multiplies per k-mer (72 VALU instructions
//     for k = 21, with hand-picked forms for rotates, x5 and the table offsets);
//   * hashes below the running threshold T (kept in SGPRs) are appended to an LDS candidate buffer
//     with one LDS atomic per wave; when the buffer fills, an in-LDS bitonic sort over the live
//     count + dedup keeps the s smallest distinct values and lowers T.
// Large genomes / small batches are split into several segments whose partial sketches are
// merged by merge_partials_kernel (bottom-s is a mergeable summary).  The segments of a genome all start
// from the genome's threshold (3x the expected s-th smallest hash), as a whole-genome workgroup does; a
// genome whose merged partial sketches hold fewer than s hashes is flagged and walked once more without it
// (a second, gated launch over the partial segments -- every other workgroup of it leaves at once).
// The candidate path -- workgroup state in LDS, threshold tests, the per-wave queue, appends, the tile protocol, the final
// fold and write-out -- is rtc_minhash_core.h's, one copy for this unit and rtc_sketch_minhash_packed.hip; what is written
// here is what ASCII input needs: the loads, the decode, the per-base roll, the express loop and the run / clean bookkeeping.
#include "rtc_minhash_core.h"

namespace {

template <int KT, bool PK>  // KT > 0: k known at compile time (uniform branches fold away); 0: runtime k.  PK: packed tables
// second launch bound: 6 waves/SIMD = 3 workgroups per CU (caps the allocation at 80 VGPRs)
__global__ __launch_bounds__(WG, 6) void sketch_minhash_kernel(const uint8_t* __restrict__ seq,
                                                            const Segment* __restrict__ segs,
                                                            int k_arg, uint32_t seed, int cap,
                                                            uint64_t* out,
                                                            uint32_t* cnt, int pass_no,
                                                            uint64_t* parts, uint32_t* pcnt,
                                                            const uint32_t* __restrict__ redo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int k = KT > 0 ? KT : k_arg;
  constexpr int WARM_DW = warm_dw(KT);
  const Segment sg = segs[blockIdx.x];
  const WgState W = carve_lds(smem, k, PK, cap, sg.sketch_size);
  uint64_t lo1;  // later passes of a large sketch: only hashes from lo1 up (0: the first pass)
  if (!pass_gate(sg, pass_no, redo, cnt, out, pcnt, lo1)) return;  // workgroup-uniform
  // compile-time-k instantiations serve the reference's seed only (MASH_SEED, the launch sends any other seed to the
  // runtime-k kernel): as an inline constant the two seed xors per k-mer stay fast-class VALU (an SGPR source makes
  // v_xor_b32 a 4.4-cycle instruction, profiles/r03_valu_issue_cost2.txt)
  const KParams P = make_kparams(k, KT > 0 ? MASH_SEED : seed, PK, KT > 0);
  const int t = W.t;
  const uint32_t s = W.s;
  const bool fastroll = true;     // four bases per step: 64-bit extended windows for k <= 28, 128-bit ones above
  uint32_t qn = 0;  // entries waiting in this wave's candidate queue (wave-uniform)

  // Starting threshold.  A whole-genome workgroup knows how many k-mers are coming: the s-th smallest of N
  // uniform hashes will be near 2^64 * s / N, so it starts at T0 = 3x that (2x for dense sketches; start_threshold, host side) instead of "everything passes".
  // This skips the first tiles' flood of candidates (a dozen merges under per-dword barriers: the cost that
  // grew with s -- 6 % of the kernel at s = 1000, 20 % with 1 Mbp genomes) and changes nothing in the
  // result as long as s distinct hashes below T0 exist (3 s expected); if fewer than s were found -- a
  // genome with few distinct k-mers -- the workgroup simply runs again from T0 = "none".
  // (A partial segment starts from the genome's T0 as well: the union of the segments' hashes below T0 holds the s
  // smallest of the genome whenever s of them exist; if not, the merge flags the genome for the second launch.)
  uint64_t Tstart = (pass_no == 0 && !redo) ? sg.t0 : SENT;
restart:
  reset_ctrl(W, Tstart);
  build_kmer_lut(W.lut, k, PK, P.cross_tab);
  __syncthreads();

  uint64_t T = uniform64(Tstart);  // scalar registers: the threshold compares write wave masks directly
  qn = 0;
  bool safe_mode = first_tile_safe(W, Tstart, (uint32_t)TILE_BASES);

  uint32_t count_at_tile_start = 0;  // carried in registers: identical in every thread
  for (uint64_t T0 = sg.s_begin & ~15ULL; T0 < sg.s_end && s > 0; T0 += TILE_BASES) {
    // owned positions of this lane relative to T0: [OWN*t, OWN*t + OWN); hash window limits
    const int64_t lo64 = (int64_t)sg.s_begin - (int64_t)T0;
    const int64_t hi64 = (int64_t)sg.s_end - (int64_t)T0;
    const int rel_lo = lo64 < 0 ? 0 : (int)lo64;
    const int rel_hi = hi64 > TILE_BASES ? TILE_BASES : (int)hi64;
    const bool interior = rel_lo == 0 && rel_hi == TILE_BASES;  // every position of the tile is owned
    const uint8_t* tile = seq + T0;                 // wave-uniform
    const int rq0 = OWN * t - 4 * WARM_DW;          // first base of this lane's window, relative to the tile
    const int64_t gb64 = (int64_t)sg.g_begin - (int64_t)T0, ge64 = (int64_t)sg.g_end - (int64_t)T0;
    const int gb = gb64 < -(1 << 30) ? -(1 << 30) : (int)gb64;   // genome extent in tile coordinates
    const int ge = ge64 > (1 << 30) ? (1 << 30) : (int)ge64;

    do {
      uint64_t fwd = 0, rc = 0;
      int run = 0;
      bool clean = true;  // wave-uniform: only valid bases in every lane of this wave so far in this pass
      int g0 = 0;
      if constexpr (KT > 16 && KT <= 28) {
        // The steady state without the general walk's per-dword decisions: a wave whose windows lie inside the
        // genome, in a tile interior to the segment, outside safe mode, with a threshold whose high word
        // decides (see below), walks whole 16-byte groups -- validity of the group in one vote, the windows,
        // the hash halves, the high-word test, possible candidates to the queue -- until a group holds a
        // character outside ACGTacgt or the queue is full; the general walk takes over from that group.
        constexpr int NG = (WARM_DW + RUN_DW) / 4;
        const int w0 = (int)uniform32((uint32_t)(t & ~63));
        const int wlo = OWN * w0 - 4 * WARM_DW, whi = OWN * (w0 + 63) - 4 * WARM_DW + 16 * NG;
        const uint32_t Thi_e = (uint32_t)(T >> 32);
        if (!safe_mode && !lo1 && interior && Thi_e < 0xffffffffu - TEST_SLACK && wlo >= gb && whi <= ge) {
          const uint8_t* base = (tile - LOAD_BIAS) + (uint32_t)(rq0 + LOAD_BIAS);
          const uint32_t Thi1 = Thi_e + TEST_SLACK;
          uint4 cur = *reinterpret_cast<const uint4*>(base), nxt1 = *reinterpret_cast<const uint4*>(base + 16);
          // Both extended windows are kept top-aligned for ONE k-mer of a dword, which is then cut without a shift:
          // the forward one as FT = F << FS (first k-mer of the dword on top; the new byte enters at bit FS), the
          // reverse-complement one as R << RE with the newest byte in the top byte (last k-mer of the dword on top):
          // one v_perm (high word) + one v_alignbit (low word) roll it.
          constexpr int FS = 58 - 2 * KT, RE = 56 - 2 * KT;
          static_assert(FS >= 0 && FS + 8 <= 32 && RE >= 0, "express walk: 17 <= k <= 28");
          constexpr uint32_t RSEL = 0x00070605u;  // {rp byte 0, Rhi bytes 3, 2, 1}
          uint64_t FT = 0;
          uint32_t Rhi = 0, Rlo = 0;
          g0 = NG;
#pragma unroll
          for (int g = 0; g < NG; g++) {
            uint4 nxt2 = cur;
            if (g + 2 < NG) nxt2 = *reinterpret_cast<const uint4*>(base + 16 * (g + 2));
            const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
            uint32_t codes[4], bad = 0;
#pragma unroll
            for (int qd = 0; qd < 4; qd++) {
              codes[qd] = ((w[qd] >> 1) ^ (w[qd] >> 2)) & 0x03030303u;
              bad = __builtin_amdgcn_bitop3_b32(bad, __builtin_amdgcn_perm(0u, 0x54474341u, codes[qd]), w[qd], 0xF6);  // bad | (perm ^ w)
            }
            if (__ballot((bad & 0xDFDFDFDFu) != 0u)) { g0 = g; break; }
            const uint64_t FT0 = FT;
            const uint32_t Rhi0 = Rhi, Rlo0 = Rlo, qn0 = qn;
            bool lost = false;  // wave-uniform: the queue could not take this group's candidates
            // The k-mers of a group run as a two-stage pipeline: the table reads of k-mer n + 1 are issued before the
            // arithmetic of k-mer n, so a wave does not park on every LDS round trip (the compiler's own order issues a
            // word's reads right in front of their use: three waits per k-mer); the pipeline drains at the group's end.
            KmerLoads pend = {};
            bool have = false;  // (folds away: everything here is unrolled)
            auto finish_pending = [&]() __attribute__((always_inline)) { express_handoff(pend, P, Thi1, W.wq, qn, lost); };
#pragma unroll
            for (int qd = 0; qd < 4; qd++) {
              const uint32_t pack = __builtin_amdgcn_udot4(codes[qd], 0x01041040u, 0u, false);
              // reverse-complement byte 255 - (c0 + 4 c1 + 16 c2 + 64 c3) as the LOW BYTE of a dot product with the
              // weights 256 - {1, 4, 16, 64} on top of 255 (only that byte is used: v_perm picks it)
              const uint32_t rp = __builtin_amdgcn_udot4(codes[qd], 0xC0F0FCFFu, 255u, false);
              FT = (FT << 8) | (uint64_t)(pack << FS);  // v_lshlrev_b64 + v_lshl_or_b32
              const uint32_t nhi = __builtin_amdgcn_perm(Rhi, rp, RSEL);
              Rlo = __builtin_amdgcn_alignbit(Rhi, Rlo, 8);
              Rhi = nhi;
              const uint64_t R = ((uint64_t)Rhi << 32) | Rlo;  // = (general walk's R) << RE
              if (g * 4 + qd >= WARM_DW) {
#pragma unroll
                for (int b = 0; b < 4; b++) {
                  const uint64_t f = FT << (2 * b);
                  const uint64_t r = R << (6 - 2 * b);
                  const KmerLoads nl = kmer_loads(f < r ? f : r, P);
                  __builtin_amdgcn_sched_barrier(0);
                  if (have) finish_pending();
                  __builtin_amdgcn_sched_barrier(0);
                  pend = nl;
                  have = true;
                }
              }
            }
            if (have) finish_pending();
            if (lost) { FT = FT0; Rhi = Rhi0; Rlo = Rlo0; qn = qn0; g0 = g; break; }
            cur = nxt1;
            nxt1 = nxt2;
          }
          fwd = FT >> FS;
          rc = (((uint64_t)Rhi << 32) | Rlo) >> (RE + 8);  // the general walk's form
          run = 16 * g0;
        }
      }
      uint4 nxt = g0 < (WARM_DW + RUN_DW) / 4 ? load_bases16(tile, rq0 + 16 * g0, gb, ge) : make_uint4(0u, 0u, 0u, 0u);
      for (int grp = g0; grp < (WARM_DW + RUN_DW) / 4; grp++) {
        const uint4 cur = nxt;
        if (grp + 1 < (WARM_DW + RUN_DW) / 4) nxt = load_bases16(tile, rq0 + 16 * (grp + 1), gb, ge);
        const uint32_t wv4[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
        for (int qd = 0; qd < 4; qd++) {
          const int d = grp * 4 + qd;
          const uint32_t wv = wv4[qd];
          const bool hashing = d >= WARM_DW;  // wave-uniform
          const int rel0 = OWN * t + 4 * (d - WARM_DW);
          // (zero-initialised on purpose: left uninitialised, the generated code issues the tile loads in an
          // order that re-reads 40 % more of the input from the fabric -- measured, tools/pmc_runlen.sh)
          uint64_t canon[4] = {0, 0, 0, 0};  // top-aligned (first base in bit 63); hashing dwords only
          bool ok[4] = {false, false, false, false};  // slow path only; the fast path derives it on demand
          bool allok = false;  // wave-uniform: all four k-mers of every lane are valid and owned
          // ---- decode four bases at once ----
          const uint32_t up = wv & 0xDFDFDFDFu;
          const uint32_t codes4 = ((wv >> 1) ^ (wv >> 2)) & 0x03030303u;  // A,C,G,T (either case) -> 0..3 per byte
          const bool allvalid = __builtin_amdgcn_perm(0u, 0x54474341u, codes4) == up;
          const bool fast = fastroll && __all(allvalid);  // wave-uniform
          clean = clean && fast;
          const int run_in = run;
          if (fast) {
            // pack = c0<<6|c1<<4|c2<<2|c3 ; rp = complement codes in reverse significance; both are
            // byte dot products of the four codes (v_dot4_u32_u8)
            const uint32_t pack = __builtin_amdgcn_udot4(codes4, 0x01041040u, 0u, false);
            const uint32_t rp = __builtin_amdgcn_udot4(codes4, 0x40100401u, 0u, false) ^ 0xffu;
            // bits of fwd above the window shift out when the windows are cut, so it carries unmasked
            // Scalar ownership test for the steady state: in a tile interior to the segment, a wave
            // that has seen only valid bases since the tile began has run = 4d >= 4*WARM_DW >= k-1 in every
            // lane, and every position of the tile is owned.  Anything else takes the per-lane test.
            if (hashing) allok = interior && clean;
            cut_kmers(fwd, rc, pack, rp, P, hashing, canon);  // warm-up dwords only roll the windows
            run += 4;
          } else {
#pragma unroll
            for (int b = 0; b < 4; b++) {
              const uint32_t c = (wv >> (8 * b)) & 0xffu;
              const uint32_t code = ((c >> 1) ^ (c >> 2)) & 3u;
              const bool valid = ((c & 0xC0u) == 0x40u) && ((0x0010008Au >> (c & 31u)) & 1u);
              fwd = ((fwd << 2) | code) & P.kmask;
              rc = (rc >> 2) | ((uint64_t)(code ^ 3u) << P.rc_shift);
              run = valid ? run + 1 : 0;
              const int rel = rel0 + b;
              ok[b] = run >= P.k && rel >= rel_lo && rel < rel_hi;
              canon[b] = (fwd < rc ? fwd : rc) << P.lshift;
            }
          }
          if (hashing) {  // wave-uniform
            kmer_step4(W, P, canon, allok, T, lo1, qn, safe_mode, [&](int b) __attribute__((always_inline)) {
              const int rel = rel0 + b;  // the fast path derives a k-mer's validity here, on demand
              return fast ? (run_in + b + 1 >= P.k && rel >= rel_lo && rel < rel_hi) : ok[b];
            });
          }
        }
      }  // 16-byte groups of the lane's window
    } while (tile_overflowed(W, T, count_at_tile_start, safe_mode));
    end_tile(W, T, qn, count_at_tile_start, safe_mode);
  }

  if (finish_sketch(W, sg, T, qn, Tstart, pass_no, out, cnt, parts, pcnt)) goto restart;
}

RTC_MINHASH_PICK(pick_kernel, sketch_minhash_kernel)

}  // namespace

extern "C" int rtc_sketch_minhash_dev(rtc_ctx* ctx, const uint8_t* d_seq, const uint64_t* h_off,
                                      uint32_t n, int k, uint32_t seed, const uint32_t* h_sizes,
                                      uint32_t size, uint64_t* d_out, uint32_t stride,
                                      uint32_t* d_cnt) {
  if (!ctx || !h_off || (n && (!d_seq || !d_out || !d_cnt))) return RTC_ERR_ARG;
  if (k < 1 || k > 32) return rtc_fail(ctx, RTC_ERR_ARG, "k=%d outside 1..32", k);
  if (n == 0) return RTC_OK;
  if (((uintptr_t)d_seq & 15) != 0) return rtc_fail(ctx, RTC_ERR_ARG, "d_seq must be 16-byte aligned");
  auto prepare = [&](const MinhashPlanInfo& pi) -> int {
    RTC_HIP(ctx, hipFuncSetAttribute((const void*)pick_kernel(k, seed, false, pi.packed_tables), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pi.lds));
    RTC_HIP(ctx, hipFuncSetAttribute((const void*)pick_kernel(k, seed, true, pi.packed_tables), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pi.lds));
    return RTC_OK;
  };
  auto launch = [&](const MinhashLaunch& L) -> int {
    hipLaunchKernelGGL(pick_kernel(k, seed, L.runtime_k, L.packed_tables), dim3(L.nseg), dim3(WG), L.lds, ctx->stream, d_seq, L.d_segs, k, seed, L.cap, d_out,
                       d_cnt, L.pass, L.d_parts, L.d_pcnt, L.d_redo);
    RTC_CHECK_LAUNCH(ctx);
    return RTC_OK;
  };
  return minhash_run(ctx, h_off, n, k, h_sizes, size, d_out, stride, d_cnt, (uint64_t)TILE_BASES, (size_t)MIN_ROOM, prepare, launch);
}

extern "C" int rtc_sketch_minhash_plan(rtc_ctx* ctx, int k, uint32_t size, int* wgs_per_cu, int* packed_tables, uint64_t* lds_bytes) {
  if (k < 1 || k > 32) return ctx ? rtc_fail(ctx, RTC_ERR_ARG, "k=%d outside 1..32", k) : RTC_ERR_ARG;
  rtc_options env;
  if (!ctx) rtc_options_from_env(&env);
  const MinhashLayout lay = minhash_layout(ctx ? ctx->opt : env, k, std::min(size, PASS_CHUNK), (size_t)MIN_ROOM);
  if (lay.cap == 0) return ctx ? rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "sketch chunk %u does not fit the LDS", std::min(size, PASS_CHUNK)) : RTC_ERR_UNSUPPORTED;
  if (wgs_per_cu) *wgs_per_cu = lay.wgs_per_cu;
  if (packed_tables) *packed_tables = lay.packed ? 1 : 0;
  if (lds_bytes) *lds_bytes = (uint64_t)lay.cap * 8 + lut_bytes(k, lay.packed) + ((sizeof(Ctrl) + 15) & ~(size_t)15) + QUEUE_BYTES;
  return RTC_OK;
}

namespace { __global__ void touch_unit_kernel() {} }
int rtc_touch_sketch_minhash(rtc_ctx* ctx) {
  hipLaunchKernelGGL(touch_unit_kernel, dim3(1), dim3(64), 0, ctx->stream);
  RTC_CHECK_LAUNCH(ctx);
  return RTC_OK;
}
