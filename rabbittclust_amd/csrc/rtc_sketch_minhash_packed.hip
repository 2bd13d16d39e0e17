// rtc_sketch_minhash_packed.hip -- bottom-s MinHash sketching straight from the 2-bit staging format (gfx950).
//
// The reference hands Sketch::MinHash::update() ASCII records (src/SketchInfo.cpp:928-948); the command lines stage
// 2-bit codes plus a run list of everything outside ACGT (rtc_host.cpp: PackedSink; include/rtclust.h,
// rtc_unpack_bases_dev for the layout).  rtc_sketch_minhash.hip reads characters -- the batch had to be expanded
// again in HBM in front of a kernel whose first act is to squeeze the characters back into two bits.  This unit is
// the same sketcher fed the packed stream as it crossed PCIe:
//   * a lane owns the 64 k-mer end positions of ONE 16-byte load; a wave's load is 1 KiB of contiguous stream
//     (4 096 bases), every line requested once.  The 32 bases in front of a lane's first come with one 8-byte load
//     of their own: no warm-up bases are walked at all (the ASCII kernel rolls 20 per 76 owned positions);
//   * a byte of the stream IS four bases: the forward window takes the byte with its pairs reversed (one v_bfrev and
//     three bit operations per 16 bases), the reverse-complement window the complemented byte as it lies (the
//     stream's order is the reverse strand's); both windows roll by one v_perm + one v_alignbit -- no SWAR decode,
//     no re-encoding votes, no v_dot4;
//   * what the characters were is the run list's business: a k-mer counts exactly when none of its k bases lies in
//     a run or outside its genome.  A wave asks once per load whether any run can touch its 4 096 bases (a scalar
//     cursor into the segment's run range, seg_runs_kernel of rtc_runs.h); only a wave that meets one builds per-lane
//     validity masks and takes the general walk.
// Everything behind the k-mers is rtc_minhash_core.h's, one copy for this unit and the ASCII one: the hash (MurmurHash3
// from LDS product tables), the workgroup state in LDS, the cut and roll of the general walk's windows, the threshold tests, the
// candidate queue, appends, the tile protocol, the in-LDS merges, the final fold and write-out, kernel selection, the
// segment plan and the partial-sketch merge.  Written here: loads, window seeds, the express loop with its rolls, the masks and
// the run cursor.  Results are identical to the ASCII unit's and to the oracle bit for bit
// (tests/test_gpu_sketch_minhash_packed.py).
#include "rtc_minhash_core.h"
#include "rtc_runs.h"

namespace {

constexpr int P_NL = 4;                        // 16-byte loads (64 bases each) per lane and tile
constexpr int P_CHUNK = 64 * 64;               // bases of one wave load
constexpr int P_TILE_BASES = WG * 64 * P_NL;   // bases per tile: the workgroup meets its tile protocol once per 131 072 bases
// The segment plan keeps counting in tiles of one load per lane (min_seg, seg_pref of minhash_run): what a tile costs the
// walk changed, what a segment should hold did not, and the plans of every shape stay what they were measured with.
constexpr uint64_t P_PLAN_BASES = (uint64_t)WG * 64;

struct PackedIn {
  const uint8_t* bytes;     // packed bases: base i at bits 2 (i & 3) of bytes[i >> 2]
  uint64_t n_bases;         // a multiple of 64
  const uint64_t* runs;     // (start, length) pairs, ascending and disjoint
};

// 16 packed bases (first base in the low bits) -> first base on top, every base's two bits in order
__device__ __forceinline__ uint32_t pair_rev(uint32_t x) {
  const uint32_t y = __brev(x);  // pairs in order, the two bits of a pair swapped
  return ((y << 1) & 0xAAAAAAAAu) | ((y >> 1) & 0x55555555u);
}

// v_perm selector of the forward window's roll: new low word = (low word << 8) | byte 3 - q of the pair-reversed dword at
// the byte boundary fsb (operands: S0 = low word -> bytes 4..7, S1 = the dword -> bytes 0..3; 0x0c = a zero byte)
__host__ __device__ constexpr uint32_t fwd_roll_sel(int fsb, int q) {
  uint32_t sel = 0;
  for (int j = 0; j < 4; j++) sel |= (j > fsb / 8 ? (uint32_t)(3 + j) : j == fsb / 8 ? (uint32_t)(3 - q) : 0x0cu) << (8 * j);
  return sel;
}

// What a tile's loads ask about it, 32-bit and relative to its first base (extents clamped to +-2^30: a tile is 2^17 bases)
struct TileView {
  int rel_lo, rel_hi;   // the tile's owned positions
  int gb, ge;           // the genome's extent
  int nb;               // bytes of the buffer from the tile's first byte on
  int pb;               // first byte offset with eight bytes of buffer in front of it
};
__device__ __forceinline__ int clamp30(int64_t x) { return x < -(1 << 30) ? -(1 << 30) : x > (1 << 30) ? (1 << 30) : (int)x; }
__device__ __forceinline__ TileView tile_view(const Segment& sg, uint64_t TB, uint64_t n_bases) {
  TileView V;
  const int lo = clamp30((int64_t)sg.s_begin - (int64_t)TB), hi = clamp30((int64_t)sg.s_end - (int64_t)TB);
  V.rel_lo = lo < 0 ? 0 : lo;
  V.rel_hi = hi > P_TILE_BASES ? P_TILE_BASES : hi;
  V.gb = clamp30((int64_t)sg.g_begin - (int64_t)TB);
  V.ge = clamp30((int64_t)sg.g_end - (int64_t)TB);
  V.nb = clamp30((int64_t)(n_bases >> 2) - (int64_t)(TB >> 2));
  V.pb = TB == 0 ? 8 : 0;  // (a tile starts at a multiple of 64 bases)
  return V;
}

// names the fields of a k-mer's table words as values without writing them (no instruction)
__device__ __forceinline__ void undefined_loads(KmerLoads& L) {
#pragma unroll
  for (int w = 0; w < 4; w++) {
    asm("" : "=v"(L.e[w].x), "=v"(L.e[w].y), "=v"(L.e[w].z), "=v"(L.e[w].w));
    asm("" : "=v"(L.bl[w].x), "=v"(L.bl[w].y));
  }
  asm("" : "=v"(L.dt));
}

template <int KT, bool PK>  // KT > 0: k known at compile time; 0: runtime k.  PK: packed hash tables (lut_bytes)
__global__ __launch_bounds__(WG, 6) void sketch_minhash_packed_kernel(PackedIn B, const Segment* __restrict__ segs,
                                                                   const uint2* __restrict__ seg_runs,
                                                                   int k_arg, uint32_t seed, int cap,
                                                                   uint64_t* out,
                                                                   uint32_t* cnt, int pass_no,
                                                                   uint64_t* parts, uint32_t* pcnt,
                                                                   const uint32_t* __restrict__ redo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int k = KT > 0 ? KT : k_arg;
  const Segment sg = segs[blockIdx.x];
  const WgState W = carve_lds(smem, k, PK, cap, sg.sketch_size);
  uint64_t lo1;  // later passes of a large sketch: only hashes from lo1 up (0: the first pass)
  if (!pass_gate(sg, pass_no, redo, cnt, out, pcnt, lo1)) return;  // workgroup-uniform
  lo1 = uniform64(lo1);
  const KParams P = make_kparams(k, KT > 0 ? MASH_SEED : seed, PK, KT > 0);  // compile-time k serves the reference's seed only
  const uint32_t lane = W.lane;
  const int wv = (int)uniform32((uint32_t)(W.t >> 6));
  const uint32_t s = W.s;
  uint32_t qn = 0;  // entries waiting in this wave's candidate queue (wave-uniform)
  const uint2 sr = seg_runs[blockIdx.x];
  const bool has_runs = sr.x != sr.y;  // workgroup-uniform: most segments of a finished genome meet no run at all

  uint64_t Tstart = (pass_no == 0 && !redo) ? sg.t0 : SENT;  // starting threshold (segment plan); lifted if it proves too optimistic
restart:
  reset_ctrl(W, Tstart);
  build_kmer_lut(W.lut, k, PK, P.cross_tab);
  __syncthreads();

  uint64_t T = uniform64(Tstart);
  qn = 0;
  bool safe_mode = first_tile_safe(W, Tstart, (uint32_t)P_TILE_BASES);
  uint32_t qlast = 0;    // what this wave's last load left in its queue (wave-uniform)
  uint32_t rcur = sr.x;  // wave-uniform cursor into the run list: every run in front of it ends before anything this wave still looks at

  uint32_t count_at_tile_start = 0;
  for (uint64_t TB = sg.s_begin & ~63ULL; TB < sg.s_end && s > 0; TB += P_TILE_BASES) {
    // Everything a load asks is 32-bit and relative to the tile.  The express walk reads two scalars of it: the loads
    // it may take start in [ex_lo, ex_hi - P_CHUNK].
    const TileView V = tile_view(sg, TB, B.n_bases);
    const uint8_t* const tile = B.bytes + (TB >> 2);              // wave-uniform
    const uint32_t rcur_tile = rcur;                              // a tile walked again starts from here again

    do {
      rcur = rcur_tile;
      // Express eligibility is a property of the wave's load (4 096 positions), not of the tile: its positions are all
      // owned ([rel_lo, rel_hi)) and they and their k - 1 predecessors lie in the genome -- so a tile at a segment or
      // genome edge still walks its clean loads express.  What holds for the whole tile (mode, pass, a high word that
      // decides) empties the range instead.
      int ex_lo = 1 << 30, ex_hi = 0;
      uint32_t Thi1 = 0;
      if constexpr (KT > 16 && KT <= 28) {
        const uint32_t Thi_e = (uint32_t)(T >> 32);
        if (!safe_mode && !lo1 && Thi_e < 0xffffffffu - TEST_SLACK) {
          ex_lo = V.rel_lo > V.gb + (KT - 1) ? V.rel_lo : V.gb + (KT - 1);
          ex_hi = V.rel_hi < V.ge ? V.rel_hi : V.ge;
          Thi1 = Thi_e + TEST_SLACK;
        }
      }
      ex_lo = (int)uniform32((uint32_t)ex_lo);  // scalars by construction: a load's branch is a scalar compare
      ex_hi = (int)uniform32((uint32_t)ex_hi);
#pragma unroll 1
      for (int j = 0; j < P_NL; j++) {
        // this wave's load: first base relative to the tile (wave-uniform).  The waves' loads interleave, so that a tile
        // only part of which is owned (a segment's last) still spreads over all eight waves; a wave's own loads ascend,
        // which is all its run cursor asks.
        const int crel = (j * NWAVE + wv) * P_CHUNK;
        // Outside safe mode a load that owns no position has nothing to do (the tile behind a segment's end, the loads
        // in front of its begin); in safe mode every wave meets the barriers of all its steps.
        if (!safe_mode && (crel >= V.rel_hi || crel + P_CHUNK <= V.rel_lo)) continue;
        // A queue that the next load could fill is drained in front of it (outside safe mode appends need no barrier: a
        // buffer that cannot take them raises the overflow flag, and the tile is walked again): as many as three times
        // what the last load queued, and a few, must fit.  At a tile's end the queue drains as before.
        if (!safe_mode && qn > 0 && qn + 3 * qlast + 8 > (uint32_t)QCAP) drain_queue(W, qn, T);
        const uint32_t q_in = qn;
        // ---- the lane's 64 bases and the 32 in front of them (zeros outside the buffer: never part of a counted k-mer) ----
        uint32_t cw[4] = {0u, 0u, 0u, 0u}, p2 = 0u, p3 = 0u;
        auto load_guarded = [&](int lrel) __attribute__((always_inline)) {
          const int lb = lrel >> 2;  // byte of the lane's first base, relative to the tile's
          if (lb + 16 <= V.nb) {
            const uint4 v = *reinterpret_cast<const uint4*>(tile + lb);
            cw[0] = v.x; cw[1] = v.y; cw[2] = v.z; cw[3] = v.w;
          }
          if (lb >= V.pb && lb <= V.nb) {
            const uint2 v = *reinterpret_cast<const uint2*>(tile + (lb - 8));
            p2 = v.x; p3 = v.y;
          }
        };
        // ---- can a run touch this wave's bases?  (scalar: the cursor only moves forward) ----
        bool wave_dirty = false;
        if (has_runs) {
          load_guarded(crel + 64 * (int)lane);  // in flight under the cursor's scalar reads, whichever walk takes the load
          const int64_t first = (int64_t)TB + crel - 32;  // runs that end at or before it are behind this wave for good
          uint32_t rc = rcur;
          while (rc < sr.y) {
            const uint64_t en = B.runs[2 * (uint64_t)rc] + B.runs[2 * (uint64_t)rc + 1];
            if ((int64_t)en > first) break;
            rc++;
            if (rc - rcur == 8) { rc = first_run_ending_after(B.runs, rc, sr.y, first); break; }  // many runs behind: the rest by bisection
          }
          rcur = uniform32(rc);
          wave_dirty = rcur < sr.y && (int64_t)B.runs[2 * (uint64_t)rcur] < (int64_t)TB + crel + P_CHUNK;
        }

        bool done = false;       // wave-uniform: the express walk took this load
        bool lost_load = false;  // wave-uniform: ... and gave it back, its queue full
        if constexpr (KT > 16 && KT <= 28) {
          // The steady state: a wave whose 4 096 bases (and the k - 1 in front) lie inside the genome and the segment
          // and clear of runs, outside safe mode, with a threshold whose high word decides, walks its
          // 64 k-mers per lane as one software pipeline (the table reads of k-mer n + 1 in flight under the arithmetic
          // of k-mer n) -- windows, hash halves, high-word test, possible candidates to the queue.  A full queue hands
          // the whole load to the general walk.
          constexpr int FS = 58 - 2 * KT;           // where a new byte enters the forward window kept top-aligned for a dword's first k-mer
          constexpr int FSB = FS & ~7, FX = FS & 7;  // ... kept at the byte boundary below it; the rest is part of every cut
          if (crel >= ex_lo && crel + P_CHUNK <= ex_hi && !wave_dirty) {
            // the lane's 64 bases and the 32 in front of them: all inside the buffer (the load lies in the genome, and
            // not at base 0 of the buffer: k - 1 predecessors lie in the genome too), so nothing is asked per lane
            uint4 cv = make_uint4(cw[0], cw[1], cw[2], cw[3]);
            uint2 pv = make_uint2(p2, p3);
            if (!has_runs) {
              const uint8_t* const src = tile + (uint32_t)((crel >> 2) + 16 * (int)lane);
              cv = *reinterpret_cast<const uint4*>(src);
              pv = *reinterpret_cast<const uint2*>(src - 8);
            }
            const uint32_t qn0 = qn;
            // both windows from the 32 bases in front: forward F << FSB (first base on top), reverse complement with the
            // newest base's complement on top -- the complemented stream as it lies
            const uint32_t q2 = pair_rev(pv.x), q3 = pair_rev(pv.y);
            uint32_t FThi = FSB ? __builtin_amdgcn_alignbit(q2, q3, 32 - FSB) : q2;
            uint32_t FTlo = FSB ? (q3 << FSB) : q3;
            uint32_t Rhi = ~pv.y, Rlo = ~pv.x;
            uint32_t w0 = cv.x, w1 = cv.y, w2 = cv.z, w3 = cv.w;
            bool lost = false;  // wave-uniform: the queue could not take a candidate
            // the pipeline's first k-mer has no predecessor to finish: its slot starts as whatever the registers hold
            // (named as values, not written: a zero-fill would be twelve moves per load), and is never finished
            KmerLoads pend;
            undefined_loads(pend);
            auto finish_pending = [&]() __attribute__((always_inline)) { express_handoff(pend, P, Thi1, W.wq, qn, lost); };
#pragma unroll 1
            for (int d = 0; d < 4; d++) {
              const uint32_t PRd = pair_rev(w0), NCd = ~w0;
#pragma unroll
              for (int q = 0; q < 4; q++) {
                // forward: (F << 8 | byte) at the byte boundary FSB; reverse: the complemented byte enters on top
                FThi = __builtin_amdgcn_alignbit(FThi, FTlo, 24);
                FTlo = __builtin_amdgcn_perm(FTlo, PRd, fwd_roll_sel(FSB, q));
                const uint32_t nhi = __builtin_amdgcn_perm(Rhi, NCd, ((uint32_t)q << 24) | 0x00070605u);
                Rlo = __builtin_amdgcn_alignbit(Rhi, Rlo, 8);
                Rhi = nhi;
                const uint64_t FT = ((uint64_t)FThi << 32) | FTlo;
                const uint64_t R = ((uint64_t)Rhi << 32) | Rlo;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                  const uint64_t f = FT << (2 * b + FX);
                  const uint64_t r = R << (6 - 2 * b);
                  const KmerLoads nl = kmer_loads(f < r ? f : r, P);
                  __builtin_amdgcn_sched_barrier(0);
                  if (q > 0 || b > 0 || d > 0) finish_pending();
                  __builtin_amdgcn_sched_barrier(0);
                  pend = nl;
                }
              }
              w0 = w1; w1 = w2; w2 = w3;
            }
            finish_pending();
            if (lost) { qn = qn0; lost_load = true; }  // the candidates this load did queue are found again by the general walk
            else done = true;
          }
        }

        // ---- the general walk: every k, runs, genome and segment edges, safe mode, later passes ----
        if (!done) {  // (safe mode never takes the express walk: every wave meets the barriers of all sixteen steps)
          // Nothing in here is worked out ahead of the branch (an express load would pay for masks it never reads): the
          // lane's position passes through an empty asm that stays where it is written, and the masks, the ownership
          // tests and, in a segment without runs, the loads with their guards all hang on it.
          int lrel = crel + 64 * (int)lane;  // the lane's first owned position
          asm volatile("" : "+v"(lrel));
          if (!has_runs) load_guarded(lrel);
          const bool owned = crel >= V.rel_lo && crel + P_CHUNK <= V.rel_hi;  // wave-uniform: every position of the load is owned
          // validity of the lane's 96 bases: bit i of (M2 : M1 : M0) set = base lrel - 32 + i lies in a run or outside the genome
          uint32_t M[3] = {0u, 0u, 0u};
          const int wstart = lrel - 32;  // tile coordinates
          auto mark = [&](int a, int b) {  // bases [a, b) of the window
            a = a < 0 ? 0 : a;
            b = b > 96 ? 96 : b;
            if (a >= b) return;
#pragma unroll
            for (int w = 0; w < 3; w++) {
              const int la = a - 32 * w < 0 ? 0 : a - 32 * w, lb = b - 32 * w > 32 ? 32 : b - 32 * w;
              if (la < lb) M[w] |= (lb - la == 32) ? ~0u : (((1u << (lb - la)) - 1u) << la);
            }
          };
          if (V.gb > wstart) mark(0, V.gb - wstart);
          if (V.ge < wstart + 96) mark(V.ge - wstart, 96);
          if (wave_dirty) {
            const int64_t wabs = (int64_t)TB + wstart;
            for (uint32_t r = first_run_ending_after(B.runs, rcur, sr.y, wabs); r < sr.y; r++) {  // from the first run that ends behind the window's first base
              const int64_t st = (int64_t)B.runs[2 * (uint64_t)r] - wabs;
              if (st >= 96) break;
              const int64_t en = st + (int64_t)B.runs[2 * (uint64_t)r + 1];
              mark(st < 0 ? 0 : (int)st, en > 96 ? 96 : (int)en);
            }
          }
          const bool clean = !__any((M[0] | M[1] | M[2]) != 0u);  // wave-uniform
          // windows in the general form (cut_kmers' fwd / rc) from the 32 bases in front
          uint64_t fwd = ((uint64_t)pair_rev(p2) << 32) | pair_rev(p3);
          uint64_t rc;
          {
            const uint64_t nc = ~(((uint64_t)p3 << 32) | p2);
            rc = k == 32 ? nc : (nc >> (64 - 2 * k));
          }
          uint32_t g0 = cw[0], g1 = cw[1], g2 = cw[2], g3 = cw[3];
#pragma unroll 1
          for (int d = 0; d < 4; d++) {
            const uint32_t wd = g0;
            g0 = g1; g1 = g2; g2 = g3;
            const uint64_t Wm = d < 2 ? (((uint64_t)M[1] << 32) | M[0]) : (((uint64_t)M[2] << 32) | M[1]);
#pragma unroll
            for (int q = 0; q < 4; q++) {
              const int i0 = 16 * d + 4 * q;           // the step's first position among the lane's 64
              const int rel0 = lrel + i0;              // ... in tile coordinates
              const uint32_t y = (wd >> (8 * q)) & 0xffu;  // four bases, the first lowest
              const uint32_t pack = ((y & 3u) << 6) | ((y & 0xcu) << 2) | ((y >> 2) & 0xcu) | (y >> 6);
              const uint32_t rp = y ^ 0xffu;
              uint64_t canon[4];
              cut_kmers(fwd, rc, pack, rp, P, true, canon);  // ... and rolls the windows on
              const bool allok = owned && clean;  // wave-uniform: every k-mer of every lane is valid and owned
              // a k-mer that ends at position i of the lane's 64 is valid when the k bits up to bit 32 + i of the mask are clear
              bool ok[4];
#pragma unroll
              for (int b = 0; b < 4; b++) {
                const int i = (i0 & 31) + b;  // position inside Wm's upper word
                const uint64_t win = (Wm >> (33 + i - k)) & (k == 32 ? 0xffffffffULL : ((1ULL << k) - 1ULL));
                const int rel = rel0 + b;
                ok[b] = win == 0 && rel >= V.rel_lo && rel < V.rel_hi;
              }
              kmer_step4(W, P, canon, allok, T, lo1, qn, safe_mode, [&](int b) __attribute__((always_inline)) { return ok[b]; });
            }
          }
        }
        qlast = lost_load ? (uint32_t)QCAP : qn - q_in;  // (a drain happens in front of a load only: qn >= q_in)
      }  // loads of the tile
    } while (tile_overflowed(W, T, count_at_tile_start, safe_mode));
    end_tile(W, T, qn, count_at_tile_start, safe_mode);
  }

  if (finish_sketch(W, sg, T, qn, Tstart, pass_no, out, cnt, parts, pcnt)) goto restart;
}

RTC_MINHASH_PICK(pick_kernel, sketch_minhash_packed_kernel)

}  // namespace

extern "C" int rtc_sketch_minhash_packed_dev(rtc_ctx* ctx, const uint8_t* d_packed, uint64_t n_bases, const uint64_t* d_runs,
                                             uint64_t n_runs, const uint64_t* h_off, uint32_t n, int k, uint32_t seed,
                                             const uint32_t* h_sizes, uint32_t size, uint64_t* d_out, uint32_t stride,
                                             uint32_t* d_cnt) {
  if (!ctx || !h_off || (n && (!d_packed || !d_out || !d_cnt)) || (n_runs && !d_runs)) return RTC_ERR_ARG;
  if (k < 1 || k > 32) return rtc_fail(ctx, RTC_ERR_ARG, "k=%d outside 1..32", k);
  if (n == 0) return RTC_OK;
  if (((uintptr_t)d_packed & 15) != 0) return rtc_fail(ctx, RTC_ERR_ARG, "d_packed must be 16-byte aligned");
  if ((n_bases & 63) || n_runs >= (1ull << 32))
    return rtc_fail(ctx, RTC_ERR_ARG, "packed batch: n_bases must be a multiple of 64, fewer than 2^32 runs");
  if (h_off[n] > n_bases) return rtc_fail(ctx, RTC_ERR_ARG, "packed batch: the genomes end at base %llu, the buffer holds %llu", (unsigned long long)h_off[n], (unsigned long long)n_bases);

  RTC_TRY(rtc_sticky_error(ctx));
  RTC_TRY(rtc_check_runs_async(ctx, d_runs, n_runs, n_bases));  // asynchronous: a violation surfaces at the next packed call or rtc_ctx_sync
  PackedIn B{d_packed, n_bases, d_runs};
  uint2* d_seg_runs = nullptr;
  auto prepare = [&](const MinhashPlanInfo& pi) -> int {
    RTC_HIP(ctx, hipFuncSetAttribute((const void*)pick_kernel(k, seed, false, pi.packed_tables), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pi.lds));
    RTC_HIP(ctx, hipFuncSetAttribute((const void*)pick_kernel(k, seed, true, pi.packed_tables), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pi.lds));
    void* ws = nullptr;
    RTC_TRY(rtc_ws(ctx, 3, pi.nsegs * sizeof(uint2) + 64, &ws));
    d_seg_runs = (uint2*)ws;
    if (ctx->opt.verbose && !ctx->quiet) fprintf(stderr, "[minhash] sketching over packed bases, k=%d, %zu segments, %llu runs\n", k, pi.nsegs, (unsigned long long)n_runs);
    hipLaunchKernelGGL(seg_runs_kernel<Segment>, dim3((uint32_t)((pi.nsegs + 255) / 256)), dim3(256), 0, ctx->stream, pi.d_segs, (uint32_t)pi.nsegs,
                       d_runs, (uint32_t)n_runs, k, d_seg_runs);
    RTC_CHECK_LAUNCH(ctx);
    return RTC_OK;
  };
  auto launch = [&](const MinhashLaunch& L) -> int {
    hipLaunchKernelGGL(pick_kernel(k, seed, L.runtime_k, L.packed_tables), dim3(L.nseg), dim3(WG), L.lds, ctx->stream, B, L.d_segs,
                       (const uint2*)(d_seg_runs + L.seg_index), k, seed, L.cap, d_out, d_cnt, L.pass, L.d_parts, L.d_pcnt, L.d_redo);
    RTC_CHECK_LAUNCH(ctx);
    return RTC_OK;
  };
  return minhash_run(ctx, h_off, n, k, h_sizes, size, d_out, stride, d_cnt, P_PLAN_BASES, (size_t)MIN_ROOM, prepare, launch);
}

namespace { __global__ void touch_unit_kernel() {} }
int rtc_touch_sketch_minhash_packed(rtc_ctx* ctx) {
  hipLaunchKernelGGL(touch_unit_kernel, dim3(1), dim3(64), 0, ctx->stream);
  RTC_CHECK_LAUNCH(ctx);
  return RTC_OK;
}
