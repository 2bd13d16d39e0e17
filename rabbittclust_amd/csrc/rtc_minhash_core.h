// rtc_minhash_core.h -- what the two MinHash sketch translation units share (rtc_sketch_minhash.hip: ASCII input,
// rtc_sketch_minhash_packed.hip: the 2-bit staging format): the MurmurHash3 evaluation from LDS product tables, the
// in-LDS bottom-s merge, the candidate path of the sketch kernels (workgroup state, pass gate, queue, express hand-off,
// window cut, the four-k-mer step, tile and kernel end), the partial-sketch merge kernel, kernel selection and the
// host-side segment plan.  A unit adds what its input format needs: loads, decode, the express loop, validity.  Everything lives in an anonymous namespace: each unit compiles its own copy of this one text.
#pragma once
#include <algorithm>

#include "rtc_internal.h"

namespace {

constexpr int WG = 512;                               // lanes per workgroup (8 waves)
constexpr int NWAVE = WG / 64;
// 19 dwords = 76 owned positions per lane and tile: lane runs 76 B apart keep the set of live 128-B
// lines (one or two lanes per line, ~1500 lanes per CU) inside the 4 MiB L2 of an XCD.  31 dwords is
// 1 % faster but re-reads 56 % of the input from the fabric (measured: TCC_EA0_RDREQ_128B, 19 dwords: 11 %).
constexpr int RUN_DW = 19;                            // dwords of owned bases per lane per tile
constexpr int OWN = RUN_DW * 4;                       // k-mer end positions a lane owns per tile
// warm-up dwords in front of a lane's owned run (they only roll the windows): k-1 bases rounded up so
// that warm-up + run are whole 16-byte loads -- 5 (20 bases, six loads per tile) for the compile-time
// k <= 21, 9 (36 bases >= 31, seven loads) otherwise
__host__ __device__ constexpr int warm_dw(int kt) { return (kt > 0 && kt <= 21) ? 5 : 9; }
static_assert((RUN_DW + warm_dw(21)) % 4 == 0 && (RUN_DW + warm_dw(0)) % 4 == 0, "a lane's window must be whole 16-byte loads");
constexpr int TILE_BASES = WG * RUN_DW * 4;           // bases per tile
// Safe mode appends ONE k-mer per lane between two looks at the candidate count (four until round 5): the room the buffer
// has to guarantee is a quarter, and a third workgroup per CU fits up to s = 3 190 at k = 21 (3 574 with the packed tables;
// 3 318 until the k2-type word's second-half table grew to 8-byte entries) instead of 1 782 (2 038) -- clust-greedy's
// containment sketches of 2 - 3.5 Mbp genomes, and BASELINE config 4's sketches
// no longer need the packed layout (its stride-16 reads cost bank conflicts): 115.6 -> 112.5 ms there, 85.8 -> 81.0 ms at s = 3000.
constexpr int STEP_APPENDS = WG;                      // worst-case appends between two looks at the count in safe mode
constexpr int MIN_ROOM = STEP_APPENDS;                // candidate room the buffer always offers
constexpr uint64_t SENT = ~0ULL;
// per-wave queue of possible candidates (unfinished hash halves) in LDS: see the steady state of the kernel
constexpr int QCAP = 32;                              // entries per wave
constexpr int QDRAIN = 16;                            // drained at a tile end once this many wait
constexpr size_t QUEUE_BYTES = (size_t)NWAVE * QCAP * 16;
// hash tables in LDS (see kmer_hash_parts): per 8 bases of k one 256-entry table of 16-byte entries
// (first four bases of the word) and, where the word has more than four bases, one for its second four: 4-byte
// entries lo(b * c) for the k1-type words (even w), 8-byte entries {lo(b * c), lo(b * c) * hi(2 c1)} for the k2-type
// ones (odd w) -- the second dword is the part of word_k2's cross product that is linear in the table index
constexpr size_t LUT_LO_BYTES = 256 * 16, LUT_HI_BYTES = 256 * 4;
// second-half tables of the plain layout: offset of word w's behind the 16-byte tables (one unit per k1-type word
// in front of it, two per k2-type one), and the bytes of the first `his` of them
// (xt, "cross term tabulated": the compile-time-k kernels.  The runtime-k kernels keep 4-byte entries for every word and
// multiply -- their general walk holds four k-mers' table words at once and spilt the extra dword inside its loop: k = 15
// from packed bases 148.7 against 145.5 ms.  The host plans every launch with the larger tables.)
__host__ __device__ constexpr size_t lut_hi_off(int w, bool xt = true) { return (size_t)(w + (xt ? w / 2 : 0)) * LUT_HI_BYTES; }
__host__ __device__ constexpr size_t lut_hi_bytes(int his, bool xt = true) { return lut_hi_off(his, xt); }
// A last word of at most five bases has a table of its own instead: 4^bases entries of 8 bytes holding the
// finished contribution (at most 8 KiB), one ds_read_b64 and two VALU instructions for the word.
__host__ __device__ constexpr int lut_words(int k) { return (k + 7) / 8; }
__host__ __device__ constexpr int lut_last_nb(int k) { return k - 8 * (lut_words(k) - 1); }   // bases of the last word, 1..8
__host__ __device__ constexpr bool lut_direct(int k) { return lut_last_nb(k) <= 5; }
__host__ __device__ constexpr int lut_los(int k) { return lut_words(k) - (lut_direct(k) ? 1 : 0); }  // words with the table pair
__host__ __device__ constexpr int lut_his(int k) { return lut_direct(k) ? lut_los(k) : (k + 3) / 8; }  // word w has a second half iff k > 8w + 4
// Packed layout (pk): lo(b * c) of the second-half tables sits in the spare fourth dword of the 16-byte entries instead
// (there is no fifth for a k2-type word's cross term: that layout keeps the four-instruction word_k2) -- 1 KiB less LDS
// per k1-type word and 2 per k2-type one, stride-16 reads (more bank conflicts: the headline shape loses 1.9 %,
// k = 23 6.5 %).  The launch picks it only where it buys a workgroup per CU (k = 21: 3190 < s <= 3574).
__host__ __device__ constexpr size_t lut_direct_bytes(int k) { return lut_direct(k) ? ((size_t)8 << (2 * lut_last_nb(k))) : 0; }
__host__ __device__ constexpr size_t lut_bytes(int k, bool pk) {
  return (size_t)lut_los(k) * LUT_LO_BYTES + (pk ? 0 : lut_hi_bytes(lut_his(k))) + lut_direct_bytes(k);
}

struct Segment {
  uint64_t g_begin, g_end;  // genome byte range in d_seq
  uint64_t s_begin, s_end;  // k-mer END positions owned by this segment (absolute)
  uint64_t out_off;         // element offset into out buffer
  uint64_t lo_off;          // pass > 0: offset (final buffer) of the largest hash kept by earlier passes
  uint32_t cnt_slot;        // index into cnt buffer
  uint32_t sketch_size;     // hashes to select in this pass
  uint32_t final_slot;      // genome index in the final count buffer
  uint32_t expect;          // pass > 0: run only if the genome already holds exactly this many hashes
  uint32_t partial;         // 1: one of several segments of a genome, writes a partial sketch for the merge kernel
  uint32_t pad;
  uint64_t t0;              // starting threshold (SENT: none), see the kernel
};

struct Ctrl {
  uint64_t T;
  uint64_t T0;       // the threshold while fewer than s hashes are held (SENT, or the segment's starting threshold)
  uint32_t sorted;   // buf[0..sorted) is ascending and distinct (what the last merge left); appends follow it
  uint32_t pad0;
  uint32_t count;
  uint32_t overflow;
  uint32_t saw_max;
  uint32_t scan_base;
  uint32_t wave_tot[NWAVE];
};

// Every LDS object is reached through address_space(3) pointers: the accesses are ds_* instructions
// by construction (not flat ones whose selection depends on what the optimiser can prove).
#define RTC_LDS __attribute__((address_space(3)))
typedef RTC_LDS uint64_t* lds_u64_ptr;
typedef RTC_LDS Ctrl* lds_ctrl_ptr;
typedef RTC_LDS unsigned char* lds_byte_ptr;
struct MergeResult { uint32_t count; uint64_t T; };
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // plain vector (HIP's uint4 is a class, unusable through LDS pointers)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ---- MurmurHash3_x64_128 (first output word) of the canonical k-mer's ASCII bytes ----------------
// MurmurHash3 turns every 64-bit input word w into  rotl(w * c, r) * c'  (c, r, c' = c1, 31, c2 for the
// k1 words, c2, 33, c1 for the k2 words) before mixing it into the state.  With w = a | b << 32
// (a = bytes 0-3, b = bytes 4-7 of the word) multiplication mod 2^64 gives
//     S = w * c :   S.lo = lo(a * c),   S.hi = hi(a * c) + lo(b * c)   (one 32-bit add, no other carry)
// and the rotation by 31 / 33 moves the two halves of S to DISJOINT bit ranges, so
//     rotl(S, r) * c' = X(S.lo) * c' + Y(S.hi) * c'
// where the first term depends on the word's first four bases only: it comes out of an LDS table
// together with hi(a * c) (16-byte entries, one ds_read_b128), lo(b * c) out of a second table
// (4-byte entries), and the second term is a 32 x 64-bit product:
//     r = 31:  Y = S.hi >> 1 | (S.hi & 1) << 63   ->  (S.hi >> 1) * c' + (S.hi << 31) in the top word
//     r = 33:  Y = S.hi << 1 (33 bits)            ->  (S.hi * c') << 1
// i.e. 6 / 5 VALU instructions per word instead of 7 (add, two-instruction rotate, 64 x 64 multiply),
// and no 2-bit -> ASCII expansion at all.  The tables are built once per workgroup for the runtime k.
__device__ __forceinline__ uint64_t fmix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

// fmix64 without its last multiply and xorshift.  With f = x * FMIX_C2 for the two halves the hash is
// (f1 ^ f1 >> 33) + (f2 ^ f2 >> 33); the last xorshift changes the low words only, so the high words of f1 and
// f2 decide almost every threshold test -- and their SUM is all the test needs, which is the high word of ONE
// product, (a + b) * C, up to a carry: hash_test_word.  The full halves are formed on demand, for the few k-mers
// that pass (mm_finish).
constexpr uint64_t FMIX_C2 = 0xc4ceb9fe1a85ec53ULL;
__device__ __forceinline__ uint64_t fmix64_open(uint64_t x) {
  x ^= x >> 33;
  // cross terms as v_mul_lo + a 32-bit mad (v_mad_u64_u32, low word) and one two-input add: the plain
  // 64-bit product compiles to two v_mul_lo and a v_add3, 1.2 issue cycles more (same-run 82.2 -> 81.5 ms)
  constexpr uint32_t cl = 0xed558ccdu, ch = 0xff51afd7u;
  const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32);
  const uint64_t D = (uint64_t)xl * cl;
  uint32_t e = xl * ch + xh * cl;
  asm("" : "+v"(e));
  x = __builtin_bit_cast(uint64_t, make_uint2((uint32_t)D, (uint32_t)(D >> 32) + e));
  x ^= x >> 33;
  return x;
}
struct HashParts { uint64_t f1, f2; };  // the two halves before their last multiply
__device__ __forceinline__ uint64_t mm_finish(const HashParts& p) {
  const uint64_t f1 = p.f1 * FMIX_C2, f2 = p.f2 * FMIX_C2;
  return (f1 ^ (f1 >> 33)) + (f2 ^ (f2 >> 33));
}
// The test word.  (f1 + f2) mod 2^64 = (a + b) * C for the halves a, b before their last multiply, and its high
// word is hi(f1) + hi(f2) + c1 (c1: the carry of the two low words), while hi(hash) = hi(f1) + hi(f2) + c2 (c2: the
// carry of the low words AFTER their xorshift).  So w = hi((a + b) * C) + 1 lies in {hi(hash), hi(hash) + 1,
// hi(hash) + 2} (mod 2^32): a hash below T has w <= hi(T) + 2, also when hi(f1) + hi(f2) wraps (w = 0 or 1 then).
// One 64-bit add and the high word of ONE 64 x 64 product (mulhi + two cross products + add3) instead of two.
constexpr uint32_t TEST_SLACK = 2;  // callers compare with hi(T) + TEST_SLACK and need hi(T) + TEST_SLACK < 2^32
__device__ __forceinline__ uint32_t hash_test_word(const HashParts& p) {
  const uint64_t S = p.f1 + p.f2;
  const uint32_t slo = (uint32_t)S, shi = (uint32_t)(S >> 32);
  const uint32_t cl = (uint32_t)FMIX_C2, ch = (uint32_t)(FMIX_C2 >> 32);
  // as a chain of two 32-bit multiply-adds (v_mad_u64_u32, low word) on top of the v_mul_hi: one three-input add fewer
  uint32_t m = __umulhi(slo, cl);
  asm("" : "+v"(m));
  uint32_t r = slo * ch + m;
  asm("" : "+v"(r));
  uint32_t r2 = shi * cl + r;
  asm("" : "+v"(r2));
  return r2 + 1u;
}

constexpr uint64_t MM_C1 = 0x87c37b91114253d5ULL, MM_C2 = 0x4cf5ad432745937fULL;
constexpr uint32_t K2_CROSS = (uint32_t)((MM_C1 << 1) >> 32);  // hi(2 c1): the cross-product constant of a k2-type word (word_k2)
constexpr uint32_t MASH_SEED = 42;  // the seed of every reference call site (Sketch::MinHash)

__device__ __forceinline__ uint32_t codes_to_ascii(uint32_t e) {
  // e holds 4 base codes, first base in bits 7..6; returns the 4 ASCII bytes, first base lowest
  const uint32_t t = ((e >> 6) & 3u) | (((e >> 4) & 3u) << 8) | (((e >> 2) & 3u) << 16) | ((e & 3u) << 24);
  return __builtin_amdgcn_perm(0u, 0x54474341u, t);
}

struct KParams {
  int k;
  uint32_t seed;
  uint32_t use64;
  int lshift;          // 64 - 2k
  int rc_shift;        // 2k - 2
  uint64_t kmask;      // low 2k bits
  bool packed;         // table layout, see lut_bytes
  bool cross_tab;      // plain layout only: the k2-type words' cross term comes out of the tables (word_k2, lut_hi_off)
};

__device__ __forceinline__ KParams make_kparams(int k, uint32_t seed, bool packed, bool cross_tab) {
  KParams P;
  P.k = k; P.seed = seed; P.use64 = k > 16 ? 1u : 0u; P.packed = packed; P.cross_tab = cross_tab && !packed;
  P.lshift = 64 - 2 * k; P.rc_shift = 2 * k - 2;
  P.kmask = k == 32 ? ~0ULL : ((1ULL << (2 * k)) - 1);
  return P;
}

// Called by all WG threads; the first 256 fill one column each.  Layout: lut_los(k) tables of
// {u64 P, u32 AH, pad} at w * LUT_LO_BYTES, then lut_his(k) tables of u32 BL (even w) or {u32 BL, u32 BLc} (odd w), then the last word's own table
// (lut_direct(k)): entry i = rotl(w * c, r) * c' of the word whose bases are the 2-bit codes of i.
__device__ __forceinline__ void build_kmer_lut(lds_byte_ptr lut, int k, bool pk, bool xt) {
  const uint32_t e = threadIdx.x;
  if (e >= 256) return;
  const uint32_t a4 = codes_to_ascii(e);
  const uint32_t hi_base = (uint32_t)(lut_los(k) * LUT_LO_BYTES);
  if (lut_direct(k)) {
    const int wl = lut_words(k) - 1, nb = lut_last_nb(k);
    typedef RTC_LDS uint64_t* lds_u64w_ptr;
    const lds_u64w_ptr dt = (lds_u64w_ptr)(lut + hi_base + (pk ? 0 : lut_hi_bytes(lut_his(k), xt)));
    for (uint32_t i = e; i < (1u << (2 * nb)); i += 256) {
      const uint32_t e4 = nb >= 4 ? ((i >> (2 * nb - 8)) & 0xffu) : ((i << (8 - 2 * nb)) & 0xffu);   // first four bases, first on top
      const uint32_t am = nb >= 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u);
      uint64_t wd = (uint64_t)(codes_to_ascii(e4) & am);
      if (nb == 5) wd |= (uint64_t)(codes_to_ascii((i & 3u) << 6) & 0xffu) << 32;
      uint64_t S, K;
      if (wl & 1) { S = wd * MM_C2; K = ((S << 33) | (S >> 31)) * MM_C1; }
      else { S = wd * MM_C1; K = ((S << 31) | (S >> 33)) * MM_C2; }
      dt[i] = K;
    }
  }
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const int nb = k - 8 * w;  // bytes of this word
    if (nb <= 0 || w >= lut_los(k)) break;
    const uint64_t c = (w & 1) ? MM_C2 : MM_C1;
    const uint32_t am = nb >= 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u);
    const uint64_t A = (uint64_t)(a4 & am) * c;
    const uint32_t AL = (uint32_t)A, AH = (uint32_t)(A >> 32);
    uint64_t P;
    if (w & 1) P = (((uint64_t)(uint32_t)(AL << 1) << 32) | (uint64_t)(AL >> 31)) * MM_C1;   // rotl33 part of S.lo, times c1
    else P = (((uint64_t)(AL >> 1) << 32) | ((uint64_t)(AL & 1u) << 31)) * MM_C2;           // rotl31 part of S.lo, times c2
    typedef RTC_LDS u32x4* lds_u4_ptr;
    const uint32_t bm = nb >= 8 ? 0xffffffffu : (nb > 4 ? ((1u << (8 * (nb - 4))) - 1u) : 0u);
    const uint32_t BL = (a4 & bm) * (uint32_t)c;  // lo(b * c) of the word whose SECOND four bases are e's codes
    // Plain layout, k2-type word: word_k2's cross product (AH + BL) * hi(2 c1) is linear in its two table indices
    // mod 2^32 -- the AH term rides in P.hi (the v_mad_u64_u32's addend carries it), the BL term (of the same masked
    // BL) beside BL.  The packed layout has no dword for the latter: its P.hi stays plain and its word_k2 multiplies.
    const bool fold = (w & 1) && !pk && xt;
    const uint32_t Phi = (uint32_t)(P >> 32) + (fold ? AH * K2_CROSS : 0u);
    const u32x4 ent = {(uint32_t)P, Phi, AH, pk ? BL : 0u};
    *(lds_u4_ptr)(lut + (size_t)w * LUT_LO_BYTES + (size_t)e * 16) = ent;
    if (nb > 4 && !pk) {
      if (fold) {
        typedef RTC_LDS u32x2* lds_u2_ptr;
        const u32x2 ent2 = {BL, BL * K2_CROSS};
        *(lds_u2_ptr)(lut + hi_base + lut_hi_off(w, xt) + (size_t)e * 8) = ent2;
      } else {
        typedef RTC_LDS uint32_t* lds_u32_ptr;
        *(lds_u32_ptr)(lut + hi_base + lut_hi_off(w, xt) + (size_t)e * 4) = BL;
      }
    }
  }
}

// 64-bit rotate as two v_alignbit_b32 (the generic shift/or form costs three to four instructions)
template <int R>
__device__ __forceinline__ uint64_t rotl64c(uint64_t x) {
  static_assert(R > 0 && R < 64 && R != 32, "rotation amount");
  const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
  uint32_t nh, nl;
  if (R < 32) {
    nh = __builtin_amdgcn_alignbit(hi, lo, 32 - R);
    nl = __builtin_amdgcn_alignbit(lo, hi, 32 - R);
  } else {
    nh = __builtin_amdgcn_alignbit(lo, hi, 64 - R);
    nl = __builtin_amdgcn_alignbit(hi, lo, 64 - R);
  }
  // assembled as a register pair and made opaque: otherwise the two halves are re-associated into
  // the 64-bit additions that follow ((lo, 0) + x + (0, hi): one more add and a move)
  uint64_t r = __builtin_bit_cast(uint64_t, make_uint2(nl, nh));
  asm("" : "+v"(r));
  return r;
}

// x*5 as one v_lshl_add_u64 ((x << 2) + x); the compiler's choice is two v_mad_u64_u32 plus moves
__device__ __forceinline__ uint64_t times5(uint64_t x) {
  uint64_t r;
  asm("v_lshl_add_u64 %0, %1, 2, %1" : "=v"(r) : "v"(x));
  return r;
}

// byte B of w, shifted left by log2 of a table's entry size (the byte offset of a table entry), as one SDWA shift.  The
// three shift amounts a k-mer's offsets need (16-, 4- and 8-byte entries) are the bytes of ONE register, picked by the
// shift operand's own byte select: a register per amount was two for every kernel and would be three with the 8-byte
// second-half tables, and these kernels sit at their 80-VGPR bound.
constexpr uint32_t ENTRY_SHIFTS = 0x00030204u;
enum EntryShift { SH16 = 0, SH4 = 1, SH8 = 2 };  // byte of ENTRY_SHIFTS
template <int B, int S>
__device__ __forceinline__ uint32_t byte_x8(uint32_t w, uint32_t shifts) {
  uint32_t r;
#define RTC_SDWA_SHIFT(SS, BB) \
  if (S == SS && B == BB) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_" #SS " src1_sel:BYTE_" #BB : "=v"(r) : "v"(shifts), "v"(w))
  RTC_SDWA_SHIFT(0, 0); RTC_SDWA_SHIFT(0, 1); RTC_SDWA_SHIFT(0, 2); RTC_SDWA_SHIFT(0, 3);
  RTC_SDWA_SHIFT(1, 0); RTC_SDWA_SHIFT(1, 1); RTC_SDWA_SHIFT(1, 2); RTC_SDWA_SHIFT(1, 3);
  RTC_SDWA_SHIFT(2, 0); RTC_SDWA_SHIFT(2, 1); RTC_SDWA_SHIFT(2, 2); RTC_SDWA_SHIFT(2, 3);
#undef RTC_SDWA_SHIFT
  return r;
}

// rotl(S, 31) * c2 for a k1 word: e = {P.lo, P.hi, AH, -}, BL = lo(b * c1)
__device__ __forceinline__ uint64_t word_k1(const u32x4 e, uint32_t BL) {
  const uint32_t SH = e.z + BL, v = SH >> 1;
  const uint64_t R = (uint64_t)v * (uint32_t)MM_C2 + __builtin_bit_cast(uint64_t, make_uint2(e.x, e.y));  // v_mad_u64_u32
  // the high word takes v * hi(c2) + (SH & 1) << 31: t = hi(R) + (SH << 31) as one v_lshl_add_u32 (a fresh register, so it can be the
  // low half of an addend pair) and v * hi(c2) + t as a 32-bit mad (v_mad_u64_u32, low word)
  uint32_t t = (SH << 31) + (uint32_t)(R >> 32);
  asm("" : "+v"(t));
  const uint32_t hi = v * (uint32_t)(MM_C2 >> 32) + t;
  return __builtin_bit_cast(uint64_t, make_uint2((uint32_t)R, hi));
}
// rotl(S, 33) * c1 for a k2 word: (S.hi * c1) << 1 + P = S.hi * (2 c1 mod 2^64) + P, the table value as the
// addend of the v_mad_u64_u32; the constant's high word is one cross product, S.hi * hi(2 c1) into the top word.
// Only its low 32 bits count, and mod 2^32 it is linear in S.hi = AH + BL: AH * hi(2 c1) + BL * hi(2 c1), one table
// index each.  The plain layout's tables hold both terms (build_kmer_lut: the first inside P.hi, the second as
// bl.y beside BL), so the word is add, mad, add.  S.hi is still summed and still feeds the 64 x 32 product: no carry
// to mend.  mul: the tables hold neither term, bl.y is not read, the sum is multiplied -- the packed layout, which has
// no dword for the second term, and the runtime-k kernels (KParams::cross_tab, lut_hi_off).
__device__ __forceinline__ uint64_t word_k2(const u32x4 e, const u32x2 bl, bool mul) {
  constexpr uint64_t C1X2 = MM_C1 << 1;
  const uint32_t SH = e.z + bl.x;
  const uint64_t R = (uint64_t)SH * (uint32_t)C1X2 + __builtin_bit_cast(uint64_t, make_uint2(e.x, e.y));  // v_mad_u64_u32
  uint32_t cross;
  if (mul) {
    cross = SH * K2_CROSS;
    asm("" : "+v"(cross));  // keep it a v_mul_lo_u32 + v_add_u32: fused into a second v_mad_u64_u32 it costs two extra moves
  } else {
    cross = bl.y;
    asm("" : "+v"(cross));  // keep it a v_add_u32 behind the mad: folded into the addend's high word it costs an add in front and moves
  }
  return __builtin_bit_cast(uint64_t, make_uint2((uint32_t)R, (uint32_t)(R >> 32) + cross));
}

// The table words of one k-mer: what its LDS reads return (fields a k does not use are never read or touched).
// Two phases so that a caller can have the reads of one k-mer in flight under the arithmetic of another:
// kmer_loads issues them (offsets + ds_read), kmer_hash_finish consumes them.
struct KmerLoads {
  u32x4 e[4];       // 16-byte entries {P.lo, P.hi, AH, (BL)} of the words with a table pair
  u32x2 bl[4];      // x: lo(b * c) of their second halves; y: the k2-type words' cross term (plain layout: the two dwords of one ds_read_b64)
  uint64_t dt;      // the last word's own table entry (lut_direct)
};
// x: canonical k-mer, 2 bits per base, first base in the top bits (canon << (64 - 2k))
__device__ __forceinline__ KmerLoads kmer_loads(uint64_t x, const KParams& P) {
  const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
  const int k = P.k;
  // the tables start at LDS address 0 (checked at kernel entry), so an LDS address is a table offset:
  // entry offset = code byte << 4 (16-byte entries), << 3 (8-byte entries) or << 2 (4-byte entries), one SDWA shift each;
  // the table bases fold into the ds_read immediates
  typedef const RTC_LDS u32x4* lds_u4_cptr;
  typedef const RTC_LDS uint32_t* lds_u32_cptr;
  typedef const RTC_LDS u32x2* lds_u2_cptr;
  const bool pk = P.packed, xt = P.cross_tab;
  const uint32_t sh = pk ? 4u : ENTRY_SHIFTS;  // (a VGPR either way: SDWA takes no constants.  The packed layout has 16-byte entries only and picks byte 0: the parent's `four`)
  const uint32_t hi_base = (uint32_t)(lut_los(k) * LUT_LO_BYTES);
  const uint32_t dt_base = hi_base + (pk ? 0u : (uint32_t)lut_hi_bytes(lut_his(k), xt));
  // the last word's own table: its 2nb bits sit at the top of the word's 16-bit slot (whatever lies below them is
  // not part of the k-mer and is cut off), entry offset = field << 3
  typedef const RTC_LDS uint64_t* lds_u64_cptr;
  const int dnb = lut_last_nb(k);
#define RTC_DT(H, odd) (*(lds_u64_cptr)(uintptr_t)(dt_base + ((odd) ? (__builtin_amdgcn_ubfe((H), 16 - 2 * dnb, 2 * dnb) << 3) \
                                                                     : (((H) >> (32 - 2 * dnb)) << 3))))
#define RTC_LO(w, off) (*(lds_u4_cptr)(uintptr_t)((off) + (uint32_t)((w) * LUT_LO_BYTES)))
#define RTC_HI(w, off) (*(lds_u32_cptr)(uintptr_t)((off) + (pk ? (uint32_t)((w) * LUT_LO_BYTES) + 12u : hi_base + (uint32_t)lut_hi_off(w, xt))))
  // a k2-type word's second half: {BL, BLc} as one 8-byte read (plain layout), BL alone out of the 16-byte entry (packed)
#define RTC_HI2(w, off) (!xt ? u32x2{RTC_HI(w, off), 0u} : *(lds_u2_cptr)(uintptr_t)((off) + hi_base + (uint32_t)lut_hi_off(w, true)))
  // a second half's offset: its own entry size in the plain layout, the 16-byte entry's in the packed one
#define RTC_OFF16(B, H) byte_x8<B, SH16>((H), sh)
#define RTC_OFF(B, H, S) (pk ? RTC_OFF16(B, H) : byte_x8<B, S>((H), sh))
#define RTC_OFF8X(B, H) (xt ? RTC_OFF(B, H, SH8) : RTC_OFF(B, H, SH4))  // a k2-type word's second half
  KmerLoads L = {};
  const int dw = lut_direct(k) ? lut_words(k) - 1 : -1;  // the word that has a table of its own
  if (dw == 0) L.dt = RTC_DT(hi, false);
  else { L.e[0] = RTC_LO(0, RTC_OFF16(3, hi)); if (k > 4) L.bl[0].x = RTC_HI(0, RTC_OFF(2, hi, SH4)); }
  if (dw == 1) L.dt = RTC_DT(hi, true);
  else if (k > 8) { L.e[1] = RTC_LO(1, RTC_OFF16(1, hi)); if (k > 12) L.bl[1] = RTC_HI2(1, RTC_OFF8X(0, hi)); }
  if (dw == 2) L.dt = RTC_DT(lo, false);
  else if (k > 16) { L.e[2] = RTC_LO(2, RTC_OFF16(3, lo)); if (k > 20) L.bl[2].x = RTC_HI(2, RTC_OFF(2, lo, SH4)); }
  if (dw == 3) L.dt = RTC_DT(lo, true);
  else if (k > 24) { L.e[3] = RTC_LO(3, RTC_OFF16(1, lo)); if (k > 28) L.bl[3] = RTC_HI2(3, RTC_OFF8X(0, lo)); }
#undef RTC_OFF8X
#undef RTC_OFF
#undef RTC_OFF16
#undef RTC_LO
#undef RTC_HI2
#undef RTC_HI
#undef RTC_DT
  return L;
}
__device__ __forceinline__ HashParts kmer_hash_finish(const KmerLoads& L, const KParams& P) {
  const int k = P.k;
  uint64_t K0 = 0, K1 = 0, K2 = 0, K3 = 0;  // the words' contributions, already rotl(w * c, r) * c'
  const int dw = lut_direct(k) ? lut_words(k) - 1 : -1;
  // The unused fourth dword of a 16-byte entry counts as live until here (an empty asm, no instruction): otherwise the
  // register allocator hands that register to the next read's address while the ds_read_b128 is still in flight and
  // has to wait for it (s_waitcnt lgkmcnt(0) between two reads of one k-mer -- the round trip this split exists to hide).
  if (!P.packed) {
    if (dw != 0) asm volatile("" :: "v"(L.e[0].w));
    if (dw != 1 && k > 8) asm volatile("" :: "v"(L.e[1].w));
    if (dw != 2 && k > 16) asm volatile("" :: "v"(L.e[2].w));
    if (dw != 3 && k > 24) asm volatile("" :: "v"(L.e[3].w));
  }
  if (dw == 0) K0 = L.dt;
  else K0 = word_k1(L.e[0], k > 4 ? L.bl[0].x : 0u);
  if (dw == 1) K1 = L.dt;
  else if (k > 8) K1 = word_k2(L.e[1], k > 12 ? L.bl[1] : u32x2{0u, 0u}, !P.cross_tab);
  if (dw == 2) K2 = L.dt;
  else if (k > 16) K2 = word_k1(L.e[2], k > 20 ? L.bl[2].x : 0u);
  if (dw == 3) K3 = L.dt;
  else if (k > 24) K3 = word_k2(L.e[3], k > 28 ? L.bl[3] : u32x2{0u, 0u}, !P.cross_tab);
  uint64_t h1 = P.seed, h2 = P.seed;
  uint64_t t0 = K0, t1 = K1;  // tail contributions
  if (k >= 16) {
    // first block with h1 == h2 == seed folded in: 5*(rotl27(seed ^ k1) + seed) + c = 5*rotl27(..) + (5*seed + c)
    h1 = rotl64c<27>(h1 ^ K0);
    h1 = times5(h1) + (5ULL * P.seed + 0x52dce729ULL);
    h2 = rotl64c<31>(h2 ^ K1) + h1;
    h2 = times5(h2) + 0x38495ab5ULL;
    t0 = K2; t1 = K3;
    if (k == 32) {
      h1 ^= K2; h1 = rotl64c<27>(h1); h1 += h2; h1 = times5(h1) + 0x52dce729;
      h2 ^= K3; h2 = rotl64c<31>(h2); h2 += h1; h2 = times5(h2) + 0x38495ab5;
      t0 = 0; t1 = 0;
    }
  }
  const int tail = k & 15;
  if (tail > 8) { h2 ^= t1; }
  if (tail > 0) {
    // h1 ^= k1; h1 ^= len: the low word as one three-input xor (v_bitop3_b32)
    const uint32_t lo = __builtin_amdgcn_bitop3_b32((uint32_t)h1, (uint32_t)t0, (uint32_t)k, 0x96);
    const uint32_t hi = (uint32_t)(h1 >> 32) ^ (uint32_t)(t0 >> 32);
    h1 = __builtin_bit_cast(uint64_t, make_uint2(lo, hi));
  } else {
    h1 ^= (uint64_t)k;
  }
  h2 ^= (uint64_t)k;
  h1 += h2; h2 += h1;
  return HashParts{fmix64_open(h1), fmix64_open(h2)};
}
__device__ __forceinline__ HashParts kmer_hash_parts(uint64_t x, const KParams& P) {
  return kmer_hash_finish(kmer_loads(x, P), P);
}
__device__ __forceinline__ uint64_t kmer_hash(uint64_t x, const KParams& P) {
  const uint64_t h = mm_finish(kmer_hash_parts(x, P));
  return P.use64 ? h : (h & 0xffffffffULL);
}

// ---- block-wide merge: sort buf[0..n), drop duplicates, keep the `s` smallest -----------------
// Normalised bitonic network (every compare-exchange ascending, first step of each merge mirrored)
// over the next power of two >= n; positions >= n stand for +infinity, which an ascending exchange
// never moves, so those exchanges are simply skipped and n may be any number.
__device__ void bitonic_sort_lds(lds_u64_ptr buf, int n) {
  const int t = threadIdx.x;
  int n2 = 2;
  while (n2 < n) n2 <<= 1;
  for (int k = 2; k <= n2; k <<= 1) {
    const int hk = k >> 1;
    for (int i = t; i < (n2 >> 1); i += WG) {
      const int off = i & (hk - 1);
      const int a = ((i - off) << 1) | off;       // block base (i / hk) * k, plus off
      const int b = (a - off) + (k - 1 - off);    // mirrored partner within the block
      if (b < n) {
        const uint64_t va = buf[a], vb = buf[b];
        if (va > vb) { buf[a] = vb; buf[b] = va; }
      }
    }
    __syncthreads();
    for (int j = k >> 2; j > 0; j >>= 1) {
      for (int i = t; i < (n2 >> 1); i += WG) {
        const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const int b = a | j;
        if (b < n) {
          const uint64_t va = buf[a], vb = buf[b];
          if (va > vb) { buf[a] = vb; buf[b] = va; }
        }
      }
      __syncthreads();
    }
  }
}

// On entry: buf[0..ctrl->count) holds candidates (unsorted, duplicates allowed), all threads
// arrive.  On exit: buf[0..count) ascending distinct, count <= s, ctrl->T updated.
// first index in the ascending run a[0..n) whose value is >= v (STRICT = false) or > v (STRICT = true)
template <bool STRICT>
__device__ __forceinline__ uint32_t lds_bound(lds_u64_ptr a, uint32_t n, uint64_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint64_t x = a[mid];
    if (STRICT ? (x <= v) : (x < v)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __noinline__ MergeResult merge_block(lds_u64_ptr buf, lds_ctrl_ptr ctrl, int cap, uint32_t s) {
  const int t = threadIdx.x;
  __syncthreads();
  const uint32_t n = ctrl->count < (uint32_t)cap ? ctrl->count : (uint32_t)cap;
  uint32_t c0 = ctrl->sorted < n ? ctrl->sorted : n;  // sorted distinct prefix left by the previous merge
  if (c0 == n && n <= s) {  // nothing was appended since: the prefix is the result (workgroup-uniform)
    const uint64_t keepT = ctrl->T;
    __syncthreads();
    if (t == 0) ctrl->overflow = 0;
    __syncthreads();
    return MergeResult{n, keepT};
  }
  bool saw = false;  // a genuine hash equal to the padding value: remembered, re-appended at the end
  for (uint32_t i = c0 + t; i < n; i += WG) saw |= buf[i] == SENT;
  if (saw) ctrl->saw_max = 1;
  if (t == 0) ctrl->scan_base = 0;
  __syncthreads();
  // Only the appended candidates buf[c0..n) are sorted; they are then merged with the sorted prefix by
  // rank (every element finds its output position with one binary search in the other run: prefix
  // elements go before equal new ones) into the free space behind them.  Sorting n log^2 n elements
  // again at every merge cost 6.6 % of the kernel at s = 1000 and 25 % at s = 2000.  Falls back to
  // sorting everything when the output does not fit (2n > cap) or there is no prefix yet.
  lds_u64_ptr src = buf;
  if (c0 > 0 && 2 * n <= (uint32_t)cap) {
    const uint32_t m = n - c0;
    bitonic_sort_lds(buf + c0, (int)m);  // ends with a barrier
    for (uint32_t idx = t; idx < n; idx += WG) {
      const uint64_t v = buf[idx];
      const uint32_t pos = idx < c0 ? idx + lds_bound<false>(buf + c0, m, v) : (idx - c0) + lds_bound<true>(buf, c0, v);
      buf[n + pos] = v;
    }
    __syncthreads();
    src = buf + n;
  } else {
    bitonic_sort_lds(buf, (int)n);
  }
  // streaming compaction in rounds of WG elements (dest <= src index when in place; disjoint otherwise)
  const uint32_t lane = t & 63, wave = t >> 6;
  for (int r = 0; r < (int)n; r += WG) {
    const int idx = r + t;
    const bool in = idx < (int)n;
    const uint64_t v = in ? src[idx] : SENT;
    const bool keep = in && v != SENT && (idx == 0 || v != src[idx - 1]);
    const uint64_t bal = __ballot(keep);
    const uint32_t before = __popcll(bal & ((1ULL << lane) - 1ULL));
    if (lane == 0) ctrl->wave_tot[wave] = (uint32_t)__popcll(bal);
    __syncthreads();  // all reads of this round done; wave totals visible
    const uint32_t sb = ctrl->scan_base;
    uint32_t base = sb, total = 0;
#pragma unroll
    for (int w = 0; w < NWAVE; w++) {
      const uint32_t wt = ctrl->wave_tot[w];
      if ((uint32_t)w < wave) base += wt;
      total += wt;
    }
    const uint32_t dest = base + before;
    if (keep && dest < s) buf[dest] = v;
    __syncthreads();  // writes done; wave_tot / scan_base may be rewritten
    if (t == 0) ctrl->scan_base = sb + total;  // read again only after the next barrier
  }
  __syncthreads();
  // every thread derives the result itself (no read after the closing barrier: a fast thread may
  // already be appending again by then)
  const uint32_t sbv = ctrl->scan_base;
  const uint32_t c = sbv < s ? sbv : s;
  const uint64_t newT = (c == s && s > 0) ? buf[s - 1] : ctrl->T0;
  __syncthreads();
  if (t == 0) { ctrl->count = c; ctrl->sorted = c; ctrl->T = newT; ctrl->overflow = 0; }
  __syncthreads();
  return MergeResult{c, newT};
}

// One lane's view of a tile: 112 consecutive bases = 36 warm-up + 76 owned k-mer end positions,
// fetched straight from global memory as seven 16-byte loads (no LDS staging: the 38 KiB tile would
// cost most of the occupancy, and each line is still read from HBM once -- neighbouring lanes
// share lines through L2).
// `tile` points at the tile's first base (wave-uniform, lives in SGPRs); rq is the lane's offset
// relative to it and [gb, ge) the genome's extent in the same coordinates (clamped to +-2^30), so the
// lane keeps 32-bit offsets only and the load is an SGPR-base + VGPR-offset global_load_dwordx4.
constexpr int LOAD_BIAS = 64;  // offsets handed to the load are rq + LOAD_BIAS >= 0 (rq >= -4*WARM_DW)
__device__ __forceinline__ uint4 load_bases16(const uint8_t* __restrict__ tile, int rq, int gb, int ge) {
  if (rq >= gb && rq + 16 <= ge)
    return *reinterpret_cast<const uint4*>((tile - LOAD_BIAS) + (uint32_t)(rq + LOAD_BIAS));
  uint32_t ww[4];
#pragma unroll
  for (int d = 0; d < 4; d++) {
    uint32_t x = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int p = rq + 4 * d + b;
      const uint32_t ch = (p >= gb && p < ge) ? (tile - LOAD_BIAS)[(uint32_t)(p + LOAD_BIAS)] : (uint32_t)'N';
      x |= ch << (8 * b);
    }
    ww[d] = x;
  }
  return make_uint4(ww[0], ww[1], ww[2], ww[3]);
}

// values every lane holds identically (read from LDS after a barrier): move them to SGPRs so the
// compiler emits scalar branches and compares against scalar operands
__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return ((uint64_t)uniform32((uint32_t)(v >> 32)) << 32) | uniform32((uint32_t)v);
}

// ---- the candidate path of the two sketch kernels ------------------------------------------------
// What a workgroup does with its k-mers once an input format has produced them: test, queue, append, merge, write
// out.  Loading, decoding, the express loop's shape and rolls and the validity bookkeeping are each unit's.

// LDS of one workgroup: [hash tables | candidate buffer (cap x u64) | Ctrl | NWAVE candidate queues]
struct WgState {
  lds_byte_ptr lut;    // at LDS offset 0: table offsets become ds_read immediates
  lds_u64_ptr buf;
  lds_ctrl_ptr ctrl;
  lds_u64_ptr wq;      // this wave's candidate queue: QCAP x {f1, f2}
  int cap;
  uint32_t s;          // hashes to select
  uint32_t room;       // cap - s, >= MIN_ROOM by construction
  uint32_t lane;
  int t;
};
__device__ __forceinline__ WgState carve_lds(unsigned char* smem, int k, bool pk, int cap, uint32_t s) {
  const lds_byte_ptr lds0 = (lds_byte_ptr)smem;
  // kmer_loads addresses the tables by absolute LDS address; the kernels have no static LDS, so the
  // dynamic allocation starts at 0 -- trap rather than hash with wrong tables if that ever changes
  if ((uint32_t)(uintptr_t)lds0 != 0u) __builtin_trap();
  WgState W;
  W.lut = lds0;
  W.buf = (lds_u64_ptr)(lds0 + lut_bytes(k, pk));
  W.ctrl = (lds_ctrl_ptr)(lds0 + lut_bytes(k, pk) + (size_t)cap * 8);
  W.wq = (lds_u64_ptr)(lds0 + lut_bytes(k, pk) + (size_t)cap * 8 + ((sizeof(Ctrl) + 15) & ~(size_t)15)) +
         (size_t)(threadIdx.x >> 6) * QCAP * 2;
  W.cap = cap;
  W.s = s;
  W.room = (uint32_t)cap - s;
  W.t = threadIdx.x;
  W.lane = threadIdx.x & 63;
  return W;
}

// Has this workgroup anything to do in this launch?  (workgroup-uniform)  Sets lo1.
// The second launch over the partial segments walks only the genomes whose merged partial sketches came out short of
// s under the starting threshold (flagged by merge_partials_kernel), from "everything passes".
// Sketch sizes beyond one LDS buffer are selected in passes of ascending hash ranges: pass p only
// admits hashes above the largest one kept so far (lo1 = that hash + 1; 0 in the first pass).
__device__ __forceinline__ bool pass_gate(const Segment& sg, int pass_no, const uint32_t* __restrict__ redo, const uint32_t* cnt,
                                          const uint64_t* out, uint32_t* pcnt, uint64_t& lo1) {
  lo1 = 0;
  if (redo && redo[sg.final_slot] == 0) return false;
  if (pass_no > 0) {
    const bool live = cnt[sg.final_slot] == sg.expect;  // genome not exhausted by earlier passes
    const uint64_t lo = live ? out[sg.lo_off] : SENT;
    if (!live || lo == SENT) {
      if (threadIdx.x == 0 && sg.partial) pcnt[sg.cnt_slot] = 0;  // nothing from this segment
      return false;
    }
    lo1 = lo + 1;
  }
  return true;
}

// (re)start of a walk from the threshold Tstart; the caller builds the tables and meets a barrier behind it
__device__ __forceinline__ void reset_ctrl(const WgState& W, uint64_t Tstart) {
  if (W.t == 0) { W.ctrl->T = Tstart; W.ctrl->T0 = Tstart; W.ctrl->sorted = 0; W.ctrl->count = 0; W.ctrl->overflow = 0; W.ctrl->saw_max = 0; W.ctrl->scan_base = 0; }
}

// Mode of a walk's first tile (workgroup-uniform).  Without a starting threshold everything passes and the tile floods
// the buffer: safe mode.  Under one, a tile of tile_bases k-mers expects tile_bases x Tstart / 2^64 candidates; below
// room / 4 -- the bound end_tile holds every later tile to -- it is walked optimistically like any other.  A tile that
// overflows all the same (a repeat whose hash lies under the threshold) is caught by tile_overflowed and walked again
// in safe mode; a restart that lifted Tstart to SENT starts in safe mode again.
__device__ __forceinline__ bool first_tile_safe(const WgState& W, uint64_t Tstart, uint32_t tile_bases) {
  // (through a scalar register: Tstart changes on the restart edge, which the compiler takes for divergent, and every
  // branch on the mode would otherwise be a vector compare under an execution mask)
  return uniform32(Tstart == SENT || __umul64hi((uint64_t)tile_bases, Tstart) >= (uint64_t)(W.room / 4) ? 1u : 0u) != 0u;
}

// finishes the queued halves (one lane each), keeps those still below T and appends them with ONE LDS
// atomic for the whole batch; called where cap - count >= NWAVE * QCAP is guaranteed
__device__ __forceinline__ void drain_queue(const WgState& W, uint32_t& qn, uint64_t T) {
  if (qn == 0) return;
  HashParts qp{0, 0};
  uint64_t h = 0;
  bool okq = false;
  if (W.lane < qn) {
    qp = HashParts{W.wq[2 * W.lane], W.wq[2 * W.lane + 1]};
    h = mm_finish(qp);
    okq = h < T || T == SENT;
  }
  const uint64_t bal = __ballot(okq);
  uint32_t left = 0;
  if (bal) {
    uint32_t base = 0;
    if (W.lane == 0) base = __hip_atomic_fetch_add(&W.ctrl->count, (uint32_t)__popcll(bal), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    base = __shfl(base, 0);
    const uint32_t idx = base + (uint32_t)__popcll(bal & ((1ULL << W.lane) - 1ULL));
    const bool fits = idx < (uint32_t)W.cap;
    if (okq && fits) W.buf[idx] = h;
    // No room (other waves filled the buffer meanwhile; cannot happen while the tile-end guarantee holds):
    // the entry stays queued and the overflow flag forces a merge -- nothing is ever dropped here.
    const uint64_t fbal = __ballot(okq && !fits);
    if (fbal) {
      if (okq && !fits) {
        const uint32_t slot = (uint32_t)__popcll(fbal & ((1ULL << W.lane) - 1ULL));
        W.wq[2 * slot] = qp.f1;
        W.wq[2 * slot + 1] = qp.f2;
        W.ctrl->overflow = 1;
      }
      left = (uint32_t)__popcll(fbal);
    }
  }
  qn = left;
}

// Express walks: finishes the pending k-mer -- hash halves, high-word test against Thi1 = hi(T) + TEST_SLACK, a possible
// candidate to the wave's queue (per k-mer, so that no halves stay live across a dword: the registers go to the reads in
// flight).  lost: the queue could not take it (wave-uniform).
__device__ __forceinline__ void express_handoff(const KmerLoads& pend, const KParams& P, uint32_t Thi1, lds_u64_ptr wq, uint32_t& qn, bool& lost) {
  const HashParts hp = kmer_hash_finish(pend, P);
  const uint64_t mq = __ballot(hash_test_word(hp) <= Thi1);
  if (__builtin_expect(mq != 0, 0)) {  // wave-uniform, rare: kept out of line, the common path falls through
    const uint32_t add = (uint32_t)__popcll(mq);
    if (qn + add <= (uint32_t)QCAP) {
      if (__builtin_amdgcn_inverse_ballot_w64(mq)) {
        const uint32_t slot = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(mq >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mq, 0u));
        wq[2 * slot] = hp.f1;
        wq[2 * slot + 1] = hp.f2;
      }
      qn += add;
    } else {
      lost = true;
    }
  }
}

// General walks, one step of four bases: the four canonical k-mers (top-aligned, first base in bit 63) that end in the four bases `pack`
// (c0<<6|c1<<4|c2<<2|c3) brings, cut out of the extended windows F = fwd << 8 | pack and R = rc | rp << 2k
// (rp: the complemented codes in reverse significance) where `cut` says so (wave-uniform: warm-up bases only roll).
// fwd carries bits above its window: they shift out in the cut.  The windows then take the extended ones' low 64 bits
// and top 2k bits -- in here so that a runtime k meets ONE branch on the k range (a unit's own roll behind the cut cost
// the runtime-k kernels 1 - 3.5 %).
__device__ __forceinline__ void cut_kmers(uint64_t& fwd, uint64_t& rc, uint32_t pack, uint32_t rp, const KParams& P, bool cut, uint64_t canon[4]) {
  if (P.k > 28) {
    // 2k + 8 bits do not fit 64: the same cuts on 128-bit extended windows (k = 29..32)
    typedef unsigned __int128 u128;
    const u128 F = ((u128)fwd << 8) | pack;
    const u128 R = (u128)rc | ((u128)rp << (2 * P.k));
    if (cut) {
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const uint64_t f = (uint64_t)(F >> (6 - 2 * b)) & P.kmask;
        const uint64_t r = (uint64_t)(R >> (2 * b + 2)) & P.kmask;
        canon[b] = (f < r ? f : r) << P.lshift;
      }
    }
    fwd = (uint64_t)F;
    rc = (uint64_t)(R >> 8);
  } else {
    const uint64_t F = (fwd << 8) | pack;
    const uint64_t R = rc | ((uint64_t)rp << (2 * P.k));
    // the four windows are cut out of F / R already top-aligned (one shift + one mask each):
    // the order of two k-mers does not depend on the alignment, and the hash wants them there
    // Bits below the window are NOT cleared: they cannot change which of two different k-mers
    // is smaller (of two equal ones either will do), and the hash never sees them -- table
    // offsets are taken from whole bytes and the tables of a partially filled byte are built
    // from the k-mer's bases only (build_kmer_lut masks by byte count).
    if (cut) {
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const uint64_t f = F << (P.lshift - 6 + 2 * b);   // lshift >= 8 in this path
        const uint64_t r = R << (P.lshift - 2 - 2 * b);
        canon[b] = f < r ? f : r;
      }
    }
    fwd = F;        // masked by whoever needs exactly 2k bits (the ASCII unit's per-base path)
    rc = R >> 8;    // R < 2^(2k+8) by construction, so this is already < 2^(2k)
  }
}

// appends the k-mers of the wave mask `bal` (their hashes in hv) with one LDS atomic
__device__ __forceinline__ void append1(const WgState& W, uint64_t bal, uint64_t hv) {
  if (bal) {  // wave-uniform
    uint32_t base = 0;
    if (W.lane == 0) base = __hip_atomic_fetch_add(&W.ctrl->count, (uint32_t)__popcll(bal), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    base = __shfl(base, 0);
    const uint32_t idx = base + (uint32_t)__popcll(bal & ((1ULL << W.lane) - 1ULL));
    if ((bal >> W.lane) & 1ULL) {
      if (idx < (uint32_t)W.cap) W.buf[idx] = hv;
      else W.ctrl->overflow = 1;
    }
  }
}

// General walks: one step of four k-mers per lane -- hash, test against T (scalar: the compares write wave masks
// directly), candidates to the queue or the buffer.  allok (wave-uniform): all four k-mers of every lane are valid
// and owned; otherwise valid(b) says so for this lane's k-mer b, and is asked on that branch only.
template <class Valid>
__device__ __forceinline__ void kmer_step4(const WgState& W, const KParams& P, const uint64_t canon[4], bool allok, uint64_t& T,
                                           uint64_t lo1, uint32_t& qn, bool safe_mode, Valid&& valid) {
  // what this wave appends directly (not through its queue): filled by the branches below, appended behind them --
  // in safe mode one k-mer per lane at a time, every wave meeting the same barriers whether it appends or not
  uint64_t am[4] = {0, 0, 0, 0}, ah[4] = {0, 0, 0, 0};
  const uint32_t Thi = (uint32_t)(T >> 32);
  if (allok && P.use64 && !lo1 && Thi < 0xffffffffu - TEST_SLACK) {
    // The steady state: hash = fin(f1) + fin(f2) where fin() touches the low word only, so
    // hi(hash) = hi(f1) + hi(f2) + carry.  The test word w (hash_test_word) is hi(hash) + {0, 1, 2}: with
    // w > hi(T) + TEST_SLACK the hash cannot be below T -- one 32-bit compare per k-mer and the halves'
    // last multiply is never formed (T != SENT here since hi(T) < 2^32 - 1 - TEST_SLACK).  The few
    // waves holding a possible candidate (~64 s / N of them) finish exactly.
    // four independent hash chains: their LDS table reads and multiplies overlap
    HashParts hp[4];
#pragma unroll
    for (int b = 0; b < 4; b++) hp[b] = kmer_hash_parts(canon[b], P);
    const uint32_t Thi1 = Thi + TEST_SLACK;
    uint64_t cm = 0, mq[4];
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const uint32_t u = hash_test_word(hp[b]);
      mq[b] = __ballot(u <= Thi1);
      cm |= mq[b];
    }
    if (cm) {  // wave-uniform, rare
      // Possible candidates are not finished here (a wave would spend ~35 instructions on what is
      // usually ONE lane's k-mer, ~5 % of the kernel at s = 1000): their two hash halves go to this
      // wave's LDS queue -- slots from the wave masks, no atomics -- and are finished, tested exactly
      // and appended a queue-full at a time (drain_queue, at tile ends where room is guaranteed).
      const uint32_t add = (uint32_t)(__popcll(mq[0]) + __popcll(mq[1]) + __popcll(mq[2]) + __popcll(mq[3]));
      if (qn + add <= (uint32_t)QCAP) {
        uint32_t qb = qn;
#pragma unroll
        for (int b = 0; b < 4; b++) {
          if (mq[b]) {  // wave-uniform
            if ((mq[b] >> W.lane) & 1ULL) {
              const uint32_t slot = qb + (uint32_t)__popcll(mq[b] & ((1ULL << W.lane) - 1ULL));
              W.wq[2 * slot] = hp[b].f1;
              W.wq[2 * slot + 1] = hp[b].f2;
            }
            qb += (uint32_t)__popcll(mq[b]);
          }
        }
        qn = qb;
      } else {  // queue full (early in a genome, T still high): finish and append on the spot
        uint64_t h[4], m[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
          // (volatile: keeps the finishing arithmetic inside this branch -- left to itself the
          // compiler computes it speculatively for every k-mer, which is the cost being avoided)
          HashParts q = hp[b];
          asm volatile("" : "+v"(q.f1), "+v"(q.f2));
          h[b] = mm_finish(q);
          m[b] = __ballot(h[b] < T);
          am[b] = m[b]; ah[b] = h[b];
        }
      }
    }
  } else {
    uint64_t h[4], m[4];
#pragma unroll
    for (int b = 0; b < 4; b++) h[b] = kmer_hash(canon[b], P);
    if (allok && T != SENT) {  // one 64-bit compare per k-mer
#pragma unroll
      for (int b = 0; b < 4; b++) m[b] = __ballot(h[b] < T);
    } else {
#pragma unroll
      for (int b = 0; b < 4; b++) {
        // T == SENT means "sketch not full yet": everything passes (also a hash == SENT)
        m[b] = __ballot(valid(b) && (h[b] < T || T == SENT));
      }
    }
    if (lo1) {  // workgroup-uniform: later passes of a large sketch
#pragma unroll
      for (int b = 0; b < 4; b++) m[b] &= __ballot(h[b] >= lo1);
    }
#pragma unroll
    for (int b = 0; b < 4; b++) { am[b] = m[b]; ah[b] = h[b]; }
  }
  if (safe_mode) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
      // bound the next appends (at most one per lane) so the buffer cannot overflow
      __syncthreads();
      const uint32_t cn = uniform32(W.ctrl->count);
      if ((uint32_t)W.cap - cn < (uint32_t)STEP_APPENDS) T = uniform64(merge_block(W.buf, W.ctrl, W.cap, W.s).T);
      __syncthreads();
      append1(W, am[b], ah[b]);
    }
  } else if (am[0] | am[1] | am[2] | am[3]) {
#pragma unroll
    for (int b = 0; b < 4; b++) append1(W, am[b], ah[b]);
  }
}

// Behind a tile's walk (all threads arrive).  True: the optimistic walk lost candidates -- what the buffer holds
// is folded (count may exceed cap: the clamp happens inside merge_block) and the caller walks the tile again, in safe mode.
__device__ __forceinline__ bool tile_overflowed(const WgState& W, uint64_t& T, uint32_t& count_at_tile_start, bool& safe_mode) {
  __syncthreads();
  if (!uniform32(W.ctrl->overflow)) return false;
  safe_mode = true;
  const MergeResult mr = merge_block(W.buf, W.ctrl, W.cap, W.s);
  count_at_tile_start = uniform32(mr.count);
  T = uniform64(mr.T);
  return true;
}

// End of a tile: decides about merging and the next tile's mode, drains a queue that is filling up.
// count_at_tile_start is carried in registers: identical in every thread.
__device__ __forceinline__ void end_tile(const WgState& W, uint64_t& T, uint32_t& qn, uint32_t& count_at_tile_start, bool& safe_mode) {
  const uint32_t cn = uniform32(W.ctrl->count);
  const uint32_t appended = cn - (count_at_tile_start < cn ? count_at_tile_start : cn);
  // merge early enough that the rank merge's output still fits behind the candidates (2n <= cap)
  const uint32_t half = (uint32_t)W.cap / 2;
  const bool need_merge = cn > ((half > W.s + 512 && half < W.s + W.room / 2) ? half : W.s + W.room / 2);
  safe_mode = appended > W.room / 4;
  __syncthreads();  // all reads of ctrl->count done before merge or the next tile's appends
  if (need_merge) {
    const MergeResult mr = merge_block(W.buf, W.ctrl, W.cap, W.s);
    count_at_tile_start = uniform32(mr.count);
    T = uniform64(mr.T);
  }
  else count_at_tile_start = cn;
  // room is guaranteed here (count <= s + room/2, so cap - count >= MIN_ROOM/2 >= NWAVE * QCAP)
  if (qn >= (uint32_t)QDRAIN) drain_queue(W, qn, T);
}

// Final fold and write-out.  True (workgroup-uniform): fewer than s hashes under a starting threshold that was too
// optimistic for this genome -- Tstart is lifted and the caller walks the segment again.
__device__ __forceinline__ bool finish_sketch(const WgState& W, const Segment& sg, uint64_t T, uint32_t& qn, uint64_t& Tstart, int pass_no,
                                              uint64_t* out, uint32_t* cnt, uint64_t* parts, uint32_t* pcnt) {
  drain_queue(W, qn, T);
  T = uniform64(merge_block(W.buf, W.ctrl, W.cap, W.s).T);   // frees room should a queue still hold entries
  drain_queue(W, qn, T);
  uint32_t n = merge_block(W.buf, W.ctrl, W.cap, W.s).count;
  if (n < W.s && Tstart != SENT && !sg.partial) {
    Tstart = SENT;
    __syncthreads();
    return true;
  }
  uint64_t* o = (sg.partial ? parts : out) + sg.out_off;
  for (uint32_t i = W.t; i < n; i += WG) o[i] = W.buf[i];
  if (W.t == 0) {
    if (W.ctrl->saw_max && n < W.s) { o[n] = SENT; n++; }
    // direct segments accumulate over passes; partial slots hold this pass's count only
    if (sg.partial) pcnt[sg.cnt_slot] = n;
    else cnt[sg.cnt_slot] = pass_no > 0 ? sg.expect + n : n;
  }
  return false;
}

// ---- merge of per-segment partial sketches (one workgroup per multi-segment genome) ---------------
struct MergeJob {
  uint64_t part_off;   // element offset of first partial in partial buffer
  uint32_t part_cnt0;  // index of first partial's count
  uint32_t nparts;
  uint64_t out_off;
  uint32_t cnt_slot;
  uint32_t sketch_size;
  uint32_t stride;
  uint32_t expect;     // hashes the genome holds from earlier passes (0 in the first pass)
  uint32_t pass;
  uint32_t t0_used;    // the segments started from a threshold: fewer than s merged hashes flag the genome for a second walk
};

__global__ __launch_bounds__(WG) void merge_partials_kernel(const MergeJob* __restrict__ jobs,
                                                            const uint64_t* __restrict__ parts,
                                                            const uint32_t* __restrict__ pcnt, int cap,
                                                            uint64_t* out,
                                                            uint32_t* cnt, uint32_t* redo, int redo_run) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const lds_u64_ptr buf = (lds_u64_ptr)(lds_byte_ptr)smem;
  const lds_ctrl_ptr ctrl = (lds_ctrl_ptr)((lds_byte_ptr)smem + (size_t)cap * 8);
  const MergeJob jb = jobs[blockIdx.x];
  const int t = threadIdx.x;
  const uint32_t s = jb.sketch_size;
  if (jb.pass > 0 && cnt[jb.cnt_slot] != jb.expect) return;  // genome exhausted by earlier passes
  if (redo_run && redo[jb.cnt_slot] == 0) return;            // second launch: flagged genomes only
  if (t == 0) { ctrl->T = SENT; ctrl->T0 = SENT; ctrl->sorted = 0; ctrl->count = 0; ctrl->overflow = 0; ctrl->saw_max = 0; ctrl->scan_base = 0; }
  __syncthreads();
  uint32_t nmerged = 0;
  for (uint32_t p = 0; p < jb.nparts; p++) {
    const uint32_t pc = pcnt[jb.part_cnt0 + p];
    const uint64_t* src = parts + jb.part_off + (uint64_t)p * jb.stride;
    const uint32_t base = nmerged;
    __syncthreads();
    for (uint32_t i = t; i < pc; i += WG) {
      uint64_t v = src[i];
      if (v == SENT) ctrl->saw_max = 1;
      buf[base + i] = v;  // SENT entries are dropped by the merge
    }
    __syncthreads();
    if (t == 0) ctrl->count = base + pc;
    nmerged = merge_block(buf, ctrl, cap, s).count;
  }
  uint32_t n = nmerged;
  uint64_t* o = out + jb.out_off;
  for (uint32_t i = t; i < n; i += WG) o[i] = buf[i];
  if (t == 0) {
    if (ctrl->saw_max && n < s) { o[n] = SENT; n++; }
    cnt[jb.cnt_slot] = jb.expect + n;
    if (!redo_run && jb.t0_used && n < s) redo[jb.cnt_slot] = 1;  // the genome may hold hashes above its starting threshold
  }
}

inline int pow2ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }


// ---- host side: the segment plan and the launch sequence of a batch (shared by the two input formats) -------------
struct MinhashPlanInfo {   // handed to `prepare` once the segment table is on the device
  const Segment* d_segs;   // all passes' segments, pass by pass
  size_t nsegs;
  size_t lds;              // dynamic LDS of the sketch kernel
  bool packed_tables;      // table layout (lut_bytes)
};
struct MinhashLaunch {     // one launch of the sketch kernel
  const Segment* d_segs;   // first segment of the launch
  size_t seg_index;        // its index in the table handed to `prepare`
  uint32_t nseg;
  int pass, cap;
  size_t lds;
  bool packed_tables, runtime_k;   // runtime_k: the gated second walk over flagged genomes
  uint64_t* d_parts;
  uint32_t* d_pcnt;
  const uint32_t* d_redo;
};

// Defines NAME(k, seed, runtime_k, packed): the instantiation of the sketch kernel template KERN<KT, PK> to launch.
// Compile-time k for 16..32: the values the reference's tune_parameters lands on for Mbp..Gbp
// genomes (recommended k = ceil(log4(maxSize * 9999)) = 17..23, accepted up to +3), its default 21
// and the customary 31/32; anything else, and any seed but the reference's, takes the runtime-k kernel.
#define RTC_MINHASH_PICK(NAME, KERN)                                                                      \
  inline decltype(&KERN<0, false>) NAME(int k, uint32_t seed, bool runtime_k, bool packed) {              \
    switch (!runtime_k && seed == MASH_SEED ? k : 0) {                                                    \
      RTC_PICK_K(KERN, 16) RTC_PICK_K(KERN, 17) RTC_PICK_K(KERN, 18) RTC_PICK_K(KERN, 19)                 \
      RTC_PICK_K(KERN, 20) RTC_PICK_K(KERN, 21) RTC_PICK_K(KERN, 22) RTC_PICK_K(KERN, 23)                 \
      RTC_PICK_K(KERN, 24) RTC_PICK_K(KERN, 25) RTC_PICK_K(KERN, 26) RTC_PICK_K(KERN, 27)                 \
      RTC_PICK_K(KERN, 28) RTC_PICK_K(KERN, 29) RTC_PICK_K(KERN, 30) RTC_PICK_K(KERN, 31)                 \
      RTC_PICK_K(KERN, 32)                                                                                \
      default: return packed ? KERN<0, true> : KERN<0, false>;                                            \
    }                                                                                                     \
  }
#define RTC_PICK_K(KERN, K) case K: return packed ? KERN<K, true> : KERN<K, false>;

// Candidate buffer of the sketch kernel: s entries + room, as large as the LDS share of a workgroup
// allows at the best occupancy that still leaves MIN_ROOM (3, 2 or 1 workgroups per CU; the sort
// works on the live count, so the capacity need not be a power of two), and the table layout that goes with it:
// packed only where it buys a workgroup per CU.  At k = 21 the plain tables are 19 KiB (two 16-byte tables, 1 + 2 KiB
// of second halves, the 8 KiB tail table) and three workgroups fit up to s = (53 248 - 19 456 - 80 - 4 096) / 8 - 512
// = 3 190; the packed ones are 16 KiB and reach s = 3 574.  cap == 0: the chunk does not fit at all.
constexpr uint32_t PASS_CHUNK = 6144;  // hashes one pass selects per genome (minhash_run)
struct MinhashLayout { int cap, wgs_per_cu; bool packed; };
inline MinhashLayout minhash_layout(const rtc_options& opt, int k, uint32_t chunk_max, size_t min_room) {
  MinhashLayout lay{0, 1, false};
  for (int wgs = 3; wgs >= 1 && lay.cap == 0; wgs--) {
    // 52 / 78 / 156 KiB: measured on MI355X, a 53.3 KiB allocation no longer runs three workgroups per CU
    const size_t share = ((size_t)156 * 1024 / wgs) & ~(size_t)2047;
    for (int pk = 0; pk < 2 && lay.cap == 0; pk++) {
      // (tests: both layouts are exercised for every k by forcing one of them; either gives the same sketches)
      if (pk && (lut_his(k) == 0 || opt.sketch_no_packed)) break;
      if (!pk && opt.sketch_packed && lut_his(k) > 0) continue;
      const size_t fixed = lut_bytes(k, pk != 0) + ((sizeof(Ctrl) + 15) & ~(size_t)15) + QUEUE_BYTES;
      // (round 1 measured ~3000 entries of room as the break-even against lost occupancy; with the merge sorting
      // only the new candidates and the express walk a third workgroup per CU wins down to the minimum room:
      // s = 2000 at 10 000 x 5 Mbp 114.5 -> 102.1 ms, the containment sketches of config 4 190 -> 164 ms)
      const size_t want_room = min_room;  // what the kernel's safe mode may append between two looks at the count
      if (share > fixed && (share - fixed) / 8 >= (size_t)chunk_max + want_room) lay = MinhashLayout{(int)((share - fixed) / 8), wgs, pk != 0};
    }
  }
  return lay;
}

// tile_bases: bases a workgroup takes per tile (the unit the segment lengths are planned in); min_room: candidate slots the
// kernel's buffer must offer beyond the sketch size.  prepare(MinhashPlanInfo)
// and launch(MinhashLaunch) return a status; everything is enqueued on the context stream.
template <class Prepare, class Launch>
int minhash_run(rtc_ctx* ctx, const uint64_t* h_off, uint32_t n, int k, const uint32_t* h_sizes, uint32_t size,
                uint64_t* d_out, uint32_t stride, uint32_t* d_cnt, uint64_t tile_bases, size_t min_room, Prepare&& prepare, Launch&& launch) {
  RTC_HIP(ctx, hipSetDevice(ctx->device));
  ctx->sketch_gen++;  // sketches on this context change: memos keyed on a sketch buffer are stale

  uint32_t smax = 0;
  for (uint32_t g = 0; g < n; g++) {
    uint32_t s = h_sizes ? h_sizes[g] : size;
    if (s > stride) return rtc_fail(ctx, RTC_ERR_ARG, "sketch size %u of genome %u exceeds stride %u", s, g, stride);
    smax = std::max(smax, s);
  }
  // One pass selects up to CHUNK hashes per genome in LDS; larger sketches take ceil(s/CHUNK) passes
  // over ascending hash ranges (pass p admits only hashes above everything kept so far).
  const uint32_t CHUNK = PASS_CHUNK;
  const uint32_t chunk_max = std::min(smax, CHUNK);
  const uint32_t npass = smax == 0 ? 1 : (smax + CHUNK - 1) / CHUNK;
  const MinhashLayout lay = minhash_layout(ctx->opt, k, chunk_max, min_room);
  const int cap = lay.cap, wgs_per_cu = lay.wgs_per_cu;
  const bool packed = lay.packed;
  if (cap == 0) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "sketch chunk %u does not fit the LDS", chunk_max);
  // partial-sketch merge: two lists fit 2*chunk_max; twice that lets the rank merge work out of place
  const int cap_merge = (int)std::max<uint32_t>(std::max<uint32_t>(2 * chunk_max, std::min<uint32_t>(4 * chunk_max, 16384)), 1024);
  const size_t lds = (size_t)cap * 8 + lut_bytes(k, packed) + ((sizeof(Ctrl) + 15) & ~(size_t)15) + QUEUE_BYTES;
  const size_t lds_m = (size_t)cap_merge * 8 + sizeof(Ctrl);
  if (lds > (size_t)160 * 1024 || lds_m > (size_t)160 * 1024)
    return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "sketch chunk %u needs %zu B of LDS (> 160 KiB)", chunk_max, std::max(lds, lds_m));

  // ---- plan segments ----
  uint64_t total = 0;
  for (uint32_t g = 0; g < n; g++) {
    if (h_off[g + 1] < h_off[g]) return rtc_fail(ctx, RTC_ERR_ARG, "offsets not monotone at genome %u", g);
    total += h_off[g + 1] - h_off[g];
  }
  const uint64_t target_segs = (uint64_t)ctx->num_cu * 12;
  uint64_t seg_len = total / target_segs;
  const uint64_t min_seg = 4ull * tile_bases;
  if (seg_len < min_seg) seg_len = min_seg;
  const uint64_t seg_pref = 24ull * tile_bases;  // preferred segment of the few-genomes plan below

  // segments per genome: ~equal-length pieces of seg_len; 1 = the whole genome in one workgroup
  std::vector<uint32_t> nsv(n);
  uint32_t n_single = 0;
  for (uint32_t g = 0; g < n; g++) {
    const uint64_t len = h_off[g + 1] - h_off[g];
    uint64_t ns = (len + seg_len / 2) / seg_len;
    if (ns < 1) ns = 1;
    if (ns > 4096) ns = 4096;
    nsv[g] = (uint32_t)ns;
    if (ns == 1) n_single++;
  }
  // Whole-genome workgroups run in rounds of `slots` at a time; n mod slots leftover genomes would
  // occupy a nearly empty final round for a full round's duration (10 000 genomes on 768 slots:
  // 16 workgroups alone for 7 % of the kernel).  Cut the last leftover genomes into enough segments
  // to fill that round instead; they go through the partial path, launched after the full rounds.
  const uint32_t slots = (uint32_t)ctx->num_cu * (uint32_t)wgs_per_cu;
  if (n_single > slots) {
    uint32_t q = n_single % slots;
    if (q > 0 && q <= slots * 3 / 5) {
      const uint32_t want = slots / q;
      const uint64_t tail_max = 8;  // more pieces fill the round better but serialise in the per-genome merge (measured: 4-8 best)
      for (uint32_t g = n; g-- > 0 && q > 0;) {
        if (nsv[g] != 1) continue;
        const uint64_t len = h_off[g + 1] - h_off[g];
        const uint64_t ns2 = std::min<uint64_t>(std::min<uint64_t>(want, len / min_seg), tail_max);
        if (ns2 >= 2) nsv[g] = (uint32_t)ns2;
        q--;
      }
    }
  }

  // Few genomes (fewer whole-genome workgroups than the chip holds at a time): the segments are dealt out so that
  // their number is a whole multiple of the slots -- every genome gets its share of R x slots segments by largest
  // remainder, so the workgroups are of nearly equal length and the last round is as full as the first (rounding
  // each genome on its own left e.g. 2 000 x 5 Mbp with 4 000 workgroups for 768 slots: 5.2 rounds).
  if (n_single <= slots && total >= (uint64_t)slots * min_seg) {
    uint64_t rounds = total / ((uint64_t)slots * seg_pref);
    if (ctx->opt.sketch_rounds > 0) rounds = (uint64_t)ctx->opt.sketch_rounds;  // tuning
    rounds = std::max<uint64_t>(1, std::min<uint64_t>(rounds, total / ((uint64_t)slots * min_seg)));
    const uint64_t want = rounds * slots;
    std::vector<std::pair<double, uint32_t>> frac;
    frac.reserve(n);
    uint64_t given = 0;
    for (uint32_t g = 0; g < n; g++) {
      const uint64_t len = h_off[g + 1] - h_off[g];
      const double quota = (double)len * (double)want / (double)total;
      uint64_t ns = (uint64_t)quota;
      const uint64_t most = std::min<uint64_t>(std::max<uint64_t>(len / min_seg, 1), 4096);
      if (ns < 1) ns = 1;
      if (ns > most) ns = most;
      nsv[g] = (uint32_t)ns;
      given += ns;
      if (ns < most) frac.emplace_back(quota - (double)ns, g);
    }
    if (given < want) {
      std::sort(frac.begin(), frac.end(), [](const std::pair<double, uint32_t>& a, const std::pair<double, uint32_t>& b) {
        return a.first != b.first ? a.first > b.first : a.second < b.second;
      });
      for (size_t i = 0; i < frac.size() && given < want; i++) { nsv[frac[i].second]++; given++; }
    }
  }

  // starting threshold = factor x the expected s-th smallest hash (0: start from "everything passes").  3 keeps
  // the restart away down to genomes whose distinct k-mers are a third of their length, and every early tile lets
  // 3 s / N of its k-mers through instead of 8 s / N: 50 000 x 1 Mbp 115 -> 107 ms, config 4's sketches 163 -> 150 ms
  // Dense sketches (a genome of fewer than 2 500 k-mers per sketch hash: the containment sketches of clust-greedy, s = length / 1000)
  // start from 2x: there the candidates and their merges are 9 % of the kernel and a third fewer of them is worth more
  // than the margin (50 000 x 1 Mbp at s = 2000: 98.4 -> 92.3 ms, at s = 1000 83.0 -> 81.1 ms; 5 000 k-mers per hash: no difference).
  const int t0_fixed = ctx->opt.sketch_t0_factor;  // (-1: by rule) tests of the restart path / tuning
  auto start_threshold = [&](uint64_t len, uint32_t s) -> uint64_t {
    if (s == 0) return SENT;
    const uint64_t f = t0_fixed >= 0 ? (uint64_t)t0_fixed : (len / s <= 2500 ? 2u : 3u);
    if (f == 0 || len <= f * s) return SENT;
    return (uint64_t)((((unsigned __int128)1 << 64) * (f * s)) / len);
  };
  struct PassPlan { size_t direct0, ndirect, partial0, npartial, job0, njobs; };
  std::vector<PassPlan> plans(npass);
  std::vector<Segment> direct, partial;
  std::vector<MergeJob> jobs;
  uint64_t part_elems_max = 0;
  uint32_t part_slots_max = 0;
  bool any_partial_t0 = false;
  for (uint32_t ps = 0; ps < npass; ps++) {
    PassPlan& pl = plans[ps];
    pl.direct0 = direct.size(); pl.partial0 = partial.size(); pl.job0 = jobs.size();
    uint64_t part_elems = 0;
    uint32_t part_slots = 0;
    for (uint32_t g = 0; g < n; g++) {
      const uint64_t b = h_off[g], e = h_off[g + 1], len = e - b;
      const uint32_t sg_full = h_sizes ? h_sizes[g] : size;
      if (ps > 0 && sg_full <= ps * CHUNK) continue;  // this genome's sketch is complete
      const uint32_t s = std::min(CHUNK, sg_full - ps * CHUNK);
      const uint32_t expect = ps * CHUNK;
      const uint64_t out_off = (uint64_t)g * stride + expect;
      const uint64_t lo_off = ps ? out_off - 1 : 0;
      const uint64_t ns = nsv[g];
      if (ns == 1) {
        const uint64_t t0 = ps == 0 ? start_threshold(len, s) : SENT;
        direct.push_back(Segment{b, e, b, e, out_off, lo_off, g, s, g, expect, 0, 0, t0});
      } else {
        const uint64_t t0 = ps == 0 ? start_threshold(len, s) : SENT;  // the genome's starting threshold, shared by its segments
        if (t0 != SENT) any_partial_t0 = true;
        jobs.push_back(MergeJob{part_elems, part_slots, (uint32_t)ns, out_off, g, s, chunk_max, expect, ps, t0 != SENT ? 1u : 0u});
        for (uint64_t i = 0; i < ns; i++) {
          const uint64_t sb = b + len * i / ns, se = b + len * (i + 1) / ns;
          partial.push_back(Segment{b, e, sb, se, part_elems, lo_off, part_slots, s, g, expect, 1, 0, t0});
          part_elems += chunk_max;
          part_slots++;
        }
      }
    }
    pl.ndirect = direct.size() - pl.direct0; pl.npartial = partial.size() - pl.partial0; pl.njobs = jobs.size() - pl.job0;
    // workgroups are dispatched in table order: longest genomes first, so that the last round ends with the short ones
    // (results go to the genome's own row, the order is free)
    std::stable_sort(direct.begin() + pl.direct0, direct.end(),
                     [](const Segment& a, const Segment& b) { return a.g_end - a.g_begin > b.g_end - b.g_begin; });
    part_elems_max = std::max(part_elems_max, part_elems);
    part_slots_max = std::max(part_slots_max, part_slots);
  }
  // one segment table, pass by pass: [whole-genome segments | partial segments] -- a single launch per
  // pass walks both (workgroups are dispatched in index order, so the partial segments fill the
  // tail of the last whole-genome round)
  std::vector<Segment> segs;
  segs.reserve(direct.size() + partial.size());
  std::vector<size_t> seg0(npass);
  for (uint32_t ps = 0; ps < npass; ps++) {
    const PassPlan& pl = plans[ps];
    seg0[ps] = segs.size();
    segs.insert(segs.end(), direct.begin() + pl.direct0, direct.begin() + pl.direct0 + pl.ndirect);
    segs.insert(segs.end(), partial.begin() + pl.partial0, partial.begin() + pl.partial0 + pl.npartial);
  }
  const size_t bseg = segs.size() * sizeof(Segment);
  const size_t bjobs = jobs.size() * sizeof(MergeJob);
  void* ws0 = nullptr;
  const size_t bredo = any_partial_t0 ? (size_t)n * 4 : 0;
  RTC_TRY(rtc_ws(ctx, 0, bseg + bjobs + bredo + 64, &ws0));
  Segment* d_segs = (Segment*)ws0;
  MergeJob* d_jobs = (MergeJob*)((char*)ws0 + bseg);
  uint32_t* d_redo = (uint32_t*)((char*)ws0 + bseg + bjobs);  // per genome: walk its segments again without the threshold
  void* hp = nullptr;
  RTC_TRY(rtc_pinned(ctx, bseg + bjobs + 64, &hp));
  RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // pinned staging may still be in flight
  memcpy(hp, segs.data(), bseg);
  memcpy((char*)hp + bseg, jobs.data(), bjobs);
  RTC_HIP(ctx, hipMemcpyAsync(ws0, hp, bseg + bjobs, hipMemcpyHostToDevice, ctx->stream));
  if (bredo) RTC_HIP(ctx, hipMemsetAsync(d_redo, 0, bredo, ctx->stream));

  uint64_t* d_parts = nullptr;
  uint32_t* d_pcnt = nullptr;
  if (!partial.empty()) {
    void* ws1 = nullptr;
    RTC_TRY(rtc_ws(ctx, 1, part_elems_max * 8 + (size_t)part_slots_max * 4 + 64, &ws1));
    d_parts = (uint64_t*)ws1;
    d_pcnt = (uint32_t*)((char*)ws1 + part_elems_max * 8);
  }


  MinhashPlanInfo pi{d_segs, segs.size(), lds, packed};
  RTC_TRY(prepare(pi));
  RTC_HIP(ctx, hipFuncSetAttribute((const void*)merge_partials_kernel,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_m));
  for (uint32_t ps = 0; ps < npass; ps++) {
    const PassPlan& pl = plans[ps];
    if (pl.ndirect + pl.npartial) {
      RTC_TRY(launch(MinhashLaunch{d_segs + seg0[ps], seg0[ps], (uint32_t)(pl.ndirect + pl.npartial), (int)ps, cap, lds, packed, false,
                                   d_parts, d_pcnt, (const uint32_t*)nullptr}));
    }
    if (pl.npartial) {
      hipLaunchKernelGGL(merge_partials_kernel, dim3((uint32_t)pl.njobs), dim3(WG), lds_m, ctx->stream,
                         d_jobs + pl.job0, d_parts, d_pcnt, cap_merge, d_out, d_cnt, d_redo, 0);
      RTC_CHECK_LAUNCH(ctx);
      if (ps == 0 && any_partial_t0) {
        // genomes the merge flagged (fewer than s hashes below the starting threshold): their segments once more
        // from "everything passes", merged again; every other workgroup of the two launches leaves at once
        // (the runtime-k instantiation: the flagged genomes are few, and the gated launch stays out of the compile-time-k
        // kernel's per-launch statistics)
        RTC_TRY(launch(MinhashLaunch{d_segs + seg0[ps] + pl.ndirect, seg0[ps] + pl.ndirect, (uint32_t)pl.npartial, (int)ps, cap, lds, packed,
                                     true, d_parts, d_pcnt, (const uint32_t*)d_redo}));
        hipLaunchKernelGGL(merge_partials_kernel, dim3((uint32_t)pl.njobs), dim3(WG), lds_m, ctx->stream,
                           d_jobs + pl.job0, d_parts, d_pcnt, cap_merge, d_out, d_cnt, d_redo, 1);
        RTC_CHECK_LAUNCH(ctx);
      }
    }
  }
  return RTC_OK;
}

}  // namespace
