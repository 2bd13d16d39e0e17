// rtc_jackknife.h -- the delete-half jackknife over sketch hashes (include/rtclust.h: rtc_nj_support): the mask word of a hash
// and the wave routine that counts, for one pair of ascending lists, the common hashes each of 64 replicates keeps -- one
// replicate per lane.  rtc_nj_support.hip runs it over the pairs of the key blocks and, through rtc_jackknife_pairs_dev, over an
// edge list; both kernels call the same __device__ code.
//
// The walk is mash_merge_wave's (rtc_dbscan_mash.h) without the truncation: one list staged in LDS (up to JK_LDS_ELEMS elements;
// a longer one is searched where it lies), the other taken in coalesced chunks of 64, every lane ranking its element by binary
// search, a ballot of the matches.  Every matching lane forms its hash's mask word; the words are then made uniform one match
// after the other and lane r adds bit r.
#pragma once
#include "rtc_internal.h"

constexpr uint32_t JK_LDS_ELEMS = 1024;  // the staged list's longest length (8 KiB of u64 per wave); api.JK_LDS_ELEMS

__host__ __device__ __forceinline__ uint64_t rtc_jk_mix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// key = rtc_jk_mix(seed + word): the same for every hash of a launch
__host__ __device__ __forceinline__ uint64_t rtc_jk_word(uint64_t hash, uint64_t key) { return rtc_jk_mix(hash ^ key); }

namespace {

// The lanes of bal hold a mask word each; lane r adds bit r of every one of them.  bal is uniform, so is the loop.
__device__ __forceinline__ uint32_t jk_add_words(uint64_t W, uint64_t bal, uint32_t lane) {
  const int lo = (int)(uint32_t)W, hi = (int)(uint32_t)(W >> 32);
  const uint32_t sh = lane & 31;
  const bool upper = lane >= 32;
  uint32_t cnt = 0;
  for (uint64_t t = bal; t; t &= t - 1) {
    const int k = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(t));
    const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane(lo, k), wh = (uint32_t)__builtin_amdgcn_readlane(hi, k);
    cnt += ((upper ? wh : wl) >> sh) & 1u;
  }
  return cnt;
}

// s[0 .. ns) into the wave's LDS when it fits; returns whether it did.  One wave per workgroup: the barriers are the wave's own.
template <typename T>
__device__ __forceinline__ bool jk_stage(T* sb, const T* __restrict__ s, uint32_t ns, uint32_t lane) {
  const bool staged = ns <= JK_LDS_ELEMS;
  __syncthreads();  // the list before is done with
  if (staged)
    for (uint32_t x = lane; x < ns; x += 64) sb[x] = s[x];
  __syncthreads();
  return staged;
}

// Lane r returns |{h in s and l : bit r of rtc_jk_word(h, key) is set}|.  s and l ascend without repeats; sb holds s when staged.
template <typename T>
__device__ __forceinline__ uint32_t jk_pair_wave(const T* __restrict__ s, uint32_t ns, const T* sb, bool staged, const T* __restrict__ l,
                                                 uint32_t nl, uint64_t key, uint32_t lane) {
  uint32_t cnt = 0, lo0 = 0;
  if (ns == 0) return 0;
  for (uint32_t base = 0; base < nl; base += 64) {  // uniform
    const uint32_t i = base + lane;
    const bool valid = i < nl;
    T v = 0;
    if (valid) v = l[i];
    // lo = the elements of s below v; the chunk before left lo0 of them below its last element
    uint32_t lo = valid ? lo0 : ns, hi = ns;
    bool m = false;
    if (staged) {
      while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (sb[mid] < v) lo = mid + 1; else hi = mid; }
      m = valid && lo < ns && sb[lo] == v;
    } else {
      while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (s[mid] < v) lo = mid + 1; else hi = mid; }
      m = valid && lo < ns && s[lo] == v;
    }
    const uint64_t bal = __ballot(m);
    if (bal) cnt += jk_add_words(rtc_jk_word((uint64_t)v, key), bal, lane);
    const uint32_t last = nl - base < 64 ? nl - base - 1 : 63;
    lo0 = __shfl(lo, last);
    if (lo0 >= ns) break;  // all of s lies below this chunk's last element: nothing further matches
  }
  return cnt;
}

// Lane r returns |{h in l : bit r of its mask word is set}|: the same accumulation with every element a match.
template <typename T>
__device__ __forceinline__ uint32_t jk_size_wave(const T* __restrict__ l, uint32_t nl, uint64_t key, uint32_t lane) {
  uint32_t cnt = 0;
  for (uint32_t base = 0; base < nl; base += 64) {  // uniform
    const uint32_t i = base + lane;
    const bool valid = i < nl;
    T v = 0;
    if (valid) v = l[i];
    cnt += jk_add_words(rtc_jk_word((uint64_t)v, key), __ballot(valid), lane);
  }
  return cnt;
}

}  // namespace
