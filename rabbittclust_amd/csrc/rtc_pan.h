// rtc_pan.h -- the path boundaries and the byte accounting of rtc_pangenome (rtc_pangenome.hip; DESIGN 3.4u has the reasons),
// mirrored by api.PAN_* and held together by tests/test_cpu_pangenome.py.
#ifndef RTC_PAN_H
#define RTC_PAN_H
#include <stdint.h>

// A slot is 12 bytes: the hash as a 64-bit key (8) and the number of members that hold it (4).  A table is never more than half
// full: a cluster of K records (the sum of its members' sketch lengths) has at most K distinct hashes and 2 K slots or more.
// The LDS of a CU is 160 KiB = 163 840 bytes; beside the table a workgroup keeps the cluster's histogram (4 bytes an entry)
// and 64 bytes of scalars.
//   clusters of up to PAN_WAVE_RECORDS records:  one wave; 1 024 slots = 12 KiB, a histogram of 512 entries = 2 KiB: 14 400
//     bytes a workgroup, 11 workgroups (11 waves) on a CU
//   clusters of up to PAN_BLOCK_RECORDS records: 256 lanes; 4 096 slots = 48 KiB, a histogram of 1 024 entries = 4 KiB: 53 312
//     bytes a workgroup, three workgroups (12 waves) on a CU = 159 936 bytes.  A histogram of 2 048 entries would leave two.
//   everything larger: the arena in global memory, 1 << max(PAN_GLOBAL_LOG2_MIN, ceil(log2(2 K))) slots a cluster
// A cluster on an LDS path with more members than its histogram has entries (most of its members then have empty sketches) adds
// to the histogram in global memory instead.
constexpr uint32_t PAN_WAVE_RECORDS = 512, PAN_WAVE_SLOTS = 1024, PAN_WAVE_HIST = 512;
constexpr uint32_t PAN_BLOCK_RECORDS = 2048, PAN_BLOCK_SLOTS = 4096, PAN_BLOCK_HIST = 1024;
constexpr uint32_t PAN_WAVE_WGS_PER_CU = 11, PAN_BLOCK_WGS_PER_CU = 3;
// An arena table starts at a multiple of 256 slots and has 256 or more (RTC_PAN_GLOBAL=1 brings small clusters here), so a tile of
// 256 slots of the sweep lies in one table.
constexpr uint32_t PAN_GLOBAL_LOG2_MIN = 8;
// The arena kernels' grids: workgroups of 256 lanes a CU.  The count and look-up kernels take a member a wave, the sweep a tile of
// 256 slots a turn, a workgroup a contiguous run of tiles.
constexpr uint32_t PAN_GLOBAL_WGS_PER_CU = 16;
// The sweep counts the slots with 2 <= occ < 2 + PAN_SWEEP_BINS in bins in the workgroup's LDS (4 KiB).
constexpr uint32_t PAN_SWEEP_BINS = 1024;
// What a group of clusters is charged against RTC_PAN_BYTES: a slot of its arena tables, a member (its place in the permutation
// 4, its record offset 8, its histogram entry 8, its record 32, its cluster's place in the arena list 4) and a cluster (its
// descriptor 24, its place in the path lists 4, its table's offset 8, its all-ones word 4, rounded up).
constexpr uint64_t PAN_SLOT_BYTES = 12, PAN_MEMBER_BYTES = 56, PAN_CLUSTER_BYTES = 48;
// The all-ones 64-bit value marks an empty slot.  A hash of that value (possible at width 8 only: the keys of width-4 sketches
// are widened) is counted in a word of its own per cluster, never in the table.
constexpr uint64_t PAN_EMPTY = ~0ull;
// slot(hash, log2_slots) = (hash * PAN_MULT mod 2^64) >> (64 - log2_slots); linear probing from there, wrapping
constexpr uint64_t PAN_MULT = 0x9E3779B97F4A7C15ull;
// rtc_pan_growth's most points
constexpr uint32_t PAN_GROWTH_POINTS = 256;

#endif  // RTC_PAN_H
