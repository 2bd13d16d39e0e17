// rtc_mcl.h -- the path boundaries, the table hash and the grids of rtc_mcl's kernels (rtc_mcl.hip; DESIGN 3.4m has the
// reasoning).  A column's work W is the number of products its expansion gathers, the sum of the lengths of the columns it
// names: known before the launch, and no column can touch more distinct rows than that.  rabbittclust_amd/api.py mirrors the
// two boundaries (MCL_WAVE_WORK, MCL_BLOCK_WORK); tests/test_cpu_mcl.py holds the two files together, and tests/mcl_sets.py
// reads every constant here to size its inputs.
#ifndef RTC_MCL_H
#define RTC_MCL_H
#include <stdint.h>

// W <= MCL_WAVE_WORK: a workgroup of one wave, MCL_WAVE_SLOTS slots of (row u32, sum u64) in LDS: 6 KiB, so the 160 KiB of a
// CU never limit the waves it holds.  The table is at most half full.
constexpr uint32_t MCL_WAVE_WORK = 256;
constexpr uint32_t MCL_WAVE_SLOTS = 512;
// W <= MCL_BLOCK_WORK: 256 lanes, MCL_BLOCK_SLOTS slots in LDS: 48 KiB, three workgroups on a CU.  At most three quarters full
// -- and that only if no two products of the column meet in a row.
constexpr uint32_t MCL_BLOCK_WORK = 3072;
constexpr uint32_t MCL_BLOCK_SLOTS = 4096;
// beyond: 256 lanes, a table of at least 2 min(W, n) slots in global memory, one per resident workgroup
constexpr uint32_t MCL_GLOBAL_LOG2_MIN = 10;
// a row's home slot in a table of 2^b slots is the top b bits of row * MCL_GOLDEN (mod 2^32); a taken slot sends the probe on
// by one, from the last slot to slot 0
constexpr uint32_t MCL_GOLDEN = 2654435761u;
// workgroups a CU of each launch, each of which takes the columns it, it + grid, ... of its list: min(n, CUs * the multiplier).
// tests/mcl_sets.py reads these to build inputs that give every workgroup more than one column.
constexpr uint32_t MCL_START_WGS_PER_CU = 8;
constexpr uint32_t MCL_WAVE_WGS_PER_CU = 32;
constexpr uint32_t MCL_BLOCK_WGS_PER_CU = 3;
constexpr uint32_t MCL_GLOBAL_WGS_PER_CU = 4;

#endif  // RTC_MCL_H
