// rtc_quality.h -- the path boundaries of rtc_silhouette's row kernel (rtc_quality.hip; DESIGN 3.4n has the reasons), mirrored by
// api.SIL_WAVE_ROW / SIL_WAVE_SLOTS / SIL_BLOCK_ROW / SIL_BLOCK_SLOTS / SIL_GLOBAL_LOG2_MIN and held together by
// tests/test_cpu_quality.py.
#ifndef RTC_QUALITY_H
#define RTC_QUALITY_H
#include <stdint.h>

// A slot is 16 bytes: the cluster id (4), the number of listed neighbours in it (4), the sum of their q (8).  A table is never
// more than half full: a row of L entries meets at most L clusters and has 2 L slots or more.
//   rows of up to SIL_WAVE_ROW entries:  one wave, 256 slots = 4 KiB of LDS: LDS never limits the workgroups on a CU
//   rows of up to SIL_BLOCK_ROW entries: 256 lanes, 2 048 slots = 32 KiB of LDS: four workgroups (16 waves) on a CU's 160 KiB
//   longer rows:                         256 lanes, a table of 1 << max(SIL_GLOBAL_LOG2_MIN, ceil(log2(2 L))) slots in global memory
// Louvain's workgroup path takes rows of 2 048 with 12-byte slots in 48 KiB, three workgroups a CU; at 16 bytes a slot the same row
// limit would leave two.
constexpr uint32_t SIL_WAVE_ROW = 128, SIL_WAVE_SLOTS = 256, SIL_BLOCK_ROW = 1024, SIL_BLOCK_SLOTS = 2048;
// RTC_SIL_GLOBAL=1 sends short rows to the global table too: theirs has 64 slots or more
constexpr uint32_t SIL_GLOBAL_LOG2_MIN = 6;
constexpr uint32_t SIL_WAVE_WGS_PER_CU = 32, SIL_BLOCK_WGS_PER_CU = 4, SIL_GLOBAL_WGS_PER_CU = 8;

#endif  // RTC_QUALITY_H
