// rtc_snn.h -- the path boundaries and the grids of rtc_graph_snn's counting kernel (rtc_snn.hip; DESIGN 3.4p has the
// reasoning).  A record is counted by the end with the longer row, its owner; the path is chosen by the length of the owner's
// row alone, by what fits the LDS of a CU at the residency wanted and not by a measured threshold.  rabbittclust_amd/api.py
// mirrors the two boundaries (SNN_WAVE_ROW, SNN_BLOCK_ROW); tests/test_cpu_snn.py holds the two files together.
#ifndef RTC_SNN_H
#define RTC_SNN_H
#include <stdint.h>

// A workgroup takes a slice of as many records as it has lanes and keeps SNN_SLICE_BYTES of LDS per record: the owner (4), the
// other end (4), the other end's row length with the "owner is u" bit (4), the record's index (8), the other row's start (8).
constexpr uint32_t SNN_SLICE_BYTES = 28;
// One wave, the owner's row in LDS.  A CU holds 32 waves and 160 KiB of LDS: 5 KiB per one-wave workgroup keep every wave slot
// usable.  5120 - 64 * 28 - 8 (the run heads) = 3320 bytes = 830 entries; 768 is the multiple of 256 below it.
constexpr uint32_t SNN_WAVE_ROW = 768;
// A 256-lane workgroup, the owner's row in LDS.  Four workgroups a CU (16 waves, half its wave slots: a probe is a chain of
// dependent LDS reads, so the waves are what hides them): 40 KiB each.  40960 - 256 * 28 - 32 = 33760 bytes = 8440 entries;
// 8192 is the multiple of 256 below it.
constexpr uint32_t SNN_BLOCK_ROW = 8192;
// beyond: a 256-lane workgroup searches the owner's row where it lies in global memory
// workgroups a CU of each launch; a workgroup takes the slices it, it + grid, ... of its path
constexpr uint32_t SNN_OWNER_WGS_PER_CU = 4;  // snn_owner_kernel: every workgroup ends in four atomics on the same four words
constexpr uint32_t SNN_WAVE_WGS_PER_CU = 32;
constexpr uint32_t SNN_BLOCK_WGS_PER_CU = 4;
constexpr uint32_t SNN_GLOBAL_WGS_PER_CU = 8;

#endif  // RTC_SNN_H
