// rtc_screen.h -- the path boundaries and the memory accounting of rtc_rep_screen's kernels (rtc_rep_screen.hip; DESIGN 3.4t has
// the reasoning).  A sample's gather is run by one workgroup; the path is chosen by the number of its eligible candidates alone,
// by what fits the LDS of a CU at the residency wanted and not by a measured threshold.  rabbittclust_amd/api.py mirrors the
// constants (SCREEN_WAVE_CANDS, SCREEN_BLOCK_CANDS, SCREEN_POS_BYTES, SCREEN_MATCH_BYTES); tests/test_cpu_screen.py holds the two
// files together.
#ifndef RTC_SCREEN_H
#define RTC_SCREEN_H
#include <stdint.h>

// One wave, the candidates' remaining counts u in LDS.  A CU holds 32 waves and 160 KiB of LDS; a one-wave workgroup that keeps to
// 2 KiB of counts (and 8 bytes of reduction scratch) lets all 32 of them be resident in 65 KiB: 2048 / 4 = 512 candidates.
constexpr uint32_t SCREEN_WAVE_CANDS = 512;
// A 256-lane workgroup, u in LDS.  Eight workgroups a CU fill its 32 wave slots: 160 KiB / 8 = 20 KiB each, of which the counts
// take 16 KiB (4 096 candidates) and the reduction scratch 32 bytes.
constexpr uint32_t SCREEN_BLOCK_CANDS = 4096;
// beyond: a 256-lane workgroup with u where it lies in global memory

// The fill pass: a lane writes the records of a run of up to SCREEN_SHORT_RUN index entries itself, a longer run is written by
// the whole wave, 64 records a step.
constexpr uint32_t SCREEN_SHORT_RUN = 8;

// What a chunk is charged against RTC_SCREEN_BYTES.  A position is one hash of one sample of the chunk: its run in the index (8),
// its count (8), its offset (8), its sample (4), its cursor (4), its alive flag (1), rounded up.  A match record is one
// (sample hash, representative) pair: the unsorted and the sorted (key, position) copies (2 x 12), the run-head flag and the run
// number (2 x 4), the entry of the position view (4); per run start, eligibility and number (3 x 4) and per candidate slot,
// common, first record, u, rank and unique (6 x 4), both charged per match since there are at most as many.
constexpr uint64_t SCREEN_POS_BYTES = 40;
constexpr uint64_t SCREEN_MATCH_BYTES = 72;

#endif  // RTC_SCREEN_H
