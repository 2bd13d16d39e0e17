// rtc_support.h -- the constants of rtc_cluster_support (rtc_support.hip; DESIGN 3.4r has the reasons), mirrored by
// api.CSUPPORT_MAX / CSUPPORT_TABLE_MAX and held together by tests/test_cpu_support.py.
#ifndef RTC_SUPPORT_H
#define RTC_SUPPORT_H
#include <stdint.h>

constexpr uint32_t CSUP_MAX_REPLICATES = 256;    // a cap, not a measurement: four words of 64 replicates
constexpr uint64_t CSUP_TABLE_MAX = 1ull << 25;  // the keep table's most entries (128 MiB of uint32): a cap, not a measurement
// The candidates of a row chunk are counted in pieces of this many: a piece's counts are 256 bytes a candidate (64 uint32), so a
// piece takes 256 MiB, and the edges it keeps 20 bytes each per word held.
constexpr uint64_t CSUP_PIECE_EDGES = 1ull << 20;
// The mask kernel gives a wave 64 candidates: one append of the kept inner edges per wave, the records written side by side.
constexpr uint32_t CSUP_TILE = 64;

#endif  // RTC_SUPPORT_H
