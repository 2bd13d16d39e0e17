// rtc_upgma.h -- the constants of rtc_upgma.hip (clust-mst --upgma; include/rtclust.h has the definition).
#pragma once
#include <stdint.h>

constexpr uint32_t UPGMA_Q1 = 1u << 20;          // distance 1 in the units of the sums
constexpr uint32_t UPGMA_W_MAX = 1u << 22;       // the sizes of one call sum to less than this: S < 2^62, a cross product < 2^106
constexpr uint32_t UPGMA_WAVE_MAX = 64;          // the wave path's largest m: S (64 x 65 cells) and the sizes in 32.75 KiB of LDS
constexpr uint32_t UPGMA_GRID_MIN = 128;         // the grid path's default first m (RTC_UPGMA_GRID_MIN; measured)
constexpr uint32_t UPGMA_SCAN_BLOCKS = 1024;     // the most workgroups of a scan launch: every merge workgroup reads their minima again
