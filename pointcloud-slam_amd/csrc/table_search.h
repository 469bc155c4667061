// table_search.h -- the one search of the kernels that walk a concatenation: which row of an ascending first-position table holds
// position g.  The crop's and the submap's entry tables (loam_dynmap.hip, loam_submap.hip), a batch's block prefix (loam_dynmap.h),
// the tile builder's distinct keys (loam_tiles.hip) and the occupancy map's scan offsets (occ_map.hip) all ask it.  Plain C++ for
// g++ as well (tests/loam_dynmap_batch_hooks.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PCM_TS_HD __host__ __device__
#else
#define PCM_TS_HD
#endif

namespace pcm {

// first: the first-position field of row 0 of a table of n >= 1 rows that lie `stride` 32-bit words apart; the positions ascend and
// neighbours may be equal (an empty row shares its position with its successor).  Returns the last row whose first position is <= g,
// so an empty row is never the answer for a position its successor holds; row 0 when g lies before the table.  The trip count
// depends on n alone: lanes with one n stay together, whatever their g.
PCM_TS_HD inline uint32_t table_row_of(const uint32_t* first, uint32_t stride, uint32_t n, uint32_t g) {
  uint32_t lo = 0, hi = n;   // first[lo] <= g < first[hi] (first[n] taken as infinite) once first[0] <= g
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (first[(size_t)mid * stride] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace pcm
