// loam_tiles.h -- the arithmetic of the localisation area tiles that device and host share (loam_tiles.hip; with a host compiler
// alone: tests/loam_tiles_hooks.cpp, no HIP header is read then).  A tile is a square of tile_size metres in x and y, open in z:
//   index   ix = (int32)floorf(x / tile_size), iy likewise -- a float division and an exact floor, so -0.0f lies in tile 0,
//           -1e-7f in tile -1 and a point exactly on k * tile_size in tile k.  |ix| or |iy| >= 32768 has no tile.
//   key     (iy + 32768) << 16 | (ix + 32768): both halves are in [1, 65535], so a key is never 0 (the key of a point without a
//           tile, which sorts in front of every tile) and ascending keys are ascending (iy, ix).
//   box     x_min = (double)ix * (double)tile_size, x_max = (double)(ix + 1) * (double)tile_size, the same for y: what
//           is_in_area (include/dynamic_map.h) selects by.  z_min / z_max are those of the tile's stored points.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PCM_TILES_HD __host__ __device__
#else
#define PCM_TILES_HD
#endif

namespace pcm {
namespace loam {

constexpr int32_t kTileIndexLimit = 32768;   // |ix|, |iy| < this
constexpr uint32_t kNoTileKey = 0u;

// the tile index of one coordinate; false: there is none (the coordinate is not finite, or the index is out of range)
PCM_TILES_HD inline bool tile_index(float v, float tile_size, int32_t* i) {
  const float f = ::floorf(v / tile_size);
  *i = 0;
  if (!(::fabsf(f) < (float)kTileIndexLimit)) return false;   // NaN and the infinities fail as well
  *i = (int32_t)f;
  return true;
}

PCM_TILES_HD inline uint32_t tile_key(int32_t ix, int32_t iy) { return ((uint32_t)(iy + kTileIndexLimit) << 16) | (uint32_t)(ix + kTileIndexLimit); }
PCM_TILES_HD inline int32_t tile_key_ix(uint32_t key) { return (int32_t)(key & 0xffffu) - kTileIndexLimit; }
PCM_TILES_HD inline int32_t tile_key_iy(uint32_t key) { return (int32_t)(key >> 16) - kTileIndexLimit; }

// x_min, y_min, x_max, y_max of a tile
inline void tile_box_xy(int32_t ix, int32_t iy, float tile_size, double* x_min, double* y_min, double* x_max, double* y_max) {
  const double t = (double)tile_size;
  *x_min = (double)ix * t; *x_max = (double)(ix + 1) * t;
  *y_min = (double)iy * t; *y_max = (double)(iy + 1) * t;
}

}  // namespace loam
}  // namespace pcm
