// C hooks around pointcloud-slam_amd/csrc/loam_tiles.h (tile index, key and box of the localisation area tiles) for
// tests/test_loam_tiles.py.  Compiled with g++ alone: no HIP.
#include "loam_tiles.h"

extern "C" {

// 1 and *i = the index, or 0 when the coordinate has no tile
int lt_tile_index(float v, float tile_size, int32_t* i) { return pcm::loam::tile_index(v, tile_size, i) ? 1 : 0; }
uint32_t lt_tile_key(int32_t ix, int32_t iy) { return pcm::loam::tile_key(ix, iy); }
void lt_key_indices(uint32_t key, int32_t* ix, int32_t* iy) { *ix = pcm::loam::tile_key_ix(key); *iy = pcm::loam::tile_key_iy(key); }
// box4 = x_min, y_min, x_max, y_max
void lt_tile_box_xy(int32_t ix, int32_t iy, float tile_size, double* box4) { pcm::loam::tile_box_xy(ix, iy, tile_size, &box4[0], &box4[1], &box4[2], &box4[3]); }

}  // extern "C"
