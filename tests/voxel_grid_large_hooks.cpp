// C hooks around vg::split of pointcloud-slam_amd/csrc/voxel_grid.h (pcl::VoxelGridLarge's decision for a piece: leaf piece, cut
// with axis and mid, or stuck) for tests/test_voxel_grid_large.py.  Compiled with g++ alone: no HIP.  With -DVGL_MAIN the file is a
// program that replays cases from a text file (one per line: six box words and the leaf's bits, in hex) and prints the decisions --
// the form that is built with -fsanitize=address,undefined.
#include "voxel_grid.h"

#include <cstdio>
#include <cstring>

extern "C" {

// mm: 6 ordered-int words (min x y z, max x y z).  Returns vg::kPieceLeaf / kPieceSplit / kPieceStuck.
int vgl_split(const unsigned int* mm, float leaf, int* axis, float* mid) { return pcm::vg::split(mm, leaf, axis, mid); }

}  // extern "C"

#ifdef VGL_MAIN
int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  unsigned int w[7];
  long n = 0;
  while (std::fscanf(f, "%x %x %x %x %x %x %x", &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6]) == 7) {
    float leaf, mid;
    int axis;
    std::memcpy(&leaf, &w[6], 4);
    const int kind = vgl_split(w, leaf, &axis, &mid);
    unsigned int mid_bits;
    std::memcpy(&mid_bits, &mid, 4);
    long long b[6];
    const bool over = pcm::vg::box(w, leaf, b);   // a leaf piece is exactly a box that does not overflow
    std::printf("%d %d %08x %d\n", kind, axis, mid_bits, over ? 1 : 0);
    n++;
  }
  std::fclose(f);
  std::fprintf(stderr, "%ld cases\n", n);
  return 0;
}
#endif
