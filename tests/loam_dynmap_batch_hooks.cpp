// loam_dynmap_batch_hooks.cpp -- the layout arithmetic of a batched crop (csrc/loam_dynmap.h: batch_layout, batch_context_of) behind
// a C interface for tests/test_loam_tile_share.py.  Plain g++, no GPU.
#include <vector>

#include "loam_dynmap.h"

using namespace pcm::loam;

extern "C" {

int dynmap_batch_hook_block() { return (int)kDmBlock; }
int dynmap_batch_hook_chunk() { return (int)kDmChunk; }

// slices: n rows of (block0, slot0, chunk0, nchunks); totals: blocks, slots, chunks.  Returns 1, or 0 when the layout does not fit.
int dynmap_batch_hook_layout(const uint32_t* nb, int n, uint32_t* slices, uint32_t* totals) {
  std::vector<BatchSlice> s((size_t)n);
  BatchLayout lay;
  if (!batch_layout(nb, n, s.data(), &lay)) return 0;
  for (int i = 0; i < n; i++) {
    slices[4 * i] = s[(size_t)i].block0; slices[4 * i + 1] = s[(size_t)i].slot0;
    slices[4 * i + 2] = s[(size_t)i].chunk0; slices[4 * i + 3] = s[(size_t)i].nchunks;
  }
  totals[0] = lay.blocks; totals[1] = lay.slots; totals[2] = lay.chunks;
  return 1;
}

uint32_t dynmap_batch_hook_context_of(const uint32_t* block0, uint32_t n, uint32_t b) { return batch_context_of(block0, n, b); }

}  // extern "C"
