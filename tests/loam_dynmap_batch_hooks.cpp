// loam_dynmap_batch_hooks.cpp -- the layout arithmetic of the crop (csrc/loam_dynmap.h: batch_layout, batch_context_of, crop_carve)
// and the table search (csrc/table_search.h) behind a C interface for tests/test_loam_tile_share.py and tests/test_loam_dynmap.py.
// Plain g++, no GPU.
#include <stdint.h>

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

// table_search.h: first[k * stride] is row k's first position
uint32_t dynmap_batch_hook_row_of(const uint32_t* first, uint32_t stride, uint32_t n, uint32_t g) { return pcm::table_row_of(first, stride, n, g); }

// crop_carve for n contexts of nb[i] workgroups and n_ent[i] entry rows, over a real 256-byte aligned block and over a null base.
// Stand-ins of the kernels' descriptor (120 bytes) and entry (16 bytes).  out: the offsets of desc, block0, ent, small, counts,
// chunk_tot, chunk_off from the base [0..6]; up_bytes, zero_bytes, bytes [7..9]; bytes over a null base [10]; whether every pointer
// of the null run is null [11]; sizeof desc and entry [12..13]; the layout's slots and chunks [14..15].  Returns 1, or 0 when the
// layout does not fit.
struct HookDesc { uint64_t w[15]; };
struct HookEntry { uint32_t w[4]; };
int dynmap_batch_hook_carve(const uint32_t* nb, int n, const uint32_t* n_ent, uint32_t small_words, uint64_t* out) {
  std::vector<BatchSlice> s((size_t)n);
  BatchLayout lay;
  if (!batch_layout(nb, n, s.data(), &lay)) return 0;
  size_t E = 0;
  for (int i = 0; i < n; i++) E += n_ent[i];
  const auto z = crop_carve<HookDesc, HookEntry>(nullptr, (size_t)n, E, small_words, lay);
  std::vector<char> mem(z.bytes + 256);
  char* base = mem.data() + (256 - (uintptr_t)mem.data() % 256) % 256;
  const auto c = crop_carve<HookDesc, HookEntry>(base, (size_t)n, E, small_words, lay);
  const char* at[7] = {(const char*)c.desc, (const char*)c.block0, (const char*)c.ent, (const char*)c.small, (const char*)c.counts,
                       (const char*)c.chunk_tot, (const char*)c.chunk_off};
  for (int k = 0; k < 7; k++) out[k] = (uint64_t)(at[k] - base);
  out[7] = c.up_bytes; out[8] = c.zero_bytes; out[9] = c.bytes; out[10] = z.bytes;
  out[11] = !z.desc && !z.block0 && !z.ent && !z.small && !z.counts && !z.chunk_tot && !z.chunk_off && z.up_bytes == c.up_bytes && z.zero_bytes == c.zero_bytes;
  out[12] = sizeof(HookDesc); out[13] = sizeof(HookEntry); out[14] = lay.slots; out[15] = lay.chunks;
  return 1;
}

}  // extern "C"
