// loam_dynmap.h -- the host logic of jueying_slam's localisation map (include/dynamic_map.h, localization.cpp:229-315,
// new_localization.cpp:454-514): which area tiles are loaded around a pose (is_in_area / create_pcd), when they are reloaded
// (dynamic_load_map_run) and the window that dynamic_load_map's pcl::PassThrough filters cut out of them on every frame.  Plain
// C++17: the API layer (loam_dynmap.hip) runs it on the host, tests/test_loam_dynmap.py compiles it with g++ and checks it against
// the numpy restatement (tests/loam_dynmap_ref.py).  Every float operation below is one IEEE operation in the order written
// (-ffp-contract=off).
//
// Pinned where the reference tree cannot pin it (pcl::PassThrough is not in it):
//   * setFilterLimits takes floats: a limit is the double expression pose -/+ max_range * 1.1 rounded once to float;
//   * a point passes iff lo <= v && v <= hi in float (both ends inclusive, a NaN never passes);
//   * a point with any non-finite coordinate is dropped whatever the window says (deviation: PassThrough reads one field).
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

#include "arena_carver.h"
#include "table_search.h"
#include "target_share.h"

#if defined(__HIPCC__)
#define PCM_DM_HD __host__ __device__
#else
#define PCM_DM_HD
#endif

namespace pcm {
namespace loam {

// dynamic_map.h:16-25 without the path
struct Area {
  double x_min, y_min, z_min, x_max, y_max, z_max;
};

// dynamic_map.h:114-117: inclusive, in double, z never tested
inline bool is_in_area(double x, double y, const Area& area, double m) {
  return ((area.x_min - m) <= x && x <= (area.x_max + m) && (area.y_min - m) <= y && y <= (area.y_max + m));
}

// create_pcd (dynamic_map.h:129-156): the areas of one list that hold (p_x, p_y) with the margin, in list order; the position
// and the margin arrive as floats (const float&, float margin) and are promoted by the call.  margin < 0: every area
// (localization.cpp:229-242 loads the whole list once).
inline std::vector<int32_t> select_areas(const Area* areas, int n, float p_x, float p_y, float margin) {
  std::vector<int32_t> sel;
  for (int i = 0; i < n; i++)
    if (margin < 0.f || is_in_area(p_x, p_y, areas[i], margin)) sel.push_back((int32_t)i);
  return sel;
}

// last_loadMap before the first load (localization.cpp:249)
constexpr float kNeverLoaded = -999999.0f;

// dynamic_load_map_run (localization.cpp:295-300): float differences of pose[3..5], the float sum of their squares left to right,
// a float square root, compared with the int area_size converted to float
inline bool need_load(const float pose[6], const float last_load[6], int32_t area_size) {
  const float distance_x = pose[3] - last_load[3];
  const float distance_y = pose[4] - last_load[4];
  const float distance_z = pose[5] - last_load[5];
  const float load_distance = sqrtf(distance_x * distance_x + distance_y * distance_y + distance_z * distance_z);
  return load_distance > (float)area_size;
}

// pass.setFilterLimits(pose - max_range * 1.1, pose + max_range * 1.1) (localization.cpp:261,269): float - float * double
inline void crop_limits(float pose_v, float max_range, float* lo, float* hi) {
  *lo = (float)((double)pose_v - (double)max_range * 1.1);
  *hi = (float)((double)pose_v + (double)max_range * 1.1);
}

struct CropWindow {
  float x_lo, x_hi, y_lo, y_hi;
  int32_t crop_x;   // 0: the y window alone (what localization.cpp:259-273 computes), 1: x and y
};

// the window of one frame; margin < 0: dynamic_load_map does nothing, the whole map is the target (infinite limits)
inline CropWindow crop_window(const float pose[6], float max_range, int32_t margin, int32_t crop_x) {
  CropWindow w;
  if (margin < 0) {
    w.x_lo = w.y_lo = -INFINITY;
    w.x_hi = w.y_hi = INFINITY;
  } else {
    crop_limits(pose[3], max_range, &w.x_lo, &w.x_hi);
    crop_limits(pose[4], max_range, &w.y_lo, &w.y_hi);
  }
  w.crop_x = crop_x ? 1 : 0;
  return w;
}

PCM_DM_HD inline bool dm_finite(float v) {
  union { float f; uint32_t u; } b;
  b.f = v;
  return (b.u & 0x7f800000u) != 0x7f800000u;
}

// 1: kept, 0: outside the window, 2: dropped for a non-finite coordinate
PCM_DM_HD inline int crop_class(float x, float y, float z, const CropWindow& w) {
  if (!(dm_finite(x) && dm_finite(y) && dm_finite(z))) return 2;
  if (!(w.y_lo <= y && y <= w.y_hi)) return 0;
  if (w.crop_x && !(w.x_lo <= x && x <= w.x_hi)) return 0;
  return 1;
}

// ---- one tile store for several contexts -------------------------------------------------------------------
// What a context keeps of the localisation map for itself: the selection of its last load and whether its last crop still stands.
// Each robot has its own pose, so this is never shared.
struct TileSelection {
  bool loaded = false;
  std::vector<int32_t> sel[2];
  uint64_t sel_gen = 0;
  float last_load[6] = {kNeverLoaded, kNeverLoaded, kNeverLoaded, kNeverLoaded, kNeverLoaded, kNeverLoaded};
  bool last_valid = false;   // the record of the last crop is current
  // back to "never loaded"; the generation moves on, so a crop record of the old selection can never match again
  void reset() {
    sel[0].clear(); sel[1].clear();
    loaded = false;
    sel_gen++;
    last_valid = false;
    for (int k = 0; k < 6; k++) last_load[k] = kNeverLoaded;
  }
};

// A context's reference to a tile store (the tile tables and the two arenas: Store) and its selection.  The rules are those of
// target_share.h: a store with more than one holder is immutable (writable() first), share_from / clear_or_detach / let_go change
// this holder alone, and the last holder to go runs the hook (device current, its stream drained) before the store is freed.
// tests/tile_share_check.cpp walks through them on the host.
template <class Store>
struct TileHolder {
  SharedTarget<Store> ts;
  TileSelection s;
  TileHolder() { (void)ts.create(); }   // an empty reference after a failed allocation: ready() says so
  bool ready() { return !ts.empty() || ts.create(); }
  int holders() const { return ts.holders(); }
  bool writable() const { return ts.mutable_by_me(); }
  // pcm_loam_tile_share: lets go of the store it had and holds src's; the selection starts over (the caller has drained both streams)
  template <class Hook>
  void share_from(const TileHolder& src, Hook&& before_free) {
    if (!ts.same_as(src.ts)) ts.attach(src.ts, std::forward<Hook>(before_free));
    s.reset();
  }
  // pcm_loam_tile_clear: the sole holder empties its store (empty_store(Store&)), a sharer detaches and goes on with an empty store
  // of its own; false: out of host memory, nothing changed
  template <class Hook, class Empty>
  bool clear_or_detach(Hook&& before_free, Empty&& empty_store) {
    if (ts.shared()) {
      if (!ts.renew(std::forward<Hook>(before_free))) return false;
    } else {
      empty_store(*ts);
    }
    s.reset();
    return true;
  }
  template <class Hook>
  void let_go(Hook&& before_free) { ts.detach(std::forward<Hook>(before_free)); }
};

// ---- the layout of a crop (one context or a batch: loam_dynmap.hip) -----------------------------------------------------------------
constexpr uint32_t kDmBlock = 256;   // points per workgroup of k_dm_count_batch / k_dm_scatter_batch
constexpr uint32_t kDmChunk = 256;   // workgroup counts per scan block

// Context i of a batch runs nb[i] workgroups.  The workgroups of all contexts form one 1-D grid, context after context; every
// context owns a slice of the count array padded to whole scan blocks, so that the chunk scan runs over the concatenation and no scan
// block straddles two contexts.  A context without workgroups owns no slot and no chunk.
struct BatchSlice {
  uint32_t block0;   // its first workgroup in the grid
  uint32_t slot0;    // its first count slot (= chunk0 * kDmChunk)
  uint32_t chunk0;   // its first scan block
  uint32_t nchunks;  // ceil(nb / kDmChunk)
};
struct BatchLayout {
  uint32_t blocks = 0, slots = 0, chunks = 0;
};
// false: the grid or the count array does not fit 31 bits (a 1-D grid holds 2^31 - 1 workgroups)
inline bool batch_layout(const uint32_t* nb, int n, BatchSlice* out, BatchLayout* total) {
  uint64_t blocks = 0, chunks = 0;
  for (int i = 0; i < n; i++) {
    const uint64_t c = ((uint64_t)nb[i] + kDmChunk - 1) / kDmChunk;
    if (blocks > 0x7fffffffull || chunks * kDmChunk > 0x7fffffffull) return false;
    out[i] = BatchSlice{(uint32_t)blocks, (uint32_t)(chunks * kDmChunk), (uint32_t)chunks, (uint32_t)c};
    blocks += nb[i];
    chunks += c;
  }
  if (blocks > 0x7fffffffull || chunks * kDmChunk > 0x7fffffffull) return false;
  total->blocks = (uint32_t)blocks; total->slots = (uint32_t)(chunks * kDmChunk); total->chunks = (uint32_t)chunks;
  return true;
}
// workgroup b of the grid -> its context: the last i with block0[i] <= b (block0: n ascending first workgroups, n >= 1, b below
// the grid size).  A context without workgroups shares its block0 with the next one and is never the last.  The trip count depends
// on n alone, and b is the same in every lane of a workgroup, so the result is uniform.
PCM_DM_HD inline uint32_t batch_context_of(const uint32_t* block0, uint32_t n, uint32_t b) { return table_row_of(block0, 1u, n, b); }

// The workspace of a crop of m contexts with E entry-table rows in all: [descriptors | block prefix | entry tables] is the upload
// range, filled by one copy from a pinned block carved the same way; [counters | count slices] is the zero range, cleared by one
// memset (the padding of a count slice must scan as zeros); then the scan-block totals and offsets.  Run over a null base it is the
// size query (bytes), run over the device or the pinned block the carve.  Desc and Entry are the kernels' types (loam_dynmap.hip).
template <class Desc, class Entry>
struct CropCarve {
  Desc* desc;            // [m]
  uint32_t* block0;      // [m]
  Entry* ent;            // [E]
  uint32_t* small;       // [m][small_words]
  uint32_t* counts;      // [lay.slots]
  uint32_t* chunk_tot;   // [lay.chunks]
  uint32_t* chunk_off;   // [lay.chunks]
  size_t up_bytes;       // the upload range, from desc
  size_t zero_bytes;     // the zero range, from small
  size_t bytes;          // everything
};
template <class Desc, class Entry>
inline CropCarve<Desc, Entry> crop_carve(void* base, size_t m, size_t E, size_t small_words, const BatchLayout& lay) {
  ArenaCarver a(base);
  CropCarve<Desc, Entry> c;
  c.desc = a.take<Desc>(m);
  c.block0 = a.take<uint32_t>(m);
  c.ent = a.take<Entry>(E);
  c.up_bytes = a.used();
  c.small = a.take<uint32_t>(small_words * m);
  c.counts = a.take<uint32_t>(lay.slots);
  c.zero_bytes = a.used() - c.up_bytes;
  c.chunk_tot = a.take<uint32_t>(lay.chunks);
  c.chunk_off = a.take<uint32_t>(lay.chunks);
  c.bytes = a.used();
  return c;
}

}  // namespace loam
}  // namespace pcm
