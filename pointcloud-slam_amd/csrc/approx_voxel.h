// approx_voxel.h -- pcl::ApproximateVoxelGrid (pcl/filters/impl/approximate_voxel_grid.hpp), the rules stated once for the device
// and the host.  The filter is a serial loop over the input: point cp has the voxel (ix, iy, iz) = floor(p * inverse_leaf) and the
// history entry h = (ix * 7171 + iy * 3079 + iz * 4231) & 511; an entry that holds another voxel is flushed (its mean is the next
// output) before the point joins it, and after the last point every entry in use is flushed in increasing h.  The output depends on
// the input order, and a voxel whose points are separated by a colliding voxel comes out more than once.
//
// Without the loop: a "run" is a maximal sequence of points that follow one another within one entry h and share the voxel.  Each
// run is one output.  A run that is not the last of its entry leaves when the head point of the next run of that entry arrives, so
// these runs are ordered by that head point's input index; the last runs of the entries follow in increasing h.  With
//   mark[i]  = point i heads a run that is not the first of its entry            (input order)
//   before[i] = marks in front of i                                               (exclusive scan)
// the run in front of the run headed by i has output slot before[i], and the last run of entry h has slot (all marks) + (rank of h
// among the entries in use): run_slot below.  Nothing is decided by an atomic, so a result does not depend on the schedule.
//
// Everything here compiles with a host compiler alone (tests/approx_voxel_hooks.cpp), no HIP header is read then: the key of a
// point, the head test, the slot rule, the serial form of the pipeline (emit_slots_host, what the kernels of approx_voxel.hip do
// lane-parallel) and the layout of the scratch.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "arena_carver.h"

#if defined(__HIPCC__)
#define PCM_AV_HD __host__ __device__
#else
#define PCM_AV_HD
#endif

namespace pcm {
namespace av {

constexpr uint32_t kEntries = 512u;       // history entries
constexpr uint32_t kNoEntry = kEntries;   // sort key of a dropped point: behind every entry
constexpr int kKeyBits = 10;              // bits of the sort key
constexpr uint32_t kNoSlot = 0xffffffffu;

struct Key { int32_t ix, iy, iz; uint32_t h; bool valid; };

// floor(v * inv) as an int; false for a non-finite v and for |floor| >= 2^31 (the cast is undefined in PCL; such a point is dropped)
PCM_AV_HD inline bool axis_index(float v, float inv, int32_t* i) {
  uint32_t bits;
  __builtin_memcpy(&bits, &v, 4);
  if ((bits & 0x7f800000u) == 0x7f800000u) return false;
  const float f = ::floorf(v * inv);
  if (!(::fabsf(f) < 2147483648.0f)) return false;
  *i = (int32_t)f;
  return true;
}

// 32-bit wrapping arithmetic: the two's-complement reading of PCL's int expression
PCM_AV_HD inline uint32_t entry_of(int32_t ix, int32_t iy, int32_t iz) {
  return ((uint32_t)ix * 7171u + (uint32_t)iy * 3079u + (uint32_t)iz * 4231u) & (kEntries - 1u);
}

// inv = 1.0f / leaf, formed once by the caller
PCM_AV_HD inline Key key_of(float x, float y, float z, float inv) {
  Key k{0, 0, 0, kNoEntry, false};
  if (!(axis_index(x, inv, &k.ix) && axis_index(y, inv, &k.iy) && axis_index(z, inv, &k.iz))) return Key{0, 0, 0, kNoEntry, false};
  k.h = entry_of(k.ix, k.iy, k.iz);
  k.valid = true;
  return k;
}

PCM_AV_HD inline bool same_voxel(const Key& a, const Key& b) { return a.ix == b.ix && a.iy == b.iy && a.iz == b.iz; }

// the output slot of a run.  next_in_entry: another run of the same entry follows it; marks_before_next_head: before[] of that
// run's head point; else the run is the last of its entry, which is the entry_rank-th entry in use.
PCM_AV_HD inline uint32_t run_slot(bool next_in_entry, uint32_t marks_before_next_head, uint32_t total_marks, uint32_t entry_rank) {
  return next_in_entry ? marks_before_next_head : total_marks + entry_rank;
}

// The pipeline of approx_voxel.hip in serial form: keys -> stable partition by entry -> heads -> marks in input order -> scan ->
// slots.  slot_of_point[i] = output slot of the run point i belongs to (kNoSlot: dropped).  Returns the number of outputs.
inline uint32_t emit_slots_host(const Key* k, uint32_t n, uint32_t* slot_of_point, uint32_t* n_dropped) {
  std::vector<uint32_t> start(kEntries + 2, 0u), order(n);
  for (uint32_t i = 0; i < n; i++) start[(k[i].valid ? k[i].h : kNoEntry) + 1]++;
  for (uint32_t h = 0; h <= kEntries; h++) start[h + 1] += start[h];
  {
    std::vector<uint32_t> at(start.begin(), start.end() - 1);
    for (uint32_t i = 0; i < n; i++) order[at[k[i].valid ? k[i].h : kNoEntry]++] = i;   // stable
  }
  const uint32_t nvalid = start[kEntries];
  std::vector<uint32_t> head(nvalid, 0u), mark(n, 0u), before(n, 0u), rank(kEntries, 0u);
  for (uint32_t j = 0; j < nvalid; j++) {
    const Key& me = k[order[j]];
    const bool first = j == 0 || k[order[j - 1]].h != me.h;
    head[j] = (first || !same_voxel(k[order[j - 1]], me)) ? 1u : 0u;
    mark[order[j]] = (head[j] && !first) ? 1u : 0u;
  }
  uint32_t total_marks = 0, in_use = 0;
  for (uint32_t i = 0; i < n; i++) { before[i] = total_marks; total_marks += mark[i]; }
  for (uint32_t h = 0; h < kEntries; h++) { rank[h] = in_use; in_use += start[h + 1] > start[h] ? 1u : 0u; }
  for (uint32_t i = 0; i < n; i++) slot_of_point[i] = kNoSlot;
  uint32_t runs = 0;
  for (uint32_t b = 0; b < nvalid;) {
    uint32_t e = b + 1;
    while (e < nvalid && !head[e]) e++;
    const uint32_t h = k[order[b]].h;
    const bool next_in_entry = e < nvalid && k[order[e]].h == h;
    const uint32_t slot = run_slot(next_in_entry, next_in_entry ? before[order[e]] : 0u, total_marks, rank[h]);
    for (uint32_t j = b; j < e; j++) slot_of_point[order[j]] = slot;
    runs++;
    b = e;
  }
  if (n_dropped) *n_dropped = n - nvalid;
  return runs;   // == total_marks + in_use
}

// the arrays of one call over n points
struct Work {
  uint32_t *keys, *keys_s;      // [n] entry of a point (kNoEntry: dropped), input and sorted order
  uint32_t *vals, *vals_s;      // [n] input index
  uint32_t *head, *run;         // [n] sorted order: 1 where a run begins; runs in front (exclusive scan)
  uint32_t *mark, *before;      // [n] input order: the marks and their exclusive scan
  uint32_t* pos;                // [n] first sorted element of every run
  uint32_t *in_use, *rank;      // [kEntries] 1: the entry holds a point; entries in use in front of it
  uint32_t* small;              // [0] runs, [1] valid points, [2] marks, [3] entries in use, [4..8) free
  void* sort_tmp; size_t sort_tmp_bytes; void* scan_tmp; size_t scan_tmp_bytes;   // rocPRIM temporaries
  static constexpr int kSmallWords = 8;
};
inline Work work_carve(ArenaCarver& a, size_t n, size_t sort_tmp_bytes, size_t scan_tmp_bytes) {
  Work W{};
  W.keys = a.take<uint32_t>(n); W.keys_s = a.take<uint32_t>(n);
  W.vals = a.take<uint32_t>(n); W.vals_s = a.take<uint32_t>(n);
  W.head = a.take<uint32_t>(n); W.run = a.take<uint32_t>(n);
  W.mark = a.take<uint32_t>(n); W.before = a.take<uint32_t>(n);
  W.pos = a.take<uint32_t>(n);
  W.in_use = a.take<uint32_t>(kEntries); W.rank = a.take<uint32_t>(kEntries);
  W.small = a.take<uint32_t>(Work::kSmallWords);
  W.sort_tmp_bytes = sort_tmp_bytes; W.scan_tmp_bytes = scan_tmp_bytes;
  W.sort_tmp = a.take<char>(sort_tmp_bytes); W.scan_tmp = a.take<char>(scan_tmp_bytes);
  return W;
}

}  // namespace av
}  // namespace pcm
