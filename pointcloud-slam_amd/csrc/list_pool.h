// list_pool.h -- the pool that holds the candidate runs of following lists (PCM_FLAG_FOLLOWING_LISTS, neighbour_lists.hip): what
// becomes of one run when its list is rewritten (in place, or moved to the pool's bump pointer), the pool's counters, and when an
// update gives way to a full build.  Plain C++ without a HIP call, so the CPU suite drives it (tests/list_pool_check.cpp); the
// update's kernels use the per-run functions, its host side the Pool.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCM_LIST_POOL_HD __host__ __device__
#else
#define PCM_LIST_POOL_HD
#endif

namespace pcm {
namespace list_pool {

constexpr uint32_t kTrip = 4;        // entries per trip of the walk (kListTrip): runs start and end on whole trips
constexpr uint32_t kTailTrips = 1;   // zeroed trips behind the pool's end (kWalkAhead)
constexpr uint32_t kGrowTo = 16;     // a relocated run's capacity: one and a half times its padded length, rounded up to this many entries
// The space a full build reserves behind its runs: the larger of one and a half times their entries and 64 Ki entries (1 MiB); set
// per target by pcm_neighbour_list_headroom.  The first batch into a fresh build moves every run it touches (capacity = length),
// each to one and a half times its length: a batch that touches most of a small map needs about that much.  It is a minimum: the
// allocation is grow-only and grows by a quarter more than asked, as the arrays of a TargetMap do, and the pool uses all of it.
constexpr float kDefaultHeadroomFraction = 1.5f;
constexpr uint64_t kDefaultHeadroomMin = 65536;

// candidates -> entries of the run: whole trips, 0 stays 0
PCM_LIST_POOL_HD inline uint32_t padded_length(uint32_t n) { return (n + (kTrip - 1u)) & ~(kTrip - 1u); }
// the capacity a run gets when it is placed at the bump pointer: half its length as slack (a run that keeps growing moves a
// logarithmic number of times, the next batches rewrite it in place), a multiple of kGrowTo; 0 stays 0.  padded < 2^31.
PCM_LIST_POOL_HD inline uint32_t grown_capacity(uint32_t padded) { return (padded + padded / 2u + (kGrowTo - 1u)) & ~(kGrowTo - 1u); }
// a run of `padded` entries stays where it is when its capacity holds it (a new list has capacity 0: only an empty one "fits")
PCM_LIST_POOL_HD inline bool rewrite_in_place(uint32_t padded, uint32_t capacity) { return padded <= capacity; }

// What one update does to the pool, summed over its dirty lists on the device and read back once.
struct Totals {
  // 64-bit sums: a run at the bump pointer takes one and a half times its length, so the entries a large batch into dense voxels
  // relocates can pass 2^32 although every run and the pool itself stay below it -- decide() must see that they do not fit
  uint64_t dirty = 0;           // lists rewritten
  uint64_t new_lists = 0;       // of them: list voxels the index did not hold
  uint64_t reloc_entries = 0;   // capacity taken at the bump pointer (relocated runs and the runs of new lists)
  uint64_t relocated = 0;       // existing runs moved
  uint64_t in_place = 0;        // existing runs rewritten where they were
  uint64_t wasted_added = 0;    // capacity of the runs left behind
  uint64_t live_added = 0, live_removed = 0;   // padded lengths: the new ones, the ones they replace
  uint64_t became_empty = 0, left_empty = 0;   // lists whose length went to 0 (new empty lists included) / away from 0
};

enum Decision { kApply = 0, kRebuildNoRoom = 1, kRebuildWasted = 2, kRebuildEmpty = 3 };

struct Pool {
  uint64_t capacity = 0;   // entries of the allocation, the tail included
  uint64_t bump = 0;       // first free entry
  uint64_t live = 0;       // sum of the runs' padded lengths
  uint64_t reserved = 0;   // sum of the runs' capacities; bump == reserved + wasted
  uint64_t wasted = 0;     // holes left by relocated runs
  uint64_t lists = 0, empty = 0;
  uint64_t updates = 0;    // since the last full build
  uint64_t in_place = 0, relocated = 0, rebuilds = 0;   // since the lists were first built

  static uint64_t tail() { return (uint64_t)kTrip * kTailTrips; }
  // entries to allocate for a build of `total` entries
  static uint64_t capacity_for(uint64_t total, float fraction, uint64_t min_entries) {
    const double f = fraction > 0.f ? (double)fraction : 0.0;
    uint64_t room = (uint64_t)(f * (double)total);
    if (room < min_entries) room = min_entries;
    room = (room + (kTrip - 1u)) & ~(uint64_t)(kTrip - 1u);
    return total + room + tail();
  }
  // a full build laid `total` entries out contiguously, capacity = length for every run
  void built(uint64_t allocation, uint64_t total, uint64_t n_lists, uint64_t n_empty, bool by_policy) {
    capacity = allocation; bump = total; live = total; reserved = total; wasted = 0; lists = n_lists; empty = n_empty; updates = 0;
    if (by_policy) rebuilds++;
  }
  // the three reasons for a full build in place of the update, looked at in this order, on the counters as the update would leave them
  Decision decide(const Totals& t) const {
    if (bump + t.reloc_entries + tail() > capacity) return kRebuildNoRoom;
    const uint64_t w = wasted + t.wasted_added, l = live + t.live_added - t.live_removed;
    if (w > l) return kRebuildWasted;
    const uint64_t e = empty + t.became_empty - t.left_empty, n = lists + t.new_lists;
    if (2 * e > n) return kRebuildEmpty;
    return kApply;
  }
  void apply(const Totals& t) {
    bump += t.reloc_entries;
    wasted += t.wasted_added;
    reserved += t.reloc_entries; reserved -= t.wasted_added;
    live += t.live_added; live -= t.live_removed;
    lists += t.new_lists;
    empty += t.became_empty; empty -= t.left_empty;
    in_place += t.in_place; relocated += t.relocated;
    updates++;
  }
};

}  // namespace list_pool
}  // namespace pcm
