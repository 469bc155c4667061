// list_pool_check.cpp -- drives csrc/list_pool.h (the pool of following candidate lists) with random sequences of growth, shrinkage
// and eviction against a brute-force model that keeps every run: no two live runs overlap, starts are whole trips, the bump
// pointer and the tail stay inside the capacity, the counters add up, and a full build is asked for exactly at the three
// thresholds.  Host code with its own main (tests/test_list_pool.py builds it plain and with -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../pointcloud-slam_amd/csrc/list_pool.h"

using namespace pcm::list_pool;

struct Run { uint64_t start; uint32_t len, cap; };

static int fail(const char* what, int seq, int step) {
  std::printf("FAIL %s (sequence %d, step %d)\n", what, seq, step);
  return 1;
}

// a full build: the runs one after the other, capacity = length
static void build(std::vector<Run>& runs, const std::vector<uint32_t>& cand, Pool& pool, float frac, uint64_t min_entries, bool by_policy) {
  runs.clear();
  uint64_t at = 0, empty = 0;
  for (uint32_t n : cand) {
    if (n == 0) { empty++; continue; }   // a full build makes no empty list
    const uint32_t p = padded_length(n);
    runs.push_back({at, p, p});
    at += p;
  }
  (void)empty;
  pool.built(Pool::capacity_for(at, frac, min_entries), at, runs.size(), 0, by_policy);
}

static int check(const std::vector<Run>& runs, const Pool& pool, int seq, int step) {
  std::vector<unsigned char> used((size_t)pool.capacity, 0);
  uint64_t live = 0, reserved = 0, empty = 0;
  for (const Run& r : runs) {
    if (r.start % kTrip || r.len % kTrip || r.len > r.cap) return fail("run not on whole trips or longer than its capacity", seq, step);
    if (r.start + r.cap > pool.bump) return fail("run beyond the bump pointer", seq, step);
    for (uint64_t k = r.start; k < r.start + r.cap; k++) {
      if (used[(size_t)k]) return fail("two live runs overlap", seq, step);
      used[(size_t)k] = 1;
    }
    live += r.len; reserved += r.cap; empty += r.len == 0;
  }
  if (pool.bump + Pool::tail() > pool.capacity) return fail("bump pointer + tail outside the capacity", seq, step);
  if (pool.live != live || pool.reserved != reserved || pool.empty != empty || pool.lists != runs.size()) return fail("counters do not match the runs", seq, step);
  if (pool.bump != pool.reserved + pool.wasted) return fail("bump != reserved + wasted", seq, step);
  return 0;
}

int main() {
  std::mt19937 rng(12345);
  // the per-run functions
  for (uint32_t n = 0; n < 5000; n++) {
    const uint32_t p = padded_length(n), g = grown_capacity(p);
    if (p < n || p >= n + kTrip || p % kTrip) return fail("padded_length", 0, (int)n);
    if (g < p || g % kTrip || (p == 0) != (g == 0)) return fail("grown_capacity", 0, (int)n);
    if (!rewrite_in_place(p, g) || (p && rewrite_in_place(p, p - 1))) return fail("rewrite_in_place", 0, (int)n);
  }
  long rebuilds_seen[4] = {0, 0, 0, 0}, in_place = 0, relocated = 0;
  for (int seq = 0; seq < 300; seq++) {
    const float frac = (seq % 3) * 0.25f;
    const uint64_t min_entries = (seq % 5) * 64;
    std::vector<uint32_t> cand(20 + rng() % 200);   // candidates per list
    for (uint32_t& n : cand) n = 1 + rng() % 60;
    std::vector<Run> runs;
    Pool pool;
    build(runs, cand, pool, frac, min_entries, false);
    if (check(runs, pool, seq, -1)) return 1;
    const int mode = seq % 4;   // 0 growth, 1 growth and shrinkage, 2 eviction-heavy, 3 new lists
    for (int step = 0; step < 60 && !runs.empty(); step++) {
      // one update: some dirty lists with new candidate counts, perhaps new lists
      std::vector<std::pair<size_t, uint32_t>> dirty;
      std::vector<unsigned char> taken(runs.size(), 0);
      const size_t nd = 1 + rng() % (runs.size() / 2 + 1);
      for (size_t k = 0; k < nd; k++) {
        const size_t i = rng() % runs.size();
        if (taken[i]) continue;
        taken[i] = 1;
        const uint32_t old = runs[i].len;
        uint32_t n = old + rng() % 24;
        if (mode == 1 && rng() % 2) n = old > 8 ? old - rng() % 8 : old;
        if (mode == 2 && rng() % 3) n = rng() % 4 ? 0 : old / 2;
        dirty.push_back({i, n});
      }
      const size_t n_new = mode == 3 ? rng() % 6 : 0;
      // the totals, as k_fl_classify sums them
      Totals t;
      uint64_t model_wasted = pool.wasted, model_live = pool.live, model_empty = pool.empty;
      for (auto& d : dirty) {
        const Run& r = runs[d.first];
        const uint32_t p = padded_length(d.second);
        t.dirty++;
        if (rewrite_in_place(p, r.cap)) t.in_place++;
        else { t.relocated++; t.wasted_added += r.cap; t.reloc_entries += grown_capacity(p); model_wasted += r.cap; }
        t.live_added += p; t.live_removed += r.len;
        model_live = model_live + p - r.len;
        if (p == 0 && r.len != 0) { t.became_empty++; model_empty++; }
        if (p != 0 && r.len == 0) { t.left_empty++; model_empty--; }
      }
      std::vector<uint32_t> fresh(n_new);
      for (uint32_t& n : fresh) {
        n = 1 + rng() % 40;
        const uint32_t p = padded_length(n);
        t.dirty++; t.new_lists++; t.reloc_entries += grown_capacity(p); t.live_added += p;
        model_live += p;
      }
      // the three thresholds, worked out apart from Pool::decide
      Decision want = kApply;
      if (pool.bump + t.reloc_entries + Pool::tail() > pool.capacity) want = kRebuildNoRoom;
      else if (model_wasted > model_live) want = kRebuildWasted;
      else if (2 * model_empty > runs.size() + n_new) want = kRebuildEmpty;
      const Decision got = pool.decide(t);
      if (got != want) return fail("a rebuild is not asked for exactly at the thresholds", seq, step);
      rebuilds_seen[got]++;
      if (got != kApply) {   // the full build of the lists as the update would have left them
        std::vector<uint32_t> all;
        for (size_t i = 0; i < runs.size(); i++) all.push_back(runs[i].len);
        for (auto& d : dirty) all[d.first] = d.second;
        for (uint32_t n : fresh) all.push_back(n);
        const uint64_t before = pool.rebuilds;
        build(runs, all, pool, frac, min_entries, true);
        if (pool.rebuilds != before + 1 || pool.updates != 0 || pool.wasted != 0) return fail("counters after a rebuild", seq, step);
      } else {
        uint64_t at = pool.bump;
        for (auto& d : dirty) {
          Run& r = runs[d.first];
          const uint32_t p = padded_length(d.second);
          if (rewrite_in_place(p, r.cap)) { r.len = p; in_place++; }
          else { r.start = at; r.len = p; r.cap = grown_capacity(p); at += r.cap; relocated++; }
        }
        for (uint32_t n : fresh) {
          const uint32_t p = padded_length(n);
          runs.push_back({at, p, grown_capacity(p)});
          at += grown_capacity(p);
        }
        const uint64_t updates = pool.updates;
        pool.apply(t);
        if (pool.bump != at || pool.updates != updates + 1) return fail("bump pointer or update count after an update", seq, step);
      }
      if (check(runs, pool, seq, step)) return 1;
    }
  }
  if (!rebuilds_seen[kRebuildNoRoom] || !rebuilds_seen[kRebuildWasted] || !rebuilds_seen[kRebuildEmpty] || !rebuilds_seen[kApply] || !in_place || !relocated) {
    std::printf("FAIL a path was never taken: apply %ld, no room %ld, wasted %ld, empty %ld, in place %ld, relocated %ld\n", rebuilds_seen[0], rebuilds_seen[1], rebuilds_seen[2], rebuilds_seen[3],
                in_place, relocated);
    return 1;
  }
  std::printf("ok: apply %ld, no room %ld, wasted %ld, empty %ld, in place %ld, relocated %ld\n", rebuilds_seen[0], rebuilds_seen[1], rebuilds_seen[2], rebuilds_seen[3], in_place, relocated);
  return 0;
}
