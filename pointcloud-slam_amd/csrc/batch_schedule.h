// batch_schedule.h -- the two round schedulers of the batch entry points as plain integer logic: which pairs a round launches
// (align_batch.hip align_batch_impl) and which lock-step group of a pclomp NDT batch may launch or stop (pclndt_align_batch).
// No HIP and no device here: the callers wait on the status bytes, launch and time; this header only decides.  It compiles
// with a host compiler alone (tests/batch_schedule_hooks.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pcm {

struct BatchPlan {
  int window;            // pairs that iterate at a time
  int per_pair_rounds;   // rounds one pair can ask for
  bool host_window;      // the window is kept by the host's launch list (no device-side hand-off)
  bool use_list;         // only listed pairs are launched (the list rides in the kernel arguments)
  int max_rounds;        // round budget of the batch
};

// max_listed_pairs: kMaxListedPairs of pcm_device.h (entries of KernelParams::active)
inline BatchPlan plan_batch(int n, int batch_window, int max_iterations, bool is_lm, int lm_max_iterations, int max_listed_pairs) {
  BatchPlan p;
  // worst case: every outer iteration = 1 linearize + lm_max_iterations trials
  // batch window: at most `window` pairs iterate at a time, a finished pair's slot goes to the next queued one on the
  // device (k_finish_round) -- the late rounds of a slow pair then overlap the early rounds of its successors
  p.window = (batch_window > 0 && max_iterations > 0) ? std::min(n, batch_window) : n;
  p.per_pair_rounds = std::max(1, max_iterations) * (is_lm ? 1 + std::max(1, lm_max_iterations) : 1);
  // Up to 256 pairs with a window of at most 64: the window is kept by the HOST.  Only the pairs of the launch list run; when the
  // status byte of a pair says "done" the next queued pair takes its place in the list (it was initialised with the others and
  // simply never launched before).  Every round then carries about `window` live pairs, so the fixed cost of a round (two launches,
  // their boundaries) is shared by that many registrations for the whole batch, not only in its first rounds.  No device-side hand-off.
  p.host_window = p.window < n && n <= 256 && p.window <= max_listed_pairs;
  // Only the pairs the host still believes active are launched (the list rides in the kernel arguments, batches of
  // <= max_listed_pairs pairs): an early-exit workgroup is not free, and the late rounds of a batch have one or two live pairs.
  // The list lags one round (the status bytes are read one round behind); a stale entry exits at once.
  p.use_list = (n <= max_listed_pairs && p.window == n) || p.host_window;
  // Round budget.  Host window: a slot serves its pairs one after the other, and every hand-over costs one extra round because the
  // status bytes are read one round behind; with every pair running to max_iterations a slot needs ceil(n / window) * (rounds + 1)
  // rounds, one more pair's worth covers an uneven hand-out (round-2 advisor finding: the old bound ran out for 256 pairs at a
  // window of 8 and 10 GN iterations and returned unfinished pairs as PCM_OK).  A pair the loop leaves unfinished is reported
  // with PCM_ERR_INTERNAL by k_pack_results, never silently.
  p.max_rounds = p.host_window ? ((n + p.window - 1) / p.window + 1) * (p.per_pair_rounds + 1) + 2
                               : p.per_pair_rounds * (n - p.window + 1) + 1 + 2 * (n - p.window);   // + the rounds a handed-over pair spends PENDING
  return p;
}

// The launch list of a batch, round by round.  Per round the caller launches current() (every pair when !use_list), waits until
// the status bytes of the PREVIOUS round's pairs (awaited) are non-zero -- the GPU then always has the next round queued -- and
// calls advance() with that round's row.  Status byte: 1 = still active, any other non-zero value = finished.
class LaunchList {
 public:
  LaunchList(int n, const BatchPlan& p) : n_(n), window_(p.window), host_window_(p.host_window), use_list_(p.use_list), act_((size_t)(p.host_window ? p.window : n)) {
    for (size_t i = 0; i < act_.size(); i++) act_[i] = (uint8_t)i;
    next_queued_ = host_window_ ? window_ : n_;
  }
  const std::vector<uint8_t>& current() const { return act_; }          // pairs of this round's grid (use_list only)
  int size() const { return use_list_ ? (int)act_.size() : n_; }        // pairs this round launches
  // pairs whose byte in the previous round's row advance() reads; none in the first round
  int num_awaited() const { return first_ ? 0 : (use_list_ ? (int)prev_list_.size() : n_); }
  int awaited(int k) const { return use_list_ ? (int)prev_list_[(size_t)k] : k; }
  // After this round's launch.  `row`: status bytes [pair] of the previous round (not read in the first round).  Computes the next
  // round's list; false: no pair is active any more.
  bool advance(const volatile unsigned char* row) {
    std::vector<uint8_t> this_list = act_;   // pairs launched in this round
    if (!first_) {
      bool any_active = false;
      std::vector<uint8_t> alive;
      const int np = num_awaited();
      for (int k = 0; k < np; k++) {
        const int i = awaited(k);
        any_active |= row[i] == 1;
        if (row[i] == 1 && use_list_) alive.push_back((uint8_t)i);
      }
      if (host_window_) {
        // pairs launched in this round but not in the one before have no status byte yet: they stay
        for (uint8_t i : this_list) {
          bool seen = false;
          for (uint8_t q : prev_list_) if (q == i) { seen = true; break; }
          if (!seen) { alive.push_back(i); any_active = true; }
        }
        while ((int)alive.size() < window_ && next_queued_ < n_) { alive.push_back((uint8_t)next_queued_++); any_active = true; }
      }
      if (!any_active) return false;
      if (use_list_) act_.swap(alive);
    }
    first_ = false;
    prev_list_.swap(this_list);
    return true;
  }

 private:
  int n_, window_;
  bool host_window_, use_list_;
  bool first_ = true;
  std::vector<uint8_t> act_;         // this round's list
  std::vector<uint8_t> prev_list_;   // the previous round's
  int next_queued_;                  // host window: first pair that has not been launched yet
};

// ---- pclomp NDT batch: lock-step groups --------------------------------------------------------------------------------------
// an object asks for at most 12 evaluations per Newton iteration (1 + 10 trials + the Hessian pass) and runs max_iterations + 2 of them
inline int pclndt_round_budget(int max_iterations) { return (max_iterations + 3) * 12 + 2; }

// One group: objects [lo, hi) advance in lock-step.  At most two rounds are in flight (the host confirms a round's status bytes
// before it queues the one after the next); a group whose objects have all finished sees that one round late and stops.
struct RoundGroup {
  int lo = 0, hi = 0, max_rounds = 0;
  int launched = 0, confirmed = 0;
  bool done = false;
  bool may_launch() const { return !done && launched - confirmed < 2 && launched < max_rounds; }
  bool awaiting() const { return !done && confirmed < launched; }   // a launched round has not been confirmed
  // `row`: status bytes [object] of round `confirmed`, the oldest unconfirmed one: have all of this group's landed?
  bool landed(const volatile unsigned char* row) const {
    bool ready = true;
    for (int i = lo; i < hi; i++) ready &= row[i] != 0;
    return ready;
  }
  // Confirms that round once all its bytes are there (true: confirmed); the group is done when none of them is 1 or at the budget.
  bool try_confirm(const volatile unsigned char* row) {
    if (!awaiting()) return false;
    bool ready = true, any_active = false;
    for (int i = lo; i < hi; i++) { const unsigned char f = row[i]; ready &= f != 0; any_active |= f == 1; }
    if (!ready) return false;
    confirmed++;
    if (!any_active || confirmed >= max_rounds) done = true;
    return true;
  }
};

inline std::vector<RoundGroup> split_round_groups(int n, int ngroups, int max_rounds) {
  std::vector<RoundGroup> groups((size_t)ngroups);
  for (int g = 0; g < ngroups; g++) {
    groups[(size_t)g].lo = (int)((long long)n * g / ngroups);
    groups[(size_t)g].hi = (int)((long long)n * (g + 1) / ngroups);
    groups[(size_t)g].max_rounds = max_rounds;
  }
  return groups;
}

}  // namespace pcm
