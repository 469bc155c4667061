// C entry points over pointcloud-slam_amd/csrc/batch_schedule.h for tests/test_batch_schedule.py (host compiler only, no HIP).
#include "batch_schedule.h"

using namespace pcm;

extern "C" {

// out: window, per_pair_rounds, host_window, use_list, max_rounds
void bs_plan(int n, int batch_window, int max_iterations, int is_lm, int lm_max_iterations, int max_listed_pairs, int* out) {
  const BatchPlan p = plan_batch(n, batch_window, max_iterations, is_lm != 0, lm_max_iterations, max_listed_pairs);
  out[0] = p.window; out[1] = p.per_pair_rounds; out[2] = p.host_window; out[3] = p.use_list; out[4] = p.max_rounds;
}

void* bs_list_new(int n, int batch_window, int max_iterations, int is_lm, int lm_max_iterations, int max_listed_pairs) {
  return new LaunchList(n, plan_batch(n, batch_window, max_iterations, is_lm != 0, lm_max_iterations, max_listed_pairs));
}
void bs_list_free(void* h) { delete static_cast<LaunchList*>(h); }
int bs_list_size(void* h) { return static_cast<LaunchList*>(h)->size(); }
int bs_list_current(void* h, unsigned char* out) {   // the list itself (use_list plans); returns its length
  const std::vector<uint8_t>& a = static_cast<LaunchList*>(h)->current();
  for (size_t i = 0; i < a.size(); i++) out[i] = a[i];
  return (int)a.size();
}
int bs_list_num_awaited(void* h) { return static_cast<LaunchList*>(h)->num_awaited(); }
int bs_list_awaited(void* h, int k) { return static_cast<LaunchList*>(h)->awaited(k); }
int bs_list_advance(void* h, const unsigned char* row) { return static_cast<LaunchList*>(h)->advance(row) ? 1 : 0; }

int bs_pclndt_round_budget(int max_iterations) { return pclndt_round_budget(max_iterations); }
void* bs_groups_new(int n, int ngroups, int max_rounds) { return new std::vector<RoundGroup>(split_round_groups(n, ngroups, max_rounds)); }
void bs_groups_free(void* h) { delete static_cast<std::vector<RoundGroup>*>(h); }
static RoundGroup& group(void* h, int g) { return (*static_cast<std::vector<RoundGroup>*>(h))[(size_t)g]; }
int bs_groups_count(void* h) { return (int)static_cast<std::vector<RoundGroup>*>(h)->size(); }
// out: lo, hi, launched, confirmed, done
void bs_group_get(void* h, int g, int* out) {
  const RoundGroup& G = group(h, g);
  out[0] = G.lo; out[1] = G.hi; out[2] = G.launched; out[3] = G.confirmed; out[4] = G.done;
}
int bs_group_try_confirm(void* h, int g, const unsigned char* row) { return group(h, g).try_confirm(row) ? 1 : 0; }
int bs_group_may_launch(void* h, int g) { return group(h, g).may_launch() ? 1 : 0; }
void bs_group_launched(void* h, int g) { group(h, g).launched++; }   // what the caller does after its launch

}  // extern "C"
