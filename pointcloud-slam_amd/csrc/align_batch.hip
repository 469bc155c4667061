// align_batch.hip -- the batch workspace and the round loops behind pcm_align / pcm_align_batch: the device-resident GN/LM loop of
// n pairs (align_batch_impl), the single-pass parity hook, and the batched pclomp NDT registration in lock-step groups.
//
// Host-side counterpart of the reference's
//   LsqRegistration::computeTransformation  ref:pointcloud_match/fast_gicp/include/fast_gicp/gicp/impl/lsq_registration_impl.hpp:52-79
// The reference crosses host<->device >= 4 times per Gauss-Newton iteration
// (SURVEY.md §2.3); here the loop state lives on the device and the host only
// polls a per-round "pairs still active" counter one round behind the GPU.
// Which pairs or groups a round launches is decided in batch_schedule.h (plain integer logic, checked without a device); this
// file waits on the status bytes, launches, times and counts.
#include "batch_schedule.h"
#include "pcm_core.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>

namespace pcm {

namespace {

// Watchdog of a host loop that spins on round status bytes (mapped pinned host memory, stored by the step kernels): idle() is
// called on every fruitless spin.  On both error returns the queued kernels may still be writing into the workspace and the flags:
// the streams are drained first, so that the caller can destroy the context safely.  The runtime is asked (hipStreamQuery: has the
// stream died?) only after a wait far beyond any round -- a query takes the locks the other slots' launches need; polled every few
// microseconds by several waiting threads it throttled every launch of the process.
class StatusWatch {
 public:
  StatusWatch(pcm_ctx* c0, const hipStream_t* streams, int nstreams, std::chrono::steady_clock::time_point t_start)
      : c0_(c0), streams_(streams), nstreams_(nstreams), t_start_(t_start), next_query_(std::chrono::steady_clock::now() + std::chrono::milliseconds(5)) {}
  void progress() { spins_ = 0; }
  // pending(k): stream k has launched a round whose status bytes have not all landed
  template <class Pending>
  int idle(Pending&& pending) {
    if ((++spins_ & 0xfff) != 0) return PCM_OK;
    const auto now = std::chrono::steady_clock::now();
    if (now - t_start_ > std::chrono::seconds(20)) { drain(); c0_->err = "timeout waiting for the GPU round status"; return PCM_ERR_HIP; }
    if (now >= next_query_) {   // a dead stream never writes its status bytes
      next_query_ = now + std::chrono::milliseconds(5);
      for (int k = 0; k < nstreams_; k++)
        if (pending(k) && hipStreamQuery(streams_[k]) == hipSuccess && pending(k)) { drain(); c0_->err = "stream drained without a round status (kernel fault?)"; return PCM_ERR_HIP; }
    }
    return PCM_OK;
  }

 private:
  void drain() { for (int k = 0; k < nstreams_; k++) (void)hipStreamSynchronize(streams_[k]); }
  pcm_ctx* c0_;
  const hipStream_t* streams_;
  int nstreams_;
  std::chrono::steady_clock::time_point t_start_, next_query_;
  unsigned spins_ = 0;
};

// spin until a round's status byte is non-zero
int wait_status_byte(pcm_ctx* c0, hipStream_t st, volatile unsigned char* p, std::chrono::steady_clock::time_point t_start) {
  StatusWatch watch(c0, &st, 1, t_start);
  while (*p == 0)
    if (int rc = watch.idle([p](int) { return *p == 0; })) return rc;
  return PCM_OK;
}

bool same_solver_config(const pcm_config& a, const pcm_config& b) {
  return a.model == b.model && a.optimizer == b.optimizer && a.max_iterations == b.max_iterations && a.lm_max_iterations == b.lm_max_iterations &&
         a.rotation_eps == b.rotation_eps && a.translation_eps == b.translation_eps && a.lm_init_lambda_factor == b.lm_init_lambda_factor &&
         a.num_neighbors == b.num_neighbors && a.neighbor_search_radius == b.neighbor_search_radius && a.max_range == b.max_range && a.plane_threshold == b.plane_threshold && a.flags == b.flags &&
         (a.model == PCM_MODEL_P2PLANE || a.voxel_resolution == b.voxel_resolution) && (!is_gicp(a.model) || a.max_corr_dist == b.max_corr_dist);
}

}  // namespace

// The workspace belongs to the first context of a batch (contexts are single-threaded
// objects), so independent batches may run concurrently from different host threads
// on their own streams -- e.g. the stragglers of one batch under the bulk of the next.
int ensure_ws(pcm_ctx* c, Workspace** out, int npairs, size_t partial_doubles, int rounds) {
  Workspace* wp = c->ws.get_or_create<Workspace>();
  if (!wp) { c->err = "out of host memory"; return PCM_ERR_HIP; }
  Workspace& w = *wp;
  w.device = c->device;
  const size_t np = (size_t)npairs, cap = (size_t)std::max(npairs, 64);
  int rc = w.d_descs.reserve(c, np, cap);
  if (rc == PCM_OK) rc = w.d_states.reserve(c, np, cap);
  if (rc == PCM_OK) rc = w.d_guesses.reserve(c, 16 * np, 16 * cap);
  if (rc == PCM_OK) rc = w.d_results.reserve(c, np, cap);
  if (rc == PCM_OK) rc = w.d_sums.reserve(c, kPartialStride * np, kPartialStride * cap);
  if (rc == PCM_OK) rc = w.d_jobs.reserve(c, np, cap);
  if (rc == PCM_OK && partial_doubles) rc = w.d_partials.reserve(c, partial_doubles, partial_doubles);
  if (rc != PCM_OK) return rc;
  {
    // per-round status bytes of every pair live in mapped pinned host memory: k_finish_round
    // stores them directly (posted writes); the host polls them, no event / copy per round
    const size_t bytes = (size_t)rounds * cap;
    if (!w.h_flags || bytes > w.h_flags.cap) w.d_flags = nullptr;
    rc = w.h_flags.reserve(c, bytes, bytes, hipHostMallocMapped);
    if (rc != PCM_OK) return rc;
    if (!w.d_flags) PCM_HIPCK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&w.d_flags), w.h_flags.p, 0));
  }
  rc = w.d_stats.reserve(c, 16, 16);
  if (rc == PCM_OK) rc = w.d_queue.reserve(c, 1, 1);
  if (rc != PCM_OK) return rc;
  while ((int)w.ev_round.size() < 2) {
    hipEvent_t e;
    PCM_HIPCK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    w.ev_round.push_back(e);
  }
  *out = &w;
  return PCM_OK;
}

int align_batch_impl(pcm_ctx* const* ctxs, int n, const float* guesses, pcm_result* host_out, void* device_out) {
  if (!ctxs || n <= 0 || !guesses) return PCM_ERR_INVALID_ARGUMENT;
  pcm_ctx* c0 = ctxs[0];
  if (!c0) return PCM_ERR_INVALID_ARGUMENT;
  size_t max_n = 0;
  for (int i = 0; i < n; i++) {
    pcm_ctx* c = ctxs[i];
    if (!c) { c0->err = "null context in batch"; return PCM_ERR_INVALID_ARGUMENT; }
    if (c->device != c0->device) { c0->err = "all contexts of a batch must live on one device"; return PCM_ERR_INVALID_ARGUMENT; }
    if (!same_solver_config(c->cfg, c0->cfg)) { c0->err = "all contexts of a batch must share the solver configuration"; return PCM_ERR_INVALID_ARGUMENT; }
    if (c->stream != c0->stream) {
      // inputs of the other contexts were produced on their own streams, which are idle after set_*()
    }
  }
  {
    // per-object preparation (the scan's kNN index and covariances of the GICP family are the heavy part: a radix sort with
    // host syncs per object): the objects are independent and own their streams, so up to 8 host threads prepare them side
    // by side; nothing is shared but the device
    std::vector<int> rcs((size_t)n, PCM_OK);
    const int nthreads = (is_gicp(c0->cfg.model) && n > 1) ? std::min(n, 8) : 1;
    bool distinct = true;
    for (int i = 0; i < n && distinct; i++) for (int j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) { distinct = false; break; }
    if (nthreads <= 1 || !distinct) {
      for (int i = 0; i < n; i++) rcs[(size_t)i] = prepare(ctxs[i]);
    } else {
      std::atomic<int> next{0};
      auto worker = [&]() {
        for (;;) {
          const int i = next.fetch_add(1);
          if (i >= n) break;
          rcs[(size_t)i] = prepare(ctxs[i]);
        }
      };
      std::vector<std::thread> th;
      for (int t = 0; t < nthreads; t++) th.emplace_back(worker);
      for (auto& t : th) t.join();
    }
    for (int i = 0; i < n; i++) {
      if (rcs[(size_t)i] != PCM_OK) { if (ctxs[i] != c0) c0->err = ctxs[i]->err; return rcs[(size_t)i]; }
      max_n = std::max(max_n, num_elements(ctxs[i]));
    }
  }
  // GICP / VGICP: the covariance kernels of the contexts were queued on their own streams without a host
  // sync (they overlap on the device); the batch kernels below run on c0's stream and read their output
  if (is_gicp(c0->cfg.model)) {
    for (int i = 0; i < n; i++) PCM_HIPCK(c0, hipStreamSynchronize(ctxs[i]->stream));
  }
  const pcm_config& g = c0->cfg;
  const bool ndt = is_ndt(g.model) || g.model == PCM_MODEL_VGICP_CUDA;   // residual kernel of the Gaussian-voxel family
  const bool gicp = is_gicp(g.model);                                     // per-point covariances, source elements = brick-major copy
  const Geom geom = pick_geom(max_n, n, ndt);
  const LsqParams lp = lsq_params(g);
  const KernelParams kp = kernel_params(g, geom);
  const bool is_lm = g.optimizer == PCM_OPT_LEVENBERG_MARQUARDT;
  const BatchPlan plan = plan_batch(n, g.batch_window, g.max_iterations, is_lm, g.lm_max_iterations, kMaxListedPairs);   // window, launch list, round budget
  const int max_rounds = plan.max_rounds;
  const bool use_list = plan.use_list;
  const size_t per_pair_partials = (size_t)std::max(geom.blocks_per_pair, geom.tiles_per_pair) * kPartialStride;
  Workspace* w = nullptr;
  int rc = ensure_ws(c0, &w, n, per_pair_partials * n, max_rounds);
  if (rc != PCM_OK) return rc;
  hipStream_t st = c0->stream;

  PCM_HIPCK(c0, hipMemcpyAsync(w->d_guesses, guesses, sizeof(float) * 16 * n, hipMemcpyHostToDevice, st));
  {  // new scans are re-ordered along the world grid (at their initial guess) in one batched pass
    std::vector<SortJob> jobs;
    uint32_t total = 0, jmax = 0;
    for (int i = 0; i < n; i++) {
      pcm_ctx* c = ctxs[i];
      if (!c->cfg.sort_source || c->src_sorted || c->cfg.model == PCM_MODEL_NDT_D2D || gicp) continue;
      SortJob j{c->src.d_pts, c->src_order, (uint32_t)c->src.n, total, (uint32_t)i, 0};
      jobs.push_back(j);
      total += j.n;
      jmax = std::max(jmax, j.n);
    }
    if (!jobs.empty()) {
      PCM_HIPCK(c0, hipMemcpyAsync(w->d_jobs, jobs.data(), sizeof(SortJob) * jobs.size(), hipMemcpyHostToDevice, st));
      rc = sort_sources_batched(st, w->d_jobs, (int)jobs.size(), jmax, total, w->d_guesses, g.voxel_resolution, &w->sort, &c0->err);
      if (rc != PCM_OK) return rc;
      for (const SortJob& j : jobs) ctxs[j.guess_index]->src_sorted = true;
    }
  }
  std::vector<PairDesc> descs(n);
  for (int i = 0; i < n; i++) fill_desc(ctxs[i], &descs[i], w->d_partials + per_pair_partials * i);
  PCM_HIPCK(c0, hipMemcpyAsync(w->d_descs, descs.data(), sizeof(PairDesc) * n, hipMemcpyHostToDevice, st));
  std::memset(w->h_flags, 0, (size_t)max_rounds * n);
  launch_init_states(st, w->d_states, w->d_guesses, n, g.max_iterations, plan.host_window ? n : plan.window, w->d_queue);
  const bool stats_on = (c0->profiling & 1) != 0;      // HIP events around the residual launches
  const bool stats_sampled = stats_on && (c0->profiling & 8) != 0;   // ... every 4th launch only; the phase moves from batch to batch
  const unsigned prof_phase = stats_sampled ? (unsigned)(c0->stats.linearize_launches & 3u) : 0u;
  uint64_t timed_launches = 0, timed_slots = 0, launched_slots = 0;
  const bool timing_on = (c0->profiling & 4) != 0;     // diagnostic: in-kernel phase stamps (stats.phase_cycles)
  const bool counters_on = (c0->profiling & 2) != 0 || timing_on;   // kNN candidate / probe counters (slower kernel variant)
  if (counters_on) PCM_HIPCK(c0, hipMemsetAsync(w->d_stats, 0, sizeof(unsigned long long) * 16, st));
  const bool write_sel = is_lm;  // trial passes re-use the planes of the selected set
  const bool counted_search = (g.flags & PCM_FLAG_COUNTED_SEARCH) != 0;   // k_linearize_counted (A/B)
  const bool ref_order = g.model == PCM_MODEL_P2PLANE && (g.flags & PCM_FLAG_REFERENCE_KNN_ORDER) != 0;   // neighbours in libstdc++'s nth_element order
  bool lists = g.model == PCM_MODEL_P2PLANE && !ref_order;   // k_linearize_lists: every context of the batch holds its map's candidate lists
  for (int i = 0; i < n && lists; i++) lists = lists_view_for(ctxs[i]).pts != nullptr;
  const bool pooled = lists && lists_pooled_for(ctxs[0]);   // one kernel per launch: a batch that mixes pooled and contiguous lists takes the tile kernel
  for (int i = 0; i < n && lists; i++) lists = lists_pooled_for(ctxs[i]) == pooled;
  if (ref_order) {
    for (int i = 0; i < n; i++) {
      if (ctxs[i]->tg->map.max_voxel_points > (uint32_t)kRefMaxVoxelPoints) {
        c0->err = "PCM_FLAG_REFERENCE_KNN_ORDER supports at most " + std::to_string(kRefMaxVoxelPoints) + " points per voxel (this map: " + std::to_string(ctxs[i]->tg->map.max_voxel_points) + ")";
        return PCM_ERR_UNSUPPORTED;
      }
    }
  }

  int rounds_done = 0;
  size_t prof_used = 0;
  LaunchList list(n, plan);
  KernelParams kpr = kp;
  for (int r = 0; r < max_rounds; r++) {
    const int nl = list.size();
    if (use_list) {
      kpr.use_list = 1;
      std::memcpy(kpr.active, list.current().data(), list.current().size());
    }
    const bool timed = stats_on && (!stats_sampled || (((unsigned)r + prof_phase) & 3u) == 0u);
    launched_slots += (uint64_t)nl;
    if (timed) {
      while (w->ev_prof.size() < prof_used + 3) { hipEvent_t e; PCM_HIPCK(c0, hipEventCreate(&e)); w->ev_prof.push_back(e); }
      PCM_HIPCK(c0, hipEventRecord(w->ev_prof[prof_used], st));
      timed_launches++;
      timed_slots += (uint64_t)nl;
    }
    // per round: correspondence search + residual/Jacobian + reduction in one launch, then the tiny
    // per-pair sum + GN/LM step launch.  LM adds the (cheap) trial-cost launch + its step.
    // PCM_FLAG_FUSED_STEP (off by default): the last workgroup of a pair's search launch takes the GN step (write-through hand-off of
    // the partial rows, kernels.hip).  Measured slower than the second launch at every round size, the single-pair rounds
    // included (profiles/r02_fused_step_threshold_sweep.txt): every workgroup pays a store drain and a returned atomic.
    const bool fuse = use_list && !is_lm && !ndt && !gicp && !counters_on && !timing_on && kp.do_step && (g.flags & PCM_FLAG_FUSED_STEP);
    if (ndt) launch_ndt(st, w->d_descs, w->d_states, kpr, nl, ndt_kind(g.model), false);
    else if (gicp) launch_gicp(st, w->d_descs, w->d_states, kpr, nl, g.model == PCM_MODEL_VGICP, false);
    else if (fuse) launch_linearize_fused(st, w->d_descs, w->d_states, kpr, lp, nl, w->d_flags + (size_t)r * n);
    else if (ref_order) launch_linearize_reforder(st, w->d_descs, w->d_states, kpr, nl, write_sel);
    else if (lists && !counters_on && !timing_on) launch_linearize_lists(st, w->d_descs, w->d_states, kpr, nl, write_sel, pooled);
    else if (counted_search) launch_linearize_counted(st, w->d_descs, w->d_states, kpr, nl, write_sel, counters_on ? w->d_stats : nullptr, timing_on);
    else launch_linearize(st, w->d_descs, w->d_states, kpr, nl, write_sel, counters_on ? w->d_stats : nullptr, timing_on);
    if (timed) PCM_HIPCK(c0, hipEventRecord(w->ev_prof[prof_used + 1], st));
    if (!fuse) launch_finish_round(st, w->d_descs, w->d_states, kpr, lp, nl, false, !is_lm, w->d_flags + (size_t)r * n, w->d_sums, use_list ? nullptr : w->d_queue, n);
    if (is_lm) {
      if (ndt) launch_ndt(st, w->d_descs, w->d_states, kpr, nl, ndt_kind(g.model), true);
      else if (gicp) launch_gicp(st, w->d_descs, w->d_states, kpr, nl, g.model == PCM_MODEL_VGICP, true);
      else launch_trial(st, w->d_descs, w->d_states, kpr, nl);
      launch_finish_round(st, w->d_descs, w->d_states, kpr, lp, nl, true, true, w->d_flags + (size_t)r * n, w->d_sums, use_list ? nullptr : w->d_queue, n);
    }
    if (timed) {
      if (!stats_sampled) PCM_HIPCK(c0, hipEventRecord(w->ev_prof[prof_used + 2], st));
      prof_used += 3;
    }
    rounds_done = r + 1;
    // look one round behind so the GPU always has the next round queued
    volatile unsigned char* row = r >= 1 ? w->h_flags + (size_t)(r - 1) * n : nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    for (int k = 0; k < list.num_awaited(); k++)
      if (int wrc = wait_status_byte(c0, st, row + list.awaited(k), t_start)) return wrc;
    if (!list.advance(row)) break;
  }
  PCM_HIPCK(c0, hipGetLastError());
  pcm_result* d_res = device_out ? static_cast<pcm_result*>(device_out) : w->d_results;
  launch_pack_results(st, w->d_states, d_res, n);
  std::vector<pcm_result> tmp;
  pcm_result* h_res = host_out;
  if (!h_res) { tmp.resize(n); h_res = tmp.data(); }
  PCM_HIPCK(c0, hipMemcpyAsync(h_res, d_res, sizeof(pcm_result) * n, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c0, hipStreamSynchronize(st));

  if (counters_on) {
    unsigned long long hs[16];
    PCM_HIPCK(c0, hipMemcpy(hs, w->d_stats, sizeof(hs), hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; k++) c0->phase_cycles[k] += hs[8 + k];
    c0->stats.candidates += hs[0];
    c0->stats.slots_probed += hs[1];
    c0->stats.tiles += hs[3];
    c0->stats.tiles_lds_grid += hs[4];
    c0->stats.tiles_lds_points += hs[2];
  }
  if (stats_on) {
    double ms = 0.0, ms2 = 0.0;
    for (size_t k = 0; k + 2 < prof_used + 1; k += 3) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, w->ev_prof[k], w->ev_prof[k + 1]) == hipSuccess) ms += t;
      if (!stats_sampled && hipEventElapsedTime(&t, w->ev_prof[k + 1], w->ev_prof[k + 2]) == hipSuccess) ms2 += t;
    }
    c0->stats.linearize_ms += ms;
    c0->stats.residual_ms += ms2;
    c0->stats.timed_launches += timed_launches;
    c0->stats.timed_pair_slots += timed_slots;
  }
  c0->stats.launched_pair_slots += launched_slots;
  c0->stats.linearize_launches += (uint64_t)rounds_done;
  uint64_t passes = 0;
  int worst = PCM_OK;
  for (int i = 0; i < n; i++) {
    passes += (uint64_t)(h_res[i].num_linearize + h_res[i].num_compute_error) * num_elements(ctxs[i]);
    if (h_res[i].status != PCM_OK && worst != PCM_ERR_INTERNAL) worst = h_res[i].status;
  }
  c0->stats.point_passes += passes;
  if (worst == PCM_ERR_INTERNAL) c0->err = "the round budget of the batch ran out before every pair finished (library bug): unfinished pairs carry PCM_ERR_INTERNAL";
  else if (worst != PCM_OK) c0->err = "lm not converged!!";
  return worst;
}

// one LINEARIZE or TRIAL pass at a caller-supplied pose (parity hook)
int single_pass(pcm_ctx* c, const double T[16], bool linearize, double sums[kPartialStride]) {
  if (c->cfg.model == PCM_MODEL_NDT_OMP) { c->err = "the pclomp NDT model is evaluated through pcm_ndt_derivatives"; return PCM_ERR_UNSUPPORTED; }
  int rc = prepare(c);
  if (rc != PCM_OK) return rc;
  const bool ndt = is_ndt(c->cfg.model) || c->cfg.model == PCM_MODEL_VGICP_CUDA;
  const Geom geom = pick_geom(num_elements(c), 1, ndt);
  const KernelParams kp = kernel_params(c->cfg, geom);
  Workspace* w = nullptr;
  rc = ensure_ws(c, &w, 1, (size_t)std::max(geom.blocks_per_pair, geom.tiles_per_pair) * kPartialStride, 2);
  if (rc != PCM_OK) return rc;
  PairDesc d;
  fill_desc(c, &d, w->d_partials);
  PairState s;
  float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  init_state(s, ident);
  // k_ndt<., true> builds R cov_A R^T of D2D / VGICP_CUDA from x0 = the pose of the last linearize, not from the trial pose (with
  // x0 = T here, pcm_compute_error at a ROTATED pose used the trial pose's rotation: 2.4e-4 / 1.3e-2 off at 0.02 rad)
  if (linearize) std::memcpy(c->lin_T, T, sizeof(double) * 16);
  for (int i = 0; i < 16; i++) { s.x0[i] = (ndt && !linearize) ? c->lin_T[i] : T[i]; s.xi[i] = T[i]; }
  s.mode = linearize ? MODE_LINEARIZE : MODE_TRIAL;
  PCM_HIPCK(c, hipMemcpyAsync(w->d_descs, &d, sizeof(d), hipMemcpyHostToDevice, c->stream));
  PCM_HIPCK(c, hipMemcpyAsync(w->d_states, &s, sizeof(s), hipMemcpyHostToDevice, c->stream));
  KernelParams kp1 = kp;
  kp1.do_step = 0;   // the last workgroup exports the sums instead of stepping
  if (ndt) launch_ndt(c->stream, w->d_descs, w->d_states, kp1, 1, ndt_kind(c->cfg.model), !linearize);
  else if (is_gicp(c->cfg.model)) launch_gicp(c->stream, w->d_descs, w->d_states, kp1, 1, c->cfg.model == PCM_MODEL_VGICP, !linearize);
  else if (linearize && (c->cfg.flags & PCM_FLAG_REFERENCE_KNN_ORDER)) {
    if (c->tg->map.max_voxel_points > (uint32_t)kRefMaxVoxelPoints) { c->err = "PCM_FLAG_REFERENCE_KNN_ORDER supports at most " + std::to_string(kRefMaxVoxelPoints) + " points per voxel"; return PCM_ERR_UNSUPPORTED; }
    launch_linearize_reforder(c->stream, w->d_descs, w->d_states, kp1, 1, true);
  }
  else if (linearize && lists_view_for(c).pts != nullptr) launch_linearize_lists(c->stream, w->d_descs, w->d_states, kp1, 1, true, lists_pooled_for(c));
  else if (linearize && (c->cfg.flags & PCM_FLAG_COUNTED_SEARCH)) launch_linearize_counted(c->stream, w->d_descs, w->d_states, kp1, 1, true, nullptr);
  else if (linearize) launch_linearize(c->stream, w->d_descs, w->d_states, kp1, 1, true, nullptr, false);
  else launch_trial(c->stream, w->d_descs, w->d_states, kp1, 1);
  launch_finish_round(c->stream, w->d_descs, w->d_states, kp1, lsq_params(c->cfg), 1, !linearize, false, w->d_flags, w->d_sums);
  PCM_HIPCK(c, hipGetLastError());
  PCM_HIPCK(c, hipMemcpyAsync(sums, w->d_sums, sizeof(double) * kPartialStride, hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

// one pclomp NDT pass on the device: launch, read the 48-double row back (pass 0/1: H, g, score; pass 2: H)
int pclndt_eval(pcm_ctx* c, int pass, const NdtOmpParams& P, ndtomp::Eval* e, double gauss_d3) {
  launch_pclndt_pass(c->stream, c->tg->map, c->tg->pleaf, c->tg->pleaf_f, ndt_lists_view(c), c->src.d_pts, (uint32_t)c->src.n, P, pass, c->ndt_partials, c->ndt_out, gauss_d3);
  PCM_HIPCK(c, hipGetLastError());
  PCM_HIPCK(c, hipMemcpyAsync(c->ndt_out_host, c->ndt_out, sizeof(double) * 48, hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  std::memcpy(e->H, c->ndt_out_host, sizeof(double) * 36);
  if (pass == 3) e->score = c->ndt_out_host[0];
  else if (pass != 2) {
    std::memcpy(e->g, c->ndt_out_host + 36, sizeof(double) * 6);
    e->score = c->ndt_out_host[42];
  }
  c->stats.linearize_launches += 1;
  c->stats.point_passes += c->src.n;
  return PCM_OK;
}

namespace {

// buffers of a batched pclomp NDT registration, owned by the first context of the batch
struct NdtBatchWs {
  DevBuf<NdtObject> d_objs{"d_objs"};
  DevBuf<ndtomp::NdtMachine> d_ms{"d_ms"};
  PinnedBuf<NdtObject> h_objs{"h_objs"};
  PinnedBuf<ndtomp::NdtMachine> h_ms{"h_ms"};
  PinnedBuf<unsigned char> h_flags{"h_flags"};   // mapped pinned: [round][object] status bytes of k_pclndt_batch_step
  unsigned char* d_flags = nullptr;              // device view of h_flags
  hipStream_t gst[4] = {nullptr, nullptr, nullptr, nullptr};   // streams of the lock-step groups, created back to back
  ~NdtBatchWs() { for (hipStream_t st : gst) if (st) (void)hipStreamDestroy(st); }
};

}  // namespace

// pclomp::NormalDistributionsTransform::computeTransformation (ndt_omp_impl.hpp:69-156) for n objects: their solvers run on the
// device (ndtomp::NdtMachine, pclndt_host.h), one derivatives launch + one step launch per round for all of them
int pclndt_align_batch(pcm_ctx* const* ctxs, int n, const float* guesses, pcm_result* res) {
  pcm_ctx* c0 = ctxs[0];
  for (int i = 0; i < n; i++) {
    int rc = prepare(ctxs[i]);
    if (rc != PCM_OK) { if (i) c0->err = ctxs[i]->err; return rc; }
    if (ctxs[i]->stream != c0->stream) PCM_HIPCK(c0, hipStreamSynchronize(ctxs[i]->stream));   // its map / leaves were built on its own stream
  }
  NdtBatchWs* wp = c0->ndt_ws.get_or_create<NdtBatchWs>();
  if (!wp) { c0->err = "out of host memory"; return PCM_ERR_HIP; }
  NdtBatchWs& w = *wp;
  {
    const size_t cap = (size_t)std::max(n, 16);
    int rc = w.d_objs.reserve(c0, (size_t)n, cap);
    if (rc == PCM_OK) rc = w.d_ms.reserve(c0, (size_t)n, cap);
    if (rc == PCM_OK) rc = w.h_objs.reserve(c0, (size_t)n, cap);
    if (rc == PCM_OK) rc = w.h_ms.reserve(c0, (size_t)n, cap);
    if (rc != PCM_OK) return rc;
  }
  int max_rounds = 2;
  int max_blocks = 1;
  for (int i = 0; i < n; i++) {
    pcm_ctx* c = ctxs[i];
    w.h_objs[i] = make_ndt_object(c->tg->map, c->tg->pleaf, c->tg->pleaf_f, ndt_lists_view(c), c->src.d_pts, (uint32_t)c->src.n, c->ndt_partials);
    max_blocks = std::max(max_blocks, (int)w.h_objs[i].nblocks);
    ndtomp::ndt_machine_start(w.h_ms[i], guesses + 16 * (size_t)i, (double)c->cfg.ndt_step_size, c->cfg.translation_eps, (double)c->cfg.ndt_outlier_ratio,
                              c->cfg.voxel_resolution, c->cfg.max_iterations, c->cfg.num_neighbors);
    max_rounds = std::max(max_rounds, pclndt_round_budget(c->cfg.max_iterations));
  }
  const size_t flag_bytes = (size_t)max_rounds * (size_t)n;
  {
    if (!w.h_flags || flag_bytes > w.h_flags.cap) w.d_flags = nullptr;
    const int rc = w.h_flags.reserve(c0, flag_bytes, std::max<size_t>(flag_bytes, 65536), hipHostMallocMapped);
    if (rc != PCM_OK) return rc;
    if (!w.d_flags) PCM_HIPCK(c0, hipHostGetDevicePointer(reinterpret_cast<void**>(&w.d_flags), w.h_flags.p, 0));
  }
  std::memset(w.h_flags, 0, flag_bytes);
  hipStream_t st = c0->stream;
  PCM_HIPCK(c0, hipMemcpyAsync(w.d_objs, w.h_objs, sizeof(NdtObject) * n, hipMemcpyHostToDevice, st));
  PCM_HIPCK(c0, hipMemcpyAsync(w.d_ms, w.h_ms, sizeof(ndtomp::NdtMachine) * n, hipMemcpyHostToDevice, st));
  PCM_HIPCK(c0, hipStreamSynchronize(st));   // the groups below run on their own streams
  // The objects advance in up to four groups, each in lock-step on the stream of its first object: registrations need 6 ... 37
  // Newton iterations on the same map, and a single lock-step batch runs every round at the pace of its largest kernel while most
  // objects have finished.  At most two rounds of a group are in flight (the host confirms a round's status bytes before it queues
  // the one after the next); a group whose objects have all finished sees that one round late and stops.
  // Measured at config 4 (100k-point scans, tools/r03_scaling.sh): 8 objects -- four groups 1 175 registrations/s, two 1 122; 16 objects --
  // one group 1 548, two 1 781, four 953; 32 objects -- one 2 340, two 2 753, three 2 217, four 1 990: one group's solver step and the
  // ragged end of its pass overlap the other's pass; more groups only add launches and host-side waiting.
  size_t total_points = 0;
  for (int i = 0; i < n; i++) total_points += ctxs[i]->src.n;
  // (the 27-cell searches -- KDTREE, DIRECT26 -- lose with two groups while they look their cells up one by one: 1 570 -> 1 213 at 32
  // scans, their pass keeps the device busy alone; on the grid's neighbour-leaf lists they gain like the others: 2 760 -> 3 203)
  const bool wide = (c0->cfg.num_neighbors == 0 || c0->cfg.num_neighbors > 7) && ndt_lists_view(c0).pts == nullptr;
  int ngroups = total_points <= 1000000 ? std::min(n, 4) : (wide ? 1 : std::min(n, 2));
  if (const char* e = getenv("PCM_NDT_GROUPS")) ngroups = std::max(1, std::min(std::min(n, 4), atoi(e)));   // measurements only
  std::vector<RoundGroup> groups = split_round_groups(n, ngroups, max_rounds);   // launched / confirmed / done per group: batch_schedule.h
  hipStream_t gst[4];
  int gblocks[4];
  for (int g = 0; g < ngroups; g++) {
    const RoundGroup& G = groups[(size_t)g];
    // Streams of the groups' own, created back to back: HIP deals streams onto a handful of hardware queues in creation order, and two
    // groups whose streams share a queue do not overlap.  (With the streams of the groups' first objects the first batch of a process
    // ran at 3 225 registrations/s and a second batch of objects created later in the same process at 2 016, or the other way round.)
    if (ngroups == 1) gst[g] = ctxs[G.lo]->stream;
    else {
      if (!w.gst[g]) PCM_HIPCK(c0, hipStreamCreateWithFlags(&w.gst[g], hipStreamNonBlocking));
      gst[g] = w.gst[g];
    }
    gblocks[g] = 1;
    for (int i = G.lo; i < G.hi; i++) gblocks[g] = std::max(gblocks[g], (int)w.h_objs[i].nblocks);
  }
  auto row_of = [&](const RoundGroup& G) -> volatile unsigned char* { return w.h_flags + (size_t)G.confirmed * n; };   // oldest unconfirmed round
  StatusWatch watch(c0, gst, ngroups, std::chrono::steady_clock::now());
  int live = ngroups;
  while (live > 0) {
    bool progress = false;
    for (int g = 0; g < ngroups; g++) {
      RoundGroup& G = groups[(size_t)g];
      if (G.done) continue;
      if (G.try_confirm(row_of(G))) {   // status bytes of the oldest unconfirmed round of this group: all landed
        progress = true;
        if (G.done) { live--; continue; }
      }
      if (G.may_launch()) {
        launch_pclndt_batch_round(gst[g], w.d_objs + G.lo, w.d_ms + G.lo, G.hi - G.lo, gblocks[g], w.d_flags + (size_t)G.launched * n + G.lo);
        G.launched++;
        progress = true;
      }
    }
    if (progress) { watch.progress(); continue; }
    if (int rc = watch.idle([&](int g) { const RoundGroup& G = groups[(size_t)g]; return G.awaiting() && !G.landed(row_of(G)); })) return rc;
  }
  PCM_HIPCK(c0, hipGetLastError());
  for (int g = 0; g < ngroups; g++) PCM_HIPCK(c0, hipStreamSynchronize(gst[g]));
  PCM_HIPCK(c0, hipMemcpyAsync(w.h_ms, w.d_ms, sizeof(ndtomp::NdtMachine) * n, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c0, hipStreamSynchronize(st));
  int worst = PCM_OK;
  for (int i = 0; i < n; i++) {
    const ndtomp::NdtMachine& m = w.h_ms[i];
    pcm_result* out = &res[i];
    std::memset(out, 0, sizeof(*out));
    for (int k = 0; k < 16; k++) { out->T[k] = m.P.T[k]; out->T64[k] = (double)m.P.T[k]; }
    std::memcpy(out->H, m.cur.H, sizeof(out->H));   // hessian_eigen_
    out->cost = m.cur.score;                        // trans_probability_ * N
    out->iterations = m.nr;
    out->converged = m.converged;
    out->num_linearize = m.n_deriv;
    out->num_compute_error = m.n_hess;
    out->status = m.request < 0 ? PCM_OK : PCM_ERR_HIP;   // a machine still asking after max_rounds cannot happen (bounded loops)
    if (out->status != PCM_OK) { worst = out->status; c0->err = "pclomp NDT solver did not finish within its round budget"; }
    ctxs[i]->stats.linearize_launches += (uint64_t)(m.n_deriv + m.n_hess);
    ctxs[i]->stats.point_passes += (uint64_t)(m.n_deriv + m.n_hess) * ctxs[i]->src.n;
  }
  return worst;
}

}  // namespace pcm
