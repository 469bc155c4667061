// lio_api.hip -- the jueying_lio entry points of include/pcm_amd.h: motion compensation (pcm_undistort), the measurement model
// (pcm_obs_model), the iterated Kalman update (pcm_lio_update), MapIncremental (pcm_map_incremental) and one LiDAR frame
// (pcm_lio_frame_begin / _begin_cloud / _end).  Every call that launches ObsModel goes through match_setup and match_record, both
// frame entries through frame_tail, and whatever replaces the source through source_replaced (pcm_host.h): a new LIO call uses
// them instead of a copy of its neighbour.  The frame outputs are in lio_outputs.hip, the propagation in lio_predict.hip.
#include "pcm_core.h"
#include "pre_layouts.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace pcm;

// residuals_.resize(cur_pts, 0); point_selected_surf_.resize(cur_pts, true)  (laser_mapping.cc:337-338): the first
// min(old, new) entries survive a new scan, appended ones take the default.  plane_coef_ (:339) needs no such care: the
// IEKF's first ObsModel call of a frame always matches (esekfom.hpp:1529) and rewrites every plane it may read later.
int pcm::lio_members_resize(pcm_ctx* c, size_t n) {
  if (n > c->lio_aux.cap) {
    const int rc = c->lio_aux.reserve_keep(c, n, n + n / 2 + 1024, c->lio_aux_n);
    if (rc != PCM_OK) return rc;
  }
  if (n > c->lio_aux_n) launch_lio_members_init(c->stream, c->lio_aux, (uint32_t)c->lio_aux_n, (uint32_t)n);
  c->lio_aux_n = n;
  return PCM_OK;
}

namespace {

#define CHECK_CTX(c)                                                   \
  do {                                                                 \
    if (!(c)) return PCM_ERR_INVALID_ARGUMENT;                         \
    if ((c)->device < 0) return PCM_ERR_HIP;                           \
  } while (0)

// the 4 x 4 guess the sort of a new scan runs at: the LiDAR's world pose, rot * off_R in double cast to float, and the float t_wl
void sort_guess(const double* rot, const double* off_R, const float* t_wl, float* g) {
  double qwl[4], Rwl[9];
  iekf::quat_mul(rot, off_R, qwl);
  iekf::quat_to_rot(qwl, Rwl);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) g[i * 4 + j] = (float)Rwl[i * 3 + j];
    g[i * 4 + 3] = t_wl[i];
    g[12 + i] = 0.f;
  }
  g[15] = 1.f;
}

// ---- one ObsModel launch sequence: pcm_obs_model and the rounds of pcm_lio_update ------------------------------------------------
struct Match {
  Workspace* w = nullptr;
  uint32_t n = 0;       // scan points
  int tiles = 0;        // 256-point tiles: rows of partial sums
  KernelParams kp;
  iekf::PoseF pose;     // the float state of the call exactly as the reference casts it (laser_mapping.cc:602-603,669-671)
  bool on_lists = false, pooled = false;   // k_lio_lists instead of the tile kernel, on the pooled form of following lists
};

// Everything in front of the launches of a call evaluated at state `s`, after prepare(): the workspace, the sort of a new scan
// along the world grid at that state's pose, the members resize of the reference semantics, the kernel parameters, and the
// descriptor (d->lio: the float pose; its rematch flag is the caller's) and pair state in the caller's storage, which the
// caller uploads.
int match_setup(pcm_ctx* c, const iekf::State& s, int extrinsic_est_en, int rematch, PairDesc* d, PairState* ps, Match* m) {
  const uint32_t n = (uint32_t)c->src.n;
  m->n = n;
  m->tiles = (int)((n + 255u) / 256u);
  int rc = ensure_ws(c, &m->w, 1, (size_t)m->tiles * kLioStride, 2);
  if (rc != PCM_OK) return rc;
  Workspace* w = m->w;
  iekf::PoseF& L = m->pose;
  L = iekf::PoseF{};
  iekf::pose_of(s, &L);
  hipStream_t st = c->stream;
  if (c->cfg.sort_source && !c->src_sorted) {   // new scan: order it along the world grid at this state's pose
    float g[16];
    sort_guess(s.rot, s.off_R, L.t_wl, g);
    SortJob j{c->src.d_pts, c->src_order, n, 0, 0, 0};
    PCM_HIPCK(c, hipMemcpyAsync(w->d_guesses, g, sizeof(g), hipMemcpyHostToDevice, st));
    PCM_HIPCK(c, hipMemcpyAsync(w->d_jobs, &j, sizeof(j), hipMemcpyHostToDevice, st));
    rc = sort_sources_batched(st, w->d_jobs, 1, n, n, w->d_guesses, c->cfg.voxel_resolution, &w->sort, &c->err);
    if (rc != PCM_OK) return rc;
    c->src_sorted = true;
    c->lio_planes_valid = false;
    if (!rematch) { c->err = "pcm_obs_model(rematch=0) on a new scan"; return PCM_ERR_INVALID_ARGUMENT; }
  }
  if (rematch) c->lio_planes_valid = false;   // being rewritten until match_record
  const bool ref = (c->cfg.flags & PCM_FLAG_LIO_REFERENCE_SEMANTICS) != 0;
  if (ref) {
    rc = lio_members_resize(c, n);
    if (rc != PCM_OK) return rc;
  }
  m->kp = kernel_params(c->cfg, pick_geom(n, 1));
  m->kp.lio_rematch = rematch ? 1 : 0;   // not read by the device-flag instance (pcm_lio_update)
  m->kp.lio_extrinsic = extrinsic_est_en ? 1 : 0;
  m->kp.lio_ref = !ref ? 0 : ((c->cfg.sort_source && c->src_sorted) ? 2 : 1);
  fill_desc(c, d, w->d_partials);
  std::memcpy(&d->lio, &L, sizeof(L));
  d->lio_aux = c->lio_aux;
  const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  init_state(*ps, ident);
  m->on_lists = lio_on_lists(c);   // d->nl is their view then
  m->pooled = m->on_lists && lists_pooled_for(c);
  return PCM_OK;
}

// The book-keeping after the host has waited for such a call: `calls` ObsModel launches ran, `rematches` of them searched, and
// `last` is the pose of the last one (null: none) -- what the effect cloud's 81 pd2^2 test is evaluated at.  `matched`: the
// planes and neighbours now belong to the current scan; pcm_map_incremental reads nn_in_lists / nn_lists_generation as left here.
void match_record(pcm_ctx* c, const Match& m, bool matched, uint64_t rematches, uint64_t calls, const iekf::PoseF* last) {
  if (matched) {
    c->lio_planes_valid = true;
    c->nn_in_lists = m.on_lists;
    c->nn_lists_generation = c->tg->nlists.generation;
  }
  c->lio_search_path[m.on_lists ? 0 : 1] += rematches;
  c->lio_last_obs.valid = false;
  if (last) c->lio_last_obs.set(last->q_wl, last->t_wl);
  c->stats.linearize_launches += calls;
  c->stats.point_passes += (uint64_t)m.n * calls;
}

// ---- the part of a frame both entries share ----------------------------------------------------------------------------------------
// `recs`: the n_flt 48-byte records of the frame after the entry's own front steps, `spare`: a second record array of that size.
int frame_tail(pcm_ctx* c, const char* who, char* recs, size_t n_flt, char* spare, float leaf_size, const pcm_imu_pose* poses, int npose, const pcm_lio_state* end_state,
               pcm_imu_pose* d_poses, void* scratch, size_t* n_scan) {
  hipStream_t st = c->stream;
  // ImuProcess::UndistortPcl backward loop  (imu_processing.hpp:245-285): in place on the records (time stamp = curvature)
  if (npose >= 2) {
    PCM_HIPCK(c, hipMemcpyAsync(d_poses, poses, sizeof(pcm_imu_pose) * (size_t)npose, hipMemcpyHostToDevice, st));
    int rc = undistort_device(st, recs, n_flt, 48, 36, d_poses, npose, state_of(end_state), &c->err);   // PointXYZINormal::curvature: byte 36
    if (rc != PCM_OK) return rc;
  }
  // voxel_scan_.filter()  (laser_mapping.cc:323-328); leaf 0 = no down-sampling.  The centroids go to the spare array.
  const char* d_scan = recs;
  size_t n_ds = n_flt;
  if (leaf_size > 0.f) {
    int rc = voxel_downsample_device(st, recs, n_flt, 48, leaf_size, reinterpret_cast<float*>(spare), &n_ds, scratch, &c->err);
    if (rc != PCM_OK) return rc;
    d_scan = spare;
  }
  if (n_ds == 0) { c->err = "empty scan after down-sampling"; return PCM_ERR_NO_INPUT; }
  // the down-sampled scan (scan_down_body_) becomes the source of this object: device -> device, no host copy
  if (c->cfg.flags & PCM_FLAG_LIO_REFERENCE_SEMANTICS) {   // one resize of residuals_ / point_selected_surf_ per frame  laser_mapping.cc:335-339
    int rc = lio_members_resize(c, n_ds);
    if (rc != PCM_OK) return rc;
  }
  int rc = set_cloud(c, &c->src, d_scan, n_ds, 48, PCM_MEM_DEVICE, 0, false);
  if (rc != PCM_OK) return rc;
  source_replaced(c, who);
  c->user_cov_src.clear();
  c->lio_frame.set(recs, n_flt, d_scan, n_ds);   // scan_undistort_ and scan_down_body_, for the frame outputs (lio_outputs.hip)
  *n_scan = n_ds;
  return PCM_OK;
}

}  // namespace

extern "C" {

// ImuProcess::UndistortPcl backward propagation  (jueying_lio/include/imu_processing.hpp:245-285)
int pcm_undistort(pcm_ctx* c, void* points, size_t n, size_t stride, size_t time_off, int memory, const pcm_imu_pose* poses, int npose, const pcm_lio_state* st) {
  CHECK_CTX(c);
  if ((!points && n) || !poses || !st || npose < 0) return PCM_ERR_INVALID_ARGUMENT;
  if (stride < 16 || (stride % 4) != 0 || time_off + 4 > stride || (time_off % 4) != 0) { c->err = "bad record layout"; return PCM_ERR_INVALID_ARGUMENT; }
  if (n == 0 || npose < 2) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  UndistortArena U;   // arena: [IMU poses | staged points]
  int rc = carve_pre_arena(c, "pcm_undistort", [&](ArenaStage& a) { U = undistort_layout(a, poses, npose, memory, points, n * stride); });
  if (rc != PCM_OK) return rc;
  rc = undistort_device(c->stream, U.pts, n, stride, time_off, U.poses, npose, state_of(st), &c->err);
  if (rc != PCM_OK) return rc;
  if ((rc = stage_back(c, memory, points, U.pts, n * stride)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

int pcm_obs_model(pcm_ctx* c, const pcm_lio_state* s, int extrinsic_est_en, int rematch, pcm_obs_result* out) {
  CHECK_CTX(c);
  if (!s || !out) return PCM_ERR_INVALID_ARGUMENT;
  if (c->cfg.model != PCM_MODEL_P2PLANE) { c->err = "pcm_obs_model needs the P2PLANE model"; return PCM_ERR_INVALID_ARGUMENT; }
  int rc = validate_config(c, c->cfg);
  if (rc != PCM_OK) return rc;
  // refused on the host, in front of any build or launch: the planes on the device are those of another scan or target
  if (!rematch && !c->lio_planes_valid) { c->err = "pcm_obs_model(rematch=0) before any matching call"; return PCM_ERR_INVALID_ARGUMENT; }
  rc = prepare(c);
  if (rc != PCM_OK) return rc;
  iekf::State x{};
  for (int a = 0; a < 4; a++) { x.rot[a] = s->rot[a]; x.off_R[a] = s->off_R[a]; }
  for (int a = 0; a < 3; a++) { x.pos[a] = s->pos[a]; x.off_T[a] = s->off_T[a]; }
  Match m;
  PairDesc d;
  PairState ps;
  rc = match_setup(c, x, extrinsic_est_en, rematch, &d, &ps, &m);
  if (rc != PCM_OK) return rc;
  Workspace* w = m.w;
  hipStream_t st = c->stream;
  PCM_HIPCK(c, hipMemcpyAsync(w->d_descs, &d, sizeof(d), hipMemcpyHostToDevice, st));
  PCM_HIPCK(c, hipMemcpyAsync(w->d_states, &ps, sizeof(ps), hipMemcpyHostToDevice, st));
  if (m.on_lists) launch_lio_lists(st, w->d_descs, w->d_states, m.kp, m.pooled, false);
  else launch_lio_obs(st, w->d_descs, w->d_states, m.kp);
  launch_lio_finish(st, w->d_partials, m.tiles, w->d_sums);
  PCM_HIPCK(c, hipGetLastError());
  double sums[kLioStride];
  PCM_HIPCK(c, hipMemcpyAsync(sums, w->d_sums, sizeof(double) * kLioStride, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipStreamSynchronize(st));
  match_record(c, m, rematch != 0, rematch ? 1 : 0, 1, &m.pose);
  int t = 0;
  for (int a = 0; a < 12; a++) for (int b = a; b < 12; b++) { out->HTH[a * 12 + b] = sums[t]; out->HTH[b * 12 + a] = sums[t]; t++; }
  for (int a = 0; a < 12; a++) out->HTh[a] = sums[78 + a];
  out->sum_h2 = sums[90];
  out->n_eff = (int32_t)sums[91];
  out->valid = out->n_eff >= 1 ? 1 : 0;
  return PCM_OK;
}

void pcm_lio_default_update_params(pcm_lio_update_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->R = 0.001;        // options.h:12 LASER_POINT_COV
  p->max_iter = 4;     // laser_mapping.cc:89
  for (int k = 0; k < 23; k++) p->limit[k] = 0.001;   // laser_mapping.cc:19
}

// esekf::update_iterated_dyn_share_modified on the device (lio_iekf.h, lio_iekf.hip): the rounds are queued up front, the host waits once
int pcm_lio_update(pcm_ctx* c, const pcm_lio_update_params* prm, pcm_lio_filter_state* x, double* P, pcm_lio_update_result* res) {
  CHECK_CTX(c);
  if (!prm || !x || !P || !res) { c->err = "pcm_lio_update: null argument"; return PCM_ERR_INVALID_ARGUMENT; }
  if (c->cfg.model != PCM_MODEL_P2PLANE) { c->err = "pcm_lio_update needs the P2PLANE model"; return PCM_ERR_INVALID_ARGUMENT; }
  if (prm->max_iter < 1 || prm->max_iter + 1 > iekf::kMaxCalls) { c->err = "pcm_lio_update: max_iter must be in 1 .. 15"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(prm->R > 0.0) || !std::isfinite(prm->R)) { c->err = "pcm_lio_update: R must be positive and finite"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int k = 0; k < iekf::N; k++)
    if (!(prm->limit[k] >= 0.0)) { c->err = "pcm_lio_update: limit must not be negative or NaN"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int k = 0; k < iekf::NN; k++)
    if (!std::isfinite(P[k])) { c->err = "pcm_lio_update: P is not finite"; return PCM_ERR_INVALID_ARGUMENT; }
  {
    const double* xs = reinterpret_cast<const double*>(x);
    for (size_t k = 0; k < sizeof(*x) / sizeof(double); k++)
      if (!std::isfinite(xs[k])) { c->err = "pcm_lio_update: the state is not finite"; return PCM_ERR_INVALID_ARGUMENT; }
  }
  int rc = validate_config(c, c->cfg);
  if (rc != PCM_OK) return rc;
  rc = prepare(c);
  if (rc != PCM_OK) return rc;
  // the record of the update: its pinned host image is filled here and uploaded up to b.tr
  rc = c->lio_upd.reserve(c, sizeof(LioUpdateRecord), sizeof(LioUpdateRecord));
  if (rc != PCM_OK) return rc;
  rc = c->lio_upd_host.reserve(c, sizeof(LioUpdateRecord), sizeof(LioUpdateRecord));
  if (rc != PCM_OK) return rc;
  c->lio_upd_calls = 0;
  LioUpdateRecord* h = reinterpret_cast<LioUpdateRecord*>(c->lio_upd_host.p);
  LioUpdateRecord* dv = reinterpret_cast<LioUpdateRecord*>(c->lio_upd.p);
  std::memcpy(&h->b.x_prop, x, sizeof(iekf::State));
  std::memcpy(h->b.P_prop, P, sizeof(double) * iekf::NN);
  h->b.prm.R = prm->R;
  h->b.prm.max_iter = prm->max_iter;
  h->b.prm.extrinsic = prm->extrinsic_est_en ? 1 : 0;
  for (int k = 0; k < iekf::N; k++) h->b.prm.limit[k] = prm->limit[k];
  iekf::begin(h->b);
  Match m;
  rc = match_setup(c, h->b.x, prm->extrinsic_est_en, 1, &h->desc, &h->ps, &m);   // a new scan is ordered at the propagated state's pose
  if (rc != PCM_OK) return rc;
  h->desc.lio.rematch = 1;   // dyn_share.converge = true  esekfom.hpp:1529
  Workspace* w = m.w;
  hipStream_t st = c->stream;
  const int rounds = prm->max_iter + 1;
  PCM_HIPCK(c, hipMemcpyAsync(dv, h, offsetof(LioUpdateRecord, b) + offsetof(iekf::Block, tr), hipMemcpyHostToDevice, st));
  for (int r = 0; r < rounds; r++) {
    if (m.on_lists) launch_lio_lists(st, &dv->desc, &dv->ps, m.kp, m.pooled, true);
    else launch_lio_obs_dev(st, &dv->desc, &dv->ps, m.kp);
    launch_lio_finish_gated(st, dv, w->d_partials, m.tiles, w->d_sums);
    launch_iekf_step(st, dv, w->d_sums);
  }
  PCM_HIPCK(c, hipGetLastError());
  const size_t back0 = offsetof(LioUpdateRecord, b) + offsetof(iekf::Block, x);
  const size_t back1 = offsetof(LioUpdateRecord, b) + offsetof(iekf::Block, tr) + sizeof(iekf::Trace) * (size_t)rounds;
  PCM_HIPCK(c, hipMemcpyAsync(reinterpret_cast<char*>(h) + back0, reinterpret_cast<const char*>(dv) + back0, back1 - back0, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipStreamSynchronize(st));
  const iekf::Ctl& ctl = h->b.ctl;
  c->lio_upd_calls = ctl.iterations;
  iekf::PoseF last{};   // the state of the last executed ObsModel call
  const bool have_last = ctl.iterations >= 1 && ctl.iterations <= iekf::kMaxCalls;
  if (have_last) iekf::pose_of(h->b.tr[ctl.iterations - 1].x, &last);
  // the first call of the loop always matches
  match_record(c, m, true, (uint64_t)std::max(ctl.rematches, 0), (uint64_t)ctl.iterations, have_last ? &last : nullptr);
  std::memcpy(x, &h->b.x, sizeof(iekf::State));
  std::memcpy(P, h->b.P, sizeof(double) * iekf::NN);
  std::memset(res, 0, sizeof(*res));
  res->iterations = ctl.iterations;
  res->rematches = ctl.rematches;
  res->valid_calls = ctl.valid_calls;
  res->t = ctl.t;
  res->n_eff_last = ctl.n_eff_last;
  res->sum_h2_last = ctl.sum_h2_last;
  res->status = PCM_OK;
  bool finite = true;
  for (int k = 0; k < iekf::NN; k++) finite = finite && std::isfinite(P[k]);
  for (size_t k = 0; k < sizeof(*x) / sizeof(double); k++) finite = finite && std::isfinite(reinterpret_cast<const double*>(x)[k]);
  if (!finite || !ctl.done) {
    c->err = !ctl.done ? "pcm_lio_update: the loop did not reach its end" : "pcm_lio_update: the updated state or covariance is not finite";
    res->status = PCM_ERR_INTERNAL;
    return PCM_ERR_INTERNAL;
  }
  return PCM_OK;
}

int pcm_lio_update_trace(pcm_ctx* c, int call, pcm_lio_filter_state* x, int32_t* converge, int32_t* n_eff, double* sums90, double* dx23) {
  CHECK_CTX(c);
  if (call < 0 || call >= c->lio_upd_calls || !c->lio_upd_host.p) { c->err = "pcm_lio_update_trace: no such call of the last pcm_lio_update"; return PCM_ERR_INVALID_ARGUMENT; }
  const iekf::Trace& t = reinterpret_cast<const LioUpdateRecord*>(c->lio_upd_host.p)->b.tr[call];
  if (x) std::memcpy(x, &t.x, sizeof(iekf::State));
  if (converge) *converge = t.converge;
  if (n_eff) *n_eff = t.n_eff;
  if (sums90) std::memcpy(sums90, t.sums, sizeof(t.sums));
  if (dx23) std::memcpy(dx23, t.dx, sizeof(t.dx));
  return PCM_OK;
}

int pcm_map_incremental(pcm_ctx* c, const pcm_lio_state* s, float filter_size_map, int ekf_inited, size_t* num_added) {
  CHECK_CTX(c);
  if (!s) return PCM_ERR_INVALID_ARGUMENT;
  if (c->tg.shared()) return refuse_shared(c, "pcm_map_incremental");
  if (c->src.n == 0) { c->err = "pcm_map_incremental without a source scan"; return PCM_ERR_NO_INPUT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  const uint32_t n = (uint32_t)c->src.n;
  int rc = reserve_target(c, c->tg->tgt.n + n);
  if (rc != PCM_OK) return rc;
  // nearest_points_ of the last matching call: positions in the map's point array (the tile kernel) or in the list entries
  // (k_lio_lists), the latter only while no update or rebuild has moved them since
  const pcm::NeighbourLists& nl = c->tg->nlists;
  const bool nn_current = !c->nn_in_lists || (nl.valid && nl.kind == 0 && !nl.stale && nl.generation == c->nn_lists_generation);
  const bool have_nn = c->lio_planes_valid && c->nn != nullptr && c->tg->map.valid && ekf_inited && nn_current;
  const float4* nn_pts = c->nn_in_lists ? nl.pts.p : c->tg->map.pts.p;
  const bool reordered = c->cfg.sort_source && c->src_sorted;
  const float4* scan = reordered ? c->src_order : c->src.d_pts;
  uint32_t added = 0;
  rc = map_incremental_device(c->stream, scan, reordered, n, state_of(s), filter_size_map, have_nn ? c->nn : nullptr, have_nn ? nn_pts : nullptr, c->tg->next_seq,
                              c->tg->tgt.d_pts + c->tg->tgt.n, &added, &c->err);
  if (rc != PCM_OK) return rc;
  c->tg->tgt.n += added;
  c->tg->next_seq += added;
  c->tg->tgt.tag = 0;
  if (added) { c->tg->map.valid = false; c->tg->tgt_dynamic = true; }
  if (num_added) *num_added = added;
  return PCM_OK;
}

// ---------------------------------------------------------------------------
// One LiDAR frame of LaserMapping::Run on device buffers (jueying_lio/src/laser_mapping.cc:323-347 front end, :525-583 back end).
// ---------------------------------------------------------------------------
int pcm_lio_frame_begin(pcm_ctx* c, const void* custom_points, size_t n, int memory, const pcm_lio_frame_params* prm, const pcm_imu_pose* poses, int npose,
                        const pcm_lio_state* end_state, size_t* n_scan) {
  CHECK_CTX(c);
  if ((!custom_points && n) || !prm || !n_scan || (npose >= 2 && (!poses || !end_state))) return PCM_ERR_INVALID_ARGUMENT;
  if (n > 0xffffffffull) { c->err = "too many points"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(prm->leaf_size >= 0.f)) { c->err = "leaf_size must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  *n_scan = 0;
  if (n == 0) { c->err = "empty frame"; return PCM_ERR_NO_INPUT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  // grow-only, so the steady state makes no allocation
  const size_t livox_bytes = livox_filter_scratch_bytes(n), vg_bytes = voxel_downsample_scratch_bytes(n);
  FrameArena F;
  int rc = carve_pre_arena(c, "pcm_lio_frame_begin", [&](ArenaStage& a) { F = frame_layout(a, memory, custom_points, n * 20, true, n, npose, {livox_bytes, vg_bytes}); });
  if (rc != PCM_OK) return rc;
  char *flt = F.rec[0], *ds = F.rec[1];
  // 1. PointCloudPreprocess::AviaHandler  (pointcloud_preprocess.cc:44-88)
  size_t n_flt = 0;
  rc = livox_filter_device(st, F.raw, n, prm->num_scans, prm->point_filter_num, prm->blind, flt, &n_flt, F.scratch, &c->err);
  if (rc != PCM_OK) return rc;
  if (n_flt == 0) { c->err = "no point of the frame passed the driver-message filter"; return PCM_ERR_NO_INPUT; }
  // 2.-4. motion compensation, down-sampling, the scan becomes the source.  The reference sorts the scan by time first
  //    (imu_processing.hpp:177-178); a Livox message is time-ordered, and the compensation of a point depends on its own stamp
  //    only, so the message order is kept.
  return frame_tail(c, "pcm_lio_frame_begin", flt, n_flt, ds, prm->leaf_size, poses, npose, end_state, F.poses, F.scratch, n_scan);
}

// The same frame for a sensor_msgs::PointCloud2 cloud: the handler of its LiDAR type (pointcloud_preprocess.cc:89-305) in front, and
// the time sort of ImuProcess::UndistortPcl (imu_processing.hpp:177-178) made definite: (curvature, input index).
int pcm_lio_frame_begin_cloud(pcm_ctx* c, const void* points, size_t n, int memory, const pcm_lidar_desc* desc, float leaf_size, const pcm_imu_pose* poses, int npose,
                              const pcm_lio_state* end_state, size_t* n_scan) {
  CHECK_CTX(c);
  if (!n_scan || (npose >= 2 && (!poses || !end_state))) return PCM_ERR_INVALID_ARGUMENT;
  *n_scan = 0;
  int rc = lidar_check_cloud(c, points, n, memory, desc);
  if (rc != PCM_OK) return rc;
  if (!(leaf_size >= 0.f)) { c->err = "leaf_size must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (n == 0) { c->err = "empty frame"; return PCM_ERR_NO_INPUT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t filter_bytes = lidar_filter_scratch_bytes(n), sort_bytes = lidar_time_sort_scratch_bytes(n), vg_bytes = voxel_downsample_scratch_bytes(n);
  FrameArena F;
  rc = carve_pre_arena(c, "pcm_lio_frame_begin_cloud", [&](ArenaStage& a) { F = frame_layout(a, memory, points, n * desc->stride_bytes, false, n, npose, {filter_bytes, sort_bytes, vg_bytes}); });
  if (rc != PCM_OK) return rc;
  char *flt = F.rec[0], *srt = F.rec[1];   // the filtered records, later the down-sampled ones; the time-sorted records
  const int hint = memory == PCM_MEM_HOST ? lidar_given_on_host(points, n, *desc) : -1;
  // 1. the handler: kept points in input order
  size_t n_flt = 0;
  int given = 1;
  rc = lidar_filter_device(st, F.raw, n, *desc, hint, flt, n, &n_flt, &given, F.scratch, &c->err);
  if (rc != PCM_OK) return rc;
  if (n_flt == 0) { c->err = "no point of the frame passed the handler"; return PCM_ERR_NO_INPUT; }
  // 2. sort by time; the radix sort is stable, so equal stamps keep their input order
  rc = lidar_time_sort_device(st, flt, n_flt, srt, F.scratch, &c->err);
  if (rc != PCM_OK) return rc;
  // 3.-5. motion compensation in place on the sorted records, down-sampling (the filtered records are free again: the centroids go
  //    there), the scan becomes the source
  return frame_tail(c, "pcm_lio_frame_begin_cloud", srt, n_flt, flt, leaf_size, poses, npose, end_state, F.poses, F.scratch, n_scan);
}

int pcm_lio_frame_end(pcm_ctx* c, const pcm_lio_state* s, float filter_size_map, int ekf_inited, size_t* num_added) {
  CHECK_CTX(c);
  if (c->tg.shared()) return refuse_shared(c, "pcm_lio_frame_end");
  return pcm_map_incremental(c, s, filter_size_map, ekf_inited, num_added);
}

int pcm_get_lio_members(pcm_ctx* c, float* residuals, uint8_t* selected, size_t n) {
  CHECK_CTX(c);
  if (!(c->cfg.flags & PCM_FLAG_LIO_REFERENCE_SEMANTICS) || !c->lio_aux || n != c->lio_aux_n || n != c->src.n) {
    c->err = "pcm_get_lio_members: needs PCM_FLAG_LIO_REFERENCE_SEMANTICS and n equal to the source size";
    return PCM_ERR_INVALID_ARGUMENT;
  }
  std::vector<float2> tmp(n);
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  if (n) PCM_HIPCK(c, hipMemcpy(tmp.data(), c->lio_aux, sizeof(float2) * n, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) {
    if (residuals) residuals[i] = tmp[i].x;
    if (selected) selected[i] = tmp[i].y != 0.f ? 1 : 0;
  }
  return PCM_OK;
}

int pcm_lio_search_path(pcm_ctx* c, uint64_t counts[2]) {
  if (!c || !counts) return PCM_ERR_INVALID_ARGUMENT;
  counts[0] = c->lio_search_path[0];
  counts[1] = c->lio_search_path[1];
  return PCM_OK;
}

}  // extern "C"
