// loam_loop.hip -- loop verification on the device (include/pcm_amd.h, pcm_loam_loop_*): jueying_slam's performLoopClosure
// (mapOptmization.cpp:619-733) from a detected pair of key frames to the loop factor.
//
// The live verifier of that function is pclomp::NormalDistributionsTransform (:683-697; the PCL ICP block is commented out), an
// operator this library has (pclndt.hip and its solver), so a verification is a composition: the two near-key-frame clouds are
// queued on the context's stream into device memory (loam_submap.hip's near pass: pcm_loam_submap_near's clouds),
// ONE wait brings their two counts back for the size gates (:652), and the clouds go as PCM_MEM_DEVICE buffers to a verifier
// context -- a PCM_MODEL_NDT_OMP pcm_ctx the LOAM context owns, created by the first verification that gets this far, run on the
// LOAM context's stream and released with it -- through the public pcm_set_target / pcm_set_source / pcm_align /
// pcm_fitness_score, whose code is unchanged.  What the caller used to write by hand, the acceptance test (:693) and the
// Eigen / GTSAM pose algebra of :706-725, is loam_loop.h, evaluated on the host.  Nothing of the LOAM context's own target, source,
// key-frame store or Scan Context store is written.
//
// performSCLoopClosure (:735-841), the Scan Context half of the loop thread, is the same composition with the other operator:
// both clouds under key frame 0's pose (:757-759), pcl::IterativeClosestPoint -- PCM_MODEL_ICP (icp.hip) in a second verifier
// context beside the NDT one -- and the factor of :817-834 (loam_loop.h's sc_loop_factor).  pcm_loam_sc_loop_*; DESIGN.md section 37.
#include "host_util.h"
#include "loam_device.h"
#include "icp.h"
#include "loam_loop.h"
#include "loam_submap.h"

#include <cfloat>
#include <cstring>

using namespace pcm;
using namespace pcm::loam;

namespace {

struct LoopStore {
  pcm_ctx* verifier = nullptr;       // pclomp NDT: performLoopClosure
  pcm_ctx* icp_verifier = nullptr;   // point-to-point ICP: performSCLoopClosure
  ~LoopStore() {
    if (verifier) pcm_destroy(verifier);
    if (icp_verifier) pcm_destroy(icp_verifier);
  }
};

int check_ctx_loop(pcm_ctx* c, LoopStore** ls) {
  return loam_check_store(c, "pcm_loam_loop_* needs a context created with PCM_MODEL_LOAM", LoamStore::loop, ls);
}

int check_lparams(pcm_ctx* c, const pcm_loam_loop_params& p) {
  if (p.history_search_num < 0) { c->err = "history_search_num must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.min_cur_points < 0 || p.min_prev_points < 0) { c->err = "min_cur_points and min_prev_points must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.near_leaf >= 0.f) || !finite_f_3e38(p.near_leaf)) { c->err = "near_leaf must be >= 0 (0: no down-sampling)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.fitness_threshold == p.fitness_threshold)) { c->err = "fitness_threshold must be a number"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.ndt_epsilon > 0.0) || !finite_d(p.ndt_epsilon)) { c->err = "ndt_epsilon must be > 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.ndt_resolution > 0.f) || !finite_f(p.ndt_resolution)) { c->err = "ndt_resolution must be > 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.ndt_num_neighbors != 0 && p.ndt_num_neighbors != 1 && p.ndt_num_neighbors != 7 && p.ndt_num_neighbors != 27) {
    c->err = "ndt_num_neighbors must be 0 (KDTREE), 1, 7 or 27"; return PCM_ERR_INVALID_ARGUMENT;
  }
  return PCM_OK;
}

// the verifier's settings: pclomp NDT's own defaults (35 iterations, step 0.1, outlier ratio 0.55: ndt_omp_impl.hpp:48,60-63)
// under the three setters of :684-686
void verifier_config(const pcm_loam_loop_params& p, pcm_config* g) {
  pcm_default_config(g);
  g->model = PCM_MODEL_NDT_OMP;
  g->max_iterations = 35;
  g->translation_eps = p.ndt_epsilon;
  g->voxel_resolution = p.ndt_resolution;
  g->num_neighbors = p.ndt_num_neighbors;
}

int ensure_verifier(pcm_ctx* c, LoopStore* S, const pcm_loam_loop_params& p) {
  pcm_config g;
  verifier_config(p, &g);
  if (!S->verifier) {
    pcm_ctx* v = pcm_create(c->device, &g);
    if (!v) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
    if (v->device < 0) { c->err = "loop verifier: " + v->err; pcm_destroy(v); return PCM_ERR_HIP; }
    S->verifier = v;
  }
  pcm_ctx* v = S->verifier;
  if (v->stream != c->stream) {   // every step of a verification runs on the LOAM context's stream
    const int rc = pcm_set_stream(v, c->stream);
    if (rc != PCM_OK) { c->err = "loop verifier: " + v->err; return rc; }
  }
  if (std::memcmp(&v->cfg, &g, sizeof(g)) != 0) {
    const int rc = pcm_set_config(v, &g);
    if (rc != PCM_OK) { c->err = "loop verifier: " + v->err; return rc; }
  }
  return PCM_OK;
}

void clear_result(pcm_loam_loop_result* r, int key_cur, int key_pre) {
  std::memset(r, 0, sizeof(*r));
  r->key_cur = key_cur; r->key_pre = key_pre;
  r->correction[0] = r->correction[5] = r->correction[10] = r->correction[15] = 1.f;
}

int verify(pcm_ctx* c, LoopStore* S, const pcm_loam_loop_params& p, int key_cur, int key_pre, pcm_loam_loop_result* out) {
  const KeyPose* kp = nullptr;
  const int K = loam_keyposes(c, &kp);
  if (K <= 0) { c->err = "pcm_loam_loop_verify: the key-frame store is empty"; return PCM_ERR_INVALID_ARGUMENT; }
  if (key_cur < 0 || key_cur >= K || key_pre < 0 || key_pre >= K) { c->err = "pcm_loam_loop_verify: key outside [0, K)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.wrt_key >= K) { c->err = "pcm_loam_loop_verify: wrt_key outside [0, K)"; return PCM_ERR_INVALID_ARGUMENT; }
  float pose_cur[6], pose_pre[6];
  if (!loam_keyframe_pose(c, key_cur, pose_cur) || !loam_keyframe_pose(c, key_pre, pose_pre)) { c->err = "pcm_loam_loop_verify: no such key frame"; return PCM_ERR_INTERNAL; }
  pcm_loam_loop_result r;
  clear_result(&r, key_cur, key_pre);
  // :650-651 loopFindNearKeyframes(cure, loopKeyCur, 0) and (prev, loopKeyPre, historyKeyframeSearchNum), both queued, one wait
  NearCloud cur{}, prev{};
  int rc = loam_near_queue(c, 0, key_cur, 0, p.wrt_key, p.near_leaf, &cur);
  if (rc != PCM_OK) return rc;
  if ((rc = loam_near_queue(c, 1, key_pre, p.history_search_num, p.wrt_key, p.near_leaf, &prev)) != PCM_OK) return rc;
  if (cur.pts || prev.pts) {
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));
    loam_near_waited(c);
  }
  if ((cur.pts && cur.h_small[2]) || (prev.pts && prev.h_small[2])) { c->err = "near_leaf too small for the extent of the cloud (index overflow)"; return PCM_ERR_OUT_OF_RANGE; }
  const uint32_t n_cur = cur.pts ? cur.h_small[0] : 0u, n_prev = prev.pts ? prev.h_small[0] : 0u;
  r.num_cur_points = (int32_t)n_cur;
  r.num_prev_points = (int32_t)n_prev;
  if (!loop::size_gate(n_cur, n_prev, p.min_cur_points, p.min_prev_points) || n_cur == 0 || n_prev == 0) {   // :652 (an empty cloud cannot be registered)
    r.status = PCM_LOAM_LOOP_REJECTED_SIZE;
    *out = r;
    return PCM_OK;
  }
  if ((rc = ensure_verifier(c, S, p)) != PCM_OK) return rc;
  pcm_ctx* v = S->verifier;
  // :688-691 setInputSource(cure), setInputTarget(prev), align(*unused): no guess = the identity
  const float I[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  pcm_result ar;
  std::memset(&ar, 0, sizeof(ar));
  double fitness = 0.0;
  rc = pcm_set_target(v, prev.pts, n_prev, sizeof(float4), PCM_MEM_DEVICE, 0);
  if (rc == PCM_OK) rc = pcm_set_source(v, cur.pts, n_cur, sizeof(float4), PCM_MEM_DEVICE, 0);   // used in place: the workspace outlives the call
  if (rc == PCM_OK) { rc = pcm_align(v, I, &ar); if (rc == PCM_ERR_NOT_CONVERGED) rc = PCM_OK; }
  if (rc == PCM_OK) rc = pcm_fitness_score(v, ar.T, DBL_MAX, &fitness);   // :693 getFitnessScore(): max_range = the largest double
  (void)pcm_clear_source(v);   // the verifier keeps no pointer into the workspace
  if (rc != PCM_OK) { c->err = "loop verifier: " + v->err; return rc; }
  r.ndt_iterations = ar.iterations;
  r.ndt_converged = ar.converged;
  r.fitness = fitness;
  r.noise_variance = (float)fitness;   // :719
  std::memcpy(r.correction, ar.T, sizeof(r.correction));
  r.status = loop::accept_status(ar.converged, fitness, p.fitness_threshold);
  if (r.status == PCM_LOAM_LOOP_ACCEPTED) loop::loop_factor(r.correction, pose_cur, pose_pre, r.pose_from, r.pose_to, r.between, r.between6);
  *out = r;
  return PCM_OK;
}

// ---- performSCLoopClosure (mapOptmization.cpp:735-841) ---------------------------------------------------------------------------
int check_scparams(pcm_ctx* c, const pcm_loam_sc_loop_params& p) {
  if (p.history_search_num < 0) { c->err = "history_search_num must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.min_cur_points < 0 || p.min_prev_points < 0) { c->err = "min_cur_points and min_prev_points must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.near_leaf >= 0.f) || !finite_f_3e38(p.near_leaf)) { c->err = "near_leaf must be >= 0 (0: no down-sampling)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.fitness_threshold == p.fitness_threshold)) { c->err = "fitness_threshold must be a number"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.icp_max_iterations < 1 || p.icp_max_iterations > (1 << 20)) { c->err = "icp_max_iterations must be in [1, 2^20]"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.icp_max_correspondence_distance > 0.0)) { c->err = "icp_max_correspondence_distance must be > 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.icp_transformation_epsilon != p.icp_transformation_epsilon || p.icp_euclidean_fitness_epsilon != p.icp_euclidean_fitness_epsilon) {
    c->err = "the ICP epsilons must be numbers"; return PCM_ERR_INVALID_ARGUMENT;
  }
  if (!(p.icp_voxel_resolution > 0.f) || !finite_f(p.icp_voxel_resolution)) { c->err = "icp_voxel_resolution must be > 0"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

// the ICP verifier: PCL's defaults under the four setters of :769-772
int ensure_icp_verifier(pcm_ctx* c, LoopStore* S, const pcm_loam_sc_loop_params& p) {
  pcm_config g;
  pcm_default_config(&g);
  g.model = PCM_MODEL_ICP;
  g.voxel_resolution = p.icp_voxel_resolution;
  if (!S->icp_verifier) {
    pcm_ctx* v = pcm_create(c->device, &g);
    if (!v) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
    if (v->device < 0) { c->err = "SC loop verifier: " + v->err; pcm_destroy(v); return PCM_ERR_HIP; }
    S->icp_verifier = v;
  }
  pcm_ctx* v = S->icp_verifier;
  int rc = PCM_OK;
  if (v->stream != c->stream) rc = pcm_set_stream(v, c->stream);   // every step of a verification runs on the LOAM context's stream
  if (rc == PCM_OK && std::memcmp(&v->cfg, &g, sizeof(g)) != 0) rc = pcm_set_config(v, &g);
  if (rc == PCM_OK) {
    pcm_icp_params ip;
    pcm_icp_default_params(&ip);
    ip.max_correspondence_distance = p.icp_max_correspondence_distance;   // :769
    ip.max_iterations = p.icp_max_iterations;                              // :770
    ip.transformation_epsilon = p.icp_transformation_epsilon;              // :771
    ip.euclidean_fitness_epsilon = p.icp_euclidean_fitness_epsilon;        // :772
    rc = pcm_icp_set_params(v, &ip);
  }
  if (rc != PCM_OK) c->err = "SC loop verifier: " + v->err;
  return rc;
}

void clear_sc_result(pcm_loam_sc_loop_result* r, int key_cur, int key_pre) {
  std::memset(r, 0, sizeof(*r));
  r->key_cur = key_cur; r->key_pre = key_pre;
  r->correction[0] = r->correction[5] = r->correction[10] = r->correction[15] = 1.f;
  r->noise_variance = icp::kScNoiseVariance;
  r->cauchy_k = icp::kScCauchyK;
}

int sc_verify(pcm_ctx* c, LoopStore* S, const pcm_loam_sc_loop_params& p, int key_cur, int key_pre, float yaw_diff, pcm_loam_sc_loop_result* out) {
  const KeyPose* kp = nullptr;
  const int K = loam_keyposes(c, &kp);
  if (K <= 0) { c->err = "pcm_loam_sc_loop_verify: the key-frame store is empty"; return PCM_ERR_INVALID_ARGUMENT; }
  if (key_cur < 0 || key_cur >= K || key_pre < 0 || key_pre >= K) { c->err = "pcm_loam_sc_loop_verify: key outside [0, K)"; return PCM_ERR_INVALID_ARGUMENT; }
  pcm_loam_sc_loop_result r;
  clear_sc_result(&r, key_cur, key_pre);
  r.yaw_diff_rad = yaw_diff;
  // :757-759 both clouds under key frame 0 (base_key), both queued, one wait
  NearCloud cur{}, prev{};
  int rc = loam_near_queue(c, 0, key_cur, 0, 0, p.near_leaf, &cur);
  if (rc != PCM_OK) return rc;
  if ((rc = loam_near_queue(c, 1, key_pre, p.history_search_num, 0, p.near_leaf, &prev)) != PCM_OK) return rc;
  if (cur.pts || prev.pts) {
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));
    loam_near_waited(c);
  }
  if ((cur.pts && cur.h_small[2]) || (prev.pts && prev.h_small[2])) { c->err = "near_leaf too small for the extent of the cloud (index overflow)"; return PCM_ERR_OUT_OF_RANGE; }
  const uint32_t n_cur = cur.pts ? cur.h_small[0] : 0u, n_prev = prev.pts ? prev.h_small[0] : 0u;
  r.num_cur_points = (int32_t)n_cur;
  r.num_prev_points = (int32_t)n_prev;
  if (!loop::size_gate(n_cur, n_prev, p.min_cur_points, p.min_prev_points) || n_cur == 0 || n_prev == 0) {   // :761
    r.status = PCM_LOAM_LOOP_REJECTED_SIZE;
    *out = r;
    return PCM_OK;
  }
  if ((rc = ensure_icp_verifier(c, S, p)) != PCM_OK) return rc;
  pcm_ctx* v = S->icp_verifier;
  // :776-779 setInputSource(cure), setInputTarget(prev), align(*unused): no guess = the identity
  const float I[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  pcm_result ar;
  std::memset(&ar, 0, sizeof(ar));
  pcm_icp_info info;
  std::memset(&info, 0, sizeof(info));
  double fitness = 0.0;
  rc = pcm_set_target(v, prev.pts, n_prev, sizeof(float4), PCM_MEM_DEVICE, 0);
  if (rc == PCM_OK) rc = pcm_set_source(v, cur.pts, n_cur, sizeof(float4), PCM_MEM_DEVICE, 0);   // used in place: the workspace outlives the call
  if (rc == PCM_OK) rc = pcm_align(v, I, &ar);
  if (rc == PCM_OK) rc = pcm_icp_last(v, &info);
  if (rc == PCM_OK) rc = pcm_fitness_score(v, ar.T, DBL_MAX, &fitness);   // :783 getFitnessScore(): max_range = the largest double
  (void)pcm_clear_source(v);   // the verifier keeps no pointer into the workspace
  if (rc != PCM_OK) { c->err = "SC loop verifier: " + v->err; return rc; }
  r.icp_iterations = ar.iterations;
  r.icp_converged = ar.converged;
  r.icp_stop_reason = info.stop_reason;
  r.fitness = fitness;
  std::memcpy(r.correction, ar.T, sizeof(r.correction));
  r.status = loop::accept_status(ar.converged, fitness, p.fitness_threshold);   // :783
  if (r.status == PCM_LOAM_LOOP_ACCEPTED) loop::sc_loop_factor(r.correction, r.pose_from, r.pose_to, r.between, r.between6);
  *out = r;
  return PCM_OK;
}

static_assert(PCM_LOAM_LOOP_ACCEPTED == loop::kAccepted && PCM_LOAM_LOOP_REJECTED_SIZE == loop::kRejectedSize && PCM_LOAM_LOOP_REJECTED_NOT_CONVERGED == loop::kRejectedNotConverged &&
                  PCM_LOAM_LOOP_REJECTED_FITNESS == loop::kRejectedFitness && PCM_LOAM_LOOP_NONE == loop::kNoLoop,
              "status codes");

}  // namespace

extern "C" {

void pcm_loam_default_loop_params(pcm_loam_loop_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->history_search_num = 25;    // utility.h:290
  p->min_cur_points = 300;       // mapOptmization.cpp:652
  p->min_prev_points = 1000;     // mapOptmization.cpp:652
  p->wrt_key = -1;               // :650-651 loopFindNearKeyframes
  p->fitness_threshold = 0.3f;   // utility.h:291
  p->near_leaf = 0.2f;           // mapOptmization.cpp:243 (utility.h:272)
  p->ndt_epsilon = 0.01;         // mapOptmization.cpp:684
  p->ndt_resolution = 1.0f;      // mapOptmization.cpp:685
  p->ndt_num_neighbors = 7;      // mapOptmization.cpp:686 DIRECT7
}

int pcm_loam_loop_verify(pcm_ctx* c, const pcm_loam_loop_params* params, int key_cur, int key_pre, pcm_loam_loop_result* result) {
  LoopStore* S = nullptr;
  int rc = check_ctx_loop(c, &S);
  if (rc != PCM_OK) return rc;
  if (!result) { c->err = "null result"; return PCM_ERR_INVALID_ARGUMENT; }
  pcm_loam_loop_params p;
  if (params) p = *params; else pcm_loam_default_loop_params(&p);
  if ((rc = check_lparams(c, p)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipSetDevice(c->device));
  return verify(c, S, p, key_cur, key_pre, result);
}

int pcm_loam_loop_closure(pcm_ctx* c, const pcm_loam_loop_params* params, float radius, double time_diff_s, double time_cur, pcm_loam_loop_result* result) {
  LoopStore* S = nullptr;
  int rc = check_ctx_loop(c, &S);
  if (rc != PCM_OK) return rc;
  if (!result) { c->err = "null result"; return PCM_ERR_INVALID_ARGUMENT; }
  pcm_loam_loop_params p;
  if (params) p = *params; else pcm_loam_default_loop_params(&p);
  if ((rc = check_lparams(c, p)) != PCM_OK) return rc;
  int32_t key_cur = -1, key_pre = -1;
  rc = pcm_loam_loop_detect_distance(c, radius, time_diff_s, time_cur, &key_cur, &key_pre);   // :638
  if (rc < 0) return rc;
  if (rc == 0) {   // :641-643
    clear_result(result, -1, -1);
    result->status = PCM_LOAM_LOOP_NONE;
    return PCM_OK;
  }
  PCM_HIPCK(c, hipSetDevice(c->device));
  return verify(c, S, p, key_cur, key_pre, result);
}

void pcm_loam_default_sc_loop_params(pcm_loam_sc_loop_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->history_search_num = 25;                     // utility.h:290
  p->min_cur_points = 300;                        // mapOptmization.cpp:761
  p->min_prev_points = 1000;                      // mapOptmization.cpp:761
  p->icp_max_iterations = 100;                    // :770
  p->fitness_threshold = 0.3f;                    // utility.h:291
  p->near_leaf = 0.2f;                            // mapOptmization.cpp:243 (utility.h:272)
  p->icp_max_correspondence_distance = 150.0;     // :769
  p->icp_transformation_epsilon = 1e-6;           // :771
  p->icp_euclidean_fitness_epsilon = 1e-6;        // :772
  p->icp_voxel_resolution = 1.0f;
}

int pcm_loam_sc_loop_verify(pcm_ctx* c, const pcm_loam_sc_loop_params* params, int key_cur, int key_pre, pcm_loam_sc_loop_result* result) {
  LoopStore* S = nullptr;
  int rc = check_ctx_loop(c, &S);
  if (rc != PCM_OK) return rc;
  if (!result) { c->err = "null result"; return PCM_ERR_INVALID_ARGUMENT; }
  pcm_loam_sc_loop_params p;
  if (params) p = *params; else pcm_loam_default_sc_loop_params(&p);
  if ((rc = check_scparams(c, p)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipSetDevice(c->device));
  return sc_verify(c, S, p, key_cur, key_pre, 0.f, result);
}

int pcm_loam_sc_loop_closure(pcm_ctx* c, const pcm_loam_sc_loop_params* params, pcm_loam_sc_loop_result* result) {
  LoopStore* S = nullptr;
  int rc = check_ctx_loop(c, &S);
  if (rc != PCM_OK) return rc;
  if (!result) { c->err = "null result"; return PCM_ERR_INVALID_ARGUMENT; }
  pcm_loam_sc_loop_params p;
  if (params) p = *params; else pcm_loam_default_sc_loop_params(&p);
  if ((rc = check_scparams(c, p)) != PCM_OK) return rc;
  const KeyPose* kp = nullptr;
  const int K = loam_keyposes(c, &kp);
  clear_sc_result(result, -1, -1);
  result->status = PCM_LOAM_LOOP_NONE;
  if (K <= 0 || pcm_loam_sc_count(c) <= 0) return PCM_OK;   // :737 no key pose, or no descriptor: no loop, nothing done
  pcm_loam_sc_result det;
  if ((rc = pcm_loam_sc_detect(c, nullptr, &det)) != PCM_OK) return rc;   // :741
  result->yaw_diff_rad = det.yaw_diff_rad;
  if (det.loop_id < 0) return PCM_OK;   // :745
  PCM_HIPCK(c, hipSetDevice(c->device));
  return sc_verify(c, S, p, K - 1, det.loop_id, det.yaw_diff_rad, result);   // :742-743
}

int pcm_loam_sc_loop_verifier_exists(pcm_ctx* c) {
  LoopStore* S = nullptr;
  int rc = check_ctx_loop(c, &S);
  if (rc != PCM_OK) return rc;
  return S->icp_verifier ? 1 : 0;
}

int pcm_loam_loop_verifier_exists(pcm_ctx* c) {
  LoopStore* S = nullptr;
  int rc = check_ctx_loop(c, &S);
  if (rc != PCM_OK) return rc;
  return S->verifier ? 1 : 0;
}

}  // extern "C"
