// pcm_api.hip -- the C ABI of include/pcm_amd.h: the extern "C" entry points of the registration objects and their small helpers
// (configuration check, cloud upload, the target log, the GICP-BFGS functor).  What a registration reads is built in prepare.hip;
// the batched device-resident GN/LM loop and the parity hooks (linearize / compute_error) run in align_batch.hip; the jueying_lio
// entry points are in lio_api.hip and use the helpers pcm_core.h declares from here.
#include "pcm_core.h"
#include "dev_scratch.h"
#include "pre_layouts.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>

using namespace pcm;

namespace {


// the same for the records + partial sums of a GICP-BFGS correspondence set of m pairs
int bfgs_scratch(pcm_ctx* c, size_t m) {
  const size_t need = gicp_bfgs_scratch_bytes(m);
  return c->bfgs.reserve(c, need, need + need / 4);
}

}  // namespace

int pcm::validate_config(pcm_ctx* c, const pcm_config& g) {
  if (g.model == PCM_MODEL_LOAM) { c->err = "PCM_MODEL_LOAM contexts run through the pcm_loam_* entry points"; return PCM_ERR_UNSUPPORTED; }
  if (g.model != PCM_MODEL_P2PLANE && !is_ndt(g.model) && !is_gicp(g.model) && g.model != PCM_MODEL_NDT_OMP && g.model != PCM_MODEL_ICP) { c->err = "unknown registration model"; return PCM_ERR_UNSUPPORTED; }
  if (g.model == PCM_MODEL_NDT_OMP) {
    if (g.num_neighbors == 19) { c->err = "pclomp NDT neighbourhoods are KDTREE / DIRECT1 / DIRECT7 / DIRECT26 (num_neighbors 0, 1, 7, 27)"; return PCM_ERR_INVALID_ARGUMENT; }
    if (!(g.ndt_step_size > 0.f) || !(g.ndt_outlier_ratio > 0.f) || !(g.ndt_outlier_ratio < 1.f)) { c->err = "bad ndt_step_size / ndt_outlier_ratio"; return PCM_ERR_INVALID_ARGUMENT; }
  }
  if ((is_ndt(g.model) || g.model == PCM_MODEL_VGICP || g.model == PCM_MODEL_VGICP_CUDA) && g.num_neighbors == 19) {
    c->err = "NDT / VGICP neighbourhoods are DIRECT1 / DIRECT7 / DIRECT27 (num_neighbors 1, 7, 27)"; return PCM_ERR_INVALID_ARGUMENT;
  }
  if (is_gicp(g.model)) {
    if (g.k_correspondences < 1 || g.k_correspondences > 64) { c->err = "k_correspondences must be in [1, 64]"; return PCM_ERR_INVALID_ARGUMENT; }
    if (g.regularization < PCM_REG_NONE || g.regularization > PCM_REG_PCLOMP || (g.regularization == PCM_REG_PCLOMP && g.model == PCM_MODEL_VGICP_CUDA)) { c->err = "bad regularization method"; return PCM_ERR_INVALID_ARGUMENT; }
    if (!(g.max_corr_dist > 0.f)) { c->err = "max_corr_dist must be > 0"; return PCM_ERR_INVALID_ARGUMENT; }
    if (g.voxel_mode < 0 || g.voxel_mode > 2) { c->err = "voxel_mode must be 0 (ADDITIVE), 1 (ADDITIVE_WEIGHTED) or 2 (MULTIPLICATIVE)"; return PCM_ERR_INVALID_ARGUMENT; }
  }
  if (g.covariance_method != PCM_COV_KNN) {
    if (g.covariance_method != PCM_COV_RBF_KERNEL || g.model != PCM_MODEL_VGICP_CUDA) { c->err = "covariance_method: PCM_COV_RBF_KERNEL is a mode of VGICP_CUDA (NearestNeighborMethod::GPU_RBF_KERNEL)"; return PCM_ERR_INVALID_ARGUMENT; }
    if (!(g.rbf_kernel_width > 0.f) || !(g.rbf_max_dist > 0.f)) { c->err = "rbf_kernel_width and rbf_max_dist must be > 0"; return PCM_ERR_INVALID_ARGUMENT; }
  }
  if (g.neighbor_search_radius != 0.f) {   // NeighborSearchMethod::DIRECT_RADIUS: "supported on only VGICP_CUDA" (gicp_settings.hpp:8) and NDTCuda
    if (!radius_model(g.model)) { c->err = "neighbor_search_radius (DIRECT_RADIUS) is a mode of NDT_P2D / NDT_D2D / VGICP_CUDA"; return PCM_ERR_INVALID_ARGUMENT; }
    if (!(g.neighbor_search_radius > 0.f) || g.neighbor_search_radius > 3.f) { c->err = "neighbor_search_radius must be in (0, 3] voxels"; return PCM_ERR_INVALID_ARGUMENT; }
  }
  if (g.optimizer != PCM_OPT_GAUSS_NEWTON && g.optimizer != PCM_OPT_LEVENBERG_MARQUARDT) { c->err = "bad optimizer"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(g.voxel_resolution > 0.f)) { c->err = "voxel_resolution must be > 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (g.num_neighbors != 1 && g.num_neighbors != 7 && g.num_neighbors != 19 && g.num_neighbors != 27 && !(g.model == PCM_MODEL_NDT_OMP && g.num_neighbors == 0)) {
    c->err = "num_neighbors must be 1, 7, 19 or 27"; return PCM_ERR_INVALID_ARGUMENT;
  }
  if (g.knn != 5 || g.min_knn != 3) { c->err = "knn/min_knn are the reference constants 5/3 (options.h:14-15)"; return PCM_ERR_UNSUPPORTED; }
  if (!(g.rotation_eps > 0) || !(g.translation_eps > 0)) { c->err = "epsilons must be > 0"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

int pcm::set_cloud(pcm_ctx* c, Cloud* cl, const void* points, size_t n, size_t stride, int memory, uint64_t tag, bool allow_borrow) {
  int rc = check_point_records(c, points, n, stride, memory, 0x7fffffffull, false);
  if (rc != PCM_OK) return rc;
  PCM_HIPCK(c, hipSetDevice(c->device));
  if (allow_borrow && memory == PCM_MEM_DEVICE && stride == sizeof(float4) && (reinterpret_cast<uintptr_t>(points) & 15u) == 0) {
    // a device-resident PointXYZ-layout scan is used in place (the kernels only read x,y,z):
    // like the reference's shared_ptr input, the caller keeps it alive and unchanged until align() returns
    cl->drop_buffer();
    cl->d_pts = const_cast<float4*>(static_cast<const float4*>(points));
    cl->borrowed = true;
    cl->n = n;
    cl->tag = tag;
    return PCM_OK;
  }
  if (cl->borrowed) cl->drop_buffer();
  if (n) rc = cl->own.reserve(c, n, n);
  cl->d_pts = cl->own;
  if (rc != PCM_OK) return rc;
  cl->n = n;
  cl->tag = tag;
  rc = load_points_to_device(c->stream, points, n, stride, memory, 0u, cl->d_pts, &c->err);
  if (rc != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));  // the caller may free/reuse its buffer on return
  return PCM_OK;
}

// the answer of every call that would change a target other contexts read
int pcm::refuse_shared(pcm_ctx* c, const char* call) {
  c->err = std::string(call) + ": the target is shared by " + std::to_string(c->tg.holders()) +
           " contexts and cannot be changed (pcm_set_target or pcm_clear_target gives this context a target of its own)";
  return PCM_ERR_UNSUPPORTED;
}

// grow the target point log to hold `need` points (keeps the content)
int pcm::reserve_target(pcm_ctx* c, size_t need) {
  Cloud& t = c->tg->tgt;
  if (need <= t.own.cap && !t.borrowed) return PCM_OK;
  const size_t cap = std::max(need, t.own.cap + t.own.cap / 2 + 1024);
  if (t.borrowed) {   // the caller's buffer is copied into an owned log on the first insert (own is empty until then)
    const int rc = t.own.reserve(c, need, cap);
    if (rc != PCM_OK) return rc;
    hipError_t e = t.n ? hipMemcpyAsync(t.own, t.d_pts, sizeof(float4) * t.n, hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { t.own.release(); return hip_failure(&c->err, "copy", t.own.what, e); }
    t.borrowed = false;
  } else {
    const int rc = t.own.reserve_keep(c, need, cap, t.n);
    if (rc != PCM_OK) return rc;
  }
  t.d_pts = t.own;
  return PCM_OK;
}

namespace {

// ---- the context's reference to its target (target_share.h) ---------------------------------------------------------------------
// What runs before the last reference frees a target: the device current and this context's stream drained (dev_buf.h).  The
// other contexts that held it drained their own streams when they let go (drain_before_letting_go), so nothing queued reads it.
auto target_release_hook(pcm_ctx* c) {
  return [c] {
    if (c->device < 0) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
  };
}

// this context's queued work may read the target it is about to let go of
void drain_before_letting_go(pcm_ctx* c) {
  if (c->device < 0 || !c->tg.shared()) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
}

// a holder of a shared target that sets or clears its target leaves the others alone: it goes on with an empty target of its own
int own_target_again(pcm_ctx* c) {
  if (!c->tg.shared()) return PCM_OK;
  drain_before_letting_go(c);
  if (!c->tg.renew(target_release_hook(c))) { c->err = "out of host memory"; return PCM_ERR_HIP; }
  c->src_cov_valid = false;   // computed with the parameters the old target recorded
  c->lio_planes_valid = false;
  return PCM_OK;
}

auto make_ndt_solver(pcm_ctx* c) {
  auto ev = [c](int pass, const NdtOmpParams& P, ndtomp::Eval* e) { return pclndt_eval(c, pass, P, e); };
  ndtomp::Solver<decltype(ev)> s{ev};
  s.step_size = (double)c->cfg.ndt_step_size;
  s.eps = c->cfg.translation_eps;            // transformation_epsilon_
  s.outlier_ratio = (double)c->cfg.ndt_outlier_ratio;
  s.resolution = c->cfg.voxel_resolution;
  s.max_iterations = c->cfg.max_iterations;
  s.num_neighbors = c->cfg.num_neighbors;
  return s;
}

}  // namespace

extern "C" {

int pcm_abi_version(void) { return PCM_ABI_VERSION; }

void pcm_default_config(pcm_config* cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->model = PCM_MODEL_P2PLANE;
  cfg->optimizer = PCM_OPT_LEVENBERG_MARQUARDT;
  cfg->max_iterations = 64;
  cfg->lm_max_iterations = 10;
  cfg->rotation_eps = 2e-3;
  cfg->translation_eps = 5e-4;
  cfg->lm_init_lambda_factor = 1e-9;
  cfg->voxel_resolution = 0.5f;
  cfg->num_neighbors = 27;
  cfg->knn = 5;
  cfg->min_knn = 3;
  cfg->max_range = 5.0f;
  cfg->plane_threshold = 0.1f;
  cfg->max_corr_dist = FLT_MAX;
  cfg->k_correspondences = 20;
  cfg->regularization = PCM_REG_PLANE;
  cfg->sort_source = 1;
  cfg->map_capacity = 1000000;   // IVox Options::capacity_  ivox3d.h:57
  cfg->ndt_step_size = 0.1f;     // ndt_omp_impl.hpp:48
  cfg->ndt_outlier_ratio = 0.55f;
  cfg->covariance_method = PCM_COV_KNN;
  cfg->rbf_kernel_width = 0.25f;   // FastVGICPCudaCore  fast_vgicp_cuda.cu:25-26
  cfg->rbf_max_dist = 3.0f;
}

pcm_ctx* pcm_create(int device, const pcm_config* cfg) {
  pcm_ctx* c = new (std::nothrow) pcm_ctx();
  if (!c) return nullptr;
  if (!c->tg.create()) { delete c; return nullptr; }
  c->device = device;
  if (cfg) c->cfg = *cfg; else pcm_default_config(&c->cfg);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    // keep the object so the caller can read the reason, but mark it unusable
    c->err = "no such HIP device (the MI355X path has no CPU fallback)";
    c->device = -1;
    return c;
  }
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    c->err = "hipStreamCreate failed";
    c->device = -1;
    return c;
  }
  {   // keep freed scratch in the device's stream-ordered pool instead of returning it to the driver at every sync
    hipMemPool_t pool = nullptr;
    if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess && pool) {
      uint64_t keep = ~0ull;
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
  }
  c->own_stream = true;
  return c;
}

void pcm_destroy(pcm_ctx* c) {
  if (!c) return;
  if (c->device >= 0) {
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
  }
  // The context's own buffers (the DevBuf / PinnedBuf members of pcm_ctx, its clouds, maps and lists) and its sub-states (the
  // SubState members) free themselves here: `delete c` runs with the device current and before the context's stream is destroyed.
  // The target goes with its last holder, under the same guarantee (target_release_hook).
  hipStream_t own = (c->device >= 0 && c->own_stream) ? c->stream : nullptr;
  c->tg.detach(target_release_hook(c));
  delete c;
  if (own) hipStreamDestroy(own);
}

const char* pcm_last_error(const pcm_ctx* c) { return c ? c->err.c_str() : "null context"; }

#define CHECK_CTX(c)                                                   \
  do {                                                                 \
    if (!(c)) return PCM_ERR_INVALID_ARGUMENT;                         \
    if ((c)->device < 0) return PCM_ERR_HIP;                           \
  } while (0)

int pcm_get_config(const pcm_ctx* c, pcm_config* out) {
  if (!c || !out) return PCM_ERR_INVALID_ARGUMENT;
  *out = c->cfg;
  return PCM_OK;
}

int pcm_set_config(pcm_ctx* c, const pcm_config* cfg) {
  CHECK_CTX(c);
  if (!cfg) return PCM_ERR_INVALID_ARGUMENT;
  int rc = validate_config(c, *cfg);
  if (rc != PCM_OK) return rc;
  if (c->tg.shared()) {
    if (const char* field = target_config_difference(c->cfg, *cfg)) {
      c->err = std::string("pcm_set_config: ") + field + " decides how the target is built, and the target is shared by " + std::to_string(c->tg.holders()) + " contexts";
      return PCM_ERR_UNSUPPORTED;
    }
  }
  c->cfg = *cfg;
  return PCM_OK;
}

int pcm_set_stream(pcm_ctx* c, void* hip_stream) {
  CHECK_CTX(c);
  if (c->own_stream && c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
  c->stream = static_cast<hipStream_t>(hip_stream);
  c->own_stream = false;
  return PCM_OK;
}

int pcm_set_target(pcm_ctx* c, const void* points, size_t n, size_t stride_bytes, int memory, uint64_t tag) {
  CHECK_CTX(c);
  if (tag != 0 && tag == c->tg->tgt.tag && c->tg->tgt.n == n) return PCM_OK;  // `if (target_ == cloud) return;`  fast_gicp_impl.hpp:83-85
  int rc = own_target_again(c);
  if (rc != PCM_OK) return rc;
  rc = set_cloud(c, &c->tg->tgt, points, n, stride_bytes, memory, tag, false);
  c->tg->user_cov.clear();   // target_covs_.clear()  fast_gicp_impl.hpp:89
  c->tg->map.valid = false;
  c->tg->map.index_n = 0;   // another log: the sorted index of the old one is of no use
  c->tg->tgt_dynamic = false;
  c->tg->next_seq = (uint32_t)n;
  c->lio_planes_valid = false;
  return rc;
}

int pcm_set_source(pcm_ctx* c, const void* points, size_t n, size_t stride_bytes, int memory, uint64_t tag) {
  CHECK_CTX(c);
  if (tag != 0 && tag == c->src.tag && c->src.n == n) return PCM_OK;  // fast_gicp_impl.hpp:72-74
  int rc = set_cloud(c, &c->src, points, n, stride_bytes, memory, tag, true);
  source_replaced(c, "pcm_set_source");
  c->user_cov_src.clear();   // source_covs_.clear()  fast_gicp_impl.hpp:78
  if (rc == PCM_OK && (c->cfg.flags & PCM_FLAG_LIO_REFERENCE_SEMANTICS)) rc = lio_members_resize(c, n);   // one resize per frame
  return rc;
}

int pcm_swap_source_and_target(pcm_ctx* c) {
  CHECK_CTX(c);
  if (c->tg.shared()) return refuse_shared(c, "pcm_swap_source_and_target");
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  c->src.swap(c->tg->tgt);
  source_replaced(c, "pcm_swap_source_and_target");
  std::swap(c->user_cov_src, c->tg->user_cov);   // source_covs_.swap(target_covs_)  fast_gicp_impl.hpp:55
  c->tg->map.valid = false;
  c->tg->map.index_n = 0; c->srcmap.index_n = 0;
  return PCM_OK;
}

// dst registers against src's target from now on (pcm_amd.h).  The target is completed in src, on src's stream, which is then
// drained: what dst -- and any later holder -- reads through its own stream was finished before this call returned, and nothing
// writes to it while it has more than one holder.
int pcm_share_target(pcm_ctx* dst, pcm_ctx* src) {
  CHECK_CTX(dst);
  if (!src) { dst->err = "pcm_share_target: null source context"; return PCM_ERR_INVALID_ARGUMENT; }
  if (src->device < 0) { dst->err = "pcm_share_target: the source context has no device"; return PCM_ERR_HIP; }
  if (dst == src) { dst->err = "pcm_share_target: a context cannot share its target with itself"; return PCM_ERR_INVALID_ARGUMENT; }
  if (dst->cfg.model == PCM_MODEL_LOAM || src->cfg.model == PCM_MODEL_LOAM) {
    dst->err = "pcm_share_target: the maps of a PCM_MODEL_LOAM context live in its own state and are not shared";
    return PCM_ERR_UNSUPPORTED;
  }
  int rc = validate_config(dst, dst->cfg);
  if (rc != PCM_OK) return rc;
  if (dst->device != src->device) { dst->err = "pcm_share_target: the contexts live on different devices (device)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (const char* field = target_config_difference(src->cfg, dst->cfg)) {
    dst->err = std::string("pcm_share_target: the configurations differ in ") + field + ", which decides how the target is built";
    return PCM_ERR_INVALID_ARGUMENT;
  }
  if (dst->tg.same_as(src->tg)) return PCM_OK;
  if (src->tg->tgt.n == 0) { dst->err = "pcm_share_target: the source context has no target"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!src->tg.shared()) {   // a target that is shared already was completed when it was first shared
    rc = validate_config(src, src->cfg);
    if (rc == PCM_OK) rc = build_target_for_sharing(src);
    if (rc != PCM_OK) { dst->err = "pcm_share_target: " + src->err; return rc; }
    PCM_HIPCK(dst, hipStreamSynchronize(src->stream));
  }
  PCM_HIPCK(dst, hipStreamSynchronize(dst->stream));   // its queued work may read the target it lets go of
  dst->tg.attach(src->tg, target_release_hook(dst));
  dst->src_cov_valid = false;   // computed with the parameters the old target recorded
  dst->lio_planes_valid = false;
  dst->stats.target_voxels = dst->tg->map.num_voxels;
  dst->stats.target_slots = dst->tg->map.cap;
  return PCM_OK;
}

int pcm_target_share_count(pcm_ctx* c) {
  CHECK_CTX(c);
  return c->tg.holders();
}

int pcm_clear_source(pcm_ctx* c) {
  CHECK_CTX(c);
  c->src.n = 0; c->src.tag = 0;
  source_replaced(c, "pcm_clear_source");
  return PCM_OK;
}

int pcm_clear_target(pcm_ctx* c) {
  CHECK_CTX(c);
  if (c->tg.shared()) return own_target_again(c);
  c->tg->tgt.n = 0; c->tg->tgt.tag = 0; c->tg->map.valid = false; c->tg->map.index_n = 0;
  return PCM_OK;
}

// pclomp::NormalDistributionsTransform::calculateScore (ndt_omp_impl.hpp:835-880) of the source transformed by T
int pcm_ndt_score(pcm_ctx* c, const float T[16], double* score) {
  CHECK_CTX(c);
  if (!T || !score) return PCM_ERR_INVALID_ARGUMENT;
  int rc = validate_config(c, c->cfg);
  if (rc != PCM_OK) return rc;
  if (c->cfg.model != PCM_MODEL_NDT_OMP) { c->err = "pcm_ndt_score needs the NDT_OMP model"; return PCM_ERR_UNSUPPORTED; }
  rc = prepare(c);
  if (rc != PCM_OK) return rc;
  auto solver = make_ndt_solver(c);
  solver.gauss_params();
  std::memcpy(solver.P.T, T, sizeof(float) * 16);
  ndtomp::Eval e{};
  rc = pclndt_eval(c, 3, solver.P, &e, solver.gauss_d3);
  if (rc != PCM_OK) return rc;
  *score = e.score / (double)c->src.n;
  return PCM_OK;
}

// pcl::Registration::getFitnessScore(max_range): mean squared distance of the source points, transformed by T, to their exact
// nearest target points, over the points whose squared distance is <= max_range (call sites: localization.cpp:325-326,
// mapOptmization.cpp:693,719, fast_gicp/src/align.cpp:63)
int pcm_fitness_score(pcm_ctx* c, const float T[16], double max_range, double* score) {
  CHECK_CTX(c);
  if (!T || !score) return PCM_ERR_INVALID_ARGUMENT;
  int rc = validate_config(c, c->cfg);
  if (rc != PCM_OK) return rc;
  rc = prepare(c);
  if (rc != PCM_OK) return rc;
  if (!c->tg->map.valid || !c->tg->map.pts || c->src.n == 0) { c->err = "pcm_fitness_score: set a source and a target first"; return PCM_ERR_INVALID_ARGUMENT; }
  PairDesc d;
  fill_desc(c, &d, nullptr);
  const uint32_t n = (uint32_t)c->src.n;
  const uint32_t nblocks = (n + 255u) / 256u;
  Workspace* w = nullptr;
  rc = ensure_ws(c, &w, 1, (size_t)std::max<uint32_t>(2u * nblocks, kPartialStride), 2);
  if (rc != PCM_OK) return rc;
  launch_fitness(c->stream, d.tgt, coord_mode_for(c->cfg.model), c->src.d_pts, n, T, max_range, w->d_partials);
  PCM_HIPCK(c, hipGetLastError());
  std::vector<double> rows(2 * (size_t)nblocks);
  PCM_HIPCK(c, hipMemcpyAsync(rows.data(), w->d_partials, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  double sum = 0.0, cnt = 0.0;
  for (uint32_t b = 0; b < nblocks; b++) { sum += rows[2 * b]; cnt += rows[2 * b + 1]; }
  *score = cnt > 0.0 ? sum / cnt : DBL_MAX;
  return PCM_OK;
}

// ---- pclomp GICP-BFGS functor (ndt_omp/include/pclomp/gicp_omp_impl.hpp) ------------------------------------------
namespace {

// applyState (:519-529): t <- R t with R from AngleAxisf(z) * AngleAxisf(y) * AngleAxisf(x) (a float quaternion product), then the translation
void bfgs_apply_state(const float* base, const double* x, float* T) {
  auto axis_quat = [](float ang, int k, float* q) { const float h = 0.5f * ang; q[0] = q[1] = q[2] = 0.f; q[k] = sinf(h); q[3] = cosf(h); };
  auto mul = [](const float* a, const float* b, float* r) {
    r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  };
  float qz[4], qy[4], qx[4], qa[4], q[4];
  axis_quat((float)x[5], 2, qz); axis_quat((float)x[4], 1, qy); axis_quat((float)x[3], 0, qx);
  mul(qz, qy, qa); mul(qa, qx, q);
  const float tx = 2.f * q[0], ty = 2.f * q[1], tz = 2.f * q[2];
  const float twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  const float R[9] = {1.f - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.f - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.f - (txx + tyy)};
  for (int i = 0; i < 16; i++) T[i] = base[i];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[i * 4 + j] = (R[i * 3] * base[j] + R[i * 3 + 1] * base[4 + j]) + R[i * 3 + 2] * base[8 + j];
    T[i * 4 + 3] = base[i * 4 + 3] + (float)x[i];
  }
}

// computeRDerivative (:125-176): g[3..5] = <dR/dphi, R>, <dR/dtheta, R>, <dR/dpsi, R>  (R row-major)
void bfgs_r_derivative(const double* x, const double* R, double* g) {
  const double cf = cos(x[3]), sf = sin(x[3]), ct = cos(x[4]), st = sin(x[4]), cp = cos(x[5]), sp = sin(x[5]);
  const double d[3][9] = {{0., sf * sp + cf * cp * st, cf * sp - cp * sf * st, 0., -cp * sf + cf * sp * st, -cf * cp - sf * sp * st, 0., cf * ct, -ct * sf},
                          {-cp * st, cp * ct * sf, cf * cp * ct, -sp * st, ct * sf * sp, cf * ct * sp, -ct, -sf * st, -cf * st},
                          {-ct * sp, -cf * cp - sf * sp * st, cp * sf - cf * sp * st, cp * ct, -cf * sp + cp * sf * st, sf * sp + cf * cp * st, 0., 0., 0.}};
  for (int k = 0; k < 3; k++) {
    double r = 0.;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) r += d[k][j * 3 + i] * R[i * 3 + j];   // matricesInnerProd (gicp_omp.h:325-334)
    g[3 + k] = r;
  }
}

}  // namespace

int pcm_gicp_bfgs_set_correspondences(pcm_ctx* c, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride, const int32_t* idx_src, const int32_t* idx_tgt,
                                      size_t m, const float* maha, int memory) {
  CHECK_CTX(c);
  if (m && (!src || !tgt || !idx_src || !idx_tgt || !maha)) return PCM_ERR_INVALID_ARGUMENT;
  if (stride < 12 || (stride % 4) != 0) { c->err = "bad record layout"; return PCM_ERR_INVALID_ARGUMENT; }
  if (m > 0xffffffffull) { c->err = "too many correspondences"; return PCM_ERR_INVALID_ARGUMENT; }
  if (memory == PCM_MEM_HOST)
    for (size_t i = 0; i < m; i++)
      if (idx_src[i] < 0 || (size_t)idx_src[i] >= n_src || idx_tgt[i] < 0 || (size_t)idx_tgt[i] >= n_tgt) { c->err = "correspondence index out of range"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  c->bfgs_m = 0;
  int rc = bfgs_scratch(c, m);
  if (rc != PCM_OK) return rc;
  if (m == 0) return PCM_OK;
  DevScratch sc(c->stream);
  BfgsStaging G;   // staged once per correspondence set; the evaluations then read the packed records only
  auto layout = [&](ArenaStage& a) { G = bfgs_staging_layout(a, memory, src, n_src, tgt, n_tgt, stride, idx_src, idx_tgt, m, maha); };
  ArenaStage size = arena_stage(c, nullptr);
  layout(size);
  char* q = nullptr;
  if (size.used() && (rc = sc.take(&q, size.used(), &c->err, "correspondence staging")) != PCM_OK) return rc;
  ArenaStage S = arena_stage(c, q);
  layout(S);
  if (S.rc != PCM_OK) return S.rc;
  rc = gicp_bfgs_pack_device(c->stream, G.src, G.tgt, stride, G.idx_src, G.idx_tgt, G.maha, m, c->bfgs, &c->err);
  sc.release();   // behind the pack, on the stream
  if (rc != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the caller's buffers are free again
  c->bfgs_m = m;
  return PCM_OK;
}

int pcm_gicp_bfgs_fdf(pcm_ctx* c, const float* base_T, const double* x, int mode, double* f, double* g) {
  CHECK_CTX(c);
  if (!base_T || !x || mode < 0 || mode > 2 || (mode != 1 && !f) || (mode != 0 && !g)) return PCM_ERR_INVALID_ARGUMENT;
  if (c->bfgs_m == 0) { c->err = "no correspondences (pcm_gicp_bfgs_set_correspondences)"; return PCM_ERR_NO_INPUT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  float T[16];
  bfgs_apply_state(base_T, x, T);
  const size_t m = c->bfgs_m;
  double* d_partials = reinterpret_cast<double*>(c->bfgs + ((64 * m + 255) & ~(size_t)255));
  int rc = c->bfgs_host.reserve(c, 16, 16);
  if (rc != PCM_OK) return rc;
  rc = gicp_bfgs_fdf_device(c->stream, c->bfgs, m, T, base_T, d_partials, c->bfgs_host, &c->err);   // the finish kernel stores to host memory
  if (rc != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  const double* s = c->bfgs_host;
  const double dm = (double)m;
  if (f && mode != 1) *f = (mode == 0 ? s[0] : s[1]) / dm;
  if (g && mode != 0) {
    double R[9];
    for (int a = 0; a < 3; a++) g[a] = s[2 + a] * (2.0 / dm);
    for (int a = 0; a < 9; a++) R[a] = s[5 + a] * (2.0 / dm);
    bfgs_r_derivative(x, R, g);
  }
  return PCM_OK;
}

int pcm_gicp_bfgs_update_correspondences(pcm_ctx* c, const float* transformation, const float* guess, size_t* m_out) {
  CHECK_CTX(c);
  if (!transformation || !guess || !m_out) return PCM_ERR_INVALID_ARGUMENT;
  *m_out = 0;
  int rc = validate_config(c, c->cfg);
  if (rc != PCM_OK) return rc;
  if (c->cfg.model != PCM_MODEL_GICP) { c->err = "pcm_gicp_bfgs_update_correspondences needs the GICP model"; return PCM_ERR_UNSUPPORTED; }
  rc = prepare(c);   // target map + its covariances, brick-major copy of the source + its covariances
  if (rc != PCM_OK) return rc;
  const size_t n = c->srcmap.num_points;
  c->bfgs_m = 0;
  rc = bfgs_scratch(c, n);
  if (rc == PCM_OK) rc = c->bfgs_idx.reserve(c, 2 * n, 2 * (n + n / 4 + 64));
  if (rc != PCM_OK) return rc;
  uint32_t m = 0;
  rc = gicp_bfgs_correspond_device(c->stream, c->tg->map, coord_mode_for(c->cfg.model), c->srcmap, c->src_cov, c->tg->tgt_cov, guess, transformation, (double)c->cfg.max_corr_dist,
                                   reinterpret_cast<float4*>(c->bfgs.p), c->bfgs_idx, c->bfgs_idx + c->bfgs_idx.cap / 2, &m, &c->err);
  if (rc != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  c->bfgs_m = m;
  *m_out = m;
  return PCM_OK;
}

int pcm_gicp_bfgs_get_correspondences(pcm_ctx* c, int32_t* idx_src, int32_t* idx_tgt, float* maha9, size_t capacity) {
  CHECK_CTX(c);
  const size_t m = c->bfgs_m;
  if (!c->bfgs_idx || capacity < m) { c->err = "pcm_gicp_bfgs_get_correspondences: no device-side correspondence set, or the buffers are too small"; return PCM_ERR_INVALID_ARGUMENT; }
  if (m == 0) return PCM_OK;
  if (idx_src) PCM_HIPCK(c, hipMemcpy(idx_src, c->bfgs_idx, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
  if (idx_tgt) PCM_HIPCK(c, hipMemcpy(idx_tgt, c->bfgs_idx + c->bfgs_idx.cap / 2, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
  if (maha9) {
    std::vector<float4> r(3 * m);   // planes 1..3 of the records hold M
    PCM_HIPCK(c, hipMemcpy(r.data(), reinterpret_cast<const float4*>(c->bfgs.p) + m, sizeof(float4) * 3 * m, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < m; i++) {
      const float4 a = r[i], b = r[m + i], d = r[2 * m + i];
      float* o = maha9 + 9 * i;
      o[0] = a.z; o[1] = a.w; o[2] = b.x; o[3] = b.y; o[4] = b.z; o[5] = b.w; o[6] = d.x; o[7] = d.y; o[8] = d.z;
    }
  }
  return PCM_OK;
}

// pcl::VoxelGrid::filter of the scan (jueying_lio/src/laser_mapping.cc:323-328)
int pcm_voxel_downsample(pcm_ctx* c, const void* points, size_t n, size_t stride, int memory, float leaf, void* out, size_t capacity_points, size_t* n_out) {
  CHECK_CTX(c);
  if ((!points && n) || !out || !n_out) return PCM_ERR_INVALID_ARGUMENT;
  if (capacity_points < n) { c->err = "the output buffer must hold as many records as the input"; return PCM_ERR_INVALID_ARGUMENT; }
  *n_out = 0;
  if (n == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  const size_t scratch_bytes = voxel_downsample_scratch_bytes(n);
  FilterArena F;
  int rc = carve_pre_arena(c, "pcm_voxel_downsample", [&](ArenaStage& a) { F = filter_layout(a, memory, points, n * stride, memory, out, n * stride, scratch_bytes); });
  if (rc != PCM_OK) return rc;
  rc = voxel_downsample_device(c->stream, F.src, n, stride, leaf, static_cast<float*>(F.dst), n_out, F.scratch, &c->err);
  if (rc != PCM_OK) return rc;
  if (memory == PCM_MEM_HOST && *n_out) {
    if ((rc = stage_back(c, memory, out, F.dst, *n_out * stride)) != PCM_OK) return rc;
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  }
  return PCM_OK;
}

// pcl::ApproximateVoxelGrid::filter (fast_gicp/src/align.cpp:136-147, src/python/main.cpp:46-92); the rules: approx_voxel.h
int pcm_approx_voxel_downsample(pcm_ctx* c, const void* points, size_t n, size_t stride, int memory, float leaf, void* out, size_t capacity_points, size_t* n_out,
                                size_t* n_dropped) {
  CHECK_CTX(c);
  if (!n_out) { c->err = "pcm_approx_voxel_downsample: n_out is null"; return PCM_ERR_INVALID_ARGUMENT; }
  *n_out = 0;
  if (n_dropped) *n_dropped = 0;
  if ((!points && n) || (!out && capacity_points)) { c->err = "pcm_approx_voxel_downsample: null buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  if (stride < 12 || stride > 64 || (stride % 4) != 0) { c->err = "records must be 3..16 floats"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(leaf > 0.f) || !std::isfinite(leaf)) { c->err = "leaf size must be finite and > 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (n > 0x7fffffffull) { c->err = "pcm_approx_voxel_downsample: more than 2^31 - 1 points"; return PCM_ERR_OUT_OF_RANGE; }
  if (n == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  const size_t scratch_bytes = approx_voxel_scratch_bytes(n), room = std::min(n, capacity_points);   // a result has at most n records
  FilterArena F;
  int rc = carve_pre_arena(c, "pcm_approx_voxel_downsample", [&](ArenaStage& a) { F = filter_layout(a, memory, points, n * stride, memory, out, room * stride, scratch_bytes); });
  if (rc != PCM_OK) return rc;
  uint32_t totals[2] = {0u, 0u};   // runs, valid points
  rc = approx_voxel_downsample_device(c->stream, F.src, n, stride, leaf, static_cast<float*>(F.dst), room, totals, F.scratch, &c->err);
  if (rc != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the one wait
  *n_out = (size_t)totals[0];
  if (n_dropped) *n_dropped = n - (size_t)totals[1];
  if (*n_out > capacity_points) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "pcm_approx_voxel_downsample: the output buffer holds %zu records, the result has %zu", capacity_points, *n_out);
    c->err = buf;
    return PCM_ERR_INVALID_ARGUMENT;
  }
  if (memory == PCM_MEM_HOST && *n_out) {
    if ((rc = stage_back(c, memory, out, F.dst, *n_out * stride)) != PCM_OK) return rc;
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the staged records reach the caller's memory
  }
  return PCM_OK;
}

// setSourceCovariances / setTargetCovariances  fast_gicp_impl.hpp:93-100: `covs` = n matrices of `elems` doubles each (9: 3x3, 16: the
// reference's Matrix4d -- its top-left 3x3 block; symmetric, so row- and column-major read the same), input order
int pcm_set_covariances(pcm_ctx* c, int target, const double* covs, size_t n, int elems) {
  CHECK_CTX(c);
  if ((!covs && n) || (elems != 9 && elems != 16)) return PCM_ERR_INVALID_ARGUMENT;
  if (!is_gicp(c->cfg.model) || c->cfg.model == PCM_MODEL_VGICP_CUDA) { c->err = "covariances can be set for the GICP / VGICP models"; return PCM_ERR_UNSUPPORTED; }
  if (target && c->tg.shared()) return refuse_shared(c, "pcm_set_covariances(target)");
  std::vector<double>& u = target ? c->tg->user_cov : c->user_cov_src;
  u.resize(n * 6);
  const int ld = elems == 9 ? 3 : 4;
  for (size_t i = 0; i < n; i++) {
    const double* m = covs + i * (size_t)elems;
    double* o = &u[i * 6];
    o[0] = m[0]; o[1] = m[1]; o[2] = m[2]; o[3] = m[ld + 1]; o[4] = m[ld + 2]; o[5] = m[2 * ld + 2];
  }
  if (target) c->tg->tgt_cov_valid = false; else c->src_cov_valid = false;
  return PCM_OK;
}

// PointCloudPreprocess::AviaHandler  (jueying_lio/src/pointcloud_preprocess.cc:44-88)
int pcm_livox_filter(pcm_ctx* c, const void* custom_points, size_t n, int memory, int num_scans, int point_filter_num, double blind, void* out, size_t capacity_points, size_t* n_out) {
  CHECK_CTX(c);
  if ((!custom_points && n) || !out || !n_out) return PCM_ERR_INVALID_ARGUMENT;
  if (capacity_points < n) { c->err = "the output buffer must hold as many records as the input"; return PCM_ERR_INVALID_ARGUMENT; }
  if (n > 0xffffffffull) { c->err = "too many points"; return PCM_ERR_INVALID_ARGUMENT; }
  *n_out = 0;
  if (n == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  const size_t scratch_bytes = livox_filter_scratch_bytes(n);
  FilterArena F;
  int rc = carve_pre_arena(c, "pcm_livox_filter", [&](ArenaStage& a) { F = filter_layout(a, memory, custom_points, n * 20, memory, out, n * 48, scratch_bytes); });
  if (rc != PCM_OK) return rc;
  rc = livox_filter_device(c->stream, F.src, n, num_scans, point_filter_num, blind, F.dst, n_out, F.scratch, &c->err);
  if (rc != PCM_OK) return rc;
  if ((rc = stage_back(c, memory, out, F.dst, *n_out * 48)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

// getSourceCovariances / getTargetCovariances  fast_gicp.hpp:64-70  (input order, row-major 3x3 blocks)
int pcm_get_covariances(pcm_ctx* c, int target, double* out, size_t capacity_points, size_t* n) {
  CHECK_CTX(c);
  int rc = validate_config(c, c->cfg);
  if (rc != PCM_OK) return rc;
  if (!is_gicp(c->cfg.model)) { c->err = "covariances exist for the GICP / VGICP models only"; return PCM_ERR_UNSUPPORTED; }
  rc = prepare(c);
  if (rc != PCM_OK) return rc;
  const TargetMap& m = target ? c->tg->map : c->srcmap;
  const double* d_cov = target ? c->tg->tgt_cov : c->src_cov;
  if (n) *n = m.num_points;
  if (!out) return PCM_OK;
  if (capacity_points < m.num_points) { c->err = "output buffer too small"; return PCM_ERR_INVALID_ARGUMENT; }
  std::vector<double> h6((size_t)m.num_points * 6);
  std::vector<uint32_t> ord(m.num_points);
  PCM_HIPCK(c, hipMemcpyAsync(h6.data(), d_cov, sizeof(double) * h6.size(), hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipMemcpyAsync(ord.data(), m.order, sizeof(uint32_t) * ord.size(), hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < ord.size(); i++) {
    const double* s = &h6[i * 6];
    double* o = out + (size_t)ord[i] * 9;
    if (c->cfg.model == PCM_MODEL_VGICP_CUDA) {   // the slot holds the 9 floats of the CUDA-core covariance
      const float* f = reinterpret_cast<const float*>(s);
      for (int a = 0; a < 9; a++) o[a] = (double)f[a];
      continue;
    }
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[1]; o[4] = s[3]; o[5] = s[4]; o[6] = s[2]; o[7] = s[4]; o[8] = s[5];
  }
  return PCM_OK;
}

int pcm_align(pcm_ctx* c, const float guess[16], pcm_result* out) {
  CHECK_CTX(c);
  if (!guess || !out) return PCM_ERR_INVALID_ARGUMENT;
  int rc = validate_config(c, c->cfg);
  if (rc != PCM_OK) return rc;
  pcm_ctx* arr[1] = {c};
  if (c->cfg.model == PCM_MODEL_NDT_OMP) return pclndt_align_batch(arr, 1, guess, out);
  if (c->cfg.model == PCM_MODEL_ICP) return icp_align(c, guess, out);
  return align_batch_impl(arr, 1, guess, out, nullptr);
}

// pclomp NDT: score, gradient, Hessian at the pose vector p = (x, y, z, roll, pitch, yaw) exactly as the line search
// evaluates them (computeDerivatives, ndt_omp_impl.hpp:168-267); pass 2 = computeHessian (:498-559) with the angle
// tables of the previous call
int pcm_ndt_derivatives(pcm_ctx* c, const double p[6], int pass, double* score, double g[6], double H[36]) {
  CHECK_CTX(c);
  if (!p || pass < 0 || pass > 2) return PCM_ERR_INVALID_ARGUMENT;
  int rc = validate_config(c, c->cfg);
  if (rc != PCM_OK) return rc;
  if (c->cfg.model != PCM_MODEL_NDT_OMP) { c->err = "pcm_ndt_derivatives needs the NDT_OMP model"; return PCM_ERR_UNSUPPORTED; }
  rc = prepare(c);
  if (rc != PCM_OK) return rc;
  auto solver = make_ndt_solver(c);
  solver.gauss_params();
  double pp[6];
  std::memcpy(pp, p, sizeof(pp));
  solver.set_pose(pp);
  solver.angle_derivatives(pp);
  ndtomp::Eval e{};
  rc = pclndt_eval(c, pass, solver.P, &e);
  if (rc != PCM_OK) return rc;
  if (score) *score = e.score;
  if (g) std::memcpy(g, e.g, sizeof(e.g));
  if (H) std::memcpy(H, e.H, sizeof(e.H));
  return PCM_OK;
}

int pcm_align_batch(pcm_ctx* const* ctxs, int n, const float* guesses, pcm_result* host_out, void* device_out) {
  if (!ctxs || n <= 0) return PCM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < n; i++) {
    CHECK_CTX(ctxs[i]);
    int rc = validate_config(ctxs[i], ctxs[i]->cfg);
    if (rc != PCM_OK) return rc;
  }
  if (ctxs[0]->cfg.model == PCM_MODEL_NDT_OMP) {
    std::vector<pcm_result> res((size_t)n);
    for (int i = 0; i < n; i++) {
      if (ctxs[i]->cfg.model != PCM_MODEL_NDT_OMP) { ctxs[0]->err = "all contexts of a batch must share the model"; return PCM_ERR_INVALID_ARGUMENT; }
      if (ctxs[i]->device != ctxs[0]->device) { ctxs[0]->err = "all contexts of a batch must live on one device"; return PCM_ERR_INVALID_ARGUMENT; }
      for (int j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) { ctxs[0]->err = "a context appears twice in the batch"; return PCM_ERR_INVALID_ARGUMENT; }
    }
    const int worst = pclndt_align_batch(ctxs, n, guesses, res.data());
    if (worst != PCM_OK && res.empty()) return worst;
    if (host_out) std::memcpy(host_out, res.data(), sizeof(pcm_result) * (size_t)n);
    if (device_out && hipMemcpy(device_out, res.data(), sizeof(pcm_result) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) return PCM_ERR_HIP;
    return worst;
  }
  for (int i = 0; i < n; i++)
    if (ctxs[i]->cfg.model == PCM_MODEL_ICP) { ctxs[0]->err = "pcm_align_batch: PCM_MODEL_ICP contexts register one at a time (pcm_align)"; return PCM_ERR_UNSUPPORTED; }
  return align_batch_impl(ctxs, n, guesses, host_out, device_out);
}

int pcm_linearize(pcm_ctx* c, const double T[16], double H[36], double b[6], double* cost, int32_t* num_inliers) {
  CHECK_CTX(c);
  if (!T) return PCM_ERR_INVALID_ARGUMENT;
  int rc = validate_config(c, c->cfg);
  if (rc != PCM_OK) return rc;
  if (c->cfg.model == PCM_MODEL_ICP) { c->err = "pcm_linearize: PCM_MODEL_ICP has no normal equations (its step is closed-form)"; return PCM_ERR_UNSUPPORTED; }
  double s[kPartialStride];
  rc = single_pass(c, T, true, s);
  if (rc != PCM_OK) return rc;
  int t = 0;
  for (int a = 0; a < 6; a++) {
    for (int k = a; k < 6; k++) {
      if (H) { H[a * 6 + k] = s[t]; H[k * 6 + a] = s[t]; }
      t++;
    }
  }
  if (b) for (int a = 0; a < 6; a++) b[a] = s[21 + a];
  if (cost) *cost = s[27];
  if (num_inliers) *num_inliers = (int32_t)s[28];
  return PCM_OK;
}

int pcm_compute_error(pcm_ctx* c, const double T[16], double* cost) {
  CHECK_CTX(c);
  if (!T || !cost) return PCM_ERR_INVALID_ARGUMENT;
  if (c->cfg.model == PCM_MODEL_ICP) { c->err = "pcm_compute_error: not a call of PCM_MODEL_ICP (pcm_fitness_score is its error)"; return PCM_ERR_UNSUPPORTED; }
  double s[kPartialStride];
  int rc = single_pass(c, T, false, s);
  if (rc != PCM_OK) return rc;
  *cost = s[27];
  return PCM_OK;
}

int pcm_target_insert(pcm_ctx* c, const void* points, size_t n, size_t stride_bytes, int memory) {
  CHECK_CTX(c);
  if (!points && n) { c->err = "null point buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  if (stride_bytes < 3 * sizeof(float) || (stride_bytes % sizeof(float)) != 0) { c->err = "stride must be a multiple of 4 and >= 12 bytes"; return PCM_ERR_INVALID_ARGUMENT; }
  if (c->tg.shared()) return refuse_shared(c, "pcm_target_insert");
  if (n == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  int rc = reserve_target(c, c->tg->tgt.n + n);
  if (rc != PCM_OK) return rc;
  rc = load_points_to_device(c->stream, points, n, stride_bytes, memory, c->tg->next_seq, c->tg->tgt.d_pts + c->tg->tgt.n, &c->err);
  if (rc != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  c->tg->tgt.n += n;
  c->tg->next_seq += (uint32_t)n;
  c->tg->tgt.tag = 0;
  c->tg->map.valid = false;
  c->tg->tgt_dynamic = true;
  return PCM_OK;
}

int pcm_get_source(pcm_ctx* c, float* out_xyz, size_t capacity_points, size_t* n) {
  CHECK_CTX(c);
  if (!n) return PCM_ERR_INVALID_ARGUMENT;
  *n = c->src.n;
  if (!out_xyz) return PCM_OK;
  if (capacity_points < c->src.n) { c->err = "pcm_get_source: buffer too small"; return PCM_ERR_INVALID_ARGUMENT; }
  std::vector<float4> tmp(c->src.n);
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  PCM_HIPCK(c, hipMemcpy(tmp.data(), c->src.d_pts, sizeof(float4) * c->src.n, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < c->src.n; i++) { out_xyz[3 * i] = tmp[i].x; out_xyz[3 * i + 1] = tmp[i].y; out_xyz[3 * i + 2] = tmp[i].z; }
  return PCM_OK;
}

int pcm_get_target(pcm_ctx* c, float* out_xyz, size_t capacity_points, size_t* n) {
  CHECK_CTX(c);
  if (!n) return PCM_ERR_INVALID_ARGUMENT;
  if (c->tg->tgt.n && c->cfg.map_capacity > 0 && !c->tg->map.valid && c->src.n) {
    int rc = prepare(c);   // apply a pending LRU eviction so the log is the current map
    if (rc != PCM_OK) return rc;
  }
  *n = c->tg->tgt.n;
  if (!out_xyz) return PCM_OK;
  if (capacity_points < c->tg->tgt.n) { c->err = "pcm_get_target: buffer too small"; return PCM_ERR_INVALID_ARGUMENT; }
  std::vector<float4> tmp(c->tg->tgt.n);
  PCM_HIPCK(c, hipMemcpy(tmp.data(), c->tg->tgt.d_pts, sizeof(float4) * c->tg->tgt.n, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < c->tg->tgt.n; i++) { out_xyz[3 * i] = tmp[i].x; out_xyz[3 * i + 1] = tmp[i].y; out_xyz[3 * i + 2] = tmp[i].z; }
  return PCM_OK;
}

int pcm_get_planes(pcm_ctx* c, float* out, size_t n) {
  CHECK_CTX(c);
  if (!out || n != c->src.n || !c->planes) { c->err = "pcm_get_planes: call pcm_linearize first; n must equal the source size"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipMemcpy(out, c->planes, sizeof(float4) * n, hipMemcpyDeviceToHost));
  return PCM_OK;
}

int pcm_get_neighbour_lists(pcm_ctx* c, uint64_t info[2], float* centres, uint32_t* starts, float* entries) {
  CHECK_CTX(c);
  const pcm::NeighbourLists& nl = c->tg->nlists;
  if (!info || !nl.valid || nl.kind != 0) { c->err = "pcm_get_neighbour_lists: the context holds no candidate lists of points (P2PLANE, static target, lists built)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (nl.pooled) {   // following lists: brought up to date first, then the pooled runs gathered into contiguous order
    if (!c->tg->map.valid && c->src.n) {
      const int rc = prepare(c);
      if (rc != PCM_OK) return rc;
    }
    if (!nl.valid || nl.stale || !c->tg->map.valid) { c->err = "pcm_get_neighbour_lists: the following lists are behind the target (set a source, or register once)"; return PCM_ERR_INVALID_ARGUMENT; }
    std::vector<uint32_t> h_starts;
    pcm::DevBuf<float4> gathered{"gathered lists"};
    const int rc = pcm::export_pooled_lists(c->stream, nl, &h_starts, &gathered, &c->err);
    if (rc != PCM_OK) return rc;
    info[0] = nl.num_lists;
    info[1] = h_starts.back();
    if (centres) PCM_HIPCK(c, hipMemcpy(centres, nl.index.pts.p, sizeof(float4) * nl.num_lists, hipMemcpyDeviceToHost));
    if (starts) std::memcpy(starts, h_starts.data(), sizeof(uint32_t) * h_starts.size());
    if (entries && info[1]) PCM_HIPCK(c, hipMemcpy(entries, gathered.p, sizeof(float4) * info[1], hipMemcpyDeviceToHost));
    return PCM_OK;
  }
  info[0] = nl.num_lists;
  info[1] = nl.num_candidates;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  if (centres) PCM_HIPCK(c, hipMemcpy(centres, nl.index.pts.p, sizeof(float4) * nl.num_lists, hipMemcpyDeviceToHost));
  if (starts) PCM_HIPCK(c, hipMemcpy(starts, nl.start.p, sizeof(uint32_t) * ((size_t)nl.num_lists + 1), hipMemcpyDeviceToHost));
  if (entries && nl.num_candidates) PCM_HIPCK(c, hipMemcpy(entries, nl.pts.p, sizeof(float4) * nl.num_candidates, hipMemcpyDeviceToHost));
  return PCM_OK;
}

int pcm_neighbour_list_info(pcm_ctx* c, uint64_t info[8]) {
  CHECK_CTX(c);
  if (!info) { c->err = "pcm_neighbour_list_info: null info"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int k = 0; k < 8; k++) info[k] = 0;
  const pcm::NeighbourLists& nl = c->tg->nlists;
  if (!nl.valid || nl.kind != 0 || pcm::lists_view_for(c).pts == nullptr) return PCM_OK;   // no candidate lists, or none this configuration reads
  info[0] = nl.num_lists;
  if (!nl.pooled) { info[1] = nl.num_candidates; info[2] = nl.pts.cap; return PCM_OK; }
  const pcm::list_pool::Pool& p = nl.pool;
  info[1] = p.live; info[2] = p.capacity; info[3] = p.wasted; info[4] = p.updates; info[5] = p.in_place; info[6] = p.relocated; info[7] = p.rebuilds;
  return PCM_OK;
}

int pcm_neighbour_list_update_ms(pcm_ctx* c, double ms[5]) {
  CHECK_CTX(c);
  if (!ms) { c->err = "pcm_neighbour_list_update_ms: null ms"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int k = 0; k < 5; k++) ms[k] = (double)c->tg->nlists.stage_ms[k];
  return PCM_OK;
}

int pcm_neighbour_list_headroom(pcm_ctx* c, float fraction, uint64_t min_entries) {
  CHECK_CTX(c);
  if (!(fraction >= 0.f) || fraction > 16.f || min_entries >= (1ull << 31)) { c->err = "pcm_neighbour_list_headroom: fraction in [0, 16], min_entries below 2^31"; return PCM_ERR_INVALID_ARGUMENT; }
  if (c->tg.shared()) return refuse_shared(c, "pcm_neighbour_list_headroom");
  c->tg->nl_follow.headroom_fraction = fraction;
  c->tg->nl_follow.headroom_min = min_entries;
  return PCM_OK;
}

int pcm_debug_phase_cycles(pcm_ctx* c, uint64_t out[8]) {
  if (!c || !out) return PCM_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 8; k++) { out[k] = c->phase_cycles[k]; c->phase_cycles[k] = 0; }
  return PCM_OK;
}

int pcm_get_stats(pcm_ctx* c, pcm_stats* out) {
  if (!c || !out) return PCM_ERR_INVALID_ARGUMENT;
  *out = c->stats;
  return PCM_OK;
}

int pcm_reset_stats(pcm_ctx* c) {
  if (!c) return PCM_ERR_INVALID_ARGUMENT;
  const uint64_t v = c->stats.target_voxels, s = c->stats.target_slots;
  c->stats = pcm_stats{};
  c->stats.target_voxels = v;
  c->stats.target_slots = s;
  c->lio_search_path[0] = c->lio_search_path[1] = 0;
  return PCM_OK;
}

int pcm_set_profiling(pcm_ctx* c, int on) {
  if (!c) return PCM_ERR_INVALID_ARGUMENT;
  c->profiling = on;
  return PCM_OK;
}

}  // extern "C"
