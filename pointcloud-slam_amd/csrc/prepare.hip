// prepare.hip -- the lazy (re)build of everything a registration reads (target map, neighbour lists, pclomp leaves, covariances
// of the GICP family, per-pair buffers) as a sequence of named steps, the neighbour-list policy, and what turns a prepared context
// into kernel arguments: the pair descriptor, the launch geometry and the kernel / solver parameters.
//
// Host-side counterpart of the reference's wrappers
//   FastVGICPCuda / NDTCuda host classes   ref:pointcloud_match/fast_gicp/include/fast_gicp/gicp/impl/fast_vgicp_cuda_impl.hpp:21-180
#include "pcm_core.h"

#include <algorithm>
#include <cmath>

namespace pcm {

int coord_mode_for(int model) {
  if (model == PCM_MODEL_P2PLANE || model == PCM_MODEL_GICP || model == PCM_MODEL_ICP) return COORD_ROUND;   // GICP, ICP: the grid is only the NN index, any convention serves
  if (model == PCM_MODEL_NDT_OMP) return COORD_FLOOR_MUL;
  return model == PCM_MODEL_VGICP ? COORD_FLOOR_HALF_D : COORD_FLOOR_HALF;
}

size_t num_elements(const pcm_ctx* c) { return c->cfg.model == PCM_MODEL_NDT_D2D ? (size_t)c->srcmap.num_voxels : c->src.n; }

bool is_ndt(int model) { return model == PCM_MODEL_NDT_P2D || model == PCM_MODEL_NDT_D2D; }
bool is_gicp(int model) { return model == PCM_MODEL_GICP || model == PCM_MODEL_VGICP || model == PCM_MODEL_VGICP_CUDA; }
bool radius_model(int model) { return is_ndt(model) || model == PCM_MODEL_VGICP_CUDA; }
int ndt_kind(int model) { return model == PCM_MODEL_NDT_D2D ? 1 : (model == PCM_MODEL_VGICP_CUDA ? 2 : 0); }

namespace {

// PCM_COV_FINE_INDEX=1 switches the fine kNN index of the covariance pass on (measured: fewer candidates, but the second index
// build and its query order cost more than they save on the bench scans -- DESIGN section 3)
bool cov_fine_index_enabled() {
  static const bool on = [] { const char* e = getenv("PCM_COV_FINE_INDEX"); return e && e[0] == '1'; }();
  return on;
}

// PCM_COV_SUBSORT=0: the scan's kNN index keeps input order inside its voxels (A/B measurements)
bool cov_subsort_enabled() {
  static const bool on = [] { const char* e = getenv("PCM_COV_SUBSORT"); return !(e && e[0] == '0'); }();
  return on;
}

// offsets examined per element: DIRECT_RADIUS walks the cube around the voxel (the list is its subset), else the table
size_t neighbor_slots(const pcm_config& g) {
  if (radius_model(g.model) && g.neighbor_search_radius > 0.f) {
    const size_t D = 2 * (size_t)std::ceil((double)g.neighbor_search_radius) + 1;
    return D * D * D;
  }
  return (size_t)g.num_neighbors;
}

// ---- neighbour lists: the policy -------------------------------------------------------------------------------------------------
// The lists of a target cost a build (several ms and, for the candidate lists, 27 x 16 B per map point), so by default they are
// made when a target is registered against the SECOND time (jueying_slam's localization registers every scan against one global
// map; fast_gicp/src/align.cpp:51-104 is no such protocol: it clears the target on every iteration and its reuse loop swaps source
// and target); PCM_FLAG_NEIGHBOUR_LISTS builds them with the map, PCM_FLAG_NO_NEIGHBOUR_LISTS never, and a build that failed is
// not tried again for this map.  Which kind (NeighbourLists::kind) the context wants now, -1 for none:
//   0  P2PLANE: k_linearize_lists runs on per-voxel candidate lists.  Against a target that grows through pcm_target_insert /
//      pcm_map_incremental only under PCM_FLAG_FOLLOWING_LISTS, which keeps the lists of the touched neighbourhoods up to date
//      with every batch (update_following_lists below); without it such a target keeps the tile kernel.
//   1  pclomp NDT: neighbour leaves of the grid (whether the target grew is not looked at)
//   2  fast_gicp NDTCuda (P2D / D2D) and VGICP of the CUDA core with a DIRECT neighbourhood: k_ndt reads rows of neighbour voxel indices
// the pooled form is what a P2PLANE context with PCM_FLAG_FOLLOWING_LISTS builds and reads; the flag means nothing to another model
bool wants_following(const pcm_ctx* c) { return c->cfg.model == PCM_MODEL_P2PLANE && (c->cfg.flags & PCM_FLAG_FOLLOWING_LISTS) != 0; }

int wanted_list_kind(const pcm_ctx* c) {
  const pcm_config& g = c->cfg;
  int kind = -1;
  if (g.model == PCM_MODEL_P2PLANE) {
    const int other_kernel = PCM_FLAG_REFERENCE_KNN_ORDER | PCM_FLAG_COUNTED_SEARCH | PCM_FLAG_NO_LDS_STAGING | PCM_FLAG_FUSED_STEP;
    if ((!c->tg->tgt_dynamic || wants_following(c)) && !(g.flags & other_kernel)) kind = 0;
  } else if (g.model == PCM_MODEL_NDT_OMP) {
    kind = 1;
  } else if (radius_model(g.model)) {
    if (!(g.neighbor_search_radius > 0.f) && c->tg->map.coord_mode == COORD_FLOOR_HALF) kind = 2;
  }
  if (kind < 0 || c->tg->nlists_failed || (g.flags & PCM_FLAG_NO_NEIGHBOUR_LISTS)) return -1;
  if (c->tg.shared()) return c->tg->nlists.valid ? kind : -1;   // nothing is built for a shared target: the lists pcm_share_target left, or none
  return ((g.flags & PCM_FLAG_NEIGHBOUR_LISTS) != 0 || wants_following(c) || c->tg->map_uses >= 2) ? kind : -1;
}

bool has_lists_of_kind(const pcm_ctx* c, int kind) {
  const NeighbourLists& l = c->tg->nlists;
  return l.valid && l.kind == kind && l.num_neighbors == c->cfg.num_neighbors && (kind != 0 || c->tg.shared() || l.pooled == wants_following(c));
}

// Following lists after the map's update (merge and LRU eviction done): the lists around the touched voxels are rewritten, or --
// the pool's policy, list_pool.h -- everything is built again.  A failure is the caller's: the flag asked for lists.
int update_following_lists(pcm_ctx* c) {
  NeighbourLists& l = c->tg->nlists;
  bool rebuild = false;
  l.time_stages = (c->profiling & 1) != 0;
  int rc = update_neighbour_lists(c->stream, c->tg->map, &l, &c->err, &rebuild);
  if (rc == PCM_OK && rebuild) {
    ListFollow f = c->tg->nl_follow; f.by_policy = true;
    rc = build_neighbour_lists(c->stream, c->tg->map, c->cfg.num_neighbors, &l, &c->err, nullptr, false, &f);
  }
  return rc;
}

// builds the lists of `kind` (wanted_list_kind; -1: nothing to do) unless the context holds them, once per (static) target
int ensure_neighbour_lists(pcm_ctx* c, int kind) {
  if (kind < 0 || c->tg.shared()) return PCM_OK;
  if (has_lists_of_kind(c, kind)) return c->tg->nlists.stale ? update_following_lists(c) : PCM_OK;
  const bool follow = kind == 0 && wants_following(c);
  const int rc = build_neighbour_lists(c->stream, c->tg->map, c->cfg.num_neighbors, &c->tg->nlists, &c->err, kind == 1 ? c->tg->pleaf.p : nullptr, kind == 2, follow ? &c->tg->nl_follow : nullptr);
  if (rc != PCM_OK) {
    if ((c->cfg.flags & PCM_FLAG_NEIGHBOUR_LISTS) || wants_following(c)) return rc;   // asked for explicitly
    c->tg->nlists_failed = true;                                   // e.g. no memory for them: the kernel without lists serves this target
    c->tg->nlists.release();
    c->err.clear();
    (void)hipGetLastError();
  }
  return PCM_OK;
}

// A shared target is complete when pcm_share_target returns and pcm_set_config refuses what would rebuild it, so no step below
// finds anything to build for one.  Should one do, it says so instead of writing to memory other contexts are reading.
int shared_target_stale(pcm_ctx* c) {
  c->err = "the shared target was not built for this configuration (library bug: pcm_share_target / pcm_set_config let it through)";
  return PCM_ERR_INTERNAL;
}

// ---- the steps of prepare() --------------------------------------------------------------------------------------------------------
// the voxel map of the target, rebuilt (or updated) when the target, the resolution or the model's needs changed; counts the use
int ensure_target_map(pcm_ctx* c) {
  const int mode = coord_mode_for(c->cfg.model);
  const bool gauss = is_ndt(c->cfg.model);
  const bool gicp = is_gicp(c->cfg.model);
  if (c->tg.shared()) {   // built by pcm_share_target for this very configuration (target_config_difference), and read-only since
    if (!c->tg->map.valid || c->tg->map.res != c->cfg.voxel_resolution || c->tg->map.coord_mode != mode) return shared_target_stale(c);
    return PCM_OK;
  }
  if (!c->tg->map.valid || c->tg->map.res != c->cfg.voxel_resolution || c->tg->map.coord_mode != mode || (gauss && !c->tg->map.gvox) || (gicp && !c->tg->map.order)) {
    uint32_t n_log = (uint32_t)c->tg->tgt.n;
    // the sliding-map capacity belongs to the iVox of the P2PLANE / LIO path; fast_gicp keeps every target point
    const uint32_t capacity = c->cfg.model == PCM_MODEL_P2PLANE ? (uint32_t)std::max(0, c->cfg.map_capacity) : 0u;
    // a map whose log only grew since its last build (pcm_target_insert / pcm_map_incremental) is updated: the new points are merged
    // into the sorted index it kept (voxel_hash.hip); anything else is built from scratch
    uint32_t hazards = 0;
    MapBuildOptions opt; opt.gauss = gauss; opt.keep_order = gicp; opt.capacity_voxels = capacity; opt.n_indexed = c->tg->map.index_n; opt.lru_hazards = &hazards;
    // following lists that are up to date with the map as it is: the update leaves them the voxels it touched
    const NeighbourLists& fl = c->tg->nlists;
    opt.collect_touched = wants_following(c) && fl.valid && fl.pooled && !fl.stale && fl.kind == 0;
    int rc = build_target_map(c->stream, c->tg->tgt.d_pts, &n_log, c->cfg.voxel_resolution, mode, &c->tg->map, &c->err, opt);
    c->stats.lru_batch_hazards += hazards;
    c->tg->tgt.n = n_log;   // LRU eviction compacts the point log
    if (rc != PCM_OK) return rc;
    c->stats.target_voxels = c->tg->map.num_voxels;
    c->stats.target_slots = c->tg->map.cap;
    c->tg->tgt_cov_valid = false;
    c->tg->pleaf_valid = false;
    if (opt.collect_touched && c->tg->map.touched_valid) c->tg->nlists.stale = true;   // brought up to date by ensure_neighbour_lists
    else c->tg->nlists.valid = false;
    c->tg->nlists_failed = false;
    c->tg->map_uses = 0;
  }
  if (c->tg->map_uses < 1000000) c->tg->map_uses++;
  return PCM_OK;
}

// pclomp NDT: VoxelGridCovariance leaves (NormalDistributionsTransform::init, ndt_omp.h:300-306), their lists, the pass buffers
int build_leaves(pcm_ctx* c) {
  int rc = c->tg->pleaf.reserve(c, c->tg->map.num_voxels, c->tg->map.num_voxels);
  if (rc == PCM_OK) rc = c->tg->pleaf_f.reserve(c, c->tg->map.num_voxels, c->tg->map.num_voxels);
  if (rc != PCM_OK) return rc;
  rc = build_pclndt_leaves(c->stream, c->tg->map, c->tg->pleaf, c->tg->pleaf_f, &c->err);
  if (rc != PCM_OK) return rc;
  c->tg->pleaf_valid = true;
  c->tg->nlists.valid = false;
  return PCM_OK;
}

int prepare_pclndt(pcm_ctx* c) {
  if (c->tg.shared() && !c->tg->pleaf_valid) return shared_target_stale(c);
  if (!c->tg->pleaf_valid) {
    const int rc = build_leaves(c);
    if (rc != PCM_OK) return rc;
  }
  // neighbour-leaf lists of the grid (neighbour_lists.hip), after the leaves they are made of
  int rc = ensure_neighbour_lists(c, wanted_list_kind(c));
  if (rc != PCM_OK) return rc;
  uint32_t per = 0;
  const size_t need = (size_t)pclndt_workgroups((uint32_t)c->src.n, &per) * 48;
  rc = c->ndt_partials.reserve(c, need, need, true);
  if (rc == PCM_OK) rc = c->ndt_out.reserve(c, 48, 48);
  if (rc == PCM_OK) rc = c->ndt_out_host.reserve(c, 48, 48);
  return rc;
}

// Covariances of one cloud of the GICP family, in the order of its map: side 1 = target (c->tg->map), 0 = source (c->srcmap).
// `if (target_covs_.size() != target_->size()) calculate_covariances(...)`  fast_gicp_impl.hpp:104-109: covariances the caller
// handed in for every point are uploaded, else RBF or kNN.  The sides differ in three places, each a visible branch below.
int ensure_covariances(pcm_ctx* c, int side) {
  const bool target = side == 1;
  bool& valid = target ? c->tg->tgt_cov_valid : c->src_cov_valid;
  if (valid) return PCM_OK;
  if (target && c->tg.shared()) return shared_target_stale(c);
  const TargetMap& map = target ? c->tg->map : c->srcmap;
  const Cloud& cloud = target ? c->tg->tgt : c->src;
  DevBuf<double>& cov = target ? c->tg->tgt_cov : c->src_cov;
  const std::vector<double>& user = target ? c->tg->user_cov : c->user_cov_src;
  const bool cuda_core = c->cfg.model == PCM_MODEL_VGICP_CUDA;
  int rc = cov.reserve(c, 6 * (size_t)map.num_points, 6 * (size_t)map.num_points);
  if (rc != PCM_OK) return rc;
  const bool whole_log = map.num_points == cloud.n;   // the map holds every point of the cloud
  const bool given = !cuda_core && user.size() == (size_t)map.num_points * 6 && whole_log;
  if (given) rc = upload_covariances(c->stream, map, user.data(), cov, &c->err);
  else if (cuda_core && c->cfg.covariance_method == PCM_COV_RBF_KERNEL)   // NearestNeighborMethod::GPU_RBF_KERNEL
    rc = compute_covariances_rbf(c->stream, map, cloud.d_pts, (uint32_t)cloud.n, c->cfg.rbf_kernel_width, c->cfg.rbf_max_dist, c->cfg.regularization, cov, &c->err);
  else {
    // a second index of the cloud on a grid 8x finer: where one voxel of the search grid holds hundreds of points (a LiDAR's near
    // field) the 20 nearest lie within a few centimetres, and a candidate box made of 0.5 m voxels is thousands of points.
    // Side difference 1: the target's only when its map holds the whole log; the source's is not asked.
    uint32_t n_fine = (uint32_t)cloud.n;
    const float fine_res = std::min(c->cfg.voxel_resolution, 0.5f) * 0.125f;   // 1/8 of the scan's own grid (prepare_gicp)
    MapBuildOptions opt; opt.keep_order = true;
    const bool fine = cov_fine_index_enabled() && (!target || whole_log) &&
                      build_target_map(c->stream, cloud.d_pts, &n_fine, fine_res, coord_mode_for(c->cfg.model), &c->covfine, &c->err, opt) == PCM_OK;
    const int reg_code = c->cfg.regularization + (cuda_core ? 16 : 0);   // + 16: float CUDA-core semantics
    rc = compute_covariances(c->stream, map, c->cfg.k_correspondences, reg_code, cov, &c->err, fine ? &c->covfine : nullptr);
  }
  if (rc != PCM_OK) return rc;
  if (target) {   // side difference 2: the voxel distributions of the target are made of its covariances
    if (cuda_core) {
      rc = c->tg->cvox.reserve(c, c->tg->map.num_voxels, c->tg->map.num_voxels);
      if (rc != PCM_OK) return rc;
      rc = build_vgc_voxels(c->stream, c->tg->map, c->tg->tgt_cov, c->tg->cvox, &c->err);
      if (rc != PCM_OK) return rc;
    }
    if (c->cfg.model == PCM_MODEL_VGICP) {
      rc = c->tg->vvox.reserve(c, c->tg->map.num_voxels, c->tg->map.num_voxels);
      if (rc != PCM_OK) return rc;
      rc = build_vgicp_voxels(c->stream, c->tg->map, c->tg->tgt_cov, c->cfg.voxel_mode, c->tg->vvox, &c->err);
      if (rc != PCM_OK) return rc;
    }
  }
  valid = true;   // (side difference 3 is the user covariances above)
  return PCM_OK;
}

// the parameters the cached covariances of both clouds were computed with follow the configuration: a change drops the caches
int sync_covariance_parameters(pcm_ctx* c) {
  const bool rbf = c->cfg.model == PCM_MODEL_VGICP_CUDA && c->cfg.covariance_method == PCM_COV_RBF_KERNEL;
  const float rbf_w = rbf ? c->cfg.rbf_kernel_width : -1.f, rbf_d = rbf ? c->cfg.rbf_max_dist : -1.f;
  if (c->tg->cov_k != c->cfg.k_correspondences || c->tg->cov_reg != c->cfg.regularization + 100 * c->cfg.model || c->tg->cov_vmode != c->cfg.voxel_mode || c->tg->cov_rbf_w != rbf_w ||
      c->tg->cov_rbf_d != rbf_d) {
    if (c->tg.shared()) return shared_target_stale(c);
    c->src_cov_valid = false; c->tg->tgt_cov_valid = false;
    c->tg->cov_k = c->cfg.k_correspondences; c->tg->cov_reg = c->cfg.regularization + 100 * c->cfg.model; c->tg->cov_vmode = c->cfg.voxel_mode;
    c->tg->cov_rbf_w = rbf_w; c->tg->cov_rbf_d = rbf_d;
  }
  return PCM_OK;
}

// FastGICP::computeTransformation: the scan's kNN index, covariances of both clouds, lazily   fast_gicp_impl.hpp:102-110
int prepare_gicp(pcm_ctx* c) {
  const int mode = coord_mode_for(c->cfg.model);
  int rc = sync_covariance_parameters(c);
  if (rc != PCM_OK) return rc;
  // the scan's own grid is only the index of its kNN search: a finer cell keeps the candidate lists short where a
  // LiDAR scan is dense (near the sensor one 0.5 m voxel holds thousands of points)
  // (measured on Livox-shaped 100 k-point scans: 0.5 m cells are the optimum; 1.0 m costs 25 %, 0.25 m 15-40 %)
  const float src_res = std::min(c->cfg.voxel_resolution, 0.5f);
  if (!c->srcmap.valid || c->srcmap.res != src_res || c->srcmap.coord_mode != mode) {
    uint32_t n_src = (uint32_t)c->src.n;
    // sub-voxel order: 64 consecutive points of the brick-major scan are one patch (k_covariances; k_gicp reads it point by point)
    MapBuildOptions opt; opt.keep_order = true; opt.subsort = cov_subsort_enabled();
    rc = build_target_map(c->stream, c->src.d_pts, &n_src, src_res, mode, &c->srcmap, &c->err, opt);
    if (rc != PCM_OK) return rc;
    c->src_cov_valid = false;
  }
  rc = ensure_covariances(c, 1);
  if (rc == PCM_OK) rc = ensure_covariances(c, 0);
  if (rc != PCM_OK) return rc;
  const size_t ncorr = c->cfg.model == PCM_MODEL_VGICP_CUDA ? 0 : c->src.n * (size_t)(c->cfg.model == PCM_MODEL_VGICP ? c->cfg.num_neighbors : 1);
  return ncorr ? c->maha.reserve(c, 6 * ncorr, 6 * ncorr) : PCM_OK;   // VGICP_CUDA keeps no cache
}

// D2D: the source elements are the source-voxel distributions (ndt_cuda.cu:120-129,156-158)
int ensure_d2d_source_map(pcm_ctx* c) {
  if (c->cfg.model != PCM_MODEL_NDT_D2D || (c->srcmap.valid && c->srcmap.res == c->cfg.voxel_resolution)) return PCM_OK;
  uint32_t n_src = (uint32_t)c->src.n;
  MapBuildOptions opt; opt.gauss = true;
  return build_target_map(c->stream, c->src.d_pts, &n_src, c->cfg.voxel_resolution, coord_mode_for(c->cfg.model), &c->srcmap, &c->err, opt);
}

// what a pair of the batch loop writes per source element, and its round ticket
int ensure_pair_buffers(pcm_ctx* c) {
  if (is_ndt(c->cfg.model) || is_gicp(c->cfg.model)) {
    const size_t need = num_elements(c) * (c->cfg.model == PCM_MODEL_GICP ? (size_t)1 : neighbor_slots(c->cfg));
    const int rc = c->corr.reserve(c, need, need);
    if (rc != PCM_OK) return rc;
  }
  if (c->cfg.sort_source && c->src_order.cap < c->src.n) {
    c->src_sorted = false;
    const int rc = c->src_order.reserve(c, c->src.n, c->src.n);
    if (rc != PCM_OK) return rc;
  }
  int rc = c->counter.reserve(c, 1, 1, true);
  if (rc == PCM_OK) rc = c->nn.reserve(c, 5 * c->src.n, 5 * c->src.n);
  // a new plane array is cleared: with PCM_FLAG_LIO_REFERENCE rows no fit has written are read back (get_planes), and the reference's
  // plane_coef_ starts as a value-initialised vector, not as whatever the allocator handed out
  if (rc == PCM_OK) rc = c->planes.reserve(c, c->src.n, c->src.n, true);
  return rc;
}

}  // namespace

bool lists_pooled_for(const pcm_ctx* c) { return c->tg->nlists.valid && c->tg->nlists.kind == 0 && c->tg->nlists.pooled; }

TargetView lists_view_for(const pcm_ctx* c) {
  const int kind = wanted_list_kind(c);
  const bool on = (kind == 0 || kind == 2) && has_lists_of_kind(c, kind);   // kind 1 is read through ndt_lists_view
  return on ? view_of_lists(c->tg->nlists) : TargetView{};
}

// The LIO calls (pcm_obs_model, pcm_lio_update, the frame calls) run k_lio_lists when the context asked for lists by a flag and
// reads them now; lists that exist through the second-use policy alone leave an LIO call on the tile kernel.
bool lio_on_lists(const pcm_ctx* c) {
  return c->cfg.model == PCM_MODEL_P2PLANE && (c->cfg.flags & (PCM_FLAG_FOLLOWING_LISTS | PCM_FLAG_NEIGHBOUR_LISTS)) != 0 && lists_view_for(c).pts != nullptr;
}

// pclomp NDT: the neighbour-leaf lists of the context's grid, or an empty view (the cells are then looked up one by one)
TargetView ndt_lists_view(const pcm_ctx* c) {
  const bool on = c->cfg.model == PCM_MODEL_NDT_OMP && c->tg->nlists.valid && c->tg->nlists.kind == 1 && c->tg->nlists.num_neighbors == c->cfg.num_neighbors &&
                  !(c->cfg.flags & PCM_FLAG_NO_NEIGHBOUR_LISTS);
  return on ? view_of_lists(c->tg->nlists) : TargetView{};
}

int prepare(pcm_ctx* c) {
  if (c->src.n == 0 || c->tg->tgt.n == 0) { c->err = "align before setInputSource/setInputTarget"; return PCM_ERR_NO_INPUT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  int rc = ensure_target_map(c);
  if (rc != PCM_OK) return rc;
  if (c->cfg.model == PCM_MODEL_NDT_OMP) return prepare_pclndt(c);   // nothing of the pair loop is touched
  if (c->cfg.model == PCM_MODEL_ICP) return PCM_OK;                  // the cloud in map order and the brick table are all ICP reads (icp.hip)
  rc = ensure_neighbour_lists(c, wanted_list_kind(c));
  if (rc == PCM_OK && is_gicp(c->cfg.model)) rc = prepare_gicp(c);
  if (rc == PCM_OK) rc = ensure_d2d_source_map(c);
  if (rc == PCM_OK) rc = ensure_pair_buffers(c);
  return rc;
}

// ---- sharing a target --------------------------------------------------------------------------------------------------------
// The fields of a configuration that decide what the target-side structures hold, i.e. everything the steps of prepare() above
// compare or pass to a build of TargetState's members:
//   model                   coord_mode_for, gauss voxels, the kept input order, the kind of lists (ensure_target_map, wanted_list_kind)
//   voxel_resolution        the map's cell size (ensure_target_map); the pclomp NDT leaves are a function of the map alone
//   num_neighbors, neighbor_search_radius
//                           the neighbourhood the lists are built for, and whether kind-2 lists exist (has_lists_of_kind, wanted_list_kind)
//   flags & kTargetFlags    PCM_FLAG_NEIGHBOUR_LISTS / PCM_FLAG_FOLLOWING_LISTS / PCM_FLAG_NO_NEIGHBOUR_LISTS and the kernel flags next to which no lists are made
//   map_capacity            P2PLANE: the LRU capacity the map was built under (ensure_target_map)
//   k_correspondences, regularization, voxel_mode, covariance_method, rbf_kernel_width, rbf_max_dist
//                           GICP family: the covariances and the voxel distributions made of them (prepare_gicp, ensure_covariances)
// Solver settings (optimizer, iteration limits, epsilons, max_range, plane_threshold, max_corr_dist, the pclomp NDT step size and
// outlier ratio, sort_source, batch_window) are read per registration and may differ between holders.
// Returns the name of the first field that differs, or null.
const char* target_config_difference(const pcm_config& a, const pcm_config& b) {
  constexpr int kTargetFlags = PCM_FLAG_NEIGHBOUR_LISTS | PCM_FLAG_FOLLOWING_LISTS | PCM_FLAG_NO_NEIGHBOUR_LISTS | PCM_FLAG_REFERENCE_KNN_ORDER | PCM_FLAG_COUNTED_SEARCH | PCM_FLAG_NO_LDS_STAGING |
                               PCM_FLAG_FUSED_STEP;
  if (a.model != b.model) return "model";
  if (a.voxel_resolution != b.voxel_resolution) return "voxel_resolution";
  if (a.num_neighbors != b.num_neighbors) return "num_neighbors";
  if (a.neighbor_search_radius != b.neighbor_search_radius) return "neighbor_search_radius";
  if ((a.flags & kTargetFlags) != (b.flags & kTargetFlags)) return "flags";
  if (a.model == PCM_MODEL_P2PLANE && a.map_capacity != b.map_capacity) return "map_capacity";
  if (is_gicp(a.model)) {
    if (a.k_correspondences != b.k_correspondences) return "k_correspondences";
    if (a.regularization != b.regularization) return "regularization";
    if (a.voxel_mode != b.voxel_mode) return "voxel_mode";
    if (a.covariance_method != b.covariance_method) return "covariance_method";
    if (a.covariance_method == PCM_COV_RBF_KERNEL && a.rbf_kernel_width != b.rbf_kernel_width) return "rbf_kernel_width";
    if (a.covariance_method == PCM_COV_RBF_KERNEL && a.rbf_max_dist != b.rbf_max_dist) return "rbf_max_dist";
  }
  return nullptr;
}

// Everything prepare() would build lazily from the target alone, now, on c's stream: the map, the lists the model's kernel reads
// (sharing a target is the repeated use the list policy waits for, so they are made unless the configuration rules them out),
// the pclomp NDT leaves, the target covariances and voxel distributions of the GICP family.  The caller synchronises the stream.
int build_target_for_sharing(pcm_ctx* c) {
  if (c->tg->tgt.n == 0) { c->err = "pcm_share_target: the source context has no target"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  int rc = ensure_target_map(c);
  if (rc != PCM_OK) return rc;
  if (c->tg->map_uses < 2) c->tg->map_uses = 2;
  if (c->cfg.model == PCM_MODEL_NDT_OMP) {
    if (!c->tg->pleaf_valid) {
      rc = build_leaves(c);
      if (rc != PCM_OK) return rc;
    }
    return ensure_neighbour_lists(c, wanted_list_kind(c));
  }
  rc = ensure_neighbour_lists(c, wanted_list_kind(c));
  if (rc == PCM_OK && is_gicp(c->cfg.model)) {
    rc = sync_covariance_parameters(c);
    if (rc == PCM_OK) rc = ensure_covariances(c, 1);
  }
  return rc;
}

Geom pick_geom(size_t max_n, int npairs, bool ndt) {
  // residual kernel: streaming 32 B/point; each lane amortises the 29-value wave
  // reduction over several points, but keep >= ~1024 workgroups in flight
  size_t total = max_n * (size_t)npairs;
  size_t ppb = (total / 1024 + 255) / 256 * 256;
  ppb = std::min<size_t>(std::max<size_t>(ppb, 256), 2048);
  Geom g;
  g.points_per_block = (int)ppb;
  g.blocks_per_pair = (int)((max_n + ppb - 1) / ppb);
  g.tiles_per_pair = ndt ? g.blocks_per_pair : (int)((max_n + 255) / 256);   // NDT linearize uses the streaming geometry
  return g;
}

void fill_desc(const pcm_ctx* c, PairDesc* d, double* partials) {
  d->tgt = view_of(c->tg->map);
  d->nl = lists_view_for(c);
  d->src.pts = (c->cfg.sort_source && c->src_sorted) ? c->src_order : c->src.d_pts;
  if (is_gicp(c->cfg.model)) d->src.pts = c->srcmap.pts;   // brick-major copy of the scan: its covariances are in that order
  d->src_cov = c->src_cov;
  d->tgt_cov = c->tg->tgt_cov;
  d->vvox = c->tg->vvox;
  d->cvox = c->tg->cvox;
  d->maha = c->maha;
  d->src.gvox = c->srcmap.gvox;
  d->src.num_points = (uint32_t)num_elements(c);
  d->corr = c->corr;
  d->nn = c->nn;
  d->planes = c->planes;
  d->partials = partials;
  d->counter = c->counter;
}

KernelParams kernel_params(const pcm_config& g, const Geom& geom) {
  KernelParams kp{};
  kp.num_neighbors = g.num_neighbors;
  if (radius_model(g.model) && g.neighbor_search_radius > 0.f) {
    kp.nb_range = (int32_t)std::ceil((double)g.neighbor_search_radius);
    kp.nb_radius = (double)g.neighbor_search_radius;
  }
  kp.knn = g.knn;
  kp.min_knn = g.min_knn;
  {  // d2 < fl  <=>  double(d2) < max_range^2  when fl is the smallest float >= max_range^2
    const double m2 = (double)g.max_range * (double)g.max_range;
    float fl = (float)m2;
    if ((double)fl < m2) fl = nextafterf(fl, INFINITY);
    kp.max_range_sq = fl;
  }
  kp.plane_threshold = g.plane_threshold;
  kp.blocks_per_pair = geom.blocks_per_pair;
  kp.points_per_block = geom.points_per_block;
  kp.tiles_per_pair = geom.tiles_per_pair;
  kp.use_lds = (g.flags & PCM_FLAG_NO_LDS_STAGING) ? 0 : 1;
  kp.do_step = 1;
  kp.lin_points_per_block = (is_ndt(g.model) || g.model == PCM_MODEL_VGICP_CUDA) ? geom.points_per_block : 256;
  kp.coord_mode = coord_mode_for(g.model);
  kp.max_corr_sq = (double)g.max_corr_dist * (double)g.max_corr_dist;
  return kp;
}

LsqParams lsq_params(const pcm_config& g) {
  LsqParams lp{};
  lp.optimizer = g.optimizer;
  lp.max_iterations = g.max_iterations;
  lp.lm_max_iterations = g.lm_max_iterations;
  lp.rotation_eps = g.rotation_eps;
  lp.translation_eps = g.translation_eps;
  lp.lm_init_lambda_factor = g.lm_init_lambda_factor;
  return lp;
}

}  // namespace pcm
