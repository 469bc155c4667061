// pcm_host.h -- host-side objects behind the C ABI (include/pcm_amd.h).
#pragma once

#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/pcm_amd.h"
#include "dev_buf.h"
#include "list_pool.h"
#include "lio_iekf.h"
#include "lio_outputs.h"
#include "lsq_step.h"
#include "pcm_device.h"
#include "sub_state.h"
#include "target_share.h"

namespace pcm {

struct Cloud {
  float4* d_pts = nullptr;  // compact float4 points, input order: what the kernels read (own, or the caller's own device buffer)
  DevBuf<float4> own{"point cloud"};   // the device copy; empty while borrowed
  size_t n = 0;
  uint64_t tag = 0;
  bool borrowed = false;    // d_pts aliases a caller-owned 16-byte-stride device buffer (zero copy)
  void drop_buffer() {
    own.release();
    d_pts = nullptr; borrowed = false;
  }
  void release() {
    drop_buffer();
    n = 0; tag = 0;
  }
  void swap(Cloud& o) {
    own.swap(o.own);
    std::swap(d_pts, o.d_pts); std::swap(n, o.n); std::swap(tag, o.tag); std::swap(borrowed, o.borrowed);
  }
};

struct TargetMap {   // layout: pcm_device.h
  // the table in use is the first `cap` slots of bricks / bmask (x 16) / bpref (x 16); the allocations only grow
  DevBuf<BrickSlot> bricks{"bricks"};
  DevBuf<uint32_t> bmask{"bmask"};
  DevBuf<uint16_t> bpref{"bpref"};
  DevBuf<uint32_t> vox_start{"vox_start"};
  DevBuf<float4> pts{"pts"};
  DevBuf<GaussVoxel> gvox{"gvox"};   // NDT models
  DevBuf<uint32_t> order{"order"};   // input index of every map point (kept on request: GICP covariances are reported in input order)
  // the sorted index of the point log the tables were built from (key, log position), kept for the next batch of a sliding map
  // (voxel_hash.hip: merged, not re-sorted), and its double buffer
  DevBuf<uint64_t> keys_s{"keys_s"}, keys_t{"keys_t"};
  DevBuf<uint32_t> idx_s{"idx_s"}, idx_t{"idx_t"};
  uint32_t index_n = 0;         // log points keys_s / idx_s cover (0: no usable index)
  DevBuf<char> arena{"map update arena"};   // scratch of the incremental updates (grow-only; the build's DevScratch carves it)
  PinnedBuf<int> h_ctr{"counters"};         // pinned host copy of the build's counter record (one read-back per synchronisation point)
  // MapBuildOptions::collect_touched, after an incremental build: the point keys (point_key) of the batch's points, sorted, then
  // of the voxels the LRU eviction removed; touched_n entries, ~0 where there is none.  What following lists are updated from.
  DevBuf<uint64_t> touched{"touched voxel keys"};
  uint32_t touched_n = 0;
  bool touched_valid = false;   // the last build was an update and left them
  uint32_t cap = 0, num_voxels = 0, num_bricks = 0, num_points = 0;
  uint32_t max_voxel_points = 0;   // most points in one voxel
  float res = 0.f, inv_res = 0.f;
  int coord_mode = 0;
  bool valid = false;
  // back to the empty map: the members free themselves, the scalars take their initial values (nothing to keep in step here)
  void release() { this->~TargetMap(); new (this) TargetMap(); }
};

// the kernels' view of a built map
inline TargetView view_of(const TargetMap& m) {
  TargetView v{};
  v.pts = m.pts; v.vox_start = m.vox_start; v.bricks = m.bricks; v.bmask = m.bmask; v.bpref = m.bpref; v.gvox = m.gvox;
  v.mask = m.cap - 1; v.num_points = m.num_points; v.inv_res = m.inv_res; v.res = m.res;
  return v;
}

// What a build of a TargetMap is asked for beyond the plain brick hash; a call site names the fields it sets.
struct MapBuildOptions {
  bool gauss = false;        // the Gauss voxels (TargetMap::gvox: NDT models)
  bool keep_order = false;   // keep the input index of every map point (TargetMap::order)
  bool subsort = false;      // a voxel's points along a Morton curve of a grid 8x finer, not in input order (full builds only)
  uint32_t capacity_voxels = 0;   // > 1: LRU eviction down to capacity - 1 voxels; log and *n_inout shrink with it
  uint32_t n_indexed = 0;    // > 0: the first n_indexed log points are what map->keys_s / idx_s index; only the points behind are new
  uint32_t* lru_hazards = nullptr;   // out: voxels the batch rule of the eviction kept whole (pcm_stats.lru_batch_hazards)
  bool collect_touched = false;      // an update leaves the voxels it added points to or evicted in TargetMap::touched
};
// Builds `map` from the point log d_pts[0 .. *n_inout): the sorted (key, log position) index, the voxel heads, the brick table,
// the points gathered brick-major.  A run of named stages over one scoped scratch (voxel_hash.hip, DESIGN.md "Build stages"); an
// incremental build (n_indexed, no gauss, no keep_order, same grid) sorts the new points only and merges, over map->arena.  After
// a failure the map is empty.
int build_target_map(hipStream_t stream, float4* d_pts, uint32_t* n_inout, float res, int coord_mode, TargetMap* map, std::string* err, const MapBuildOptions& opt = {});
int load_points_to_device(hipStream_t stream, const void* points, size_t n, size_t stride, int memory, uint32_t seq0, float4* d_out, std::string* err);
// batched scan re-ordering (voxel_hash.hip)
struct SortJob {
  const float4* src;   // scan in input order
  float4* dst;         // scan along the world-grid Morton curve
  uint32_t n;
  uint32_t offset;     // first element of this scan in the concatenated key array
  uint32_t guess_index;
  uint32_t pad;
};
struct SortScratch {
  DevBuf<uint64_t> keys{"sort keys"};    // 2 x cap
  DevBuf<uint32_t> vals{"sort values"};  // 2 x cap
  DevBuf<char> tmp{"sort temporary"};
  size_t cap = 0;                        // points the key / value arrays hold
};
// MapIncremental on the device (voxel_hash.hip)
struct LioStateD { double rot[4], pos[3], off_R[4], off_T[3]; };
inline LioStateD state_of(const pcm_lio_state* st) {
  LioStateD s;
  for (int a = 0; a < 4; a++) { s.rot[a] = st->rot[a]; s.off_R[a] = st->off_R[a]; }
  for (int a = 0; a < 3; a++) { s.pos[a] = st->pos[a]; s.off_T[a] = st->off_T[a]; }
  return s;
}
int map_incremental_device(hipStream_t stream, const float4* scan, bool scan_reordered, uint32_t n, const LioStateD& s, float filter_size_map, const uint32_t* nn,
                           const float4* map_pts, uint32_t seq0, float4* out_append, uint32_t* num_added, std::string* err);
// preprocess.hip
int undistort_device(hipStream_t stream, void* d_points, size_t n, size_t stride, size_t time_off, const pcm_imu_pose* d_poses, int npose, const LioStateD& s, std::string* err);
size_t voxel_downsample_scratch_bytes(size_t n);
size_t livox_filter_scratch_bytes(size_t n);
int livox_filter_device(hipStream_t stream, const void* d_msg, size_t n, int num_scans, int point_filter_num, double blind, void* d_out, size_t* n_out, void* scratch, std::string* err);
int voxel_downsample_device(hipStream_t stream, const void* d_in, size_t n, size_t stride, float leaf, float* d_out, size_t* n_out, void* scratch, std::string* err);
// approx_voxel.hip: pcl::ApproximateVoxelGrid; queues everything, totals = {runs, valid points} after the caller's wait
size_t approx_voxel_scratch_bytes(size_t n);
int approx_voxel_downsample_device(hipStream_t stream, const void* d_in, size_t n, size_t stride, float leaf, float* d_out, size_t capacity, uint32_t* totals, void* scratch,
                                   std::string* err);
// lidar_handlers.hip: the PointCloud2 handlers (the descriptor has passed lidar_check_cloud; n >= 1) and the stable time sort
size_t lidar_filter_scratch_bytes(size_t n);
int lidar_check_cloud(pcm_ctx* c, const void* points, size_t n, int memory, const pcm_lidar_desc* desc);
int lidar_given_on_host(const void* points, size_t n, const pcm_lidar_desc& D);
int lidar_filter_device(hipStream_t stream, const void* d_pts, size_t n, const pcm_lidar_desc& D, int given_hint, void* d_out, size_t capacity, size_t* n_out, int* given_out,
                        void* scratch, std::string* err);
size_t lidar_time_sort_scratch_bytes(size_t m);
int lidar_time_sort_device(hipStream_t stream, const void* d_in, size_t m, void* d_out, void* scratch, std::string* err);
// gicp_bfgs.hip
constexpr int kGicpBfgsMaxBlocks = 512;   // rows of the partial-sum table
size_t gicp_bfgs_scratch_bytes(size_t m);
int gicp_bfgs_pack_device(hipStream_t stream, const void* d_src, const void* d_tgt, size_t stride, const int* d_idx_src, const int* d_idx_tgt, const float* d_maha, size_t m,
                          void* d_records, std::string* err);
int upload_covariances(hipStream_t stream, const TargetMap& map, const double* h_cov6, double* d_cov, std::string* err);   // input-order 6-double rows -> map order
// correspondence step of pclomp GICP-BFGS on the device (gicp.hip): packs the functor's records in source order, returns their number
int gicp_bfgs_correspond_device(hipStream_t stream, const TargetMap& tmap, int coord_mode, const TargetMap& smap, const double* src_cov, const double* tgt_cov,
                                const float* guess, const float* transformation, double max_corr_dist, float4* d_records, int32_t* d_idx_src, int32_t* d_idx_tgt, uint32_t* m_out,
                                std::string* err);
int gicp_bfgs_fdf_device(hipStream_t stream, const void* d_records, size_t m, const float T[16], const float base[16], double* d_partials, double* d_sums, std::string* err);
int sort_sources_batched(hipStream_t stream, const SortJob* d_jobs, int njobs, uint32_t max_n, uint32_t total, const float* d_guesses, float res,
                         SortScratch* ws, std::string* err);

// residual-kernel launchers (kernels.hip, ndt.hip, gicp.hip)
struct LaunchGeom {
  int npairs;
  int blocks_per_pair;
  int points_per_block;
};
void launch_linearize(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp, int npairs, bool write_planes,
                      unsigned long long* d_stats, bool timing);
void launch_linearize_counted(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp, int npairs, bool write_planes,
                           unsigned long long* d_stats, bool timing = false);
// per-voxel candidate lists of a static point-to-plane map (neighbour_lists.hip)
struct NeighbourLists {
  TargetMap index;            // brick hash over one stand-in point per voxel of the dilated occupied set: voxel -> list rank
  DevBuf<uint32_t> start{"list starts"};  // [num_lists + 1] first candidate of every list
  DevBuf<float4> pts{"list candidates"};  // candidates, a list after the other, in the reference's visit order; w = index in the map's point array
  size_t num_candidates = 0;
  uint32_t num_lists = 0;
  int num_neighbors = 0;      // the neighbourhood the lists were built for
  int kind = 0;               // 0: candidate points (P2PLANE); 1: neighbour leaves of a pclomp NDT grid (centroid, leaf index); 2: rows of neighbour voxel indices (k_ndt)
  bool valid = false;
  // Following lists (PCM_FLAG_FOLLOWING_LISTS; kind 0): the runs live in a pool -- `pts` with room behind the runs -- and a list
  // is a (start, length) record.  A list's id is the position of its stand-in point in `centres`, the log `index` is built from and
  // merged into, so it survives the renumbering of the ranks; `rec` / `rec_cap` are kept by id, `rank_rec` is what the kernel reads.
  bool pooled = false;
  bool stale = false;         // the map was updated since the lists were: update_neighbour_lists is due
  DevBuf<float4> centres{"list voxel centres"};
  DevBuf<uint2> rec{"list records"};
  DevBuf<uint32_t> rec_cap{"list capacities"};
  DevBuf<uint2> rank_rec{"list records by rank"};
  PinnedBuf<unsigned long long> h_totals{"list update totals"};
  bool time_stages = false;   // HIP events around the update's stages (pcm_set_profiling bit 0)
  float stage_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};   // the last timed update: dirty lists, classify + read-back, rewrite, index merge + rank table, all
  list_pool::Pool pool;
  // counts every build and every update that wrote entries: whoever keeps positions in `pts` (pcm_ctx::nn after a matching LIO call
  // on the lists) remembers the value they belong to.  It survives release().
  uint64_t generation = 0;
  void release() { const uint64_t g = generation; this->~NeighbourLists(); new (this) NeighbourLists(); generation = g + 1; }   // as TargetMap::release
};
// follow != nullptr (kind 0 only): the pooled form, with the room behind the runs that *follow asks for
struct ListFollow {
  float headroom_fraction = list_pool::kDefaultHeadroomFraction;
  uint64_t headroom_min = list_pool::kDefaultHeadroomMin;
  bool by_policy = false;   // this build replaces an update (counted as a full rebuild)
};
int build_neighbour_lists(hipStream_t stream, const TargetMap& map, int num_neighbors, NeighbourLists* out, std::string* err, const PclLeaf* ndt_leaves = nullptr, bool voxel_slots = false,
                          const ListFollow* follow = nullptr);
// Following lists after an update of `map` that left map.touched: the lists within the neighbourhood of a touched voxel are
// rewritten (in place, or at the pool's bump pointer), new list voxels are merged into the index.  *rebuild: the pool's policy
// (list_pool.h) asks for a full build instead, nothing was changed.  One read-back, plus the index merge's own when there are new list voxels.
int update_neighbour_lists(hipStream_t stream, const TargetMap& map, NeighbourLists* nl, std::string* err, bool* rebuild);
// the pooled runs gathered into contiguous order by rank (parity hook): starts [num_lists + 1] on the host, the entries on the device
int export_pooled_lists(hipStream_t stream, const NeighbourLists& nl, std::vector<uint32_t>* starts, DevBuf<float4>* entries, std::string* err);
TargetView view_of_lists(const NeighbourLists& l);
void launch_linearize_lists(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp, int npairs, bool write_planes, bool pooled = false);
// the jueying_lio measurement model on candidate lists (k_lio_lists, neighbour_lists.hip): what launch_lio_obs (dev: launch_lio_obs_dev)
// computes, through the lists of the descriptor's `nl`
void launch_lio_lists(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp, bool pooled, bool dev);
void launch_linearize_reforder(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp, int npairs, bool write_planes);
void launch_linearize_fused(hipStream_t stream, const PairDesc* d_descs, PairState* d_states, const KernelParams& kp, const LsqParams& lp, int npairs, unsigned char* d_flags_row);
void launch_lio_obs(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp);
void launch_lio_finish(hipStream_t stream, const double* d_partials, int nblocks, double* d_out);
// pcm_lio_update (lio_iekf.hip): a round = launch_lio_obs_dev + launch_lio_finish_gated + launch_iekf_step on the record `blk`
void launch_lio_obs_dev(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp);
struct LioUpdateRecord {   // device-resident for the whole update; the host image is uploaded up to b.tr and read back from b.x on
  PairDesc desc;           // desc.lio: the float pose + converge flag of the next ObsModel call
  PairState ps;            // mode: MODE_LINEARIZE while the loop runs, MODE_DONE after its exit
  iekf::Block b;
};
void launch_lio_finish_gated(hipStream_t stream, const LioUpdateRecord* rec, const double* d_partials, int nblocks, double* d_out);
void launch_iekf_step(hipStream_t stream, LioUpdateRecord* rec, const double* d_sums);
void launch_lio_members_init(hipStream_t stream, float2* aux, uint32_t first, uint32_t last);   // entries [first, last) = (residual 0, selected)
void launch_trial(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp, int npairs);
void launch_finish_round(hipStream_t stream, const PairDesc* d_descs, PairState* d_states, const KernelParams& kp, const LsqParams& lp, int npairs, bool trial_round,
                         bool write_flags, unsigned char* d_flags_row, double* d_sums, unsigned int* d_queue = nullptr, int total_pairs = 0);
void launch_ndt(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp, int npairs, int kind, bool trial);   // kind 0 P2D, 1 D2D, 2 VGICP_CUDA
void launch_fitness(hipStream_t stream, const TargetView& tg, int coord_mode, const float4* src, uint32_t n, const float* T, double max_range, double* d_out);
void launch_gicp(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp, int npairs, bool vgicp, bool trial);
// gicp.hip: kNN covariances of every point of a built map (map order, 6 doubles each); VGICP voxel distributions
int compute_covariances(hipStream_t stream, const TargetMap& map, int k, int regularization, double* d_out, std::string* err, const TargetMap* fine = nullptr);
// RBF-kernel covariances of the CUDA core (GPU_RBF_KERNEL): map order out, sums over the input order
int compute_covariances_rbf(hipStream_t stream, const TargetMap& map, const float4* d_input_order, uint32_t n, double kernel_width, double max_dist, int regularization, double* d_out,
                            std::string* err);
int build_vgicp_voxels(hipStream_t stream, const TargetMap& map, const double* d_cov, int mode, VgVoxel* d_out, std::string* err);
int build_vgc_voxels(hipStream_t stream, const TargetMap& map, const double* d_cov, VgcVoxel* d_out, std::string* err);
// pclndt.hip: pclomp NDT leaves and derivative passes (pass 0: score+gradient+Hessian, 1: score+gradient, 2: double Hessian only)
int build_pclndt_leaves(hipStream_t stream, const TargetMap& map, PclLeaf* d_out, PclLeafF* d_out_f, std::string* err);
int pclndt_workgroups(uint32_t n, uint32_t* per_out);
namespace ndtomp { struct NdtMachine; }
NdtObject make_ndt_object(const TargetMap& map, const PclLeaf* leaves, const PclLeafF* leaves_f, const TargetView& nl, const float4* src, uint32_t n, double* d_partials);
// one round of a batched pclomp NDT registration: the pass every live object waits for, then the sums + solver step per object
void launch_pclndt_batch_round(hipStream_t stream, const NdtObject* d_objs, ndtomp::NdtMachine* d_ms, int nobj, int max_blocks, unsigned char* d_flags_row);
void launch_pclndt_pass(hipStream_t stream, const TargetMap& map, const PclLeaf* leaves, const PclLeafF* leaves_f, const TargetView& nl, const float4* src, uint32_t n, const NdtOmpParams& P, int pass, double* d_partials, double* d_out,
                        double gauss_d3 = 0.0);   // pass 3: calculateScore (needs gauss_d3)
void launch_init_states(hipStream_t stream, PairState* d_states, const float* d_guesses, int npairs, int max_iterations, int window, unsigned int* d_queue);
void launch_pack_results(hipStream_t stream, const PairState* d_states, pcm_result* d_results, int npairs);

// The target of a registration context and everything built from it.  A context holds it through a counted reference
// (pcm_ctx::tg, target_share.h); contexts that pcm_share_target joined hold the same one, which nothing changes while more than
// one of them does.  Per-context scratch (correspondences, planes, the source and its index, workspaces) stays in pcm_ctx.
struct TargetState {
  Cloud tgt;
  TargetMap map;
  bool tgt_dynamic = false;       // the target grew since pcm_set_target (pcm_target_insert / pcm_map_incremental)
  bool nlists_failed = false;     // the lists of this map could not be built (memory): not tried again
  int map_uses = 0;               // prepare() calls since the map was (re)built; stands still while the target is shared
  NeighbourLists nlists;          // candidate lists of `map` (static targets, or following ones; NeighbourLists::kind)
  ListFollow nl_follow;           // pcm_neighbour_list_headroom: the room a full build of following lists reserves
  // GICP / VGICP: per-point covariances in MAP order, voxel distributions
  DevBuf<double> tgt_cov{"tgt_cov"};   // 6 doubles per point
  bool tgt_cov_valid = false;
  int cov_k = 0, cov_reg = -1, cov_vmode = -1;   // what the cached covariances (these and every holder's src_cov) were computed with
  float cov_rbf_w = -1.f, cov_rbf_d = -1.f;   // RBF parameters the cached covariances were computed with (-1: kNN covariances)
  DevBuf<VgVoxel> vvox{"vvox"};
  DevBuf<VgcVoxel> cvox{"cvox"};   // VGICP_CUDA
  // pclomp NDT: leaf payload of the map
  DevBuf<PclLeaf> pleaf{"pleaf"};
  DevBuf<PclLeafF> pleaf_f{"pleaf_f"};   // the float passes' 64-byte view of the same leaves
  bool pleaf_valid = false;
  std::vector<double> user_cov;   // target covariances handed in by the caller (6 per point, input order); empty = compute
  uint32_t next_seq = 0;          // next insertion sequence number of the target point log
};

}  // namespace pcm

// A device array of the context is a DevBuf member (pinned host memory: a PinnedBuf): it frees itself when pcm_destroy deletes the
// context, with the device current and before the stream goes.  Nothing is added to pcm_destroy for it.
// State whose type one translation unit keeps to itself is a SubState member (sub_state.h), made on first use by that unit and
// deleted at the same point under the same guarantee: device current, stream synchronised, stream still alive.  What such a
// state must undo beyond its own members (events, streams, an inner context) is its destructor's business, and a new one needs
// nothing but its member here.  A context with device < 0 never makes one -- every creator tests the device first (CHECK_CTX,
// check_ctx_occ, loam_check_ctx) -- so deleting it touches no HIP call.
struct pcm_ctx {
  int device = 0;
  pcm_config cfg{};
  hipStream_t stream = nullptr;
  bool own_stream = false;
  pcm::Cloud src;
  pcm::SharedTarget<pcm::TargetState> tg;   // the target and what is built from it (TargetState); made by pcm_create, shared by pcm_share_target
  pcm::TargetMap srcmap;          // NDT D2D: the source's own voxel distributions
  pcm::TargetMap covfine;         // GICP: the cloud whose covariances are being computed, on a grid 8x finer (kNN index of dense neighbourhoods only)
  pcm::DevBuf<int32_t> corr{"corr"};   // NDT: matched voxel per (element, offset) of the last linearize
  // GICP / VGICP: per-point covariances of the source in the order of srcmap.pts (6 doubles per point), Mahalanobis cache
  pcm::DevBuf<double> src_cov{"src_cov"};
  bool src_cov_valid = false;   // computed with the parameters tg->cov_* name
  pcm::DevBuf<double> maha{"maha"};          // 6 doubles per correspondence
  // pclomp NDT: partial rows, result row (device + pinned host)
  pcm::DevBuf<double> ndt_partials{"ndt_partials"};
  pcm::DevBuf<double> ndt_out{"ndt_out"};
  pcm::PinnedBuf<double> ndt_out_host{"ndt_out_host"};
  // pose of the last pcm_linearize: linearized_x of the CUDA-core models (ndt_cuda.cu:149), whose trial passes keep R cov_A R^T at it
  double lin_T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  pcm::DevBuf<float4> src_order{"src_order"};   // the scan re-ordered along the world-grid Morton curve (speed only)
  bool src_sorted = false;       // src_order holds the current source
  pcm::DevBuf<float4> planes{"planes"};
  pcm::DevBuf<unsigned int> counter{"counter"};   // round tickets (device, one word)
  std::string err;
  pcm_stats stats{};
  uint64_t phase_cycles[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // diagnostic (profiling bit2)
  pcm::DevBuf<uint32_t> nn{"nn"};  // LIO: the <= 5 neighbours (indices into map.pts) of every scan point from the last matching call
  bool lio_planes_valid = false;   // planes of the last pcm_obs_model(rematch=1) belong to the current scan
  // which array `nn` indexes: the map's points (the tile kernel) or the list entries (k_lio_lists), and for the latter the
  // generation of the lists at that call -- an update or a rebuild since moves the entries, and `nn` then serves nobody
  bool nn_in_lists = false;
  uint64_t nn_lists_generation = 0;
  uint64_t lio_search_path[2] = {0, 0};   // matching ObsModel launches served by k_lio_lists / by the tile kernel (pcm_lio_search_path)
  pcm::DevBuf<float2> lio_aux{"lio_aux"};   // PCM_FLAG_LIO_REFERENCE_SEMANTICS: residuals_ / point_selected_surf_ of LaserMapping, in the caller's scan order;
  size_t lio_aux_n = 0;                     // they outlive the scan (std::vector::resize semantics, laser_mapping.cc:337-338)
  pcm::DevBuf<char> lio_upd{"lio_upd"};      // pcm_lio_update: descriptor, pair state, filter record and trace of the last update (lio_iekf.hip)
  pcm::PinnedBuf<char> lio_upd_host{"lio_upd_host"};   // its pinned host image (one upload, one download)
  int lio_upd_calls = 0;                    // ObsModel calls the trace of the last update holds
  pcm::DevBuf<char> lio_prop{"lio_prop"};    // pcm_lio_propagate: the uploaded frame block and the downloaded result block (lio_predict.hip)
  pcm::PinnedBuf<char> lio_prop_host{"lio_prop_host"};   // their pinned host image
  pcm::SubState ws;       // pcm::Workspace: batch workspace owned by this context (align_batch.hip)
  pcm::SubState ndt_ws;   // pclomp NDT: objects + solver machines of a batch (align_batch.hip)
  pcm::DevBuf<char> pre_arena{"pre_arena"};   // grow-only device scratch of the pre-processing operators
  // jueying_lio frame outputs (lio_outputs.hip): where the current frame's records lie in pre_arena (gone with the next call that
  // takes the arena: take_pre_arena), the pose of the last ObsModel call, and the saved-map log (lio_out::MapLog)
  pcm::lio_out::FrameRecord lio_frame;
  pcm::lio_out::LastObs lio_last_obs;
  pcm::SubState lio_map;
  pcm::DevBuf<char> bfgs{"bfgs"};             // GICP-BFGS functor: packed correspondence records + partial sums (gicp_bfgs.hip)
  size_t bfgs_m = 0;
  std::vector<double> user_cov_src;   // source covariances handed in by the caller (6 per point, input order); empty = compute
  pcm::DevBuf<int32_t> bfgs_idx{"bfgs_idx"};   // source indices of the packed pairs in the first half, target indices in the second (device-side correspondence step)
  pcm::PinnedBuf<double> bfgs_host{"bfgs_host"};   // pinned, device-visible: the 14 sums land here without a copy command
  pcm::SubState loam;      // PCM_MODEL_LOAM: maps, features, device state and the stores (loam_api.hip)
  pcm::SubState loam_fe;   // PCM_MODEL_LOAM: the front end's cross-frame state and last-frame outputs (loam_features.hip)
  pcm::SubState loam_cloud;   // PCM_MODEL_LOAM: the staged raw cloud and the prepared records of cachePointCloud (loam_cloud.hip)
  pcm::SubState occ;       // any model: the 2D occupancy map (occ_map.hip)
  pcm::SubState octo;      // any model: the 3D occupancy map (octo_map.hip)
  pcm::SubState icp;       // PCM_MODEL_ICP: parameters, state block, sum rows and trace of the device loop (icp.hip)
  // any model: scan fusion (scan_fuse.hip): staged host segments, the fused records (pcm_scan_fused), counters + tables + scan scratch
  pcm::DevBuf<char> scan_in{"scan_in"}, scan_out{"scan_out"}, scan_tmp{"scan_tmp"};
  size_t scan_n = 0;     // records of the last pcm_scan_fuse with out = NULL that scan_out still holds
  int profiling = 0;  // bit0: HIP-event timing of residual launches, bit1: kNN counters
};

namespace pcm {
// room for `bytes` in the grow-only device scratch the pre-processing operators share (a quarter of headroom: no allocation per
// frame in the steady state); the contents do not survive the call, so the frame record of the LIO outputs goes, and `who` (a
// string literal, the entry point) is what their refusal names
inline int take_pre_arena(pcm_ctx* c, size_t bytes, const char* who) {
  c->lio_frame.take(who);
  return c->pre_arena.reserve(c->stream, &c->err, bytes, bytes + bytes / 4);
}
// the source is another cloud from now on (set, swapped, cleared, or a frame's scan adopted by the entry point `who`): nothing
// derived from the old one serves it -- the frame record, the pose of the last ObsModel call, the re-ordered copy, the planes
// and neighbours of the last matching call, the source's voxel map and its covariances.  Every call that replaces the source
// comes here; covariances the caller handed in (user_cov_src) are its own business
inline void source_replaced(pcm_ctx* c, const char* who) {
  c->lio_frame.take(who);
  c->lio_last_obs.valid = false;
  c->src_sorted = false;
  c->lio_planes_valid = false;
  c->srcmap.valid = false;
  c->src_cov_valid = false;
}
// the copies of a Stage (arena_carver.h) on a stream
struct StreamCopy {
  hipStream_t st;
  std::string* err;
  int h2d(void* dst, const void* src, size_t bytes) const { PCM_HIPCK_ERR(err, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st)); return PCM_OK; }
  int d2h(void* dst, const void* src, size_t bytes) const { PCM_HIPCK_ERR(err, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); return PCM_OK; }
};
using ArenaStage = Stage<StreamCopy>;
inline ArenaStage arena_stage(pcm_ctx* c, void* base) { return ArenaStage(base, StreamCopy{c->stream, &c->err}); }
// The two passes of an entry point over the pre-processing arena: `layout(ArenaStage&)` run over a null base is the size
// take_pre_arena makes room for; run again over the arena it carves the blocks and queues the staged input.
template <class Layout> int carve_pre_arena(pcm_ctx* c, const char* who, Layout&& layout) {
  ArenaStage size = arena_stage(c, nullptr);
  layout(size);
  const int rc = take_pre_arena(c, size.used(), who);
  if (rc != PCM_OK) return rc;
  ArenaStage S = arena_stage(c, c->pre_arena.p);
  layout(S);
  return S.rc;
}
inline int stage_back(pcm_ctx* c, int memory, void* user, const void* dev, size_t bytes) { return stage_back(StreamCopy{c->stream, &c->err}, memory, user, dev, bytes); }
// `name`: "memory" or "out_memory", the argument
inline int check_memory(pcm_ctx* c, int memory, const char* name) {
  if (memory == PCM_MEM_HOST || memory == PCM_MEM_DEVICE) return PCM_OK;
  c->err = std::string(name) + " must be PCM_MEM_HOST or PCM_MEM_DEVICE";
  return PCM_ERR_INVALID_ARGUMENT;
}
template <typename T> int DevBuf<T>::reserve(pcm_ctx* c, size_t need, size_t new_cap, bool zero) { return reserve(c->stream, &c->err, need, new_cap, zero); }
template <typename T> int DevBuf<T>::reserve_keep(pcm_ctx* c, size_t need, size_t new_cap, size_t keep) { return reserve_keep(c->stream, &c->err, need, new_cap, keep); }
template <typename T> int PinnedBuf<T>::reserve(pcm_ctx* c, size_t need, size_t new_cap, unsigned flags) { return reserve(c->stream, &c->err, need, new_cap, flags); }
}  // namespace pcm
