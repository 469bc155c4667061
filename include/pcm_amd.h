/*
 * include/pcm_amd.h -- C ABI of the MI355X-native scan-to-submap registration path.
 *
 * This is the drop-in boundary: a plain C interface (pointers + sizes, no
 * Eigen / PCL / torch types) that the reference's PCL-style operator surface
 * binds to.  Each entry point cites the reference interface it replaces
 * (paths relative to /root/reference/src/pointcloud_match/fast_gicp unless
 * they start with jueying_lio/ or ndt_omp/).  The header-only C++ adapter
 * include/pcm_amd/registration.hpp re-creates the pcl::Registration subclass
 * on top of these calls; INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *   - every 4x4 transform is ROW-MAJOR (Eigen::Matrix4f is column-major: the
 *     adapter transposes);
 *   - point clouds are arrays of records whose first three floats are x,y,z
 *     (pcl::PointXYZ stride 16, PointXYZI 32, PointXYZINormal 48 bytes);
 *   - all functions return 0 on success, a negative pcm_status otherwise, and
 *     never throw or abort (the reference abort()s on bad enums:
 *     include/fast_gicp/gicp/fast_vgicp_voxel.hpp:13-15);
 *   - a context is single-threaded like a pcl::Registration object; different
 *     contexts may live on different threads / GPUs.
 */
#ifndef PCM_AMD_H
#define PCM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCM_ABI_VERSION 3

typedef enum pcm_status {
  PCM_OK = 0,
  PCM_ERR_INVALID_ARGUMENT = -1,
  PCM_ERR_NO_INPUT = -2,       /* align() before setInputSource/Target */
  PCM_ERR_HIP = -3,            /* a HIP runtime call failed; see pcm_last_error */
  PCM_ERR_UNSUPPORTED = -4,
  PCM_ERR_OUT_OF_RANGE = -5,   /* voxel coordinate outside +-2^20 cells */
  PCM_ERR_NOT_CONVERGED = -6,  /* "lm not converged!!"  impl/lsq_registration_impl.hpp:69-72 (result still written) */
  PCM_ERR_INTERNAL = -7,       /* a pair of a batch was not driven to the end of its loop (library bug); its pose is not a result */
  PCM_ERR_TOO_FEW_FEATURES = -8 /* LOAM: not more than edge_min_valid corner / surf_min_valid surf features; pose left as given
                                 * (the "Not enough features!" branch of scan2MapOptimization, jueying_slam/src/mapOptmization.cpp:1584-1585) */
} pcm_status;

/* residual models */
typedef enum pcm_model {
  PCM_MODEL_P2PLANE = 0, /* jueying_lio/src/laser_mapping.cc:592-701  5-NN plane fit, n.p+d */
  PCM_MODEL_GICP = 1,    /* impl/fast_gicp_impl.hpp:114-237 */
  PCM_MODEL_VGICP = 2,   /* impl/fast_vgicp_impl.hpp:72-204, src/fast_gicp/cuda/compute_derivatives.cu */
  PCM_MODEL_NDT_P2D = 3, /* src/fast_gicp/cuda/ndt_compute_derivatives.cu:33-102 */
  PCM_MODEL_NDT_D2D = 4, /* src/fast_gicp/cuda/ndt_compute_derivatives.cu:104-175 */
  PCM_MODEL_VGICP_CUDA = 6, /* FastVGICPCuda's float core: src/fast_gicp/cuda/{covariance_estimation,covariance_regularization,gaussian_voxelmap,
                             * find_voxel_correspondences,compute_derivatives}.cu (resolution 1.0, DIRECT1, PLANE: impl/fast_vgicp_cuda_impl.hpp:24-27) */
  PCM_MODEL_LOAM = 7,    /* jueying_slam LOAM edge / plane scan-to-map optimisation (mapOptmization.cpp:1255-1586): pcm_loam_* entry points only */
  PCM_MODEL_ICP = 8,     /* point-to-point ICP, pcl::IterativeClosestPoint as jueying_slam/src/mapOptmization.cpp:768-779 uses it: pcm_icp_* below */
  PCM_MODEL_NDT_OMP = 5  /* pclomp::NormalDistributionsTransform: pointcloud_match/ndt_omp/include/pclomp/ndt_omp_impl.hpp:69-880
                          * (Newton step + More-Thuente line search; max_iterations 35, translation_eps 0.1 = transformation_epsilon_,
                          *  voxel_resolution 1.0, num_neighbors 7 = DIRECT7 are that class's defaults) */
} pcm_model;

/* LSQ_OPTIMIZER_TYPE  include/fast_gicp/gicp/lsq_registration.hpp:13 */
typedef enum pcm_optimizer { PCM_OPT_GAUSS_NEWTON = 0, PCM_OPT_LEVENBERG_MARQUARDT = 1 } pcm_optimizer;

/* RegularizationMethod  include/fast_gicp/gicp/gicp_settings.hpp:6 */
typedef enum pcm_regularization {
  PCM_REG_NONE = 0, PCM_REG_MIN_EIG = 1, PCM_REG_NORMALIZED_MIN_EIG = 2, PCM_REG_PLANE = 3, PCM_REG_FROBENIUS = 4,
  PCM_REG_PCLOMP = 5   /* pclomp::GeneralizedIterativeClosestPoint::computeCovariances (ndt_omp/include/pclomp/gicp_omp_impl.hpp:48-122):
                        * raw second moments with float products, singular values -> (1, 1, gicp_epsilon_ = 0.001) */
} pcm_regularization;

/* where a point buffer lives */
typedef enum pcm_memory { PCM_MEM_HOST = 0, PCM_MEM_DEVICE = 1 } pcm_memory;

/*
 * Registration knobs = the reference's plain setters
 * (setMaximumIterations, setRotationEpsilon, setTransformationEpsilon,
 *  setInitialLambdaFactor: impl/lsq_registration_impl.hpp:8-38;
 *  setResolution / setNeighborSearchMethod: impl/fast_vgicp_impl.hpp:28-40;
 *  ivox_grid_resolution / ivox_nearby_type / esti_plane_threshold:
 *  jueying_lio/config/livox.yaml:44-46).
 */
typedef struct pcm_config {
  int32_t model;                 /* pcm_model */
  int32_t optimizer;             /* pcm_optimizer; default LM (lsq_registration_impl.hpp:15) */
  int32_t max_iterations;        /* 64   (:11) */
  int32_t lm_max_iterations;     /* 10   (:17) */
  double rotation_eps;           /* 2e-3 (:12) */
  double translation_eps;        /* 5e-4 (:13) */
  double lm_init_lambda_factor;  /* 1e-9 (:18) */
  float voxel_resolution;        /* iVox / voxel-map cell size [m] */
  int32_t num_neighbors;         /* 1, 7, 19 or 27 cells searched around the query; pclomp NDT: 0 = KDTREE radius search */
  int32_t knn;                   /* NUM_MATCH_POINTS 5      jueying_lio/include/options.h:14 */
  int32_t min_knn;               /* MIN_NUM_MATCH_POINTS 3  jueying_lio/include/options.h:15 */
  float max_range;               /* GetClosestPoint max_range 5.0  jueying_lio/include/ivox3d/ivox3d.h:80 */
  float plane_threshold;         /* ESTI_PLANE_THRESHOLD 0.1  jueying_lio/src/options.cc:10 */
  float max_corr_dist;           /* corr_dist_threshold_ FLT_MAX  impl/fast_gicp_impl.hpp:18 */
  int32_t k_correspondences;     /* 20  impl/fast_gicp_impl.hpp:16 */
  int32_t regularization;        /* pcm_regularization; PLANE  impl/fast_gicp_impl.hpp:20 */
  int32_t sort_source;           /* 1: order the scan along a Morton curve on device (speed only; default 1) */
  int32_t flags;                 /* PCM_FLAG_*: bits 0-1, 3, 4 and 6 speed / debugging only (never change a result), bit 2 selects the ObsModel semantics, bit 5 the neighbour row order */
  int32_t map_capacity;          /* sliding map: max voxels kept, LRU beyond (IVox capacity_ 1000000, ivox3d.h:57); 0 = unlimited */
  float ndt_step_size;           /* pclomp NDT: step_size_ 0.1 (maximum More-Thuente step)  ndt_omp_impl.hpp:48 */
  float ndt_outlier_ratio;       /* pclomp NDT: outlier_ratio_ 0.55  ndt_omp_impl.hpp:48 */
  int32_t batch_window;          /* pcm_align_batch: pairs iterating at a time; finished pairs hand their slot to queued ones (0 = all at once; speed only) */
  int32_t voxel_mode;            /* VGICP VoxelAccumulationMode (gicp_settings.hpp:10): 0 ADDITIVE (default), 1 ADDITIVE_WEIGHTED, 2 MULTIPLICATIVE */
  float neighbor_search_radius;  /* NDT_P2D / NDT_D2D / VGICP_CUDA: > 0 selects NeighborSearchMethod::DIRECT_RADIUS -- every voxel offset with
                                  * |offset| <= radius + 1e-3, radius in voxels (cuda/ndt_cuda.cu:70-83, cuda/fast_vgicp_cuda.cu:77-90;
                                  * setNeighborSearchMethod(method, radius)); num_neighbors is not read then.  0 (default): off */
  int32_t covariance_method;     /* VGICP_CUDA: PCM_COV_KNN (k nearest neighbours, default) or PCM_COV_RBF_KERNEL -- NearestNeighborMethod::GPU_RBF_KERNEL
                                  * of FastVGICPCuda (fast_vgicp_cuda_impl.hpp:107,136; cuda/covariance_estimation_rbf.cu:59-151) */
  float rbf_kernel_width;        /* 0.25: the weight of a point at squared distance d2 is expf(-rbf_kernel_width * d2)  (fast_vgicp_cuda.cu:25, :81) */
  float rbf_max_dist;            /* 3.0: points farther than this do not take part  (fast_vgicp_cuda.cu:26; setKernelWidth: 5 x width when not given) */
} pcm_config;

#define PCM_COV_KNN 0
#define PCM_COV_RBF_KERNEL 1

#define PCM_FLAG_NO_LDS_STAGING 1   /* probe the global table per lane instead of the per-tile LDS grid */
#define PCM_FLAG_LIO_REFERENCE_SEMANTICS 4
/* pcm_obs_model keeps residuals_ and point_selected_surf_ across calls AND scans exactly as the members of LaserMapping do
 * (jueying_lio/src/laser_mapping.cc:335-339 one resize-with-default per frame; :616-636 a selected point that fails the
 * `p_body.norm() > 81 pd2^2` test keeps its flag and contributes the residual an earlier call -- possibly of an older frame --
 * stored for its index; a point never stored contributes 0).  Set it before pcm_set_source of the first scan.  Off (default):
 * such a point is dropped for that call, the result depends on the current scan, map and state only. */
#define PCM_FLAG_COUNTED_SEARCH 8    /* P2PLANE: k_linearize_counted (linearize_counted.hip: voxel point counts in the LDS cell grid, four candidates per cell and
                                     * trip, rolled cell loop, DPP reductions) instead of k_linearize; same neighbour lists, planes and sums bit for bit.
                                     * 14 % fewer vector instructions and a third of the code, measured 12 % SLOWER (profiles/r03_bench_ab_*.json): A/B switch */
#define PCM_FLAG_NEIGHBOUR_LISTS 16   /* P2PLANE against a static target: the linearize pass runs on per-voxel candidate lists -- for every voxel a query can fall
                                       * into, the points of its neighbour voxels in the reference's visit order, contiguous (27 x 16 B per map point), built
                                       * on the device (neighbour_lists.hip) -- instead of re-deriving the candidates per pass through LDS.  Same candidates
                                       * in the same order: bit-identical results, 1.8x the kernel speed.  DEFAULT: the lists are built when a target is
                                       * registered against the second time; this flag builds them with the map (first registration already).  Never for a
                                       * target that has grown (pcm_target_insert / pcm_map_incremental) or next to another kernel flag.  A context that
                                       * sets this flag (or PCM_FLAG_FOLLOWING_LISTS) itself also runs the LIO model -- pcm_obs_model, pcm_lio_update,
                                       * the frame calls -- on the lists (k_lio_lists, same bits as the tile kernel; pcm_lio_search_path tells which
                                       * ran); lists made by the second-use default alone leave the LIO calls on the tile kernel.
                                       * pclomp NDT (PCM_MODEL_NDT_OMP): the same policy for the grid's neighbour-LEAF lists (the leaves a point's search
                                       * visits, in visiting order; 16 B per (voxel, neighbour leaf)). */
#define PCM_FLAG_FOLLOWING_LISTS 128  /* P2PLANE: candidate lists that follow a growing target.  Built with the map as under PCM_FLAG_NEIGHBOUR_LISTS; when the
                                       * target grows through pcm_target_insert / pcm_map_incremental, the lists within one neighbourhood of a voxel the batch
                                       * added points to (or the LRU eviction removed) are rewritten at the next registration -- in place where the run's
                                       * capacity holds them, else at the end of a pool with reserved room (pcm_neighbour_list_headroom) -- instead of
                                       * being dropped, and every linearize pass keeps running k_linearize_lists.  Same candidates in the same order as the
                                       * tile kernel finds: bit-identical results.  A full build replaces the update when the pool is full, when the holes
                                       * left by moved runs exceed the live entries, or when more than half the lists are empty.  No lists next to
                                       * PCM_FLAG_NO_NEIGHBOUR_LISTS or another kernel flag (REFERENCE_KNN_ORDER, COUNTED_SEARCH, NO_LDS_STAGING, FUSED_STEP);
                                       * pcm_obs_model, pcm_lio_update and the frame calls run the lists kernel too (k_lio_lists; bit-identical
                                       * to the tile kernel, pcm_lio_search_path tells which ran).  Measured (DESIGN section 26, 1 M-point map, 7 000-point
                                       * batches): pays from one align per insert on; the pool takes 2.5 x the lists' memory.  The update rewrites a run per
                                       * wave (0.07-0.14 ms of a 0.65-1.7 ms update, section 28).  Measured on the LIO frame loop (1 M-point map, 14 frames): the
                                       * flag LOSES in all three settings tried -- 1.4 -> 2.3 ms per frame with the 0.5 m scan filter, 4.6 -> 5.8-6.4 ms unfiltered,
                                       * 1.2 -> 4.0-4.2 ms at 0.2 m voxels -- because the per-frame list update and its synchronisations cost more than the
                                       * search saves on a map of that size.  Fails loudly when the lists cannot be kept (no memory). */
#define PCM_FLAG_NO_NEIGHBOUR_LISTS 64 /* never build them: the tile kernel (kernels.hip) serves every pass */
#define PCM_FLAG_REFERENCE_KNN_ORDER 32
/* P2PLANE align / linearize: hand esti_plane its neighbours in the row order the reference's IVox::GetClosestPoint leaves -- the
 * order of libstdc++'s std::nth_element (jueying_lio/include/ivox3d/ivox3d.h:173-178, ivox3d_node.hpp:176-181) -- instead of
 * ascending distance.  Same neighbour set; the float plane fit of a row-permuted system rounds differently (measured on the
 * bench pairs: ~17 % of the planes differ in the last bits, poses by up to 8e-5 m when an LM iteration count flips;
 * profiles/r03_knn_order_sensitivity.json).  Compatibility mode: a slower kernel (private candidate array per scan point, no LDS
 * staging), maps with at most 121 points per voxel (PCM_ERR_UNSUPPORTED beyond); pcm_obs_model does not take it. */
#define PCM_FLAG_FUSED_STEP 2       /* GN: take the step in the search kernel's last workgroup (write-through hand-off of the partial rows) instead of
                                     * a second launch; same sums in the same order; measured slower at every round size, off by default */

/* out-parameters of align(): getFinalTransformation / hasConverged /
 * getFinalHessian / nr_iterations_  (lsq_registration_impl.hpp:40-79) */
typedef struct pcm_result {
  float T[16];          /* final_transformation_ = x0.cast<float>()  (:77) */
  double T64[16];       /* x0 before the float cast */
  double H[36];         /* final_hessian_ (:119,166) */
  double cost;          /* cost of the last linearize */
  int32_t iterations;   /* nr_iterations_ */
  int32_t converged;    /* converged_ */
  int32_t num_linearize;      /* linearize passes executed */
  int32_t num_compute_error;  /* compute_error passes executed (LM) */
  int32_t num_inliers;        /* correspondences used by the last linearize */
  int32_t status;             /* pcm_status of this pair */
} pcm_result;

/* counters for byte accounting / roofline (bench.py) */
typedef struct pcm_stats {
  uint64_t linearize_launches;   /* residual-kernel launches since reset */
  uint64_t point_passes;         /* scan points evaluated (sum over launches) */
  uint64_t candidates;           /* map points scanned by the kNN search */
  uint64_t slots_probed;         /* hash slots read */
  double linearize_ms;           /* HIP-event time of those launches on the context stream */
  uint64_t target_voxels;        /* occupied voxels of the current target */
  uint64_t target_slots;         /* hash-table capacity */
  uint64_t tiles;                /* 256-point tiles searched (counter passes only) */
  uint64_t tiles_lds_grid;       /* ... whose voxel box fitted the LDS grid */
  uint64_t tiles_lds_points;     /* ... whose map points were staged through LDS as well */
  double residual_ms;            /* HIP-event time of the residual/reduction launches (every-launch mode only) */
  uint64_t timed_launches;       /* launches bracketed by HIP events (= linearize_launches unless profiling bit3 samples them) */
  uint64_t timed_pair_slots;     /* sum of the pair-list lengths of the timed launches ... */
  uint64_t launched_pair_slots;  /* ... and of all launches: the share of point_passes that falls to the timed ones */
  uint64_t lru_batch_hazards;    /* sliding map: voxels a batch touched whose previous touch was older than the batch's eviction cut-off -- the
                                  * reference's sequential LRU list (ivox3d.h:256-281) may have dropped such a voxel before the batch reached it
                                  * and re-created it with the batch's points only; the batch rule here keeps it whole.  0 = the map equals the
                                  * sequential result.  Conservative (every voxel that MIGHT differ is counted): 0-24 per frame out of 10^6
                                  * voxels in the synthetic config-5 loops */
} pcm_stats;

typedef struct pcm_ctx pcm_ctx;

/* fills the reference defaults listed above */
void pcm_default_config(pcm_config *cfg);

/* construct / destroy one registration object bound to a HIP device.
 * Replaces: FastGICP()/FastVGICPCuda()/NDTCuda() constructors
 * (impl/fast_gicp_impl.hpp:8-24, impl/fast_vgicp_cuda_impl.hpp:21-38) and the
 * LaserMapping iVox construction (jueying_lio/src/laser_mapping.cc:16). */
pcm_ctx *pcm_create(int device, const pcm_config *cfg);
void pcm_destroy(pcm_ctx *ctx);
const char *pcm_last_error(const pcm_ctx *ctx);
int pcm_get_config(const pcm_ctx *ctx, pcm_config *out);
int pcm_set_config(pcm_ctx *ctx, const pcm_config *cfg);   /* setters; target structures rebuilt lazily if needed */
int pcm_set_stream(pcm_ctx *ctx, void *hip_stream);        /* run on a caller stream (hipStream_t) */

/* setInputTarget / setInputSource  (impl/fast_gicp_impl.hpp:71-90): `tag` is
 * the caller's pointer identity; an equal non-zero tag makes the call a no-op,
 * like the reference's `if (target_ == cloud) return;`.  The library copies
 * the xyz fields into device memory it owns (voxel hash built lazily at the next
 * align).  One exception, for speed: a SOURCE given as a device buffer with a
 * 16-byte stride (pcl::PointXYZ layout) is used in place, not copied -- like the
 * reference's shared_ptr input it must stay alive and unchanged until the
 * align() that uses it has returned. */
int pcm_set_target(pcm_ctx *ctx, const void *points, size_t n, size_t stride_bytes, int memory, uint64_t tag);
int pcm_set_source(pcm_ctx *ctx, const void *points, size_t n, size_t stride_bytes, int memory, uint64_t tag);
int pcm_swap_source_and_target(pcm_ctx *ctx);              /* impl/fast_gicp_impl.hpp:50-58 */
int pcm_clear_source(pcm_ctx *ctx);                        /* :60-64 */
int pcm_clear_target(pcm_ctx *ctx);                        /* :66-69 */

/* One built target for several contexts.  The reference's registration objects take one PointCloud::ConstPtr and cache by
 * pointer identity (impl/fast_gicp_impl.hpp:72-90), so N objects against one map hold the map once; here a context owns its
 * target, and pcm_share_target makes `dst` register against the target `src` holds from now on: the cloud, its voxel map and
 * what the model derives from them (candidate / neighbour lists, pclomp NDT leaves, GICP-family covariances and voxel
 * distributions) exist once, however many contexts hold them.
 *   - Both contexts live on one device, are of the same model (not PCM_MODEL_LOAM: PCM_ERR_UNSUPPORTED) and agree in every
 *     configuration field that decides how a target is built: model, voxel_resolution, num_neighbors, neighbor_search_radius,
 *     the flags NEIGHBOUR_LISTS / NO_NEIGHBOUR_LISTS / REFERENCE_KNN_ORDER / COUNTED_SEARCH / NO_LDS_STAGING / FUSED_STEP,
 *     map_capacity (P2PLANE), and for the GICP family k_correspondences, regularization, voxel_mode, covariance_method and the
 *     RBF parameters.  A difference, a `src` without a target or dst == src: PCM_ERR_INVALID_ARGUMENT, and pcm_last_error(dst)
 *     names the first field that differs.  Solver settings may differ.
 *   - The call completes the target in `src` on src's stream -- everything a registration would otherwise build lazily,
 *     the lists included unless the configuration rules them out (sharing is the repeated use their policy waits for) -- and
 *     waits for that stream.  From then on the target is immutable while more than one context holds it, and any stream reads it.
 *   - `dst` lets go of the target it had.  pcm_set_target, pcm_clear_target and pcm_destroy on a holder detach that holder only;
 *     the memory goes with the last holder, so `src` may be destroyed first.
 *   - What would change a target that has more than one holder returns PCM_ERR_UNSUPPORTED and changes nothing:
 *     pcm_target_insert, pcm_map_incremental, pcm_lio_frame_end, pcm_set_covariances(target), pcm_swap_source_and_target, and a
 *     pcm_set_config that changes one of the fields above.  There is no copy-on-write.
 *   - A target that aliases a caller's device buffer (it arrived as a zero-copy source and was swapped into the target's place)
 *     stays the caller's to keep alive and unchanged, now for as long as any holder registers against it.
 *   - Neither context may be in another call while pcm_share_target runs.  Afterwards the holders are as independent as any
 *     two contexts: each on its own stream and thread, or together in one pcm_align_batch.
 * pcm_target_share_count: the contexts holding ctx's target (1 = not shared), or a negative pcm_status. */
int pcm_share_target(pcm_ctx *dst, pcm_ctx *src);
int pcm_target_share_count(pcm_ctx *ctx);

/* pcl::Registration::align(out, guess) -> computeTransformation
 * (impl/lsq_registration_impl.hpp:52-79).  Transforming the output cloud is
 * left to the adapter (pcl::transformPointCloud, :78). */
int pcm_align(pcm_ctx *ctx, const float guess[16], pcm_result *out);

/* LsqRegistration::evaluateCost -> linearize (lsq_registration_impl.hpp:46-49)
 * and compute_error (impl/fast_gicp_impl.hpp:213-237). H,b may be NULL.
 * pcm_compute_error evaluates the correspondences of the last pcm_linearize; for NDT D2D and VGICP_CUDA it keeps R cov_A R^T at
 * the pose of that pcm_linearize (linearized_x, ndt_cuda.cu:149). pcm_align keeps its own linearisation pose and does not
 * change the one pcm_compute_error uses: call pcm_linearize first. */
int pcm_linearize(pcm_ctx *ctx, const double T[16], double H[36], double b[6], double *cost, int32_t *num_inliers);
int pcm_compute_error(pcm_ctx *ctx, const double T[16], double *cost);

/* parity hook: the plane (nx,ny,nz,d) fitted to every scan point by the last
 * pcm_linearize (plane_coef_ of jueying_lio/src/laser_mapping.cc:621-622), in the
 * scan's device order; nx = NaN marks a point that was not selected.  `out`
 * holds 4*n floats. */
int pcm_get_planes(pcm_ctx *ctx, float *out, size_t n);

/* parity hook: the per-voxel candidate lists of a static P2PLANE target (PCM_FLAG_NEIGHBOUR_LISTS) as the device holds them.
 * info[0] = number of list voxels L, info[1] = number of entries E (pad entries included).  Each of the other arguments may be
 * NULL: `centres` 4*L floats (the centre of list voxel r in xyz), `starts` L+1 entries (run r = entries starts[r] .. starts[r+1];
 * every start is a multiple of 4 and a run ends with 0..3 pad entries), `entries` 4*E floats (x, y, z, bit pattern of the point's
 * index in the map's own array; a pad entry is +inf, +inf, +inf, 0xffffffff).  Fails unless the context holds such lists. */
/* Following lists (PCM_FLAG_FOLLOWING_LISTS) are brought up to date first (a source must be set if the target grew since the last
 * registration) and their pooled runs are gathered into this contiguous form, list voxels in the index's current order.  After an
 * update the fourth component of a real entry is NOT maintained: the map's point array is renumbered by every merge and the walk
 * never reads it; only a pad entry's 0xffffffff is kept.  A list voxel all of whose neighbours were evicted stays, with an empty run. */
int pcm_get_neighbour_lists(pcm_ctx *ctx, uint64_t info[2], float *centres, uint32_t *starts, float *entries);

/* The candidate lists the context's linearize pass reads: info[0] lists, [1] live entries (pad entries included), [2] capacity of
 * the allocation in entries, and for following lists [3] wasted entries (holes left by moved runs), [4] updates since the last
 * full build, [5] runs rewritten in place, [6] runs relocated, [7] full builds the pool's policy asked for ([5]-[7] since the
 * lists were first built).  All zero when the context holds no lists or its configuration reads none. */
int pcm_neighbour_list_info(pcm_ctx *ctx, uint64_t info[8]);

/* Diagnostic: the device time of the last update of following lists that ran while pcm_set_profiling bit 0 was on, from HIP events
 * (they cost the update one more synchronisation): ms[0] dirty lists (dilation, sort, distinct), [1] classify + the read-back,
 * [2] rewrite, [3] index merge (only with new list voxels) + rank table, [4] the whole update.  Zeros when none was timed or a full
 * build took the update's place. */
int pcm_neighbour_list_update_ms(pcm_ctx *ctx, double ms[5]);

/* Which search served the jueying_lio measurement model: counts[0] = matching ObsModel launches (pcm_obs_model with rematch != 0,
 * the matching rounds of pcm_lio_update) that ran the lists kernel (k_lio_lists), counts[1] = those that ran the tile kernel, since
 * pcm_create or pcm_reset_stats.  The lists kernel serves a context that set PCM_FLAG_FOLLOWING_LISTS or PCM_FLAG_NEIGHBOUR_LISTS
 * itself and whose configuration reads lists (no other kernel flag; on a shared target, the lists its owner left); lists that
 * exist through the second-use default alone leave these calls on the tile kernel.  Both kernels give the same bits. */
int pcm_lio_search_path(pcm_ctx *ctx, uint64_t counts[2]);

/* Following lists: the free room a full build reserves behind the runs -- max(fraction * entries, min_entries) entries of 16
 * bytes.  Default: one and a half times the entries, at least 65536 (1 MiB).  A minimum, applied when a full build has to
 * allocate: the allocation only grows (by a quarter more than asked) and the pool uses all of it. */
int pcm_neighbour_list_headroom(pcm_ctx *ctx, float fraction, uint64_t min_entries);

/* parity hook for PCM_FLAG_LIO_REFERENCE_SEMANTICS: residuals_[i] and point_selected_surf_[i]
 * (jueying_lio/src/laser_mapping.cc:337-338, 619-635) as the last pcm_obs_model left them, in the order of the
 * caller's scan; n must equal the source size. */
int pcm_get_lio_members(pcm_ctx *ctx, float *residuals, uint8_t *selected, size_t n);

/* jueying_lio measurement model: the h_dyn_share callback LaserMapping::ObsModel
 * (jueying_lio/src/laser_mapping.cc:592-701) together with the reduction the IEKF applies
 * to its output, HTH = h_x^T h_x (12x12) and h_x^T h (esekfom.hpp:1687,1706).
 * State = the pose part of state_ikfom; quaternions in Eigen coefficient order (x,y,z,w).
 * rematch = ekfom_data.converge: non-zero -> 5-NN + plane fit for every scan point;
 * zero -> the planes of the previous call are re-used (laser_mapping.cc:616).
 * Target = the map (pcm_set_target), source = the down-sampled scan in the LiDAR frame.
 * Two semantics for a selected point that fails the ||p|| > 81 pd2^2 test (laser_mapping.cc:631-635):
 *   default                           -- the point is dropped for this call (a function of scan, map and state only);
 *   PCM_FLAG_LIO_REFERENCE_SEMANTICS  -- the reference's: point_selected_surf_[i] stays set and the row carries the residual an
 *                                        earlier call (of this frame or of an older one, by index) stored in residuals_[i];
 *                                        both members persist across calls and scans with std::vector::resize semantics
 *                                        (laser_mapping.cc:335-339).  Parity hook: pcm_get_lio_members. */
typedef struct pcm_lio_state {
  double rot[4];     /* s.rot            world <- imu */
  double pos[3];     /* s.pos */
  double off_R[4];   /* s.offset_R_L_I   imu <- lidar */
  double off_T[3];   /* s.offset_T_L_I */
} pcm_lio_state;

typedef struct pcm_obs_result {
  double HTH[144];   /* row-major 12x12 */
  double HTh[12];
  double sum_h2;     /* sum of squared residuals */
  int32_t n_eff;     /* effect_feat_num_ */
  int32_t valid;     /* ekfom_data.valid (0 when n_eff < 1, laser_mapping.cc:657-661) */
} pcm_obs_result;

int pcm_obs_model(pcm_ctx *ctx, const pcm_lio_state *state, int extrinsic_est_en, int rematch, pcm_obs_result *out);

/* Sliding submap (jueying_lio): IVox::AddPoints (jueying_lio/include/ivox3d/ivox3d.h:256-281) --
 * append points to the target; voxels beyond cfg.map_capacity are dropped least-recently-
 * touched first.  The voxel hash is rebuilt on the device at the next matching call. */
int pcm_target_insert(pcm_ctx *ctx, const void *points, size_t n, size_t stride_bytes, int memory);

/* LaserMapping::MapIncremental (jueying_lio/src/laser_mapping.cc:525-583): transform the current
 * scan with the updated state (PointBodyToWorld, :855-864), apply the map add-filter against the
 * neighbours found by the last pcm_obs_model(rematch != 0), and insert the survivors
 * (points_to_add first, then point_no_need_downsample).  ekf_inited = flg_EKF_inited_. */
int pcm_map_incremental(pcm_ctx *ctx, const pcm_lio_state *state, float filter_size_map, int ekf_inited, size_t *num_added);

/* current target points in insertion order (x,y,z per point); *n receives the count (query with out = NULL) */
int pcm_get_target(pcm_ctx *ctx, float *out_xyz, size_t capacity_points, size_t *n);

/* pclomp NDT (PCM_MODEL_NDT_OMP): one derivatives evaluation at the pose vector p = (x, y, z, roll, pitch, yaw)
 * exactly as the line search runs it.  pass 0: score + gradient + Hessian (float inner products), pass 1: score +
 * gradient, pass 2: the double-precision Hessian of computeHessian (uses the angle tables of p as well).
 * Replaces NormalDistributionsTransform::computeDerivatives / computeHessian
 * (pointcloud_match/ndt_omp/include/pclomp/ndt_omp_impl.hpp:168-267, 498-559). */
int pcm_ndt_derivatives(pcm_ctx *ctx, const double p[6], int pass, double *score, double g[6], double H[36]);

/* pcl::Registration::getFitnessScore(max_range) on the device: the source cloud transformed by the float pose T (row-major 4x4),
 * exact nearest target point of every source point, mean of the squared distances that are <= max_range (PCL compares the SQUARED
 * distance with max_range; its default is the largest double).  No point in range: the largest double, as PCL returns.
 * Replaces the CPU kd-tree pass every call site runs right after align(): jueying_slam/src/localization.cpp:325-326,
 * jueying_slam/src/mapOptmization.cpp:693,719, fast_gicp/src/align.cpp:63, fast_gicp/src/python/main.cpp get_fitness_score. */
int pcm_fitness_score(pcm_ctx *ctx, const float T[16], double max_range, double *score);

/* pclomp NDT: calculateScore (ndt_omp_impl.hpp:835-880) of the source cloud transformed by T (row-major float 4x4) */
int pcm_ndt_score(pcm_ctx *ctx, const float T[16], double *score);

/*
 * Point-to-point ICP (PCM_MODEL_ICP): pcl::IterativeClosestPoint, the verifier of jueying_slam's performSCLoopClosure
 * (mapOptmization.cpp:768-779).  PCL is not in the reference tree: the rules are restated from PCL 1.10's IterativeClosestPoint /
 * DefaultConvergenceCriteria and are this library's definition (csrc/icp.h); the closed-form step is Eigen's
 * umeyama without scaling (fast_gicp/thirdparty/Eigen/Eigen/src/Geometry/Umeyama.h:118-158).  A context of this model goes through
 * pcm_set_target / pcm_set_source (a PCM_MEM_DEVICE source of 16-byte records is read in place) / pcm_align / pcm_fitness_score;
 * of pcm_config it reads voxel_resolution (the cell of the search grid: speed only, the nearest neighbour is exact).  One align(guess):
 *   F = double(guess); per iteration every source point goes through float(F) (the cloud itself is never rewritten: PCL transforms
 *   the cloud and composes increments in float), pairs with its exact nearest target point when the float squared distance is
 *   <= max_correspondence_distance^2 (inclusive; non-finite points have no pair); fewer than 3 pairs stop the loop unconverged
 *   with the pose as it was; else the SVD step of the pairs is composed onto F in double and the criteria run in this order:
 *   iteration count >= max_iterations (converged = 1: PCL counts the cap as convergence), cos(angle) >= rotation threshold and
 *   |t|^2 <= transformation_epsilon (the epsilon meets the squared translation, as in PCL), |mse - previous mse| < mse_absolute,
 *   |mse - previous mse| / previous mse < euclidean_fitness_epsilon.
 * pcm_result: T = float(F), T64 = F, iterations, converged, cost = the last mean squared pair distance, num_inliers = the last
 * pair count, num_linearize = iterations that ran; pcm_align returns PCM_OK also when converged = 0.  Sums are taken in a fixed
 * order without atomics: two runs give the same bytes.  The loop is device-resident; the host waits once per
 * PCM_ICP_CHUNK_ITERATIONS iterations.
 */
#define PCM_ICP_STOP_NONE 0                 /* no align() yet */
#define PCM_ICP_STOP_ITERATIONS 1           /* the iteration cap (converged = 1) */
#define PCM_ICP_STOP_TRANSFORM 2            /* rotation and translation of the last step below their thresholds */
#define PCM_ICP_STOP_ABS_MSE 3              /* |mse - previous mse| < mse_absolute */
#define PCM_ICP_STOP_REL_MSE 4              /* |mse - previous mse| / previous mse < euclidean_fitness_epsilon */
#define PCM_ICP_STOP_NO_CORRESPONDENCES 5   /* fewer than 3 pairs (converged = 0) */
#define PCM_ICP_CHUNK_ITERATIONS 8

typedef struct pcm_icp_params {
  int32_t max_iterations;                /* 10            setMaximumIterations */
  double max_correspondence_distance;    /* sqrt(DBL_MAX) setMaxCorrespondenceDistance */
  double transformation_epsilon;         /* 0             setTransformationEpsilon */
  double rotation_epsilon;               /* 0             setTransformationRotationEpsilon: a cosine; <= 0 means 1 - transformation_epsilon */
  double euclidean_fitness_epsilon;      /* -DBL_MAX      setEuclideanFitnessEpsilon: the relative-MSE threshold */
  double mse_absolute;                   /* 1e-12         DefaultConvergenceCriteria's absolute MSE threshold */
  int32_t reserved[8];
} pcm_icp_params;

typedef struct pcm_icp_info {
  int32_t stop_reason;           /* PCM_ICP_STOP_* of the last pcm_align */
  int32_t iterations;            /* completed iterations */
  int32_t converged;
  int32_t reserved0;
  uint64_t num_pairs;            /* N of the last iteration that ran */
  double mse;                    /* sum d2 / N of the last iteration that had >= 3 pairs */
  int32_t reserved[8];
} pcm_icp_info;

void pcm_icp_default_params(pcm_icp_params *params);
/* PCM_MODEL_ICP contexts only (PCM_ERR_UNSUPPORTED otherwise).  max_iterations in [1, 2^20], max_correspondence_distance > 0, no
 * NaN: PCM_ERR_INVALID_ARGUMENT, nothing changed.  A context that never set any runs with the defaults. */
int pcm_icp_set_params(pcm_ctx *ctx, const pcm_icp_params *params);
int pcm_icp_get_params(pcm_ctx *ctx, pcm_icp_params *params);
/* stop reason, iterations, last pair count and mse of the last pcm_align (zeros before one) */
int pcm_icp_last(pcm_ctx *ctx, pcm_icp_info *info);
/* parity hook: pair count and mse of every iteration that ran in the last pcm_align (*n entries; an iteration stopped for
 * fewer than 3 pairs has mse 0); num_pairs / mse may be NULL to ask for the count */
int pcm_icp_trace(pcm_ctx *ctx, int32_t capacity, uint64_t *num_pairs, double *mse, int32_t *n);

/* GICP / VGICP: regularised per-point covariances (row-major 3x3 doubles, INPUT order) of the source
 * (target = 0) or target (target = 1) cloud; computes them if needed.  Query the count with out = NULL.
 * Replaces FastGICP::getSourceCovariances / getTargetCovariances
 * (fast_gicp/include/fast_gicp/gicp/fast_gicp.hpp:64-70; computed at impl/fast_gicp_impl.hpp:239-298). */
int pcm_get_covariances(pcm_ctx *ctx, int target, double *out, size_t capacity_points, size_t *n);
/* setSourceCovariances / setTargetCovariances (impl/fast_gicp_impl.hpp:93-100; pclomp gicp_omp.h:165,186): hand in the
 * per-point covariances instead of having them computed -- n matrices of `elems` doubles (9 = 3x3, 16 = Matrix4d, its 3x3
 * block is read), input order.  As in the reference they are used while their count equals the cloud's (:104-109), dropped by the
 * next pcm_set_source / pcm_set_target (:78,89) and swapped by pcm_swap_source_and_target (:55).  GICP and VGICP models. */
int pcm_set_covariances(pcm_ctx *ctx, int target, const double *covs, size_t n, int elems);

/* common::Pose6D (jueying_lio/msg/Pose6D.msg): one propagated IMU pose of the frame (rot row-major) */
typedef struct pcm_imu_pose {
  double offset_time;   /* seconds after the first lidar point */
  double acc[3], gyr[3], vel[3], pos[3], rot[9];
} pcm_imu_pose;

/* Motion compensation of a scan into its frame-end pose, in place (x, y, z of every record are rewritten).
 * Replaces the backward-propagation loop of ImuProcess::UndistortPcl (jueying_lio/include/imu_processing.hpp:245-285).
 * `time_offset_bytes`: where the float time stamp of a point [ms] sits in its record (PointXYZINormal::curvature = 36: x y z pad | normal_x normal_y normal_z pad | intensity curvature);
 * points sorted by time (imu_processing.hpp:177-178); `poses`: IMUpose_ (host memory), `end_state`: the propagated state. */
int pcm_undistort(pcm_ctx *ctx, void *points, size_t n, size_t stride_bytes, size_t time_offset_bytes, int memory, const pcm_imu_pose *poses, int num_poses,
                  const pcm_lio_state *end_state);

/* pcl::VoxelGrid down-sampling of a scan: one centroid per occupied leaf, in increasing leaf-index order, every float
 * field of the record averaged (records of 3..16 floats, x y z first).  `out` must hold n records; *n_out = cells.
 * Replaces voxel_scan_.filter() of LaserMapping::Run (jueying_lio/src/laser_mapping.cc:323-328). */
int pcm_voxel_downsample(pcm_ctx *ctx, const void *points, size_t n, size_t stride_bytes, int memory, float leaf_size, void *out, size_t capacity_points, size_t *n_out);

/* pcl::VoxelGridLarge (jueying_slam/include/voxel_grid_large.cpp:23-255): pcm_voxel_downsample past 2^31 - 1 leaves.  While the
 * leaf index of a piece of the cloud overflows, the piece is cut in two along its longest axis (x where dx is strictly the
 * largest, else y where dy is, else z -- ties go to z) at mid = min + (max - min) / 2 in float: the first half keeps v <= mid, the
 * second v > mid, both in input order.  Every piece that does not overflow is filtered by the plain VoxelGrid in its own box, and
 * the results are concatenated in depth-first order, first half first.  A lattice cell that a cut plane crosses therefore gives
 * one centroid per piece.  Without an overflow the result is pcm_voxel_downsample's bit for bit.
 * A cut that would leave a piece whole (mid >= max: a flat axis chosen by the tie rule, adjacent floats) and a piece that still
 * overflows after PCM_VOXEL_LARGE_MAX_DEPTH cuts are PCM_ERR_OUT_OF_RANGE; pcm_last_error names the piece's extent and the axis.
 * Records of 3..16 floats, n <= 2^31 - 1, host or device buffers.  `out` must hold result->cells records: when capacity_points
 * is smaller, PCM_ERR_INVALID_ARGUMENT is returned with the needed count in result->cells.  An error writes nothing to `out`. */
#define PCM_VOXEL_LARGE_MAX_DEPTH 64
typedef struct pcm_voxel_large_result {
  uint64_t cells;            /* centroids written (needed, when capacity_points was too small) */
  uint64_t finite_points;    /* points with finite x, y, z: the others count nowhere */
  uint64_t pieces;           /* non-empty leaf pieces */
  uint32_t depth;            /* cuts above the deepest piece */
  uint32_t levels;           /* box passes run: depth + 1 */
  uint32_t host_waits;       /* times the call waited for the device */
  uint32_t reserved;
  uint64_t workspace_bytes;  /* device memory allocated for the call and released before it returned */
} pcm_voxel_large_result;
int pcm_voxel_downsample_large(pcm_ctx *ctx, const void *points, size_t n, size_t stride_bytes, int memory, float leaf_size, void *out, size_t capacity_points,
                               pcm_voxel_large_result *result);

/* pcl::ApproximateVoxelGrid (fast_gicp/src/align.cpp:136-147, kitti.cpp:81, src/python/main.cpp:46-92), one leaf for the three
 * axes.  In input order a point has the voxel (ix, iy, iz) = floorf(v * (1.0f / leaf_size)) and the history entry
 * h = (ix * 7171 + iy * 3079 + iz * 4231) & 511 (32-bit wrapping); an entry that holds another voxel is flushed -- its mean is
 * the next output record -- before the point joins it, and after the last point the entries in use are flushed in increasing h.
 * The result depends on the input order, and a voxel can come out more than once; count, membership and order are PCL's.
 * Every float of a record is averaged (records of 3..16 floats, x y z first); a mean is a double sum in a fixed order divided
 * in double and cast to float (pcm_voxel_downsample's rule; PCL keeps a running float sum).  A point with a non-finite x, y or z,
 * or with |floorf(v / leaf)| >= 2^31, is dropped, counted in *n_dropped (may be NULL) and neither joins nor breaks a run.
 * leaf_size <= 0 or not finite: PCM_ERR_INVALID_ARGUMENT; n <= 2^31 - 1.  `memory` holds for `points` and `out` alike, which do
 * not overlap.  *n_out = records of the result; when capacity_points is smaller, PCM_ERR_INVALID_ARGUMENT is returned with the
 * needed count in *n_out and nothing is written to `out`.  Two calls on one input give the same bytes. */
int pcm_approx_voxel_downsample(pcm_ctx *ctx, const void *points, size_t n, size_t stride_bytes, int memory, float leaf_size, void *out, size_t capacity_points,
                                size_t *n_out, size_t *n_dropped);

/* PointCloudPreprocess::AviaHandler (jueying_lio/src/pointcloud_preprocess.cc:44-88): the n points of a livox_ros_driver::CustomMsg
 * (20-byte records {uint32 offset_time; float x, y, z; uint8 reflectivity, tag, line; pad} -- msg->points.data()) filtered by line, tag,
 * point_filter_num, the duplicate test against the previous copied point and the blind radius, with the reference's own operator
 * precedence; the kept points leave in input order as pcl::PointXYZINormal records (48 bytes: x y z 1, 0 0 0 0, intensity, curvature
 * = offset_time / 1e6 [ms], 0 0).  `out` must hold n records; *n_out = kept points. */
int pcm_livox_filter(pcm_ctx *ctx, const void *custom_points, size_t n, int memory, int num_scans, int point_filter_num, double blind, void *out, size_t capacity_points,
                     size_t *n_out);

/* pclomp GICP-BFGS (jueying_slam's GICP_OMP option): the functor its BFGS minimises, evaluated on the device.
 * set_correspondences packs the outer iteration's correspondence set once -- tmp_src_/tmp_tgt_ (records of
 * stride_bytes, x y z first), tmp_idx_src_/tmp_idx_tgt_ (m indices, in range: checked for host memory only) and
 * mahalanobis_ (n_src Matrix4f, column-major, indexed by the source index) -- as estimateRigidTransformationBFGS sets
 * them (ndt_omp/include/pclomp/gicp_omp_impl.hpp:199-203, filled at :430-480).
 * fdf evaluates OptimizationFunctorWithIndices at x = (tx ty tz roll pitch yaw) on top of base_transformation_
 * (`base_T`, row-major 4x4): mode 0 = operator() (:246-274, f only), 1 = df (:278-327, g only), 2 = fdf (:331-365). */
int pcm_gicp_bfgs_set_correspondences(pcm_ctx *ctx, const void *src, size_t n_src, const void *tgt, size_t n_tgt, size_t stride_bytes, const int32_t *idx_src,
                                      const int32_t *idx_tgt, size_t m, const float *mahalanobis, int memory);
int pcm_gicp_bfgs_fdf(pcm_ctx *ctx, const float *base_T, const double *x, int mode, double *f, double *g);
/* The correspondence step of pclomp GICP's computeTransformation on the device (gicp_omp_impl.hpp:405-472), for a GICP context whose
 * source / target are *input_ / *target_ (regularization PCM_REG_PCLOMP = pclomp's computeCovariances): output = guess * input,
 * query = transformation * output, exact nearest target point within max_corr_dist, mahalanobis_ = (R C1 R^T + C2)^-1 cast to
 * float; the pairs, in source order, become the record set pcm_gicp_bfgs_fdf evaluates (cloud_src = output, as at :479) without
 * leaving the device.  `transformation`, `guess`: row-major 4x4 (transformation_, guess).  *m = number of pairs. */
int pcm_gicp_bfgs_update_correspondences(pcm_ctx *ctx, const float *transformation, const float *guess, size_t *m);
/* parity hook: the pairs of the last update (source_indices / target_indices, :466-472) and their 3x3 float matrices (row-major);
 * any pointer may be NULL */
int pcm_gicp_bfgs_get_correspondences(pcm_ctx *ctx, int32_t *idx_src, int32_t *idx_tgt, float *mahalanobis9, size_t capacity);

/* One LiDAR frame of LaserMapping::Run with the scan resident on the device from the driver message to the map update
 * (jueying_lio/src/laser_mapping.cc:323-347, 525-583): the hand-offs between the operators above never pass through host memory.
 *   pcm_lio_frame_begin   raw livox_ros_driver::CustomMsg points (20-byte records, see pcm_livox_filter) -- the ONLY host -> device
 *                         copy of the frame -- -> AviaHandler filter (pointcloud_preprocess.cc:44-88) -> motion compensation into
 *                         the frame-end pose (imu_processing.hpp:245-285; skipped when num_poses < 2) -> voxel-grid down-sampling
 *                         (laser_mapping.cc:323-328; leaf_size 0 = none) -> the result (scan_down_body_) becomes the SOURCE of
 *                         this object; *n_scan = its size.  The reference sorts the scan by time before compensating it
 *                         (imu_processing.hpp:177-178); the message order is kept here (a point's compensation depends on its own
 *                         stamp only and a Livox message is time-ordered).
 *   pcm_lio_update        the whole iterated Kalman update (esekfom.hpp:1526-1834) on the device: k ObsModel calls and the 23 x 23
 *                         algebra between them behind one synchronisation -- or pcm_obs_model x k with the caller's own filter
 *                         between the calls, as before
 *   pcm_lio_frame_end     = pcm_map_incremental with the updated state: add-filter + AddPoints, the map stays on the device
 * Target = the map (pcm_set_target once, then it slides by itself). */
typedef struct pcm_lio_frame_params {
  int32_t num_scans;         /* 6   config/livox.yaml:8  scan_line */
  int32_t point_filter_num;  /* 2   config/livox.yaml:40 */
  double blind;              /* 0.1 config/livox.yaml:9 (compared squared, pointcloud_preprocess.cc:70-72) */
  float leaf_size;           /* filter_size_surf 0.5  config/livox.yaml:38; 0 = no down-sampling */
  int32_t reserved;
} pcm_lio_frame_params;
int pcm_lio_frame_begin(pcm_ctx *ctx, const void *custom_points, size_t n, int memory, const pcm_lio_frame_params *params, const pcm_imu_pose *poses, int num_poses,
                        const pcm_lio_state *end_state, size_t *n_scan);
int pcm_lio_frame_end(pcm_ctx *ctx, const pcm_lio_state *state, float filter_size_map, int ekf_inited, size_t *num_added);
/* the current source scan, x y z per point in its stored order (tests: the scan pcm_lio_frame_begin produced); out may be NULL */
int pcm_get_source(pcm_ctx *ctx, float *out_xyz, size_t capacity_points, size_t *n);

/* The outputs of a frame and the saved map: the last block of LaserMapping::Run (jueying_lio/src/laser_mapping.cc:361-385) and
 * Finish (:887-900), on the records pcm_lio_frame_begin / pcm_lio_frame_begin_cloud left on the device.  Every output record is
 * 16 bytes, (x, y, z, intensity) as floats; every transform runs in double in Eigen's operation order and each coordinate is cast
 * to float (`po->x = p_global(0)`, :860-862).  `state`: the state the reference would publish with (state_point_).
 *   pcm_lio_frame_world   PublishFrameWorld's cloud (:747-762): dense = 1 every record of scan_undistort_ through
 *                         PointBodyToWorld(const PointType*, ...) (:855-864); dense = 0 scan_down_world_ as MapIncremental leaves it
 *                         (:540), in the order of the caller's scan (pcm_get_source's), whatever cfg.sort_source does inside
 *   pcm_lio_frame_body    PublishFrameBody (:794-808): PointBodyLidarToIMU (:877-885) over scan_undistort_
 *   pcm_lio_frame_effect  PublishFrameEffectWorld (:810-823): the points that gave a row to the LAST ObsModel call (corr_pts_,
 *                         :641-655), in scan order, through PointBodyToWorld(const V3F&, ...) (:866-875): intensity = |z| of the
 *                         float written.  *n equals that call's n_eff (pcm_obs_result.n_eff, pcm_lio_update_result.n_eff_last).
 *                         Under PCM_FLAG_LIO_REFERENCE_SEMANTICS the points are those with point_selected_surf_ set; otherwise
 *                         those with a plane and |p_body| > 81 pd2^2 at the state of that call.  No such call on this frame's
 *                         scan: PCM_ERR_NO_INPUT.
 *   pcm_lio_map_append    `*pcl_wait_save_ += *laserCloudWorld` (:777) straight into a grow-only device log (capacity x 1.5), and
 *                         the chunk counter of :779-790: scan_wait_num goes up by one; when pcd_save_interval > 0, the log is not
 *                         empty and scan_wait_num >= pcd_save_interval, chunk_ready = 1 and pcd_index is the k of the reference's
 *                         jueying_<k>.pcd: the caller fetches the log (pcm_lio_map_get / _export), writes the file and calls
 *                         pcm_lio_map_clear, as :787-789 do.  pcd_save_interval <= 0 never reports a chunk (:781).  The call
 *                         queues its work and returns; info may be NULL.
 *   pcm_lio_map_get       records [first, first + count) of the log
 *   pcm_lio_map_clear     pcl_wait_save_->clear(); scan_wait_num = 0 (:788-789); pcd_index and the buffer stay
 *   pcm_lio_map_export    Finish followed by the consumer of jueying.pcd (src/tool/pcd2map/src/pcd2map.cpp:60-72): leaf_size > 0
 *                         runs pcm_voxel_downsample_large over the log (more than 2^31 - 1 points: PCM_ERR_OUT_OF_RANGE);
 *                         z_min <= z_max then keeps, in order, the records with finite x, y, z and z_min <= z <= z_max
 *                         (pcl::PassThrough, setFilterLimitsNegative(false); at most 2^32 - 1 records enter it).  leaf_size 0 with
 *                         z_min > z_max: the log as it is.  No file is written.
 * Validity: the frame's records live in the context's pre-processing scratch.  Any later call on the context that takes that
 * scratch (pcm_voxel_downsample, pcm_approx_voxel_downsample, pcm_livox_filter, pcm_lidar_filter, pcm_undistort, a frame that fails) or replaces the source
 * (pcm_set_source, pcm_clear_source, pcm_swap_source_and_target) ends them: the three frame clouds and the append then return
 * PCM_ERR_NO_INPUT and pcm_last_error names that call.  The log is not affected.
 * Buffers: `out` in host or device memory (`memory`); NULL returns the count in *n only; a capacity below the count returns
 * PCM_ERR_INVALID_ARGUMENT with the count in *n and writes nothing.  The calls with `out` wait for the stream. */
typedef struct pcm_lio_map_info {
  uint64_t points, capacity, frames_appended, growths;   /* growths: allocations of the log, the first included */
  int32_t scan_wait_num, pcd_index, chunk_ready, reserved;
} pcm_lio_map_info;
int pcm_lio_frame_world(pcm_ctx *ctx, const pcm_lio_state *state, int dense, void *out, size_t capacity_points, int memory, size_t *n);
int pcm_lio_frame_body(pcm_ctx *ctx, const pcm_lio_state *state, void *out, size_t capacity_points, int memory, size_t *n);
int pcm_lio_frame_effect(pcm_ctx *ctx, const pcm_lio_state *state, void *out, size_t capacity_points, int memory, size_t *n);
int pcm_lio_map_append(pcm_ctx *ctx, const pcm_lio_state *state, int dense, int pcd_save_interval, pcm_lio_map_info *info);
int pcm_lio_map_info_get(pcm_ctx *ctx, pcm_lio_map_info *info);
int pcm_lio_map_get(pcm_ctx *ctx, size_t first, size_t count, void *out, int memory);
int pcm_lio_map_clear(pcm_ctx *ctx);
int pcm_lio_map_export(pcm_ctx *ctx, float leaf_size, double z_min, double z_max, void *out, size_t capacity_points, int memory, size_t *n);

/* esekf::update_iterated_dyn_share_modified of jueying_lio (IKFoM_toolkit/esekfom/esekfom.hpp:1526-1834, called at
 * laser_mapping.cc:347) for state_ikfom, on the device: every ObsModel call of the loop, the manifold algebra (SO3 / S2 boxplus and
 * boxminus, A_matrix, S2_Nx_yy, S2_Mx), the two 23 x 23 inverses per iteration and the closing covariance re-projection.  One call per
 * frame between pcm_lio_frame_begin and pcm_lio_frame_end (or after pcm_set_source); the context requirements are those of
 * pcm_obs_model (P2PLANE, source and target set).  One upload (state, P, parameters), max_iter + 1 rounds of kernels queued up front,
 * one download, one stream synchronisation; a round after the loop's exit returns at once.  The gain is the information form
 * (esekfom.hpp:1685-1713) for every n_eff >= 1: the dense form the reference takes for fewer than 23 effective points needs the rows
 * of h_x (equal in exact arithmetic).  DESIGN.md section 17. */
typedef struct pcm_lio_filter_state {   /* state_ikfom, use-ikfom.hpp:14-15; DOF 23 in this order; quaternions x, y, z, w */
  double pos[3], rot[4], off_R[4], off_T[3], vel[3], bg[3], ba[3], grav[3];
} pcm_lio_filter_state;
typedef struct pcm_lio_update_params {
  double R;                  /* 0.001  options.h:12 LASER_POINT_COV */
  int32_t max_iter;          /* 4      laser_mapping.cc:89 (livox.yaml: 3-4); 1 .. 15 */
  int32_t extrinsic_est_en;
  double limit[23];          /* 0.001 each, laser_mapping.cc:19 */
  int32_t reserved[8];
} pcm_lio_update_params;
typedef struct pcm_lio_update_result {
  int32_t iterations;        /* ObsModel calls made (<= max_iter + 1) */
  int32_t rematches;         /* of those, with converge = true */
  int32_t valid_calls;       /* calls with n_eff >= 1 */
  int32_t t;                 /* the loop's converge counter at exit */
  int32_t n_eff_last;
  int32_t status;            /* PCM_OK, or PCM_ERR_INTERNAL when the updated state or covariance is not finite */
  double sum_h2_last;
  int32_t reserved[8];
} pcm_lio_update_result;
void pcm_lio_default_update_params(pcm_lio_update_params *params);
/* x: in the propagated state x_, out the updated one; P: 23 x 23 row-major, in P_ propagated, out updated (as the reference leaves its
 * member: untouched when no call was valid) */
int pcm_lio_update(pcm_ctx *ctx, const pcm_lio_update_params *params, pcm_lio_filter_state *x, double *P, pcm_lio_update_result *result);
/* parity hook: ObsModel call `call` (0-based) of the last pcm_lio_update -- the state it was evaluated at, its converge flag, n_eff,
 * HTH upper triangle (78) + HTh (12), and dx_ (23; zeros for an invalid call).  Any pointer may be NULL. */
int pcm_lio_update_trace(pcm_ctx *ctx, int call, pcm_lio_filter_state *x, int32_t *converge, int32_t *n_eff, double *sums90, double *dx23);

/* What ImuProcess::Process does before the frame (jueying_lio/include/imu_processing.hpp:287-318): IMUInit and the init branch
 * (:113-163, :295-315; host arithmetic, no context), and for every later frame the forward loop of UndistortPcl with esekf::predict
 * per IMU sample and the closing predict (:167-243, esekfom.hpp:269-374) on the device -- one upload, one launch of one wave that
 * runs the whole sample loop, one download, one stream synchronisation.  The members of ImuProcess live in the caller's
 * pcm_lio_imu_state.  Outputs feed the calls above with no other glue: poses / *num_poses (IMUpose_) and the pose part of x go to
 * pcm_lio_frame_begin, pcm_lio_frame_begin_cloud or pcm_undistort, x and P (x_, P_) to pcm_lio_update.  DESIGN.md section 18. */
typedef struct pcm_imu_sample { double t, acc[3], gyr[3]; } pcm_imu_sample;   /* sensor_msgs::Imu: stamp, linear_acceleration, angular_velocity */
typedef struct pcm_lio_imu_state {                                            /* the members of ImuProcess, owned by the caller */
  double mean_acc[3], mean_gyr[3], cov_acc[3], cov_gyr[3], cov_bias_gyr[3], cov_bias_acc[3];
  double cov_acc_scale[3], cov_gyr_scale[3];                                  /* SetAccCov / SetGyrCov */
  double lidar_T_wrt_imu[3], lidar_R_wrt_imu[4];                              /* SetExtrinsic; quaternion x y z w */
  double angvel_last[3], acc_s_last[3], last_lidar_end_time;
  pcm_imu_sample last_imu;
  int32_t init_iter_num, first_frame, need_init, reserved[5];
} pcm_lio_imu_state;
/* the constructor's values (:71-84); acc_s_last, which the reference never initialises, is zero; the two scales are 0.1 (laser_mapping.cc:97-98) */
void pcm_lio_default_imu_state(pcm_lio_imu_state *s);
/* one frame of the init branch over the n >= 1 samples of the frame: running mean / covariance, then grav, bg, the extrinsics and
 * the initial P (23 x 23 row-major) into x and P; s->need_init drops to 0 once init_iter_num exceeds MAX_INI_COUNT (20) */
int pcm_lio_imu_init(pcm_lio_imu_state *s, const pcm_imu_sample *imu, int n, pcm_lio_filter_state *x, double *P);
/* one frame of forward propagation on any context (its device and stream are all it uses).  1 <= n <= 1024 samples
 * (PCM_ERR_OUT_OF_RANGE beyond), capacity >= n + 1 poses, s->need_init == 0.  x, P: in the filter's x_, P_; out the propagated ones.
 * Updates s->last_imu, last_lidar_end_time, angvel_last, acc_s_last as the reference does; a bad argument leaves s, x and P untouched. */
int pcm_lio_propagate(pcm_ctx *ctx, pcm_lio_imu_state *s, const pcm_imu_sample *imu, int n, double pcl_beg_time, double pcl_end_time, pcm_lio_filter_state *x,
                      double *P, pcm_imu_pose *poses, int capacity, int *num_poses);

/* Batch of independent registration objects on one device (BASELINE config 3:
 * independent scan/submap pairs): all GN/LM loops advance in lock-step kernel
 * launches, no host round trip per iteration.  `guesses` = n x 16 floats.
 * `host_out` (n results) and/or `device_out` (device pointer to n packed
 * pcm_result records, e.g. the buffer handed to an RCCL all_gather) may be NULL. */
int pcm_align_batch(pcm_ctx *const *ctxs, int n, const float *guesses, pcm_result *host_out, void *device_out);

/*
 * LOAM (LIO-SAM style) scan-to-map registration of jueying_slam: scan2MapOptimization
 * (jueying_slam/src/mapOptmization.cpp:1560-1586; cornerOptimization :1255-1347, surfOptimization :1349-1419,
 * combineOptimizationCoeffs :1421-1440, LMOptimization :1442-1558) and the fitness scores of its localisation variant
 * (jueying_slam/src/localization.cpp:674-1031).  A context created with PCM_MODEL_LOAM holds two maps (corner, surf) and one
 * scan of two feature clouds; the whole iteration loop runs on the device.  The pose is transformTobeMapped:
 * (roll, pitch, yaw, x, y, z), floats.  transformUpdate (IMU blending and clamps) stays with the caller.  DESIGN.md section 9.
 */
typedef struct pcm_loam_params {
  int32_t iter_num;              /* 30   utility.h:253 (iter_num) */
  int32_t edge_min_valid;        /* 10   utility.h:267 edgeFeatureMinValidNum: run only if corner features > this ... */
  int32_t surf_min_valid;        /* 100  utility.h:268 surfFeatureMinValidNum: ... and surf features > this */
  int32_t reserved0;
  double rot_conv_deg;           /* 0.01 deltaR threshold (mapOptmization.cpp:1551); the localisation nodes use 0.05 (localization.cpp:985) */
  double trans_conv_cm;          /* 0.05 deltaT threshold */
  double degeneracy_threshold;   /* 100  eignThre (mapOptmization.cpp:1524) */
  float search_cell;             /* 1.0  cell size [m] of the maps' search grid, >= 1.0; speed only (results do not depend on it) */
  int32_t reserved[7];
} pcm_loam_params;

typedef struct pcm_loam_result {
  float x[6];                    /* transformTobeMapped after the loop */
  int32_t iterations;            /* loop iterations run (iter_num when it did not converge; 0 when it did not run) */
  int32_t converged;             /* LMOptimization returned true */
  int32_t degenerate;            /* isDegenerate of iteration 0 */
  int32_t status;                /* PCM_OK or PCM_ERR_TOO_FEW_FEATURES */
  double eigenvalues[6];         /* of A^T A at iteration 0, descending (0 when iteration 0 had < 50 rows) */
  int32_t num_corner;            /* selected corner rows of the last iteration */
  int32_t num_surf;              /* selected surf rows of the last iteration */
  double corner_fitness;         /* Corner_fitness_score / Surf_fitness_score of the last iteration: mean sqDis[0] over the features */
  double surf_fitness;           /*   with sqDis[0] <= 1, the largest double when at most one (localization.cpp:1012-1021) */
  int32_t maps_built;            /* 1: this call (re)built the search grids of the two maps */
  int32_t reserved;
} pcm_loam_result;

void pcm_loam_default_params(pcm_loam_params *params);
/* laserCloudCornerFromMapDS / laserCloudSurfFromMapDS (records of stride_bytes, x y z first).  An equal non-zero tag makes the call a
 * no-op (the maps and their search grids are kept). */
int pcm_loam_set_target(pcm_ctx *ctx, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes, int memory, uint64_t tag);
/* laserCloudCornerLastDS / laserCloudSurfLastDS: the scan's features in the body frame; same tag rule */
int pcm_loam_set_source(pcm_ctx *ctx, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes, int memory, uint64_t tag);
/* scan2MapOptimization from x6_in; params NULL = defaults */
int pcm_loam_align(pcm_ctx *ctx, const pcm_loam_params *params, const float x6_in[6], pcm_loam_result *result);
/* n independent contexts on one device in lock-step launches; x6_in = n x 6 floats, results = n records.  Returns the first
 * non-OK status of a context (each record carries its own). */
int pcm_loam_align_batch(pcm_ctx *const *ctxs, int n, const pcm_loam_params *params, const float *x6_in, pcm_loam_result *results);
/* parity hook: one correspondence pass at the fixed pose x6.  corner_out / surf_out: (coeff.x, coeff.y, coeff.z, coeff.intensity)
 * per feature, NaN when the feature is not selected (4 floats each).  AtA (36, row-major), AtB (6): the normal equations as the
 * step reads them.  counts: selected corner rows, selected surf rows, corner / surf features with sqDis[0] <= 1.  Any may be NULL. */
int pcm_loam_coefficients(pcm_ctx *ctx, const float x6[6], float *corner_out, float *surf_out, double AtA[36], double AtB[6], int32_t counts[4]);
/* parity hook: the 5 nearest map points (caller indices, ascending (d^2, index)) of every feature at x6 among those with d^2 <= 1,
 * -1 where there are fewer; 5 int32 per feature.  Either may be NULL. */
int pcm_loam_neighbours(pcm_ctx *ctx, const float x6[6], int32_t *corner_nn, int32_t *surf_nn);

/*
 * LOAM front end of jueying_slam: imageProjection (projectPointCloud / cloudExtraction, imageProjection.cpp:736-823),
 * featureExtraction (calculateSmoothness / markOccludedPoints / extractFeatures with one pcl::VoxelGrid per ring,
 * featureExtraction.cpp:84-247) and downsampleCurrentScan's two mapping VoxelGrids (mapOptmization.cpp:1232-1247), on the device.
 * Input: ring-tagged records (PointXYZIRT, imageProjection.cpp:7-19: x y z floats at 0, uint8 intensity, uint16 ring; 48 / 16 / 32
 * by default); a point with a non-finite coordinate is skipped.  The entry points without a deskew descriptor never read the
 * timestamp (the reference's deskew is the identity as written); the *_deskew entry points below take IMU /
 * odometry tables, read every record's time field and run the live deskewPoint in front of the features (section 34), and the
 * *_cloud entry points further down make the records themselves, ring and time included, from a raw organised cloud (section 36).
 * The context keeps the nodes' cross-frame arrays (zero at creation), so a stream of frames through one context reproduces the
 * nodes frame for frame.  Needs a PCM_MODEL_LOAM context.
 */
#define PCM_LOAM_FEATURES_FORCE_SERIAL_SORT 1u   /* flags: every sector through the serial std::sort restatement (tests) */

typedef struct pcm_loam_feature_params {
  int32_t n_scan;                /* 16    utility.h:241 N_SCAN (<= 256) */
  int32_t horizon_scan;          /* 1800  :242 Horizon_SCAN (<= 4096) */
  int32_t downsample_rate;       /* 1     :244 downsampleRate (rows with ring % rate != 0 are skipped; the row is the ring) */
  int32_t area_num;              /* 6     :252 sectors per ring, >= 1 (every value within these caps runs, area_num 1 at
                                  *       horizon_scan 4096 included: one sector sorts in LDS up to 4096 entries) */
  float min_range;               /* 1.0   :223 */
  float max_range;               /* 150.0 :224 */
  float edge_threshold;          /* 0.1   :265 (the configs use 1.0) */
  float surf_threshold;          /* 0.1   :266 */
  float odometry_surf_leaf;      /* 0.2   :270 per-ring VoxelGrid of the surf scan, > 0 */
  float mapping_corner_leaf;     /* 0.2   :271 downsampleCurrentScan; 0 = no down-sampling */
  float mapping_surf_leaf;       /* 0.2   :272 same; the localisation node passes 1.5 x (localization.cpp:160) */
  uint32_t flags;                /* PCM_LOAM_FEATURES_* */
  int32_t reserved[8];
} pcm_loam_feature_params;

typedef struct pcm_loam_features_result {
  int32_t num_extracted;         /* extractedCloud */
  int32_t num_corner_scan;       /* cornerCloud (before the mapping VoxelGrid) */
  int32_t num_surf_scan;         /* surfaceCloud (rings after their own VoxelGrid, before the mapping one) */
  int32_t num_corner;            /* laserCloudCornerLastDS */
  int32_t num_surf;              /* laserCloudSurfLastDS */
  int32_t sectors;               /* sectors sorted */
  int32_t sectors_serial;        /* of which through the serial std::sort restatement: ties that could change the selection,
                                  * a tie group of more than 256 entries, or a tied minimum in the sector that holds slot 4 */
  int32_t status;                /* PCM_OK, PCM_ERR_OUT_OF_RANGE (VoxelGrid index overflow) */
  int32_t reserved[8];
} pcm_loam_features_result;

void pcm_loam_default_feature_params(pcm_loam_feature_params *params);
/* one frame to host PointXYZI records (x, y, z, intensity): corner = laserCloudCornerLastDS, surf = laserCloudSurfLastDS.  The
 * context's LOAM source is not touched.  params NULL = defaults.  Capacities in points; when too small the counts are in *res,
 * the frame has advanced the cross-frame state and PCM_ERR_INVALID_ARGUMENT is returned. */
int pcm_loam_extract_features(pcm_ctx *ctx, const void *points, size_t n, size_t stride_bytes, size_t intensity_offset_bytes, size_t ring_offset_bytes,
                              int memory, const pcm_loam_feature_params *params, float *corner, size_t cap_corner, float *surf, size_t cap_surf,
                              pcm_loam_features_result *res);
/* the same frame's features become the context's LOAM source without leaving the device (pcm_loam_set_source's state; then
 * pcm_loam_align as before) */
int pcm_loam_frame_begin(pcm_ctx *ctx, const void *points, size_t n, size_t stride_bytes, size_t intensity_offset_bytes, size_t ring_offset_bytes,
                         int memory, const pcm_loam_feature_params *params, pcm_loam_features_result *res);
/* n frames of n distinct contexts on one device in one set of launches; each context keeps its own cross-frame state */
int pcm_loam_frame_begin_batch(pcm_ctx *const *ctxs, int n, const void *const *points, const size_t *n_points, size_t stride_bytes,
                               size_t intensity_offset_bytes, size_t ring_offset_bytes, int memory, const pcm_loam_feature_params *params,
                               pcm_loam_features_result *results);
/* parity hook: the last frame's intermediate arrays.  counts: extracted points n, cornerCloud, surfaceCloud, n_scan.
 * start_ring / end_ring: n_scan int32; col_ind, range, curvature, neighbor_picked (after markOccludedPoints), label (final):
 * n entries of the context's arrays; cloud: n x 4 floats; corner_scan / surf_scan: cornerCloud in pick order / surfaceCloud,
 * 4 floats per point.  Any pointer may be NULL. */
int pcm_loam_feature_info(pcm_ctx *ctx, int32_t counts[4], int32_t *start_ring, int32_t *end_ring, int32_t *col_ind, float *range, float *cloud,
                          float *curvature, int32_t *neighbor_picked, int32_t *label, float *corner_scan, float *surf_scan);

/*
 * IMU / odometry deskew in front of the LOAM features (an option of this library, off by default).
 * imageProjection.cpp:709 hands findRotation / findPosition a relative point time, so the reference's deskewPoint is the identity
 * as written; new_localization.cpp:1948-1977 holds the live form, pointTime = timeScanCur + relTime, which these entry points run:
 * pointTime = time_scan_cur + (t_i - t_0), t_0 the stamp of record 0 of the input, the difference in the field's type.  The column,
 * the raw range test and the ownership of a cell stay the raw point's; the stored point and its range (and through it smoothness,
 * occlusion and the features) are the deskewed point's (imageProjection.cpp:760-782).  transStartInverse comes from the first
 * record that passes the ring, column and range tests (firstPointFlag).  pcm_loam_feature_info then returns cloud_deskewed.
 *
 * A table is n entries in arrival order (the times need not increase; the look-up is findRotation's linear scan, served by a
 * binary search over the prefix maximum of the times): at most 1024 (PCM_ERR_UNSUPPORTED beyond; the reference's arrays hold
 * imuFrequency = 500 and overflow).  n_odom = 0: no odometry table, the translation is 0.  A NULL descriptor or imu_available = 0
 * is the call without _deskew, bit for bit.  A time field past the record, or one that is not aligned to its size in every record
 * (device records are read where they lie): PCM_ERR_INVALID_ARGUMENT before any device work.
 */
#define PCM_LOAM_TIME_DOUBLE 0   /* PointXYZIRT's `double timestamp` (offset 24 of the 48-byte record) */
#define PCM_LOAM_TIME_FLOAT 1    /* the 32-byte fused XYZIRT record's float (pcm_scan_fuse, PCM_SCAN_OUT_XYZIRT) */
#define PCM_LOAM_DESKEW_READY 0
#define PCM_LOAM_DESKEW_WAITING 1   /* deskewInfo's "Waiting for IMU data ...": not an error, nothing popped or written */

typedef struct pcm_loam_deskew {
  double time_scan_cur;          /* timeScanCur: the header stamp of the scan */
  const double *imu_time;        /* imuTime, imuRotX / Y / Z: n_imu host doubles each */
  const double *imu_rot_x;
  const double *imu_rot_y;
  const double *imu_rot_z;
  const double *odom_time;       /* odomTime, odomIncreX / Y / Z: n_odom host doubles each (NULL with n_odom = 0) */
  const double *odom_incre_x;
  const double *odom_incre_y;
  const double *odom_incre_z;
  int32_t n_imu;                 /* imuPointerCur + 1 */
  int32_t n_odom;                /* OdomPointerCur + 1, or 0 */
  int32_t imu_available;         /* cloudInfo.imuAvailable; 0: the points stay as they are */
  int32_t time_kind;             /* PCM_LOAM_TIME_* of the field at time_offset_bytes */
  size_t time_offset_bytes;
  int32_t reserved[8];
} pcm_loam_deskew;

typedef struct pcm_loam_imu_sample { double t, gyro[3]; } pcm_loam_imu_sample;     /* sensor_msgs::Imu through imuConverter: stamp, angular_velocity */
typedef struct pcm_loam_odom_sample { double t, xyz[3]; } pcm_loam_odom_sample;   /* nav_msgs::Odometry: stamp, pose.pose.position */

typedef struct pcm_loam_deskew_input {
  double time_scan_cur;          /* timeScanCur */
  double time_scan_next;         /* timeScanNext (imageProjection.cpp: the `back < timeScanNext` gate and the `> timeScanNext + 0.01` break);
                                  * +inf: new_localization.cpp's form, neither */
  const pcm_loam_imu_sample *imu;     /* imuQueue, front first */
  const pcm_loam_odom_sample *odom;   /* odomQueue, front first */
  int32_t n_imu;
  int32_t n_odom;
  int32_t reserved[4];
} pcm_loam_deskew_input;

typedef struct pcm_loam_deskew_result {
  int32_t status;                /* PCM_LOAM_DESKEW_READY or PCM_LOAM_DESKEW_WAITING */
  int32_t imu_skipped;           /* samples older than timeScanCur - 0.01 at the front of each queue: the reference pops them, the caller */
  int32_t odom_skipped;          /*   pops as many from its own */
  int32_t n_imu;                 /* table entries written */
  int32_t n_odom;
  int32_t imu_available;         /* cloudInfo.imuAvailable */
  int32_t odom_available;        /* cloudInfo.odomAvailable */
  int32_t odom_deskew;           /* odomDeskewFlag */
  int32_t start_odom_index;      /* startOdomMsg as an index into `odom` as given (initialGuess* are the caller's: getRPY is not here); -1: none */
  int32_t reserved[7];
} pcm_loam_deskew_result;

/* deskewInfo = the gate, imuDeskewInfo, odomDeskewInfo (imageProjection.cpp:483-642, new_localization.cpp:1733-1886); no context.
 * imu_table / odom_table: four rows of cap_imu / cap_odom doubles (time, x, y, z), written up to the counts of *res; a capacity
 * below a count: PCM_ERR_INVALID_ARGUMENT with the counts in *res; more than 1024 entries: PCM_ERR_UNSUPPORTED.  deskew (may be
 * NULL) is filled to point at the two tables, with time_offset_bytes = 24 and PCM_LOAM_TIME_DOUBLE (PointXYZIRT). */
int pcm_loam_deskew_tables(const pcm_loam_deskew_input *in, double *imu_table, size_t cap_imu, double *odom_table, size_t cap_odom, pcm_loam_deskew *deskew,
                           pcm_loam_deskew_result *res);
/* pcm_loam_extract_features / pcm_loam_frame_begin / pcm_loam_frame_begin_batch with the deskew in front; deskew NULL = those calls.
 * The batch takes NULL or one descriptor per frame, any of which may be NULL. */
int pcm_loam_extract_features_deskew(pcm_ctx *ctx, const void *points, size_t n, size_t stride_bytes, size_t intensity_offset_bytes, size_t ring_offset_bytes,
                                     int memory, const pcm_loam_feature_params *params, float *corner, size_t cap_corner, float *surf, size_t cap_surf,
                                     pcm_loam_features_result *res, const pcm_loam_deskew *deskew);
int pcm_loam_frame_begin_deskew(pcm_ctx *ctx, const void *points, size_t n, size_t stride_bytes, size_t intensity_offset_bytes, size_t ring_offset_bytes,
                                int memory, const pcm_loam_feature_params *params, pcm_loam_features_result *res, const pcm_loam_deskew *deskew);
int pcm_loam_frame_begin_batch_deskew(pcm_ctx *const *ctxs, int n, const void *const *points, const size_t *n_points, size_t stride_bytes,
                                      size_t intensity_offset_bytes, size_t ring_offset_bytes, int memory, const pcm_loam_feature_params *params,
                                      pcm_loam_features_result *results, const pcm_loam_deskew *const *deskew);

/*
 * cachePointCloud on the device: from the driver's organised cloud to the node's laserCloudIn (DESIGN.md section 36;
 * imageProjection.cpp:258-479, new_localization.cpp:1560-1731, myremoveNaNFromPointCloud :211-256).  For the three RoboSense
 * types the reference makes the ring, the per-point time (when the message has none) and the NaN removal there, in per-point host
 * loops; here raw message bytes go in and the records pcm_loam_frame_begin[_deskew] reads come out, in a buffer of the context.
 *
 * Input: height x width records of point_step bytes, record (w, h) at index h * width + w, in host or device memory at a 4-byte
 * aligned address.  point_step is a multiple of 2; the offsets of x (y, z behind it), of a float intensity and of the time field
 * are multiples of 4 inside the record, the ring's a multiple of 2; device records are read where they lie.  The intensity, the
 * ring and the time are copied in their own kind: a kind that is not the output record's is PCM_ERR_INVALID_ARGUMENT (PCL's field
 * matching is not in the reference tree, so no conversion is defined).  An absent ring or time field leaves 0 in the record.
 *
 * Output (record_kind), padding bytes zero:
 *   PCM_LOAM_CLOUD_MAPPING       48 bytes (imageProjection.cpp:7-19): x y z 1.0f, uint8 intensity @16, double timestamp @24, uint16 ring @32
 *   PCM_LOAM_CLOUD_LOCALIZATION  32 bytes (new_localization.cpp:26-38, the layout pcm_scan_fuse writes): float intensity @16,
 *                                uint16 ring @20, float time @24
 *
 * synth_ring (RoboSense types): for h in [0, height-1) and w in [0, width-1) -- the last row and the last column are NOT written
 * (:326-327) and keep the message's ring, or 0 -- ring = h < 8 ? h : 15 - (h - 8) (RSLIDAR_16, :328) or h (RUBY :369, RSLIDAR_32
 * :444), converted to uint16.  When it runs is the caller's: the node's static ringFlag, and the difference between
 * imageProjection.cpp:437 and new_localization.cpp:1692, stay with the caller.
 * synth_time (RoboSense types): the same bounds; evaluated as written, in double, rounded once to float for the 32-byte record:
 *   RSLIDAR_16    h*2.8*1e-6 + w*55.5*1e-6                                                  (:349)
 *   RSLIDAR_RUBY  3.236*((((h+1)%64==0?64:(h+1)%64)-1)/4.f)*1e-6 + w*55.552*1e-6            (:386, the division in float)
 *   RSLIDAR_32    (w*55.52 + h%16*2.88 + 1.44*float(h/16))*1e-6                             (:461)
 * The reference synthesises on the first frame only (deskewFlag becomes 1); whether a later frame does is this flag, per call.
 * is_dense == 0 on a RoboSense type: records with a non-finite x, y or z are dropped, the rest keep their order; is_dense == 1:
 * every record is copied, NaN or not.  So record 0 of the prepared cloud -- whose time is the deskew's t_0 -- is the first finite
 * record of a non-dense cloud.  VELODYNE: the records are copied; is_dense == 0, an absent ring field (the node shuts down,
 * :280-303) or a synth flag is PCM_ERR_INVALID_ARGUMENT; an absent time field is reported (time_available = 0).
 * This library's definitions: height == 0 or width == 0 is an empty cloud and PCM_OK (the reference's unsigned height-1 is
 * undefined there); a ring beyond n_scan is no error here (the projection skips the point).  myPassThrough (:182-209) has no
 * call site and is not built.
 */
#define PCM_LOAM_LIDAR_VELODYNE 0        /* utility.h:116-121, elidar_type */
#define PCM_LOAM_LIDAR_RSLIDAR_RUBY 1
#define PCM_LOAM_LIDAR_RSLIDAR_16 2
#define PCM_LOAM_LIDAR_RSLIDAR_32 3
#define PCM_LOAM_CLOUD_MAPPING 0
#define PCM_LOAM_CLOUD_LOCALIZATION 1
#define PCM_LOAM_INTENSITY_UINT8 0
#define PCM_LOAM_INTENSITY_FLOAT 1
#define PCM_LOAM_RING_UINT16 0
#define PCM_LOAM_FIELD_ABSENT ((size_t)-1)   /* ring_offset_bytes / time_offset_bytes: the message has no such field */

typedef struct pcm_loam_cloud_desc {
  uint32_t height;
  uint32_t width;
  size_t point_step;
  size_t xyz_offset_bytes;
  size_t intensity_offset_bytes;
  size_t ring_offset_bytes;      /* or PCM_LOAM_FIELD_ABSENT */
  size_t time_offset_bytes;      /* or PCM_LOAM_FIELD_ABSENT */
  int32_t intensity_kind;        /* PCM_LOAM_INTENSITY_*: must be the record's (UINT8 mapping, FLOAT localisation) */
  int32_t ring_kind;             /* PCM_LOAM_RING_UINT16 */
  int32_t time_kind;             /* PCM_LOAM_TIME_*: must be the record's (DOUBLE mapping, FLOAT localisation) when the field is there */
  int32_t is_dense;
  int32_t lidar_type;            /* PCM_LOAM_LIDAR_* */
  int32_t record_kind;           /* PCM_LOAM_CLOUD_* */
  int32_t synth_ring;
  int32_t synth_time;
  int32_t reserved[8];
} pcm_loam_cloud_desc;

typedef struct pcm_loam_cloud_result {
  uint64_t n_in;                 /* height * width */
  uint64_t n_out;                /* records of the prepared cloud */
  uint64_t n_nonfinite;          /* records dropped for a non-finite x, y or z (a dense cloud is not examined: 0) */
  int32_t ring_synthesised;
  int32_t time_synthesised;
  int32_t time_available;        /* the records carry a time: the message's field or the synthesised one */
  int32_t status;
  int32_t reserved[8];
} pcm_loam_cloud_result;

/* the descriptor of the reference's own struct of that node (the record kind's layout as the message's: point_step 48 or 32, both
 * fields present), height = width = 0, is_dense = 1; the RoboSense types with synth_ring = 1, and synth_time = 0 (a time field is there) */
int pcm_loam_cloud_default_desc(int lidar_type, int record_kind, pcm_loam_cloud_desc *desc);
/* out NULL: the prepared cloud stays in a buffer of the context (pcm_loam_cloud_cached).  Else `out` takes up to capacity_points
 * records (device memory: 16-byte aligned); a capacity below n_out returns the counts in *result and PCM_ERR_INVALID_ARGUMENT, and
 * nothing is written past the capacity.  One synchronisation (the kept count of a non-dense cloud).  Needs a PCM_MODEL_LOAM
 * context.  Every misuse -- an offset past point_step, a misaligned field, an unknown type or kind, another model's context --
 * returns its status with a readable pcm_last_error before any device work. */
int pcm_loam_cloud_prepare(pcm_ctx *ctx, const void *data, const pcm_loam_cloud_desc *desc, int memory, void *out, size_t capacity_points, int out_memory,
                           pcm_loam_cloud_result *result);
/* the records of the last pcm_loam_cloud_prepare with out = NULL (or pcm_loam_frame_begin_cloud) on the device, alive until the
 * next such call; *n = 0 and a null pointer when there are none */
int pcm_loam_cloud_cached(pcm_ctx *ctx, const void **device_records, size_t *n, size_t *stride_bytes);
/* pcm_loam_cloud_prepare into the context's buffer, then pcm_loam_frame_begin_deskew on it where it lies: the raw cloud is the only
 * bulk upload of the frame.  The front end reads the record kind's layout (intensity @16: of a float intensity its low byte, as
 * with pcm_scan_fuse's records).  deskew may be NULL; its time_offset_bytes and time_kind are overridden by the record kind's, and
 * it is ignored when time_available == 0. */
int pcm_loam_frame_begin_cloud(pcm_ctx *ctx, const void *data, const pcm_loam_cloud_desc *desc, int memory, const pcm_loam_feature_params *feature_params,
                               pcm_loam_features_result *features_result, const pcm_loam_deskew *deskew, pcm_loam_cloud_result *cloud_result);
/* n clouds of n distinct contexts on one device: one round of launches prepares them all (one read-back), then
 * pcm_loam_frame_begin_batch_deskew.  The descriptors may differ in everything but record_kind.  deskews: NULL, or one per frame
 * (any may be NULL). */
int pcm_loam_frame_begin_cloud_batch(pcm_ctx *const *ctxs, int n, const void *const *data, const pcm_loam_cloud_desc *descs, int memory,
                                     const pcm_loam_feature_params *feature_params, pcm_loam_features_result *results, const pcm_loam_deskew *const *deskews,
                                     pcm_loam_cloud_result *cloud_results);

/*
 * LOAM key-frame store and surrounding-key-frame submap of jueying_slam on the device: saveKeyFramesAndFactor's clouds
 * (mapOptmization.cpp:1779-1846), correctPoses (:1886-1917), extractSurroundingKeyFrames (:1153-1230) and loopFindNearKeyframes
 * (:972-1018).  A PCM_MODEL_LOAM context keeps every key frame's corner / surf cloud (body frame, PointXYZI) and pose on the
 * device; pcm_loam_submap_update selects the key frames as the reference does, transforms, concatenates and down-samples their
 * clouds and makes the result the context's LOAM target, so a mapping frame is
 *   pcm_loam_frame_begin -> pcm_loam_submap_update -> pcm_loam_align -> pcm_loam_keyframe_add
 * with the scan as the only bulk upload.  DESIGN.md section 11.
 */
typedef struct pcm_loam_submap_params {
  float search_radius;           /* 50.0  utility.h:282 surroundingKeyframeSearchRadius */
  float keypose_density;         /* 1.0   utility.h:283 surroundingKeyframeDensity: leaf of the VoxelGrid over the key poses, > 0 */
  float corner_leaf;             /* 0.2   utility.h:271 mappingCornerLeafSize; 0 = no down-sampling */
  float surf_leaf;               /* 0.2   utility.h:272 mappingSurfLeafSize; 0 = no down-sampling */
  double recent_window_s;        /* 10.0  mapOptmization.cpp:1174: key frames younger than this are always taken */
  int32_t reserved[8];
} pcm_loam_submap_params;

typedef struct pcm_loam_submap_result {
  int32_t num_keyframes;         /* K */
  int32_t num_near;              /* key poses inside the radius of the last one */
  int32_t num_pose_leaves;       /* leaves of the VoxelGrid over them */
  int32_t num_selected;          /* list entries used (a key frame may be used more than once) */
  int32_t num_skipped;           /* list entries farther than the radius from the last key pose */
  int32_t num_corner_in;         /* points of the concatenated clouds, before the VoxelGrids */
  int32_t num_surf_in;
  int32_t num_corner_map;        /* laserCloudCornerFromMapDS / laserCloudSurfFromMapDS */
  int32_t num_surf_map;
  int32_t rebuilt;               /* 0: selection, poses and leaves equal those of the last update: nothing done on the device */
  int32_t status;                /* PCM_OK, PCM_ERR_OUT_OF_RANGE (VoxelGrid index overflow) */
  int32_t reserved[5];
} pcm_loam_submap_result;

void pcm_loam_default_submap_params(pcm_loam_submap_params *params);
/* saveKeyFramesAndFactor: key frame K gets pose6 (roll, pitch, yaw, x, y, z, as pcm_loam_align), time and the two clouds (records
 * of stride_bytes, x y z first, intensity the fourth float when stride_bytes >= 16, else 0).  corner == NULL and surf == NULL:
 * the context's current LOAM source is copied on the device (after pcm_loam_frame_begin with the features' averaged intensity,
 * after pcm_loam_set_source with the records' fourth float).  Returns PCM_OK; pcm_loam_keyframe_count gives the new K.
 * The fourth float is read as it lies in memory: a pcl::PointXYZI buffer must NOT be passed as it is (its fourth float is the
 * padding of the xyz block, the intensity sits at byte 16 of 32); repack to (x, y, z, intensity) records first, as
 * pcm_amd::LoamKeyFrameMap and LoamScanToMap::setInputFeatures do.  The same holds for pcm_loam_set_source when key frames are
 * to be taken from the source. */
int pcm_loam_keyframe_add(pcm_ctx *ctx, const float pose6[6], double time, const void *corner, size_t n_corner, const void *surf, size_t n_surf,
                          size_t stride_bytes, int memory);
/* correctPoses: key frames first .. first + n - 1 get new poses (n x 6 floats); their times and clouds stay */
int pcm_loam_keyframe_set_poses(pcm_ctx *ctx, int first, int n, const float *pose6);
int pcm_loam_keyframe_count(pcm_ctx *ctx);   /* K, or a negative pcm_status */
int pcm_loam_keyframe_clear(pcm_ctx *ctx);
/* one stored key frame as host PointXYZI records (body frame); capacities in points; the counts are always set, and
 * PCM_ERR_INVALID_ARGUMENT is returned when a capacity is too small (corner / surf may be NULL with capacity 0 to ask for them) */
int pcm_loam_keyframe_get(pcm_ctx *ctx, int key, float *corner, size_t cap_corner, float *surf, size_t cap_surf, size_t *n_corner, size_t *n_surf);
/* extractSurroundingKeyFrames at timeLaserInfoCur = time_cur: the result becomes the context's LOAM target (the caller index of a
 * map point is its position in the down-sampled cloud).  params NULL = defaults.  No key frame yet: PCM_OK, nothing done. */
int pcm_loam_submap_update(pcm_ctx *ctx, const pcm_loam_submap_params *params, double time_cur, pcm_loam_submap_result *result);
/* loopFindNearKeyframes (wrt_key < 0: every key frame under its own pose) / loopFindNearKeyframesWithRespectTo (all under the pose
 * of wrt_key): key frames key - search_num .. key + search_num inside [0, K), corner then surf of each, one VoxelGrid(leaf)
 * (0 = none); host PointXYZI out, capacity in points, *n_out always set.  The context's target is not touched. */
int pcm_loam_submap_near(pcm_ctx *ctx, int key, int search_num, int wrt_key, float leaf, float *out, size_t cap, size_t *n_out);
/* parity hook: the last update's selection (key frame per used entry: num_selected int32) and its clouds before (concatenated,
 * transformed: num_*_in x 4 floats) and after the VoxelGrids (num_*_map x 4 floats).  Any pointer may be NULL. */
int pcm_loam_submap_info(pcm_ctx *ctx, int32_t *keys, float *corner_in, float *surf_in, float *corner_map, float *surf_map);

/*
 * Scan Context descriptors and loop detection of jueying_slam on the device: SCManager::makeAndSaveScancontextAndKeys
 * (Scancontext.cpp:151-250, called from saveKeyFramesAndFactor, mapOptmization.cpp:1848-1866), detectLoopClosureID (:253-344)
 * and detectLoopClosureDistance (mapOptmization.cpp:843-880).  A PCM_MODEL_LOAM context keeps one descriptor (num_ring x
 * num_sector, stored as float), its ring key, sector key and column norms per call of pcm_loam_sc_add / pcm_loam_sc_put; the
 * loop thread is
 *   pcm_loam_sc_add (per key frame) ... pcm_loam_sc_detect (per tick) -> pcm_loam_submap_near x 2 -> the caller's verification.
 * DESIGN.md section 12.
 */
#define PCM_LOAM_SC_POINTS 0          /* the given cloud (SINGLE_SCAN_FULL), through the VoxelGrid of `leaf` */
#define PCM_LOAM_SC_KEYFRAME_SURF 1   /* the stored surf cloud of key frame `key`, no VoxelGrid (SINGLE_SCAN_FEAT) */
#define PCM_LOAM_SC_KEYFRAME_NEAR 2   /* MULTI_SCAN_FEAT: pcm_loam_sc_add_near (it needs search_num and leaf; pcm_loam_sc_add: PCM_ERR_UNSUPPORTED) */

typedef struct pcm_loam_sc_params {
  double lidar_height;           /* 0.3   Scancontext.h:80 LIDAR_HEIGHT */
  double max_radius;             /* 80.0  :84 PC_MAX_RADIUS, > 0 */
  double search_ratio;           /* 0.1   :93 SEARCH_RATIO, in [0, 1] */
  double dist_threshold;         /* 0.3   :95 SC_DIST_THRES */
  int32_t num_ring;              /* 20    :82 PC_NUM_RING, 1..64; fixed by the first descriptor of a store */
  int32_t num_sector;            /* 60    :83 PC_NUM_SECTOR, 1..360; fixed by the first descriptor of a store */
  int32_t num_exclude_recent;    /* 30    :89 NUM_EXCLUDE_RECENT */
  int32_t num_candidates;        /* 3     :90 NUM_CANDIDATES_FROM_TREE, 1..64; 0 = every entry of the search set (extension) */
  int32_t tree_making_period;    /* 10    :99 TREE_MAKING_PERIOD_, >= 1 */
  float leaf;                    /* 0.5   mapOptmization.cpp:239 kSCFilterSize (PCM_LOAM_SC_POINTS only); 0 = no down-sampling */
  int32_t reserved[8];
} pcm_loam_sc_params;

typedef struct pcm_loam_sc_add_result {
  int32_t index;                 /* of the new descriptor */
  int32_t num_points_in;         /* points of the cloud */
  int32_t num_points;            /* points the descriptor was built from (after the VoxelGrid) */
  int32_t status;
  int32_t reserved[4];
} pcm_loam_sc_add_result;

typedef struct pcm_loam_sc_result {
  int32_t loop_id;               /* nn_idx when min_dist < dist_threshold, else -1 */
  float yaw_diff_rad;            /* deg2rad(nn_align * 360 / num_sector), returned in both cases as the reference does */
  double min_dist;               /* 10000000 when no candidate had a distance (all-empty descriptors) */
  int32_t nn_idx;
  int32_t nn_align;
  int32_t num_descriptors;
  int32_t tree_size;             /* entries of the (possibly stale) search set */
  int32_t tree_rebuilt;          /* 1: this call took the search set anew */
  int32_t num_evaluated;         /* candidates through distanceBtnScanContext */
  int32_t status;
  int32_t reserved0;
  /* parity hooks: the first 64 candidates in candidate order (ascending (d2, index); with num_candidates 0, in index order) */
  int32_t cand_index[64];
  float cand_d2[64];             /* nanoflann's squared ring-key distance */
  double cand_dist[64];          /* distanceBtnScanContext().first (10000000: no shift had an effective column) */
  int32_t cand_shift[64];        /* .second */
  int32_t reserved[8];
} pcm_loam_sc_result;

void pcm_loam_default_sc_params(pcm_loam_sc_params *params);
/* makeAndSaveScancontextAndKeys of one cloud; `input` = PCM_LOAM_SC_*.  POINTS: n records of stride_bytes (x y z first) in host or
 * device memory; KEYFRAME_SURF: key frame `key` of the context's key-frame store (points / n / stride_bytes / memory unused).
 * A point with a non-finite coordinate is skipped.  params NULL = defaults; result may be NULL. */
int pcm_loam_sc_add(pcm_ctx *ctx, const pcm_loam_sc_params *params, int input, int key, const void *points, size_t n, size_t stride_bytes, int memory,
                    pcm_loam_sc_add_result *result);
/* MULTI_SCAN_FEAT (input PCM_LOAM_SC_KEYFRAME_NEAR): the descriptor of the near-key-frame cloud of `key` -- pcm_loam_submap_near's
 * cloud for (key, search_num, wrt_key, leaf), built in device memory and read where it lies.  Descriptor and keys equal, bit for
 * bit, pcm_loam_submap_near followed by pcm_loam_sc_add(PCM_LOAM_SC_POINTS) with params->leaf = 0 (params->leaf is not read here).
 * An empty key-frame store, a key outside [0, K) and a bad search_num / leaf: PCM_ERR_INVALID_ARGUMENT; a VoxelGrid index
 * overflow: PCM_ERR_OUT_OF_RANGE; nothing is stored then.  params NULL = defaults; result may be NULL. */
int pcm_loam_sc_add_near(pcm_ctx *ctx, const pcm_loam_sc_params *params, int key, int search_num, int wrt_key, float leaf, pcm_loam_sc_add_result *result);
/* a ready descriptor (column-major doubles, ring fastest: the reference's Eigen::MatrixXd; every value must be representable as a
 * float): the keys are derived on the device.  This is how the descriptors of a saved map are loaded. */
int pcm_loam_sc_put(pcm_ctx *ctx, const double *desc, int num_ring, int num_sector);
/* descriptor `index`: desc num_ring x num_sector doubles column-major, ring_key num_ring floats, sector_key num_sector doubles;
 * any may be NULL */
int pcm_loam_sc_get(pcm_ctx *ctx, int index, double *desc, float *ring_key, double *sector_key);
int pcm_loam_sc_count(pcm_ctx *ctx);   /* descriptors, or a negative pcm_status */
int pcm_loam_sc_shape(pcm_ctx *ctx, int *num_ring, int *num_sector);   /* of the stored descriptors; 0, 0 for an empty store */
int pcm_loam_sc_clear(pcm_ctx *ctx);   /* also resets the tree counter */
/* detectLoopClosureID: the last descriptor against the search set [0, count - num_exclude_recent) as of the last call whose
 * counter was a multiple of tree_making_period.  Everything runs on the device; `result` is read back once.  The shape is the
 * store's: num_ring / num_sector of params are not read here or in pcm_loam_sc_distance. */
int pcm_loam_sc_detect(pcm_ctx *ctx, const pcm_loam_sc_params *params, pcm_loam_sc_result *result);
/* distanceBtnScanContext(descriptor i, descriptor j) on the kernel of pcm_loam_sc_detect; params NULL = defaults (search_ratio) */
int pcm_loam_sc_distance(pcm_ctx *ctx, const pcm_loam_sc_params *params, int i, int j, double *dist, int32_t *shift);
/* detectLoopClosureDistance on the host mirror of the key poses (z replaced by 1.1f): the nearest key pose inside `radius`
 * (10.0, historyKeyframeSearchRadius), in ascending (d2, index), whose |time - time_cur| > time_diff_s (30.0) and that lies more
 * than 10 key frames back.  Returns 1 (found: *key_cur = K - 1, *key_pre), 0, or a negative pcm_status.  The loopIndexContainer
 * test stays with the caller. */
int pcm_loam_loop_detect_distance(pcm_ctx *ctx, float radius, double time_diff_s, double time_cur, int32_t *key_cur, int32_t *key_pre);

/*
 * Loop verification of jueying_slam on the device: performLoopClosure (mapOptmization.cpp:619-733) from a detected pair to the
 * loop factor, with the key frames never leaving the device.  The live verifier of that function is
 * pclomp::NormalDistributionsTransform (:683-697; the PCL ICP block above it is commented out).  DESIGN.md section 19.
 *
 * pcm_loam_submap_near_dev: pcm_loam_submap_near -- same selection, transform, order and VoxelGrid, the same bits -- with the
 * (x, y, z, intensity) float4 records written to a host or a DEVICE buffer (`memory`; capacity in points; *n_out always set,
 * PCM_ERR_INVALID_ARGUMENT when the capacity is too small).  It waits for the stream only when the count has to come back
 * (leaf > 0) or the result goes to host memory: with leaf == 0 and a device buffer the call returns with the work queued on the
 * context's stream.  A device buffer with room for every input point of the window is written in place.
 */
int pcm_loam_submap_near_dev(pcm_ctx *ctx, int key, int search_num, int wrt_key, float leaf, void *out, size_t cap, int memory, size_t *n_out);

#define PCM_LOAM_LOOP_ACCEPTED 0
#define PCM_LOAM_LOOP_REJECTED_SIZE 1            /* :652 a cloud below its gate; NDT did not run */
#define PCM_LOAM_LOOP_REJECTED_NOT_CONVERGED 2   /* :693 hasConverged() == false */
#define PCM_LOAM_LOOP_REJECTED_FITNESS 3         /* :693 getFitnessScore() > historyKeyframeFitnessScore */
#define PCM_LOAM_LOOP_NONE 4                     /* pcm_loam_loop_closure: detectLoopClosureDistance found no pair */

typedef struct pcm_loam_loop_params {
  int32_t history_search_num;    /* 25    utility.h:290 historyKeyframeSearchNum: the previous cloud spans key_pre -/+ this */
  int32_t min_cur_points;        /* 300   mapOptmization.cpp:652 */
  int32_t min_prev_points;       /* 1000  mapOptmization.cpp:652 */
  int32_t wrt_key;               /* -1    every key frame under its own pose, as performLoopClosure (:650-651).  >= 0: both clouds
                                  *       under the pose of that key frame (loopFindNearKeyframesWithRespectTo) -- an option of this
                                  *       library, NOT performSCLoopClosure, which verifies with PCL ICP: pcm_loam_sc_loop_verify */
  float fitness_threshold;       /* 0.3   utility.h:291 historyKeyframeFitnessScore */
  float near_leaf;               /* 0.2   mapOptmization.cpp:243 downSizeFilterICP = mappingSurfLeafSize (utility.h:272); 0 = none */
  double ndt_epsilon;            /* 0.01  mapOptmization.cpp:684 setTransformationEpsilon */
  float ndt_resolution;          /* 1.0   mapOptmization.cpp:685 setResolution */
  int32_t ndt_num_neighbors;     /* 7     mapOptmization.cpp:686 DIRECT7 (0 KDTREE, 1, 7, 27 as pcm_config::num_neighbors) */
  int32_t reserved[8];
} pcm_loam_loop_params;

typedef struct pcm_loam_loop_result {
  int32_t status;                /* PCM_LOAM_LOOP_* */
  int32_t key_cur, key_pre;      /* the pair (pcm_loam_loop_closure: as detected; -1, -1 without one) */
  int32_t num_cur_points;        /* cureKeyframeCloud->size() */
  int32_t num_prev_points;       /* prevKeyframeCloud->size() */
  int32_t ndt_iterations;        /* 0 when NDT did not run */
  int32_t ndt_converged;
  float noise_variance;          /* :719 float noiseScore = getFitnessScore(): the six variances of the loop's noise model */
  double fitness;                /* ndt->getFitnessScore() (PCL's default max_range); 0 when NDT did not run */
  float correction[16];          /* ndt->getFinalTransformation(), row-major; identity when NDT did not run */
  /* the loop factor, written when the status is ACCEPTED (zero otherwise); poses as (roll, pitch, yaw, x, y, z) */
  double pose_from[6];           /* :715 poseFrom: getTranslationAndEulerAngles(correction * tWrong), floats promoted */
  double pose_to[6];             /* :716 poseTo = pose of key_pre */
  double between[16];            /* :725 poseFrom.between(poseTo), row-major 4 x 4 */
  double between6[6];            /* the same as (roll, pitch, yaw, x, y, z) */
  int32_t reserved[8];
} pcm_loam_loop_result;

void pcm_loam_default_loop_params(pcm_loam_loop_params *params);
/* performLoopClosure :645-731 for the pair (key_cur, key_pre): both near clouds are built in device memory (one wait, for their
 * two counts), the size gates, pclomp NDT from the identity in a verifier context the LOAM context owns (created by the first
 * verification that passes the gates, released with the context), its fitness score, the acceptance test and -- on the host -- the
 * pose algebra of :706-725.  Returns PCM_OK with the outcome in result->status.  The context's target, source, key frames and Scan
 * Context store are not touched.  An empty store, a key outside [0, K) and bad parameters: PCM_ERR_INVALID_ARGUMENT, nothing
 * changed.  params NULL = defaults.  GTSAM's factor and the loopIndexContainer bookkeeping (:730) stay with the caller. */
int pcm_loam_loop_verify(pcm_ctx *ctx, const pcm_loam_loop_params *params, int key_cur, int key_pre, pcm_loam_loop_result *result);
/* detectLoopClosureDistance (pcm_loam_loop_detect_distance with the same radius / time_diff_s / time_cur) followed by
 * pcm_loam_loop_verify of the pair it finds.  No pair: PCM_OK with status PCM_LOAM_LOOP_NONE, at the cost of the host search alone
 * (no device work, no verifier).  The loopIndexContainer test and insert (:730, :848) stay with the caller: a pair the caller has
 * already closed is verified again unless the caller filters it. */
int pcm_loam_loop_closure(pcm_ctx *ctx, const pcm_loam_loop_params *params, float radius, double time_diff_s, double time_cur, pcm_loam_loop_result *result);
/* 1 when the context holds a verifier context, 0 when none has been created yet, or a negative pcm_status */
int pcm_loam_loop_verifier_exists(pcm_ctx *ctx);

/*
 * performSCLoopClosure (mapOptmization.cpp:735-841), the Scan Context half of the loop thread, on the device: both near clouds
 * under the pose of key frame 0 (base_key, :757-759; cur = key_cur +- 0, prev = key_pre +- history_search_num, each through the
 * VoxelGrid of near_leaf), the size gates (:761), pcl::IterativeClosestPoint from the identity (:768-779: PCM_MODEL_ICP in a second
 * verifier context the LOAM context owns, created by the first verification that passes the gates, run on the LOAM context's
 * stream, released with the context), pcm_fitness_score(..., DBL_MAX), the acceptance test (:783) and -- on the host -- the factor
 * of :817-834: poseFrom = getTranslationAndEulerAngles(correction), poseTo = the identity, between = poseFrom.between(poseTo).
 * Nothing of the LOAM context's target, source, key frames or Scan Context store is written, and the NDT verifier of
 * pcm_loam_loop_verify is neither created nor used.  GTSAM's factor and the loopIndexContainer insert (:833-840) stay with the caller.
 */
typedef struct pcm_loam_sc_loop_params {
  int32_t history_search_num;        /* 25    utility.h:290 */
  int32_t min_cur_points;            /* 300   mapOptmization.cpp:761 */
  int32_t min_prev_points;           /* 1000  mapOptmization.cpp:761 */
  int32_t icp_max_iterations;        /* 100   :770 */
  float fitness_threshold;           /* 0.3   :783 historyKeyframeFitnessScore */
  float near_leaf;                   /* 0.2   downSizeFilterICP (mapOptmization.cpp:243); 0 = none */
  double icp_max_correspondence_distance;   /* 150   :769 */
  double icp_transformation_epsilon;        /* 1e-6  :771 */
  double icp_euclidean_fitness_epsilon;     /* 1e-6  :772 */
  float icp_voxel_resolution;        /* 1.0   cell of the verifier's search grid (speed only) */
  int32_t reserved[9];
} pcm_loam_sc_loop_params;

typedef struct pcm_loam_sc_loop_result {
  int32_t status;                /* PCM_LOAM_LOOP_* */
  int32_t key_cur, key_pre;      /* the pair (pcm_loam_sc_loop_closure: as detected; -1, -1 without one) */
  int32_t num_cur_points;
  int32_t num_prev_points;
  int32_t icp_iterations;        /* 0 when ICP did not run */
  int32_t icp_converged;
  int32_t icp_stop_reason;       /* PCM_ICP_STOP_* */
  float yaw_diff_rad;            /* :744 detectResult.second (pcm_loam_sc_loop_closure; unused by the reference); 0 from pcm_loam_sc_loop_verify */
  float noise_variance;          /* 0.5   :822 robustNoiseScore: the six variances */
  double cauchy_k;               /* 1     :827 mEstimator::Cauchy::Create(1) */
  double fitness;                /* icp.getFitnessScore(); 0 when ICP did not run */
  float correction[16];          /* icp.getFinalTransformation(), row-major; identity when ICP did not run */
  /* the loop factor, written when the status is ACCEPTED (zero otherwise); poses as (roll, pitch, yaw, x, y, z) */
  double pose_from[6];           /* :817-818 */
  double pose_to[6];             /* :819 the identity */
  double between[16];            /* :834 poseFrom.between(poseTo), row-major 4 x 4 */
  double between6[6];
  int32_t reserved[8];
} pcm_loam_sc_loop_result;

void pcm_loam_default_sc_loop_params(pcm_loam_sc_loop_params *params);
/* performSCLoopClosure :750-834 for the pair (key_cur, key_pre).  Returns PCM_OK with the outcome in result->status.  An empty
 * store, a key outside [0, K) and bad parameters: PCM_ERR_INVALID_ARGUMENT, nothing changed.  params NULL = defaults. */
int pcm_loam_sc_loop_verify(pcm_ctx *ctx, const pcm_loam_sc_loop_params *params, int key_cur, int key_pre, pcm_loam_sc_loop_result *result);
/* pcm_loam_sc_detect of the last descriptor with its default parameters (:741) and key_cur = K - 1 (:742), then
 * pcm_loam_sc_loop_verify of the pair.  No loop (:745): PCM_OK with status PCM_LOAM_LOOP_NONE and no further device work.  A caller
 * with other detection parameters calls pcm_loam_sc_detect and pcm_loam_sc_loop_verify itself. */
int pcm_loam_sc_loop_closure(pcm_ctx *ctx, const pcm_loam_sc_loop_params *params, pcm_loam_sc_loop_result *result);
/* 1 when the context holds an ICP verifier context, 0 when none has been created yet, or a negative pcm_status */
int pcm_loam_sc_loop_verifier_exists(pcm_ctx *ctx);

/*
 * The two clouds a mapping run of jueying_slam exists to produce, from the key frames on the device: publishGlobalMap
 * (mapOptmization.cpp:547-590, every five seconds) and the saved map (:524-542, jueying.pcd).  DESIGN.md section 20.
 * Both read the key-frame store and write nothing of the context: not its target or source, the key frames, the Scan Context
 * store or the workspaces of the near clouds.  Their per-point device workspace (up to about 44 bytes per selected point) is
 * allocated by the call and released before it returns; a table of 32 bytes per selected key frame stays.
 */
typedef struct pcm_loam_global_params {
  float search_radius;           /* 1000.0 utility.h:293 globalMapVisualizationSearchRadius */
  float keypose_density;         /* 10.0   utility.h:294 globalMapVisualizationPoseDensity: leaf of the VoxelGrid over the key poses, > 0 */
  float leaf;                    /* 1.0    utility.h:295 globalMapVisualizationLeafSize; 0 = no down-sampling */
} pcm_loam_global_params;

typedef struct pcm_loam_global_result {
  int32_t num_near;              /* key poses inside the radius of the last one */
  int32_t num_pose_leaves;       /* leaves of the VoxelGrid over them */
  int32_t num_skipped;           /* leaves whose centroid is farther than the radius from the last key pose (:578) */
  int32_t num_used;              /* leaves used; each names one key frame (the truncated mean of the key indices in it) */
  uint64_t points_in;            /* points of the selected clouds */
  uint64_t points_out;           /* cells written */
} pcm_loam_global_result;

void pcm_loam_default_global_params(pcm_loam_global_params *params);
/* the selection alone, on the host: the key frame of every used leaf in list order; capacity in keys, *n always set
 * (PCM_ERR_INVALID_ARGUMENT when the capacity is too small).  An overflow of the pose grid: PCM_ERR_OUT_OF_RANGE. */
int pcm_loam_global_keys(pcm_ctx *ctx, const pcm_loam_global_params *params, int32_t *keys, size_t cap, size_t *n);
/* publishGlobalMap: corner then surf cloud of every selected key frame under its pose, one VoxelGrid(leaf): (x, y, z, intensity)
 * float4 cells in leaf-index order into a host or DEVICE buffer (`memory`; capacity in points).  It is pcm_loam_submap_near_dev's
 * pass on this selection and follows its rules: result->points_out is set before a "capacity too small" error
 * (PCM_ERR_INVALID_ARGUMENT); a 16-byte-aligned device buffer with room for points_in points is written in place; with leaf == 0
 * the count (= points_in) is known before anything runs -- so leaf == 0 with capacity 0 is a host-only query of points_in -- and
 * a device result is queued on the context's stream without a wait; with leaf > 0 the call waits once, for the count.  More than
 * 2^31 - 1 selected points and a VoxelGrid index overflow: PCM_ERR_OUT_OF_RANGE.  An empty store: PCM_OK, zero points.  A bad
 * argument: nothing written.  params NULL = defaults; result may be NULL. */
int pcm_loam_global_map(pcm_ctx *ctx, const pcm_loam_global_params *params, void *out, size_t cap, int memory, pcm_loam_global_result *result);
/* The saved map (:530-541) of key frames [first, first + n): which 0 = their corner clouds (globalCornerCloud), 1 = their surf
 * clouds (globalSurfCloud), 2 = all corner clouds, then all surf clouds (globalMapCloud).  Every point is transformPointCloud's
 * value under its key frame's pose, bit for bit (a negative zero stays negative); no VoxelGrid.  Buffer rules as above; *n_out is
 * known before anything runs and always set, and a device result is not waited for.  More than 2^31 - 1 points in one call:
 * PCM_ERR_OUT_OF_RANGE.  A whole session through a bounded buffer is a loop over [first, first + n) with which = 0, then the
 * same loop with which = 1: the pieces concatenate to globalCornerCloud and globalSurfCloud, and those two to jueying.pcd.
 * which = 2 equals jueying.pcd over the full range [0, K) only: its pieces over sub-ranges do not concatenate to it. */
int pcm_loam_map_export(pcm_ctx *ctx, int which, int first, int n, void *out, size_t cap, int memory, size_t *n_out);
/* measurement hook (tools/bench_loam_global.py): one timed run, device events around it, of the gather of pcm_loam_global_map's
 * selection -- variant 0: the near pass's gather (per-wave atomics on the box), 1: the global pass's (partial boxes) -- with the
 * box either leaves (6 ordered words), the bytes of the workspace pcm_loam_global_map allocates for that selection with
 * leaf > 0 and an in-place buffer, and the host time (ms) its allocation and its release took in this call on an idle stream.
 * box6, workspace_bytes and workspace_ms may be NULL. */
int pcm_loam_global_gather_ms(pcm_ctx *ctx, const pcm_loam_global_params *params, int variant, float *ms, uint32_t *box6, size_t *workspace_bytes,
                              float *workspace_ms);

/*
 * Localisation map of jueying_slam on the device: the saved global map cut into area tiles (include/dynamic_map.h:16-156), the
 * reload of the tiles around the robot (dynamic_load_map_run, localization.cpp:281-315) and the per-frame crop of the loaded
 * tiles (dynamic_load_map, :256-280).  A PCM_MODEL_LOAM context keeps every tile of the corner list and of the surf list (map
 * frame, PointXYZI) on the device; pcm_loam_dynmap_load selects tiles on the host and moves no points; pcm_loam_dynmap_crop
 * compacts the selected tiles through the frame's window, in order, straight into the context's LOAM target
 * (laserCloudCornerFromMapDS / laserCloudSurfFromMapDS), so a localisation frame is
 *   pcm_loam_frame_begin -> pcm_loam_dynmap_crop -> pcm_loam_align
 * with the scan as the only bulk upload.  DESIGN.md section 14.  A mapping context can hand its map over without the host:
 * pcm_loam_tiles_build (below) cuts its key frames into these tiles on the device.
 */
typedef struct pcm_loam_dynmap_params {
  float max_range;               /* 150.0 utility.h:224: the window is pose -/+ max_range * 1.1 */
  int32_t margin;                /* -1    utility.h:186: a tile is loaded when the pose lies in its box grown by margin; < 0: every
                                  *       tile is selected and the crop keeps every (finite) point: the whole map is the target */
  int32_t area_size;             /* -1    utility.h:185: reload after moving farther than this from the last load */
  int32_t crop_x;                /* 0     0: only the y window has an effect, as localization.cpp:259-273 behaves (its x filters are
                                  *       overwritten); 1: x and y windows both */
  int32_t reserved[8];
} pcm_loam_dynmap_params;

typedef struct pcm_loam_dynmap_load_result {
  int32_t num_corner_tiles;      /* tiles stored per list */
  int32_t num_surf_tiles;
  int32_t num_corner_selected;   /* tiles selected per list (empty tiles included) */
  int32_t num_surf_selected;
  int64_t num_corner_points;     /* points of the selected tiles */
  int64_t num_surf_points;
  uint64_t generation;           /* of the selection: changes only when a selected index list differs from the last load's */
  int32_t changed;               /* 1: this load changed the selection */
  int32_t reserved[5];
} pcm_loam_dynmap_load_result;

typedef struct pcm_loam_dynmap_crop_result {
  int32_t num_corner_in;         /* points of the selected tiles */
  int32_t num_surf_in;
  int32_t num_corner;            /* points kept: laserCloudCornerFromMapDS / laserCloudSurfFromMapDS */
  int32_t num_surf;
  int32_t num_nonfinite;         /* points of both lists dropped for a non-finite x, y or z */
  int32_t rebuilt;               /* 0: selection, limits and crop_x equal those of the last crop and the target is still its
                                  * result: nothing done on the device */
  float x_lo, x_hi, y_lo, y_hi;  /* the float limits (x_* are computed even where crop_x = 0 does not apply them) */
  int32_t status;                /* PCM_OK */
  int32_t reserved[5];
} pcm_loam_dynmap_crop_result;

void pcm_loam_default_dynmap_params(pcm_loam_dynmap_params *params);
/* one area tile of list `which` (0 corner, 1 surf): box = x_min, y_min, z_min, x_max, y_max, z_max (the CSV area list's columns)
 * and its n points (records of stride_bytes, x y z first, intensity the fourth float when stride_bytes >= 16, else 0; n may be 0).
 * The intensity rule of pcm_loam_keyframe_add holds: a pcl::PointXYZI buffer must be repacked to (x, y, z, intensity) first, as
 * pcm_amd::LoamDynamicMap does.  Returns the tile's index in its list (>= 0) or a negative pcm_status. */
int pcm_loam_tile_add(pcm_ctx *ctx, int which, const double box[6], const void *points, size_t n, size_t stride_bytes, int memory);
int pcm_loam_tile_count(pcm_ctx *ctx, int which);   /* tiles of the list, or a negative pcm_status */
int pcm_loam_tile_clear(pcm_ctx *ctx);              /* both lists and the selection; device memory is kept */
/* the trigger of dynamic_load_map_run: 1 when pose6 (roll, pitch, yaw, x, y, z) is farther than area_size from the pose of the
 * last pcm_loam_dynmap_load (before the first one the last pose is -999999 on every axis, as last_loadMap starts), else 0; or a
 * negative pcm_status.  The comparison is the reference's float arithmetic (localization.cpp:295-300).  params NULL = defaults. */
int pcm_loam_dynmap_need_load(pcm_ctx *ctx, const pcm_loam_dynmap_params *params, const float pose6[6]);
/* create_pcd for both lists at pose6: selects the tiles whose grown boxes hold (x, y), in list order, and records the pose as
 * the last load.  No bulk data moves.  result may be NULL. */
int pcm_loam_dynmap_load(pcm_ctx *ctx, const pcm_loam_dynmap_params *params, const float pose6[6], pcm_loam_dynmap_load_result *result);
/* dynamic_load_map(pose6): the selected tiles, concatenated in list order, through the window; the result becomes the context's
 * LOAM target (the caller index of a map point is its position in the cropped cloud) and the next pcm_loam_align builds the
 * search grids.  PCM_ERR_NO_INPUT before a load. */
int pcm_loam_dynmap_crop(pcm_ctx *ctx, const pcm_loam_dynmap_params *params, const float pose6[6], pcm_loam_dynmap_crop_result *result);
/* parity hook: the selected tile indices of both lists (num_*_selected int32 each) and the two cropped clouds (num_corner /
 * num_surf x 4 floats, to the host).  Any pointer may be NULL.  PCM_ERR_NO_INPUT when the context's target is not the result
 * of pcm_loam_dynmap_crop (the clouds; the indices need only a load). */
int pcm_loam_dynmap_info(pcm_ctx *ctx, int32_t *corner_tiles, int32_t *surf_tiles, float *corner, float *surf);
/* globalMap (localization.cpp:274): the cropped corner cloud, then the cropped surf cloud, as (x, y, z, intensity) records into
 * a host buffer or a caller's device buffer (memory) of `capacity` points; *n is always set, PCM_ERR_INVALID_ARGUMENT when the
 * capacity is too small.  The Matching_method == "ndt" branch feeds it to an NDT context with PCM_MEM_DEVICE. */
int pcm_loam_dynmap_global(pcm_ctx *ctx, void *out, size_t capacity, size_t *n, int memory);

/* One tile store for several localisation contexts (a fleet of robots on one site map).  The store -- both tile lists and their
 * points on the device -- exists once however many contexts hold it; the selection of the last load, the crop workspace and the
 * record of the last crop stay per context: each robot has its own pose and its own window.  DESIGN.md section 33.
 *   - pcm_loam_tile_share: `dst` reads the store `src` holds from now on.  Both are PCM_MODEL_LOAM contexts on one device and
 *     dst != src, else PCM_ERR_INVALID_ARGUMENT (pcm_last_error(dst) names the reason).  The call waits for src's stream (every
 *     upload of pcm_loam_tile_add and the copies of pcm_loam_tiles_build are complete before any holder reads) and for dst's,
 *     lets go of the store dst had and resets dst's selection: a crop needs a new pcm_loam_dynmap_load (PCM_ERR_NO_INPUT before).
 *     dst's LOAM target and search grids are not touched.  An empty store may be shared.
 *   - While a store has more than one holder nothing writes to it: pcm_loam_tile_add and pcm_loam_tiles_build on any holder return
 *     PCM_ERR_UNSUPPORTED (the build before any device work) and change nothing.  pcm_loam_tile_clear on a holder of a shared
 *     store detaches that holder only and gives it an empty store of its own.  There is no copy-on-write.
 *   - The reading calls work on every holder: pcm_loam_tile_count / _info / _get, pcm_loam_dynmap_need_load / _load / _crop /
 *     _crop_batch / _info / _global.
 *   - pcm_destroy detaches; the memory goes with the last holder, so `src` may be destroyed first.
 *   - Neither context may be in another call while pcm_loam_tile_share runs.
 * pcm_loam_tile_share_count: the contexts holding ctx's store (1 = not shared), or a negative pcm_status. */
int pcm_loam_tile_share(pcm_ctx *dst, pcm_ctx *src);
int pcm_loam_tile_share_count(pcm_ctx *ctx);

/* pcm_loam_dynmap_crop for n contexts in one round of launches on the stream of ctxs[0]: one upload, four launches, one read-back
 * and one wait for the whole batch instead of one of each per context.  Context i is cropped at poses6[6 i .. 6 i + 5] with the
 * one params (NULL = defaults); results[i] is the record a single pcm_loam_dynmap_crop would have written, bit for bit, and so
 * is the context's target.  The contexts may hold one store, different stores, or a mix; they are distinct and live on one device.
 * A context whose crop is unchanged reports rebuilt = 0 and takes no part in the launches.  A context that cannot be cropped (no
 * load yet, a pose that is not finite, a duplicate, another device, more than 2^31 - 1 points selected, no room for its target)
 * gets its status in results[i].status and is left out; the others run.  Returns the first status that is not PCM_OK (the text
 * is pcm_last_error(ctxs[0])).  n <= 0 or a null array: PCM_ERR_INVALID_ARGUMENT; more workgroups than one grid holds:
 * PCM_ERR_OUT_OF_RANGE, nothing done.  A fleet frame is
 *   pcm_loam_frame_begin_batch -> pcm_loam_dynmap_crop_batch -> pcm_loam_align_batch */
int pcm_loam_dynmap_crop_batch(pcm_ctx *const *ctxs, int n, const pcm_loam_dynmap_params *params, const float *poses6, pcm_loam_dynmap_crop_result *results);

/*
 * The key-frame map cut into area tiles on the device: what a mapping session leaves a localisation session, with no host copy
 * of the map in between (mapping context -> pcm_loam_tiles_build -> pcm_loam_dynmap_load / _crop -> pcm_loam_align).  The reference
 * reads area lists (dynamic_map.h:37-88) and holds no program that writes them, so the rules of the cut are this library's:
 *   tile index  ix = (int32)floorf(x / tile_size), iy likewise, on transformPointCloud's float values: -0.0f lies in tile 0,
 *               -1e-7f in tile -1, a point exactly on k * tile_size in tile k
 *   order       a list holds the tiles that have a point of it, by ascending (iy, ix); the two lists are independent
 *   cloud       leaf == 0: the tile's points in export order (key frame, then point; the values are the segmented VoxelGrid
 *               pass's one-point means, so a negative zero is stored as zero); leaf > 0: the pcl::VoxelGrid of the tile's points
 *               alone -- the bits pcm_voxel_downsample(those points, leaf) returns
 *   box         x_min = (double)ix * (double)tile_size, x_max = (double)(ix + 1) * (double)tile_size, the same for y (what
 *               is_in_area selects by); z_min / z_max: the stored points' range
 * DESIGN.md section 31.
 */
typedef struct pcm_loam_tiles_params {
  float tile_size;     /* 50.0  edge of a square tile in x and y, metres; finite, > 0 */
  float leaf_corner;   /* 0.2   utility.h:271 mappingCornerLeafSize; 0 = no down-sampling */
  float leaf_surf;     /* 0.2   utility.h:272 mappingSurfLeafSize;   0 = no down-sampling */
  int32_t reserved[9];
} pcm_loam_tiles_params;

typedef struct pcm_loam_tiles_result {
  int32_t  num_corner_tiles, num_surf_tiles;
  uint64_t corner_points_in, surf_points_in;      /* points of key frames [first, first+n) */
  uint64_t corner_points_out, surf_points_out;    /* points stored in the tiles */
  uint64_t num_nonfinite;                         /* dropped: non-finite x, y or z */
  int32_t  reserved[6];
} pcm_loam_tiles_result;

void pcm_loam_default_tiles_params(pcm_loam_tiles_params *params);
/* Replaces both tile lists of the context (and clears the selection, as pcm_loam_tile_clear followed by adds would) with the tiles
 * of key frames [first, first + n) under their current poses.  Only counts and the per-tile table (16 bytes per tile) leave the
 * device; the call waits twice -- for the number of tiles, then for the table (a third time when the two lists together hold more
 * than 2^31 - 1 points and are exported one after the other).  The key-frame store, the context's target and source, the Scan
 * Context store and the occupancy map are not touched.  The workspace (88 bytes per point plus the sort's temporaries, both lists
 * alive together) is released before the call returns.  A bad argument (tile_size not finite or <= 0, a negative leaf, a range outside
 * [0, K]): PCM_ERR_INVALID_ARGUMENT; |ix| or |iy| >= 32768, a tile whose VoxelGrid index overflows (tiles are not cut as
 * pcm_voxel_downsample_large cuts) and more than 2^31 - 1 points in one list: PCM_ERR_OUT_OF_RANGE; every error leaves the tiles
 * as they were.  An empty range or store: PCM_OK, zero tiles.  params NULL = defaults; result may be NULL. */
int pcm_loam_tiles_build(pcm_ctx *ctx, const pcm_loam_tiles_params *params, int first, int n, pcm_loam_tiles_result *result);
/* measurement hook (tools/bench_loam_tiles.py): pcm_loam_tiles_build with device events at its stage boundaries.  stage_ms takes
 * PCM_LOAM_TILES_STAGES floats per list (corner, then surf): host ms of the workspace requests, then device ms of the tile keys,
 * the key sort, the distinct keys, rank + table init, the per-tile min / max, boxes + cell keys + cell sort, the means (the
 * scatter), the per-tile count and z range; then two more: the gather of both lists and the copies into the arenas.  The timed
 * call waits once more than the untimed one. */
#define PCM_LOAM_TILES_STAGES 9
int pcm_loam_tiles_build_ms(pcm_ctx *ctx, const pcm_loam_tiles_params *params, int first, int n, pcm_loam_tiles_result *result, float *stage_ms);
/* tile `index` of list `which`, from pcm_loam_tile_add or pcm_loam_tiles_build: its box (x_min, y_min, z_min, x_max, y_max,
 * z_max), its index pair (0, 0 for a tile the caller added) and its number of points; any pointer may be NULL */
int pcm_loam_tile_info(pcm_ctx *ctx, int which, int index, double box[6], int32_t ixy[2], size_t *n_points);
/* the tile's (x, y, z, intensity) records into a host or device buffer of capacity_points; *n is always set,
 * PCM_ERR_INVALID_ARGUMENT when the capacity is too small (the rules of pcm_loam_dynmap_global).  With pcm_loam_tile_info this is
 * what a caller writes the PCD files and the area list from. */
int pcm_loam_tile_get(pcm_ctx *ctx, int which, int index, void *out, size_t capacity_points, int memory, size_t *n);

/*
 * 2D occupancy grid mapping of jueying_slam's map tool (src/tool/occupancy_mapping) on the device: getScan (cloud -> virtual
 * laser scan), processScan + TraceLine (rays into the grid), getGridMap (crop, -1 / 0 / 100) and saveMap's PGM bytes.  The map
 * belongs to a context of any model; a PCM_MODEL_LOAM context can also feed it from its key-frame store in place.  Offline
 * (OccupancyServerFromFile, use_file_num 2) and after a loop closure:
 *   pcm_occ_reset -> pcm_occ_insert_keyframes [0, K) -> pcm_occ_info / pcm_occ_get_map;
 * online (OccupancyServerRealTime): pcm_occ_insert_scans per cloud.  A cell holds two uint32 counters (end-point hits, ray
 * passes; they wrap after 2^32 updates of one cell) and its value is defined from them:
 *   logit = (double)n_occ * log_occ + (double)n_free * log_free, occupied when 1 / (1 + exp(-logit)) * 100 >= 50
 * (the reference adds the updates in visit order, which is not associative).  The grid is a dense rectangle of at most 2^28
 * cells that grows with the poses; a batch that would exceed it returns PCM_ERR_INVALID_ARGUMENT.  DESIGN.md section 13.
 */
typedef struct pcm_occ_params {
  double min_z;                  /* -0.15  config/rslidar.yaml: points with min_z <= z <= max_z (sensor frame) make the scan */
  double max_z;                  /* 1.5 */
  double angle_increment;        /* 0.006  beam width in rad: ceil(2 * 3.1415927 / angle_increment) beams, at most 2^20 */
  double min_range;              /* 0.5    a beam keeps the smallest range in [min_range, max_range] */
  double max_range;              /* 200 */
  double log_occ;                /* 0.1    update of the end cell */
  double log_free;               /* -0.01  update of a cell a ray passes */
  double resolution;             /* 0.1    metres per cell */
  double max_radius;             /* 20     longer beams are clipped to max_radius + 0.1 and hit nothing */
  int32_t fill_with_white;       /* 1      trace clipped beams as free space */
  int32_t use_nan;               /* 0      empty beams count as clipped beams */
  int32_t reserved[8];
} pcm_occ_params;

void pcm_occ_default_params(pcm_occ_params *params);
/* an empty map with these parameters (NULL = defaults); they hold until the next reset.  Device memory is kept. */
int pcm_occ_reset(pcm_ctx *ctx, const pcm_occ_params *params);
/* num_scans clouds in the sensor frame, one after the other in `points` (records of stride_bytes, x y z first; host or device
 * memory), n_points[s] records and poses6 + 6 s (roll, pitch, yaw, x, y, z as pcm_loam_align; yaw, x, y are used) for scan s, in one
 * set of launches.  The first scan after a reset also initialises the map at its cell (initializeMap).  A point with a
 * non-finite coordinate is skipped.  The counters do not depend on how scans are split into calls. */
int pcm_occ_insert_scans(pcm_ctx *ctx, const void *points, const size_t *n_points, const float *poses6, int num_scans, size_t stride_bytes, int memory);
/* PCM_MODEL_LOAM: key frames first .. first + n - 1 of the context's store, each one virtual scan from its corner and surf
 * cloud together under its stored pose, read where they lie on the device */
int pcm_occ_insert_keyframes(pcm_ctx *ctx, int first, int n);
/* parity hook: virtual scan s of the last call (of its last 2^24 / beams scans): beam_size ranges (NaN = empty beam) and angles;
 * either may be NULL */
int pcm_occ_get_scan(pcm_ctx *ctx, int s, float *ranges, double *angles);
/* beam_size, scans inserted since the reset, updates dropped outside the allocation (always 0; an insert that drops one returns
 * PCM_ERR_INTERNAL) and the allocated rectangle {x0, y0, width, height} in cells; any pointer may be NULL */
int pcm_occ_status(pcm_ctx *ctx, int32_t *beam_size, uint64_t *n_scans, uint64_t *overflow, int64_t rect[4]);
/* the map cropped to the bounding box of its known cells, as nav_msgs/OccupancyGrid: origin = first cell index * resolution;
 * width = height = 0 for an empty map; any pointer may be NULL */
int pcm_occ_info(pcm_ctx *ctx, int32_t *width, int32_t *height, double *origin_x, double *origin_y, double *resolution, int64_t *n_known);
/* width x height values, row-major (i + j * width): -1 unknown, 0 free, 100 occupied; capacity in cells */
int pcm_occ_get_map(pcm_ctx *ctx, int8_t *data, size_t capacity);
/* the body of saveMap's P5 image: width x height bytes, rows top-down (205 unknown, 254 free, 0 occupied) */
int pcm_occ_get_pgm(pcm_ctx *ctx, uint8_t *data, size_t capacity);
/* the counters of the same rectangle (either may be NULL): what a caller needs to apply a threshold of its own */
int pcm_occ_get_counts(pcm_ctx *ctx, uint32_t *n_occ, uint32_t *n_free, size_t capacity);

/*
 * octomap_server's 3D occupancy map and its projected 2D map on the device (src/tool/octomap_server: insertCloudCallback,
 * insertScan, publishAll's projected_map and octomap_point_cloud_centers) with map_saver's files: the cloud_to_map route of the
 * reference (pcd2map -> octomap_server -> map_saver).  A sparse set of finest-level cells, each a float log-odds, in a hash table
 * on the device that grows by doubling up to max_cells.  A scan updates a cell at most once (a hit when an end point fell into
 * it, else a miss), so the map does not depend on the order of rays.  The map belongs to a context of any model; a PCM_MODEL_LOAM
 * context can also feed it from its key-frame store in place.  Not built: filter_ground (the caller passes a ground cloud of its
 * own), colour, markers, the octomap messages, clearBBX, the incremental projection.  DESIGN.md section 38.
 */
typedef struct pcm_octo_params {
  double resolution;             /* 0.05   metres per cell; keys are 16 bit per axis, so the map spans +-32768 cells */
  double prob_hit;               /* 0.7    sensor_model/hit: a cell's update is (float)log(p / (1 - p)) */
  double prob_miss;              /* 0.4    sensor_model/miss */
  double clamp_min;              /* 0.12   sensor_model/min */
  double clamp_max;              /* 0.97   sensor_model/max */
  double max_range;              /* -1     sensor_model/max_range: longer rays are cut there and clear only; < 0: off */
  double min_range;              /* -1     closer points are skipped; <= 0: off */
  double pointcloud_min_x;       /* -DBL_MAX  the three PassThrough windows of insertCloudCallback (world frame), applied as floats */
  double pointcloud_max_x;       /* DBL_MAX */
  double pointcloud_min_y;
  double pointcloud_max_y;
  double pointcloud_min_z;
  double pointcloud_max_z;
  double occupancy_min_z;        /* -DBL_MAX  cells whose z extent meets (occupancy_min_z, occupancy_max_z) enter the projection */
  double occupancy_max_z;        /* DBL_MAX */
  double min_x_size;             /* 0      the projected map covers at least [-min_x_size / 2, min_x_size / 2] */
  double min_y_size;             /* 0 */
  int32_t filter_speckles;       /* 0      occupied cells without an occupied cell among their 26 neighbours are left out */
  int32_t reserved0;
  uint64_t initial_cells;        /* 65536  cells the first table has room for */
  uint64_t max_cells;            /* 2^28   the table never grows beyond room for this many cells */
  int32_t reserved[8];
} pcm_octo_params;

typedef struct pcm_octo_insert_result {
  uint64_t points_in;            /* ground + non-ground */
  uint64_t dropped_nonfinite;    /* a non-finite coordinate (after sensor_to_world) */
  uint64_t skipped_window;       /* outside a pointcloud_min / max window */
  uint64_t skipped_min_range;
  uint64_t truncated;            /* rays cut at max_range */
  uint64_t rejected_rays;        /* origin or end outside the key range, or the walk left it: the ray clears nothing */
  uint64_t cells_touched;        /* cells that received their one update */
  uint64_t new_cells;            /* of those, cells that were unknown before */
  uint32_t table_growths;        /* rehashes into a larger table during this call */
  int32_t status;                /* the call's return value */
  int32_t reserved[8];
} pcm_octo_insert_result;

typedef struct pcm_octo_map_info {
  uint64_t cells;                /* known cells */
  uint64_t occupied;             /* log-odds >= 0 */
  uint64_t free_cells;
  uint64_t capacity;             /* cells the table has room for */
  uint64_t epoch;                /* mark passes since the reset */
  int32_t key_min[3];            /* key box of the known cells; cells == 0: 0, 0, 0 */
  int32_t key_max[3];
  double metric_min[3];          /* keyToCoord(key_min) - res / 2 */
  double metric_max[3];          /* keyToCoord(key_max) + res / 2 */
  double resolution;
  float hit, miss, clamp_min, clamp_max;   /* the four log-odds constants in use */
  int32_t reserved[8];
} pcm_octo_map_info;

typedef struct pcm_octo_grid_info {
  int32_t width, height;         /* 0, 0: at most one known cell, nothing is produced (publishAll :501) */
  int32_t min_key_x, min_key_y;  /* key of column 0 / row 0 */
  double resolution;
  double origin_x, origin_y;     /* nav_msgs/MapMetaData origin.position */
  int32_t reserved[8];
} pcm_octo_grid_info;

void pcm_octo_default_params(pcm_octo_params *params);
/* an empty map with these parameters (NULL = defaults); they hold until the next reset.  Device memory is kept when the first
 * table is no larger than the one in place. */
int pcm_octo_reset(pcm_ctx *ctx, const pcm_octo_params *params);
/* insertCloudCallback + insertScan of one cloud, given as its ground part (clears only) and its non-ground part: records of
 * stride_bytes, x y z first, host or device memory (device, stride 16, 16-byte aligned: read in place); either may be empty.
 * origin: the sensor origin in the world frame; sensor_to_world: row-major float 4x4 applied to every point first, or NULL.  One
 * stream synchronisation when the table does not grow.  A table that would exceed max_cells: PCM_ERR_OUT_OF_RANGE, and every
 * log-odds is as it was before the call.  result may be NULL. */
int pcm_octo_insert_scan(pcm_ctx *ctx, const void *ground, size_t n_ground, const void *nonground, size_t n_nonground, size_t stride_bytes,
                         int memory, const float origin[3], const float *sensor_to_world, pcm_octo_insert_result *result);
/* PCM_MODEL_LOAM: key frames first .. first + n - 1 of the context's store, one scan each: the corner and surf cloud where they lie
 * on the device, moved by the stored pose, every point non-ground, the origin the pose's translation.  Stops at the first error. */
int pcm_octo_insert_keyframes(pcm_ctx *ctx, int first, int n);
int pcm_octo_info(pcm_ctx *ctx, pcm_octo_map_info *info);
/* the known cells as 16-byte records (int32 key x, y, z; float log-odds) sorted by the packed key (x << 32 | y << 16 | z) into a
 * host or device buffer of capacity records; *n is always set; out NULL with capacity 0 asks for the count */
int pcm_octo_get_cells(pcm_ctx *ctx, void *out, size_t capacity, int memory, size_t *n);
/* octomap_point_cloud_centers: (x, y, z, log-odds) floats of the occupied cells inside the occupancy z window (and past the
 * speckle filter), in the same order and under the same buffer rules */
int pcm_octo_get_occupied(pcm_ctx *ctx, void *out, size_t capacity, int memory, size_t *n);
/* projected_map rebuilt completely at full depth: the geometry, and width x height values (row-major, i + j * width: -1 unknown,
 * 0 free, 100 occupied) into a host or device buffer of capacity cells when grid is not NULL */
int pcm_octo_project(pcm_ctx *ctx, pcm_octo_grid_info *info, int8_t *grid, size_t capacity, int memory);
/* the body of map_saver's P5 image of that map: width x height bytes, rows top-down (205 unknown, 254 free, 0 occupied) */
int pcm_octo_get_pgm(pcm_ctx *ctx, uint8_t *data, size_t capacity, int memory);
/* measurement hooks (tools/bench_octo_map.py).  mark_variant: 0 one ray per lane (the default), 1 one ray per wave (the same map,
 * bit for bit), + 2: without the dry walk in front of the marking walk -- a measurement only: a rejected ray then leaves its marks.
 * timed: device events around the mark pass and around apply + fold of every insert (one more wait per insert).  The phases of
 * the context's last insert: ms[0] mark, ms[1] apply + fold (both summed over the passes of a call that grew the table; zero
 * unless timed), ms[2] host ms spent rehashing, ms[3] mark passes timed. */
int pcm_octo_debug(pcm_ctx *ctx, int mark_variant, int timed);
int pcm_octo_phase_ms(pcm_ctx *ctx, float ms[4]);

/*
 * The ring-tagged scan the LOAM front end reads, made on the device from the sensors' own buffers: jueying_slam's
 * fusion_lidar_camera node (src/tool/integrate_points/src/fusion_lidar_camera.cpp: the LiDAR cloud, then 1-3 depth-camera clouds
 * moved into the LiDAR frame with a ring from their pitch angle) and its rs_to_velodyne / hesai_to_velodyne converters
 * (src/tool/rs_to_velodyne, src/tool/hesai_to_velodyne), which are the one-segment case.  The output is the kept points of the segments in segment
 * order, each segment in input order, as 32-byte records:
 *   PCM_SCAN_OUT_XYZIRT  x y z 1.0f | float intensity @16 | uint16 ring @20, 2 zero bytes | float time @24 | 4 zero bytes
 *   PCM_SCAN_OUT_XYZIR   the same, time bytes zero          PCM_SCAN_OUT_XYZI   x y z 1.0f | intensity | 12 zero bytes
 * i.e. stride 32, intensity offset 16, ring offset 20 for the front end.  Ring tables are the caller's (the node's own `int`
 * arrays); the library embeds none.  A context of any model.  DESIGN.md section 15.
 */
#define PCM_SCAN_MAX_SEGMENTS 8
#define PCM_SCAN_LIDAR_XYZIRT 0 /* vendor XYZIRT records: ring and double timestamp read from the record (handle_pc_msg) */
#define PCM_SCAN_LIDAR_XYZI 1   /* organised XYZI cloud: ring from the point's position through ring_table, time 0 */
#define PCM_SCAN_DEPTH 2        /* depth-camera cloud (pcl::PointXYZRGB, x y z first): convert_depth */
#define PCM_SCAN_INTENSITY_FLOAT 0
#define PCM_SCAN_INTENSITY_UINT8 1 /* converted to float by value */
#define PCM_SCAN_RING_BY_HEIGHT 0  /* the reference's rule: height 16 -> table[id / width], height 128 -> table[id % height], else an error */
#define PCM_SCAN_RING_DIV_WIDTH 1  /* table[id / width] whatever the height */
#define PCM_SCAN_RING_MOD_HEIGHT 2 /* table[id % height] whatever the height */
#define PCM_SCAN_OUT_XYZI 0        /* the converters' output_type */
#define PCM_SCAN_OUT_XYZIR 1
#define PCM_SCAN_OUT_XYZIRT 2

typedef struct pcm_scan_segment {
  int32_t kind;                  /* PCM_SCAN_LIDAR_XYZIRT / PCM_SCAN_LIDAR_XYZI / PCM_SCAN_DEPTH */
  int32_t memory;                /* PCM_MEM_HOST (staged in one upload) or PCM_MEM_DEVICE (read in place) */
  const void *points;            /* n records of stride_bytes, three floats x y z first; 4-byte aligned */
  size_t n;
  size_t stride_bytes;
  size_t intensity_offset_bytes; /* LiDAR kinds */
  size_t ring_offset_bytes;      /* LIDAR_XYZIRT: a uint16 */
  size_t timestamp_offset_bytes; /* LIDAR_XYZIRT: a double (4-byte aligned); time = float(timestamp[i] - timestamp[0]) */
  int32_t intensity_type;        /* PCM_SCAN_INTENSITY_* */
  int32_t ring_rule;             /* LIDAR_XYZI: PCM_SCAN_RING_* */
  int32_t width, height;         /* LIDAR_XYZI: the organised cloud's */
  const int *ring_table;         /* LIDAR_XYZI: host memory; every index the rule can reach must lie inside it */
  int32_t ring_table_len;
  int32_t dt_sec, dt_nsec;       /* DEPTH: camera stamp - LiDAR stamp; time = float(dt_sec * 1.0 + dt_nsec / 1000000000.0) */
  int32_t reserved;
  double T[16];                  /* DEPTH: camera_T of the node (the transposed 4x4): out.x = x T[0] + y T[4] + z T[8] + T[12], ... */
} pcm_scan_segment;

typedef struct pcm_scan_fuse_params {
  double depth_filter;           /* 1.8  config/fusion_param.yaml: a camera point with z > depth_filter is dropped; < 0 = off */
  double pitch_scale;            /* 28.6478897565  pitch = asin(z / dist) * pitch_scale */
  double pitch_min;              /* -40  pitch_min <= pitch < pitch_max: ring = table[int(round(pitch + pitch_offset))] */
  double pitch_max;              /* 12 */
  double pitch_offset;           /* 40 */
  const int *pitch_ring_table;   /* host memory (the node's RING_MAP_16); NULL only without DEPTH segments */
  int32_t pitch_ring_table_len;  /* an index outside the table gives ring_otherwise and is counted (n_pitch_index_clamped) */
  int32_t ring_below;            /* 47  pitch < pitch_min */
  int32_t ring_otherwise;        /* 51  pitch >= pitch_max or NaN */
  float depth_intensity;         /* 100 */
  int32_t output_layout;         /* PCM_SCAN_OUT_XYZIRT */
  int32_t reserved[9];
} pcm_scan_fuse_params;

typedef struct pcm_scan_segment_counts {
  uint32_t n_in, n_nan, n_depth_filtered, n_kept;
  uint32_t out_offset;           /* first record of this segment in the output */
  uint32_t reserved[3];
} pcm_scan_segment_counts;

typedef struct pcm_scan_fuse_result {
  pcm_scan_segment_counts seg[PCM_SCAN_MAX_SEGMENTS];
  uint32_t n_out;
  uint32_t n_pitch_index_clamped;
  int32_t status;
  int32_t reserved[5];
} pcm_scan_fuse_result;

/* the reference's scalars; no table */
void pcm_scan_default_fuse_params(pcm_scan_fuse_params *params);
/* 1..8 segments of any kinds in any order, at most 2^27 points together.  params NULL = defaults (no DEPTH segment then).
 * out NULL: the records stay in a buffer of the context (pcm_scan_fused), nothing but the counters returns to the host.
 * Else `out` (out_memory: host or device) holds capacity_points records; when that is too small the counts are set, no
 * record past the capacity is written and PCM_ERR_INVALID_ARGUMENT returns. */
int pcm_scan_fuse(pcm_ctx *ctx, const pcm_scan_segment *segs, int n_segs, const pcm_scan_fuse_params *params, void *out, size_t capacity_points, int out_memory,
                  pcm_scan_fuse_result *res);
/* the last pcm_scan_fuse with out = NULL: device memory of the context, valid until the next call of it */
int pcm_scan_fused(pcm_ctx *ctx, const void **device_points, size_t *n);

/* ---- spinning-LiDAR handlers of jueying_lio's PointCloudPreprocess on sensor_msgs::PointCloud2 records ------------------------------
 * VelodyneHandler (jueying_lio/src/pointcloud_preprocess.cc:151-227), RslidarHandler (:229-305), Oust64Handler (:120-149) and
 * LivoxHandler (:89-118): n records of msg->data.data() -> the kept points, in input order, as pcl::PointXYZINormal records (48
 * bytes: x y z 1, 0 0 0 0, intensity, curvature [ms], 0 0), exactly what pcm_livox_filter writes.  The record is described by a
 * stride and byte offsets (x, with y and z behind it, intensity: floats; the time and ring fields by their kinds); every offset
 * but the ring's is a multiple of 4 and the buffer is 4-byte aligned.  Velodyne and RoboSense clouds whose last point's time is
 * not > 0 get their offset times from the yaw of each point and per-ring state carried through the cloud; on the device that
 * serial chain runs as an exact scan over composed functions.  A context of any model.  DESIGN.md section 16. */
#define PCM_LIDAR_VELODYNE 2   /* the reference's LidarType values (pointcloud_preprocess.h) */
#define PCM_LIDAR_OUSTER 3
#define PCM_LIDAR_RSLIDAR 4
#define PCM_LIDAR_LIVOX_STD 5  /* livox in PointCloud2 form */
#define PCM_LIDAR_TIME_FLOAT 0
#define PCM_LIDAR_TIME_DOUBLE 1
#define PCM_LIDAR_TIME_UINT32 2
#define PCM_LIDAR_RING_UINT8 0
#define PCM_LIDAR_RING_UINT16 1
#define PCM_LIDAR_MAX_SCANS 256

typedef struct pcm_lidar_desc {
  int32_t type;                  /* PCM_LIDAR_* */
  int32_t time_kind;             /* PCM_LIDAR_TIME_* of the field at time_offset_bytes */
  int32_t ring_kind;             /* PCM_LIDAR_RING_* of the field at ring_offset_bytes (Velodyne / RoboSense without times only) */
  int32_t num_scans;             /* scan_line: rings are 0 .. num_scans - 1, at most PCM_LIDAR_MAX_SCANS */
  int32_t point_filter_num;      /* point i is a candidate iff i % point_filter_num == 0 */
  float time_scale;              /* Velodyne, RoboSense, Livox: time unit -> ms */
  size_t stride_bytes;
  size_t xyz_offset_bytes;
  size_t intensity_offset_bytes;
  size_t time_offset_bytes;
  size_t ring_offset_bytes;
  double blind;                  /* compared squared: kept when r^2 > blind^2 (Velodyne, RoboSense), when !(r^2 < blind^2) (Ouster, Livox) */
  int32_t reserved[8];
} pcm_lidar_desc;

/* the reference's PCL struct of the type (velodyne_ros / rslidar_ros / ouster_ros / livox_ros ::Point, pointcloud_preprocess.h:12-88)
 * and blind, scan_line, point_filter_num, time_scale of its config file (velodyne / ouster64 / rslidar / livox .yaml) */
int pcm_lidar_default_desc(int type, pcm_lidar_desc *desc);
/* points: n records in host or device memory; out: capacity_points 48-byte records in host or device memory (out_memory).  *n_out is
 * the number of kept points; when it exceeds the capacity no record past the capacity is written and PCM_ERR_INVALID_ARGUMENT
 * returns.  *given_offset_time (may be NULL): 0 when a Velodyne / RoboSense cloud took the yaw path, else 1.  n = 0 gives *n_out = 0.
 * A ring >= num_scans on the yaw path, num_scans > PCM_LIDAR_MAX_SCANS, point_filter_num < 1 or a record too short for its
 * offsets: PCM_ERR_INVALID_ARGUMENT. */
int pcm_lidar_filter(pcm_ctx *ctx, const void *points, size_t n, int memory, const pcm_lidar_desc *desc, void *out, size_t capacity_points, int out_memory,
                     size_t *n_out, int *given_offset_time);
/* pcm_lio_frame_begin for a PointCloud2 cloud: the handler above -> stable sort by (curvature, input index) (the reference's
 * std::sort by curvature, imu_processing.hpp:177-178, made definite) -> motion compensation (skipped when num_poses < 2) ->
 * voxel-grid down-sampling (leaf_size 0: none, the sorted order stays) -> the SOURCE of this object.  The raw cloud is the only
 * bulk upload.  pcm_obs_model and pcm_lio_frame_end follow as after pcm_lio_frame_begin. */
int pcm_lio_frame_begin_cloud(pcm_ctx *ctx, const void *points, size_t n, int memory, const pcm_lidar_desc *desc, float leaf_size, const pcm_imu_pose *poses,
                              int num_poses, const pcm_lio_state *end_state, size_t *n_scan);

/* profiling flags: bit0 = bracket every residual launch with HIP events on the
 * launch stream (pcm_stats.linearize_ms); bit1 = collect the kNN candidate /
 * probe counters (slower kernel variant; use in an untimed pass); bit2 = in-kernel
 * phase stamps of the correspondence-search kernel (diagnostic build); bit3 (with
 * bit0) = bracket only every 4th launch, the phase moving from batch to batch: an
 * event costs a few microseconds on the critical path of every round, which at one
 * pair per round is a tenth of the round (pcm_stats.timed_launches counts them) */
int pcm_set_profiling(pcm_ctx *ctx, int flags);
/* diagnostic (profiling bit2): per-phase s_memtime sums of k_linearize, [7] = tiles; resets on read */
int pcm_debug_phase_cycles(pcm_ctx *ctx, uint64_t out[8]);
int pcm_get_stats(pcm_ctx *ctx, pcm_stats *out);
int pcm_reset_stats(pcm_ctx *ctx);
int pcm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PCM_AMD_H */
