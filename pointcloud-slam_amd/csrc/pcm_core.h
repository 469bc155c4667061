// pcm_core.h -- what the four translation units behind the core C ABI share: pcm_api.hip (the extern "C" entry points of the
// registration objects), lio_api.hip (those of jueying_lio: measurement model, IEKF update, map growth, the frame), prepare.hip
// (lazy build of everything a registration reads, the pair descriptor and the kernel parameters) and align_batch.hip (the
// batch workspace and the round loops).  Internal: nothing here is exported (exports.map).
#pragma once

#include "host_util.h"
#include "pclndt_host.h"

namespace pcm {

// ---- pcm_api.hip: what the LIO entry points (lio_api.hip) use of it -------------------------------------------------------------
int validate_config(pcm_ctx* c, const pcm_config& g);
int set_cloud(pcm_ctx* c, Cloud* cl, const void* points, size_t n, size_t stride, int memory, uint64_t tag, bool allow_borrow);
int refuse_shared(pcm_ctx* c, const char* call);   // the answer of every call that would change a target other contexts read
int reserve_target(pcm_ctx* c, size_t need);       // grow the target point log to hold `need` points (keeps the content)
// ---- lio_api.hip ---------------------------------------------------------------------------------------------------------------
int lio_members_resize(pcm_ctx* c, size_t n);      // residuals_ / point_selected_surf_ follow the scan size (pcm_set_source)

// ---- prepare.hip -------------------------------------------------------------------------------------------------------------
bool is_ndt(int model);         // fast_gicp NDTCuda P2D / D2D
bool is_gicp(int model);        // models with per-point covariances
bool radius_model(int model);   // models that know DIRECT_RADIUS
int ndt_kind(int model);        // template argument of k_ndt: 0 P2D, 1 D2D, 2 VGICP_CUDA
int coord_mode_for(int model);
size_t num_elements(const pcm_ctx* c);   // source elements of a pass: points, or the source voxels of D2D

// lazy (re)build of everything the residual kernel needs
int prepare(pcm_ctx* c);
// sharing a target (pcm_share_target): the first configuration field that decides how a target is built and differs, or null;
// the eager build of everything prepare() derives from the target alone, on c's stream
const char* target_config_difference(const pcm_config& a, const pcm_config& b);
int build_target_for_sharing(pcm_ctx* c);
// the lists the context's residual kernel reads (kind 0 or 2), or an empty view: they exist and the policy still wants them
TargetView lists_view_for(const pcm_ctx* c);
// ... and whether they are the pooled form of following lists (k_linearize_lists' second template argument)
bool lists_pooled_for(const pcm_ctx* c);
// the LIO calls take k_lio_lists: the context set PCM_FLAG_FOLLOWING_LISTS or PCM_FLAG_NEIGHBOUR_LISTS and lists_view_for is not empty
bool lio_on_lists(const pcm_ctx* c);
// pclomp NDT: the neighbour-leaf lists of the context's grid, or an empty view (the cells are then looked up one by one)
TargetView ndt_lists_view(const pcm_ctx* c);

struct Geom {
  int blocks_per_pair;   // residual/reduction kernel
  int points_per_block;
  int tiles_per_pair;    // correspondence-search kernel (256-point tiles)
};
Geom pick_geom(size_t max_n, int npairs, bool ndt = false);
void fill_desc(const pcm_ctx* c, PairDesc* d, double* partials);
KernelParams kernel_params(const pcm_config& g, const Geom& geom);
LsqParams lsq_params(const pcm_config& g);

// ---- icp.hip -------------------------------------------------------------------------------------------------------------------
// one point-to-point ICP registration of a PCM_MODEL_ICP context (the configuration has passed validate_config)
int icp_align(pcm_ctx* c, const float* guess, pcm_result* out);

// ---- align_batch.hip ---------------------------------------------------------------------------------------------------------
// grow-only device workspace shared by the batch launches of one device
struct Workspace {
  int device = -1;
  DevBuf<PairDesc> d_descs{"d_descs"};      // the per-pair arrays grow together (ensure_ws)
  DevBuf<PairState> d_states{"d_states"};
  DevBuf<float> d_guesses{"d_guesses"};     // 16 per pair
  DevBuf<pcm_result> d_results{"d_results"};
  DevBuf<double> d_partials{"d_partials"};
  DevBuf<double> d_sums{"d_sums"};          // kPartialStride per pair
  PinnedBuf<unsigned char> h_flags{"h_flags"};   // mapped pinned host memory: [round][pair] status bytes written by k_finish_round
  unsigned char* d_flags = nullptr;              // device view of h_flags
  DevBuf<unsigned long long> d_stats{"d_stats"};
  DevBuf<unsigned int> d_queue{"d_queue"};   // batch window: index of the next queued pair
  DevBuf<SortJob> d_jobs{"d_jobs"};
  SortScratch sort;
  std::vector<hipEvent_t> ev_round;
  std::vector<hipEvent_t> ev_prof;
  ~Workspace() {
    for (hipEvent_t e : ev_round) hipEventDestroy(e);
    for (hipEvent_t e : ev_prof) hipEventDestroy(e);
  }
};
int ensure_ws(pcm_ctx* c, Workspace** out, int npairs, size_t partial_doubles, int rounds);

int align_batch_impl(pcm_ctx* const* ctxs, int n, const float* guesses, pcm_result* host_out, void* device_out);
// one LINEARIZE or TRIAL pass at a caller-supplied pose (parity hook)
int single_pass(pcm_ctx* c, const double T[16], bool linearize, double sums[kPartialStride]);
// one pclomp NDT pass on the device: launch, read the 48-double row back (pass 0/1: H, g, score; pass 2: H)
int pclndt_eval(pcm_ctx* c, int pass, const NdtOmpParams& P, ndtomp::Eval* e, double gauss_d3 = 0.0);
int pclndt_align_batch(pcm_ctx* const* ctxs, int n, const float* guesses, pcm_result* res);

}  // namespace pcm
