// icp.hip -- point-to-point ICP on the device (PCM_MODEL_ICP, include/pcm_amd.h): pcl::IterativeClosestPoint as
// jueying_slam's performSCLoopClosure uses it (mapOptmization.cpp:768-779), by the rules of icp.h.
//
// The target is the brick-major cloud and its brick table (prepare.hip, as GICP's without covariances); the source is read
// where pcm_set_source left it -- a PCM_MEM_DEVICE buffer of 16-byte records in place.  The loop is device-resident: per
// iteration
//   k_icp_pairs   one source point per lane: the point through the float view of the pose, its exact nearest target point by the
//                 voxel-column walk of nn_walk.h (nearest1), the pair's 17 terms in double; a wave butterfly, then the four waves
//                 in order: one row of 17 sums per workgroup.  No atomics: two runs give the same bytes.
//   k_icp_step    one workgroup: the rows added in block order (eight strided slices, each in ascending block order, then the
//                 slices in order), and one thread takes the closed-form step, composes the pose, tests convergence and writes
//                 the pose, the counters, the trace entry and the done flag into the state block.
// Both return at once when the flag is set.  The host queues icp::kChunk iterations, reads the state block back and waits: one
// wait per chunk, never one per iteration.  Compiled with -ffp-contract=off.
#include "pcm_core.h"
#include "icp.h"
#include "nn_walk.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

using namespace pcm;

namespace {

struct DevState {
  icp::Loop L;
  icp::Params P;
  double walk_sq;   // the next double above P.max_sq: nearest1's exclusive threshold made inclusive
};

struct IcpState {
  pcm_icp_params params;
  pcm_icp_info info;
  DevBuf<DevState> d_state{"icp state"};
  DevBuf<double> d_rows{"icp rows"};       // kSums per workgroup of the pair kernel
  DevBuf<double> d_trace{"icp trace"};     // (N, mse) per iteration
  PinnedBuf<DevState> h_state{"icp state image"};   // [0] what is uploaded, [1] what comes back
  int trace_n = 0;
  IcpState() { pcm_icp_default_params(&params); std::memset(&info, 0, sizeof(info)); }
};

__global__ void __launch_bounds__(256) k_icp_pairs(TargetView tg, int coord_mode, const float4* __restrict__ src, uint32_t n, const DevState* __restrict__ st, double* __restrict__ rows) {
  if (st->L.done) return;
  float m[12];
  icp::pose_to_float(st->L.F, m);
  const double max_sq = st->P.max_sq, walk_sq = st->walk_sq;
  double v[icp::kSums];
#pragma unroll
  for (int a = 0; a < icp::kSums; a++) v[a] = 0.0;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) {
    const float4 p = gload4(src + i);
    float c[3];
    icp::transform_point(m, p.x, p.y, p.z, c);
    const int j = nearest1(tg, coord_mode, c, walk_sq);   // -1: non-finite, no target point, or beyond the threshold
    if (j >= 0) {
      const float4 mp = gload4(tg.pts + j);
      const float q[3] = {mp.x, mp.y, mp.z};
      const float d2 = icp::sq_dist(q, c);
      if (icp::keep_pair(d2, max_sq)) icp::pair_terms(c, q, d2, v);
    }
  }
  __shared__ double s_w[4][icp::kSums];
#pragma unroll
  for (int a = 0; a < icp::kSums; a++) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[a] += __shfl_xor(v[a], off, 64);
  }
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int a = 0; a < icp::kSums; a++) s_w[threadIdx.x >> 6][a] = v[a];
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)icp::kSums) {
    const uint32_t a = threadIdx.x;
    gstore_d(rows + (size_t)blockIdx.x * icp::kSums + a, ((s_w[0][a] + s_w[1][a]) + s_w[2][a]) + s_w[3][a]);
  }
}

__global__ void __launch_bounds__(256) k_icp_step(DevState* __restrict__ st, const double* __restrict__ rows, uint32_t nblocks, double* __restrict__ trace) {
  if (st->L.done) return;   // read by every thread before the barriers below, written by thread 0 after them
  __shared__ double s_part[8][icp::kSums];
  __shared__ double s_sum[icp::kSums];
  const uint32_t a = threadIdx.x & 31u, slice = threadIdx.x >> 5;
  if (a < (uint32_t)icp::kSums) {
    double acc = 0.0;
    for (uint32_t b = slice; b < nblocks; b += 8u) acc += gload_d(rows + (size_t)b * icp::kSums + a);
    s_part[slice][a] = acc;
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)icp::kSums) {
    double acc = s_part[0][threadIdx.x];
#pragma unroll
    for (int s = 1; s < 8; s++) acc += s_part[s][threadIdx.x];
    s_sum[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x != 0u) return;
  double s[icp::kSums];
  for (int k = 0; k < icp::kSums; k++) s[k] = s_sum[k];
  icp::Loop L = st->L;
  const int slot = L.iterations;   // < max_iterations: the loop is done once iterations reaches it
  icp::loop_step(st->P, s, &L);
  trace[2 * slot] = s[16];
  trace[2 * slot + 1] = s[16] >= 3.0 ? L.mse : 0.0;
  st->L = L;
}

int check_icp_params(pcm_ctx* c, const pcm_icp_params& p) {
  if (p.max_iterations < 1 || p.max_iterations > (1 << 20)) { c->err = "pcm_icp_set_params: max_iterations must be in [1, 2^20]"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.max_correspondence_distance > 0.0)) { c->err = "pcm_icp_set_params: max_correspondence_distance must be > 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.transformation_epsilon != p.transformation_epsilon || p.rotation_epsilon != p.rotation_epsilon || p.euclidean_fitness_epsilon != p.euclidean_fitness_epsilon ||
      p.mse_absolute != p.mse_absolute) {
    c->err = "pcm_icp_set_params: the epsilons must be numbers"; return PCM_ERR_INVALID_ARGUMENT;
  }
  return PCM_OK;
}

int need_icp(pcm_ctx* c, const char* who) {
  if (!c) return PCM_ERR_INVALID_ARGUMENT;
  if (c->device < 0) return PCM_ERR_HIP;
  if (c->cfg.model != PCM_MODEL_ICP) { c->err = std::string(who) + " needs a context created with PCM_MODEL_ICP"; return PCM_ERR_UNSUPPORTED; }
  return PCM_OK;
}

}  // namespace

int pcm::icp_align(pcm_ctx* c, const float* guess, pcm_result* out) {
  IcpState* S = c->icp.get_or_create<IcpState>();
  if (!S) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  int rc = prepare(c);
  if (rc != PCM_OK) return rc;
  if (!c->tg->map.valid || !c->tg->map.pts) { c->err = "pcm_align: the target map is not built"; return PCM_ERR_INTERNAL; }
  const pcm_icp_params& p = S->params;
  const uint32_t n = (uint32_t)c->src.n, nblocks = (n + 255u) / 256u;
  rc = S->d_state.reserve(c, 1, 1);
  if (rc == PCM_OK) rc = S->d_rows.reserve(c, (size_t)nblocks * icp::kSums, (size_t)nblocks * icp::kSums);
  if (rc == PCM_OK) rc = S->d_trace.reserve(c, 2 * (size_t)p.max_iterations, 2 * (size_t)p.max_iterations);
  if (rc == PCM_OK) rc = S->h_state.reserve(c, 2, 2);
  if (rc != PCM_OK) return rc;
  DevState& up = S->h_state.p[0];
  DevState& down = S->h_state.p[1];
  std::memset(&up, 0, sizeof(up));
  icp::loop_begin(&up.L, guess);
  up.P.max_iterations = p.max_iterations;
  up.P.max_sq = icp::max_sq_of(p.max_correspondence_distance);
  up.P.transformation_epsilon = p.transformation_epsilon;
  up.P.rot_thr = icp::rot_thr_of(p.rotation_epsilon, p.transformation_epsilon);
  up.P.euclidean_fitness_epsilon = p.euclidean_fitness_epsilon;
  up.P.mse_absolute = p.mse_absolute;
  up.walk_sq = std::nextafter(up.P.max_sq, INFINITY);
  std::memset(&down, 0, sizeof(down));
  S->trace_n = 0;
  std::memset(&S->info, 0, sizeof(S->info));
  PCM_HIPCK(c, hipMemcpyAsync(S->d_state.p, &up, sizeof(DevState), hipMemcpyHostToDevice, c->stream));
  const TargetView tg = view_of(c->tg->map);
  const int mode = coord_mode_for(c->cfg.model);
  for (int queued = 0; queued < p.max_iterations && !down.L.done;) {
    const int m = std::min(icp::kChunk, p.max_iterations - queued);
    for (int k = 0; k < m; k++) {
      k_icp_pairs<<<nblocks, 256, 0, c->stream>>>(tg, mode, c->src.d_pts, n, S->d_state.p, S->d_rows.p);
      k_icp_step<<<1, 256, 0, c->stream>>>(S->d_state.p, S->d_rows.p, nblocks, S->d_trace.p);
    }
    queued += m;
    PCM_HIPCK(c, hipGetLastError());
    PCM_HIPCK(c, hipMemcpyAsync(&down, S->d_state.p, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the one wait of this chunk
  }
  const icp::Loop& L = down.L;
  if (!L.done) { c->err = "pcm_align (ICP): the loop did not end within max_iterations (library bug)"; return PCM_ERR_INTERNAL; }
  S->info.stop_reason = L.stop;
  S->info.iterations = L.iterations;
  S->info.converged = L.converged;
  S->info.num_pairs = (uint64_t)L.num_pairs;
  S->info.mse = L.mse;
  S->trace_n = L.iterations + (L.stop == icp::kStopNoCorrespondences ? 1 : 0);
  std::memset(out, 0, sizeof(*out));
  for (int a = 0; a < 16; a++) { out->T64[a] = L.F[a]; out->T[a] = (float)L.F[a]; }
  out->cost = L.mse;
  out->iterations = L.iterations;
  out->converged = L.converged;
  out->num_linearize = S->trace_n;
  out->num_inliers = (int32_t)std::min(L.num_pairs, 2147483647.0);
  out->status = PCM_OK;
  return PCM_OK;
}

static_assert(PCM_ICP_STOP_NONE == icp::kStopNone && PCM_ICP_STOP_ITERATIONS == icp::kStopIterations && PCM_ICP_STOP_TRANSFORM == icp::kStopTransform &&
                  PCM_ICP_STOP_ABS_MSE == icp::kStopAbsMse && PCM_ICP_STOP_REL_MSE == icp::kStopRelMse && PCM_ICP_STOP_NO_CORRESPONDENCES == icp::kStopNoCorrespondences &&
                  PCM_ICP_CHUNK_ITERATIONS == icp::kChunk,
              "ICP constants");

extern "C" {

void pcm_icp_default_params(pcm_icp_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_iterations = 10;                              // pcl::Registration: max_iterations_ (10)
  p->max_correspondence_distance = std::sqrt(DBL_MAX); // corr_dist_threshold_ (sqrt of the largest double)
  p->transformation_epsilon = 0.0;                     // transformation_epsilon_
  p->rotation_epsilon = 0.0;                           // transformation_rotation_epsilon_: <= 0 means 1 - transformation_epsilon
  p->euclidean_fitness_epsilon = -DBL_MAX;             // euclidean_fitness_epsilon_ (minus the largest double)
  p->mse_absolute = 1e-12;                             // DefaultConvergenceCriteria: mse_threshold_absolute_
}

int pcm_icp_set_params(pcm_ctx* c, const pcm_icp_params* params) {
  int rc = need_icp(c, "pcm_icp_set_params");
  if (rc != PCM_OK) return rc;
  if (!params) { c->err = "pcm_icp_set_params: null params"; return PCM_ERR_INVALID_ARGUMENT; }
  if ((rc = check_icp_params(c, *params)) != PCM_OK) return rc;
  IcpState* S = c->icp.get_or_create<IcpState>();
  if (!S) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  S->params = *params;
  std::memset(S->params.reserved, 0, sizeof(S->params.reserved));
  return PCM_OK;
}

int pcm_icp_get_params(pcm_ctx* c, pcm_icp_params* params) {
  int rc = need_icp(c, "pcm_icp_get_params");
  if (rc != PCM_OK) return rc;
  if (!params) { c->err = "pcm_icp_get_params: null params"; return PCM_ERR_INVALID_ARGUMENT; }
  const IcpState* S = c->icp.get<IcpState>();
  if (S) *params = S->params; else pcm_icp_default_params(params);
  return PCM_OK;
}

int pcm_icp_last(pcm_ctx* c, pcm_icp_info* info) {
  int rc = need_icp(c, "pcm_icp_last");
  if (rc != PCM_OK) return rc;
  if (!info) { c->err = "pcm_icp_last: null info"; return PCM_ERR_INVALID_ARGUMENT; }
  const IcpState* S = c->icp.get<IcpState>();
  if (S) *info = S->info; else std::memset(info, 0, sizeof(*info));
  return PCM_OK;
}

int pcm_icp_trace(pcm_ctx* c, int32_t capacity, uint64_t* num_pairs, double* mse, int32_t* n) {
  int rc = need_icp(c, "pcm_icp_trace");
  if (rc != PCM_OK) return rc;
  if (!n) { c->err = "pcm_icp_trace: null n"; return PCM_ERR_INVALID_ARGUMENT; }
  const IcpState* S = c->icp.get<IcpState>();
  const int count = S ? S->trace_n : 0;
  *n = count;
  if (!num_pairs && !mse) return PCM_OK;
  if (capacity < count) { c->err = "pcm_icp_trace: buffer too small"; return PCM_ERR_INVALID_ARGUMENT; }
  if (count == 0) return PCM_OK;
  std::vector<double> t(2 * (size_t)count);
  PCM_HIPCK(c, hipSetDevice(c->device));
  PCM_HIPCK(c, hipMemcpyAsync(t.data(), S->d_trace.p, sizeof(double) * t.size(), hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < count; k++) {
    if (num_pairs) num_pairs[k] = (uint64_t)t[2 * k];
    if (mse) mse[k] = t[2 * k + 1];
  }
  return PCM_OK;
}

}  // extern "C"
