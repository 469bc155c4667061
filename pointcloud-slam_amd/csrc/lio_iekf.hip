// lio_iekf.hip -- the step kernel of pcm_lio_update: jueying_lio's iterated Kalman update between two ObsModel calls, on the device
// (include/pcm_amd.h, pcm_lio_update).  The arithmetic is lio_iekf.h, shared with the host tests.
//
// A round of the update is three launches on the context's stream: the ObsModel search kernel in its device-flag instance
// (kernels.hip, launch_lio_obs_dev), the fixed-order sum of its partial rows (k_lio_finish_gated: k_lio_finish behind the done
// flag) and k_iekf_step.  All max_iter + 1 rounds are queued before the host waits once; a round behind the loop's exit finds
// PairState::mode == MODE_DONE / Ctl::done and returns.
//
// k_iekf_step: ONE wave of 64 lanes, the five 23 x 23 work matrices in LDS (21 KB), FP64, no MFMA -- a latency kernel.  Lane map:
//   state-sized pieces (boxminus, boxplus, A_matrix, S2 matrices, the limit test)   every lane alike, in registers (wave-uniform)
//   re-projections  rows <- G * rows: one COLUMN per lane;  columns <- columns * G: one ROW per lane
//   LU factorisation (partial pivoting)  pivot search: every lane reads column k (LDS broadcast); row swap and multipliers: one
//                   element per lane; trailing update: the (22 - k)^2 elements dealt round-robin over the 64 lanes
//   inverse from the factors   one column of the inverse per lane (forward + back substitution in its own LDS column)
//   K_h, K_x, dx_   one row per lane;   P_ = L_ - K_x P_   element-wise over the 64 lanes
#include "pcm_host.h"

namespace pcm {

static_assert(sizeof(iekf::PoseF) == sizeof(LioPose), "iekf::PoseF mirrors LioPose");
static_assert(offsetof(iekf::PoseF, rematch) == offsetof(LioPose, rematch), "iekf::PoseF mirrors LioPose");
static_assert(sizeof(iekf::State) == sizeof(pcm_lio_filter_state), "iekf::State mirrors pcm_lio_filter_state");

namespace {
struct WaveExec {
  __device__ int lane() const { return (int)threadIdx.x; }
  __device__ int lanes() const { return 64; }
  __device__ void sync() const { __syncthreads(); }   // one wave: orders its LDS traffic
};
}  // namespace

__global__ void __launch_bounds__(64) k_iekf_step(LioUpdateRecord* __restrict__ rec, const double* __restrict__ sums) {
  __shared__ iekf::Work w;
  __shared__ double s_sums[kLioStride];
  if (rec->b.ctl.done) return;
  for (int k = threadIdx.x; k < kLioStride; k += 64) s_sums[k] = k < kLioSums ? sums[k] : 0.0;
  __syncthreads();
  iekf::step(WaveExec{}, rec->b, s_sums, w, reinterpret_cast<iekf::PoseF*>(&rec->desc.lio));
  if (threadIdx.x == 0 && rec->b.ctl.done) rec->ps.mode = MODE_DONE;
}

// k_lio_finish (kernels.hip) behind the done flag: same rows, same order of additions
__global__ void __launch_bounds__(1024) k_lio_finish_gated(const LioUpdateRecord* __restrict__ rec, const double* __restrict__ partials, int nblocks,
                                                           double* __restrict__ out) {
  __shared__ double s_grp[10 * kLioStride];
  if (rec->b.ctl.done) return;
  const int t = threadIdx.x % kLioStride, r = threadIdx.x / kLioStride;
  if (r < 10) {
    double v = 0.0;
    if (t < kLioSums) for (int b = r; b < nblocks; b += 10) v += partials[(size_t)b * kLioStride + t];
    s_grp[r * kLioStride + t] = v;
  }
  __syncthreads();
  if (threadIdx.x < kLioSums) {
    double v = 0.0;
    for (int k = 0; k < 10; k++) v += s_grp[k * kLioStride + threadIdx.x];
    out[threadIdx.x] = v;
  }
}

void launch_lio_finish_gated(hipStream_t stream, const LioUpdateRecord* rec, const double* d_partials, int nblocks, double* d_out) {
  k_lio_finish_gated<<<1, 1024, 0, stream>>>(rec, d_partials, nblocks, d_out);
}
void launch_iekf_step(hipStream_t stream, LioUpdateRecord* rec, const double* d_sums) { k_iekf_step<<<1, 64, 0, stream>>>(rec, d_sums); }

}  // namespace pcm
