// lio_predict.hip -- pcm_lio_imu_init / pcm_lio_propagate: what ImuProcess::Process does before a jueying_lio frame (include/pcm_amd.h;
// DESIGN.md section 18).  The arithmetic is lio_predict.h, shared with the host tests.
//
// k_imu_propagate: ONE wave of 64 lanes runs the whole forward loop of UndistortPcl -- one esekf::predict per kept IMU pair and the
// closing one -- so a frame is one upload, one launch, one download.  P, F_x1, one 23 x 23 temporary (3 x 529 doubles), the 23 x 12
// dt * f_w_final and the state-sized pieces of the current predict live in LDS (15.6 KB), FP64, no MFMA -- a latency kernel.  Lane map:
//   state-sized pieces (f, the df_dx / df_dw blocks, oplus, A_matrix, the S2 matrices)   every lane alike, in registers; lane 0
//                   leaves them in LDS for the element-wise phases
//   F_x1, dt * f_w_final                      element-wise over the 64 lanes
//   T = F_x1 P;  P = T F_x1^T + W Q W^T       element-wise; each element is summed by one lane from k = 0 up, zeros included
#include <cmath>
#include <cstddef>
#include <cstring>

#include "lio_predict.h"
#include "pcm_host.h"

namespace pcm {

static_assert(sizeof(predict::Sample) == sizeof(pcm_imu_sample), "predict::Sample mirrors pcm_imu_sample");
static_assert(sizeof(predict::Pose) == sizeof(pcm_imu_pose), "predict::Pose mirrors pcm_imu_pose");
static_assert(offsetof(predict::Pose, rot) == offsetof(pcm_imu_pose, rot), "predict::Pose mirrors pcm_imu_pose");
static_assert(sizeof(predict::ImuState) == sizeof(pcm_lio_imu_state), "predict::ImuState mirrors pcm_lio_imu_state");
static_assert(offsetof(predict::ImuState, last_imu) == offsetof(pcm_lio_imu_state, last_imu), "predict::ImuState mirrors pcm_lio_imu_state");
static_assert(offsetof(predict::ImuState, need_init) == offsetof(pcm_lio_imu_state, need_init), "predict::ImuState mirrors pcm_lio_imu_state");
static_assert(sizeof(predict::Frame) % 8 == 0 && sizeof(predict::Result) % 8 == 0, "the samples and the poses follow their headers aligned");

namespace {
struct WaveExec {
  __device__ int lane() const { return (int)threadIdx.x; }
  __device__ int lanes() const { return 64; }
  __device__ void sync() const { __syncthreads(); }   // one wave: orders its LDS traffic
};
}  // namespace

// in: predict::Frame + n samples; out: predict::Result + room for n + 1 poses
__global__ void __launch_bounds__(64) k_imu_propagate(const char* __restrict__ in, char* __restrict__ out) {
  __shared__ predict::Work w;
  const predict::Frame* fr = reinterpret_cast<const predict::Frame*>(in);
  const predict::Sample* smp = reinterpret_cast<const predict::Sample*>(in + sizeof(predict::Frame));
  predict::Result* res = reinterpret_cast<predict::Result*>(out);
  predict::Pose* poses = reinterpret_cast<predict::Pose*>(out + sizeof(predict::Result));
  predict::propagate(WaveExec{}, *fr, smp, *res, poses, w);
}

}  // namespace pcm

using namespace pcm;

void pcm_lio_default_imu_state(pcm_lio_imu_state* s) {
  if (s) predict::default_imu_state(reinterpret_cast<predict::ImuState*>(s));
}

namespace {
bool all_finite(const double* v, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (!std::isfinite(v[k])) return false;
  return true;
}
bool samples_finite(const pcm_imu_sample* imu, int n) { return all_finite(reinterpret_cast<const double*>(imu), (size_t)n * (sizeof(pcm_imu_sample) / sizeof(double))); }
}  // namespace

int pcm_lio_imu_init(pcm_lio_imu_state* s, const pcm_imu_sample* imu, int n, pcm_lio_filter_state* x, double* P) {
  if (!s || !imu || !x || !P || n < 1) return PCM_ERR_INVALID_ARGUMENT;
  if (!s->need_init || !samples_finite(imu, n)) return PCM_ERR_INVALID_ARGUMENT;
  predict::imu_init(reinterpret_cast<predict::ImuState*>(s), reinterpret_cast<const predict::Sample*>(imu), n, reinterpret_cast<iekf::State*>(x), P);
  return PCM_OK;
}

int pcm_lio_propagate(pcm_ctx* c, pcm_lio_imu_state* s, const pcm_imu_sample* imu, int n, double pcl_beg_time, double pcl_end_time, pcm_lio_filter_state* x, double* P,
                      pcm_imu_pose* poses, int capacity, int* num_poses) {
  if (!c) return PCM_ERR_INVALID_ARGUMENT;
  if (c->device < 0) return PCM_ERR_HIP;
  if (!s || !imu || !x || !P || !poses || !num_poses) { c->err = "pcm_lio_propagate: null argument"; return PCM_ERR_INVALID_ARGUMENT; }
  if (n < 1) { c->err = "pcm_lio_propagate: no IMU sample (ImuProcess::Process returns on an empty queue)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (n > predict::kMaxSamples) { c->err = "pcm_lio_propagate: more than 1024 IMU samples in one call"; return PCM_ERR_OUT_OF_RANGE; }
  if (capacity < n + 1) { c->err = "pcm_lio_propagate: poses must hold n + 1 entries"; return PCM_ERR_INVALID_ARGUMENT; }
  if (s->need_init) { c->err = "pcm_lio_propagate: the IMU state is not initialised (pcm_lio_imu_init until need_init is 0)"; return PCM_ERR_INVALID_ARGUMENT; }
  const predict::ImuState* is = reinterpret_cast<const predict::ImuState*>(s);
  if (!samples_finite(imu, n) || !std::isfinite(pcl_beg_time) || !std::isfinite(pcl_end_time) || !all_finite(reinterpret_cast<const double*>(x), sizeof(*x) / sizeof(double)) ||
      !all_finite(P, iekf::NN) || !all_finite(reinterpret_cast<const double*>(s), offsetof(pcm_lio_imu_state, init_iter_num) / sizeof(double))) {
    c->err = "pcm_lio_propagate: an input is not finite";
    return PCM_ERR_INVALID_ARGUMENT;
  }
  if (!((is->mean_acc[0] * is->mean_acc[0] + is->mean_acc[1] * is->mean_acc[1]) + is->mean_acc[2] * is->mean_acc[2] > 0.0)) {
    c->err = "pcm_lio_propagate: mean_acc is zero";
    return PCM_ERR_INVALID_ARGUMENT;
  }
  PCM_HIPCK(c, hipSetDevice(c->device));
  const size_t in_bytes = sizeof(predict::Frame) + sizeof(predict::Sample) * (size_t)n;
  const size_t out_bytes = sizeof(predict::Result) + sizeof(predict::Pose) * (size_t)(n + 1);
  const size_t o_out = up256(in_bytes), total = o_out + up256(out_bytes);
  const size_t cap = up256(sizeof(predict::Frame) + sizeof(predict::Sample) * (size_t)predict::kMaxSamples) +
                     up256(sizeof(predict::Result) + sizeof(predict::Pose) * (size_t)(predict::kMaxSamples + 1));   // one allocation serves every n
  int rc = c->lio_prop.reserve(c, total, cap);
  if (rc != PCM_OK) return rc;
  rc = c->lio_prop_host.reserve(c, total, cap);
  if (rc != PCM_OK) return rc;
  char* h = c->lio_prop_host.p;
  char* d = c->lio_prop.p;
  const iekf::State& xs = *reinterpret_cast<const iekf::State*>(x);
  predict::fill_frame(*is, reinterpret_cast<const predict::Sample*>(imu), n, pcl_beg_time, pcl_end_time, xs, P, reinterpret_cast<predict::Frame*>(h),
                      reinterpret_cast<predict::Sample*>(h + sizeof(predict::Frame)));
  hipStream_t st = c->stream;
  PCM_HIPCK(c, hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
  k_imu_propagate<<<1, 64, 0, st>>>(d, d + o_out);
  PCM_HIPCK(c, hipGetLastError());
  PCM_HIPCK(c, hipMemcpyAsync(h + o_out, d + o_out, out_bytes, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipStreamSynchronize(st));
  const predict::Result& r = *reinterpret_cast<const predict::Result*>(h + o_out);
  if (r.num_poses < 1 || r.num_poses > n + 1 || !all_finite(reinterpret_cast<const double*>(&r), offsetof(predict::Result, num_poses) / sizeof(double))) {
    c->err = "pcm_lio_propagate: the propagated state or covariance is not finite";
    return PCM_ERR_INTERNAL;
  }
  predict::take_result(r, reinterpret_cast<const predict::Sample*>(imu), n, pcl_end_time, reinterpret_cast<predict::ImuState*>(s), reinterpret_cast<iekf::State*>(x), P);
  std::memcpy(poses, h + o_out + sizeof(predict::Result), sizeof(pcm_imu_pose) * (size_t)r.num_poses);
  *num_poses = r.num_poses;
  return PCM_OK;
}
