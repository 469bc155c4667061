// g++ view of pointcloud-slam_amd/csrc/lio_predict.h for tests/test_lio_predict.py: the very functions k_imu_propagate runs, with one
// lane.  With -DLIO_PREDICT_HOOKS_MAIN it is a stand-alone program that replays a file of propagation cases (the host-code check
// under -fsanitize=address,undefined).
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "lio_predict.h"
#include "pcm_amd.h"

using namespace pcm::predict;
using pcm::iekf::SerialExec;

static_assert(sizeof(Sample) == sizeof(pcm_imu_sample), "sample layout");
static_assert(sizeof(Pose) == sizeof(pcm_imu_pose), "pose layout");
static_assert(sizeof(ImuState) == sizeof(pcm_lio_imu_state), "imu state layout");
static_assert(offsetof(ImuState, last_imu) == offsetof(pcm_lio_imu_state, last_imu), "imu state layout");
static_assert(offsetof(ImuState, need_init) == offsetof(pcm_lio_imu_state, need_init), "imu state layout");
static_assert(sizeof(State) == sizeof(pcm_lio_filter_state), "state layout");

extern "C" {

// f (24), f_x (24 x 23) and f_w (24 x 12) at a state and an input (acc, gyro)
void pred_hook_f(const double* x26, const double* in6, double* f24, double* f_x, double* f_w) {
  State s; memcpy(&s, x26, sizeof(s));
  Input in; memcpy(&in, in6, sizeof(in));
  Lin L;
  memset(&L, 0, sizeof(L));
  get_f(s, in, f24);
  df_blocks(s, in, L);
  for (int r = 0; r < 24; r++) {
    for (int c = 0; c < N; c++) f_x[r * N + c] = fx(L, r, c);
    for (int a = 0; a < NW; a++) f_w[r * NW + a] = fw(L, r, a);
  }
}

// one esekf::predict: x, P in / out; F_x1 (23 x 23) and dt * f_w_final (23 x 12) out
void pred_hook_predict(double* x26, double* P, double dt, const double* q12, const double* in6, double* F, double* W) {
  static Work w;
  State s; memcpy(&s, x26, sizeof(s));
  Input in; memcpy(&in, in6, sizeof(in));
  memcpy(w.P, P, sizeof(w.P));
  predict(SerialExec{}, s, w, dt, q12, in);
  memcpy(x26, &s, sizeof(s));
  memcpy(P, w.P, sizeof(w.P));
  if (F) memcpy(F, w.F, sizeof(w.F));
  if (W) memcpy(W, w.W, sizeof(w.W));
}

// the forward loop + closing predict as pcm_lio_propagate runs it, with one lane; poses must hold n + 1
int pred_hook_propagate(pcm_lio_imu_state* st, const pcm_imu_sample* imu, int n, double beg, double end, double* x26, double* P, pcm_imu_pose* poses) {
  static Work w;
  ImuState* s = reinterpret_cast<ImuState*>(st);
  const Sample* smp_in = reinterpret_cast<const Sample*>(imu);
  State x; memcpy(&x, x26, sizeof(x));
  std::vector<char> blk(sizeof(Frame) + sizeof(Sample) * (size_t)n), ob(sizeof(Result) + sizeof(Pose) * (size_t)(n + 1));
  Frame* fr = reinterpret_cast<Frame*>(blk.data());
  Sample* smp = reinterpret_cast<Sample*>(blk.data() + sizeof(Frame));
  fill_frame(*s, smp_in, n, beg, end, x, P, fr, smp);
  Result* r = reinterpret_cast<Result*>(ob.data());
  Pose* ps = reinterpret_cast<Pose*>(ob.data() + sizeof(Result));
  propagate(SerialExec{}, *fr, smp, *r, ps, w);
  take_result(*r, smp_in, n, end, s, &x, P);
  memcpy(x26, &x, sizeof(x));
  memcpy(poses, ps, sizeof(Pose) * (size_t)r->num_poses);
  return r->num_poses;
}

void pred_hook_default(pcm_lio_imu_state* st) { default_imu_state(reinterpret_cast<ImuState*>(st)); }

void pred_hook_imu_init(pcm_lio_imu_state* st, const pcm_imu_sample* imu, int n, double* x26, double* P) {
  State x; memcpy(&x, x26, sizeof(x));
  imu_init(reinterpret_cast<ImuState*>(st), reinterpret_cast<const Sample*>(imu), n, &x, P);
  memcpy(x26, &x, sizeof(x));
}

void pred_hook_layout(long* o) {
  o[0] = sizeof(pcm_imu_sample); o[1] = sizeof(pcm_lio_imu_state); o[2] = offsetof(pcm_lio_imu_state, cov_acc_scale);
  o[3] = offsetof(pcm_lio_imu_state, lidar_R_wrt_imu); o[4] = offsetof(pcm_lio_imu_state, last_lidar_end_time); o[5] = offsetof(pcm_lio_imu_state, last_imu);
  o[6] = offsetof(pcm_lio_imu_state, init_iter_num); o[7] = offsetof(pcm_lio_imu_state, reserved); o[8] = sizeof(pcm_imu_pose);
  o[9] = sizeof(Frame); o[10] = sizeof(Result); o[11] = kMaxSamples;
}

}  // extern "C"

#ifdef LIO_PREDICT_HOOKS_MAIN
// file: records of { int32 kind (0 propagate, 1 init), int32 n, double beg, end, pcm_lio_imu_state, x (26), P (529), n samples };
// prints one line per record: kind, n, poses, and the sums of x and of P (the caller compares them with the library build)
int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  int32_t head[2];
  int records = 0;
  while (fread(head, sizeof(head), 1, fp) == 1) {
    const int n = head[1];
    if (n < 1 || n > kMaxSamples) { fprintf(stderr, "bad record\n"); return 2; }
    double t[2], x[26];
    pcm_lio_imu_state st;
    std::vector<double> P(NN);
    std::vector<pcm_imu_sample> imu((size_t)n);
    std::vector<pcm_imu_pose> poses((size_t)n + 1);
    if (fread(t, sizeof(t), 1, fp) != 1 || fread(&st, sizeof(st), 1, fp) != 1 || fread(x, sizeof(x), 1, fp) != 1 ||
        fread(P.data(), sizeof(double) * NN, 1, fp) != 1 || fread(imu.data(), sizeof(pcm_imu_sample) * (size_t)n, 1, fp) != 1) {
      fprintf(stderr, "short record\n");
      return 2;
    }
    int np = 0;
    if (head[0] == 0) np = pred_hook_propagate(&st, imu.data(), n, t[0], t[1], x, P.data(), poses.data());
    else pred_hook_imu_init(&st, imu.data(), n, x, P.data());
    double sx = 0.0, sp = 0.0;
    for (int k = 0; k < 26; k++) sx += x[k];
    for (int k = 0; k < NN; k++) sp += P[k];
    printf("%d %d %d %a %a\n", head[0], n, np, sx, sp);
    records++;
  }
  fclose(fp);
  return records ? 0 : 2;
}
#endif
