// g++ view of pointcloud-slam_amd/csrc/loam_loop.h for tests/test_loam_loop.py: the very functions pcm_loam_loop_verify evaluates
// on the host after its NDT.  With -DLOAM_LOOP_HOOKS_MAIN it is a stand-alone program that runs seeded loop factors, the cases
// near pitch = +-pi/2 included (the host-code check under -fsanitize=address,undefined).
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "loam_loop.h"
#include "pcm_amd.h"

using namespace pcm::loam::loop;

static_assert(PCM_LOAM_LOOP_ACCEPTED == kAccepted && PCM_LOAM_LOOP_REJECTED_SIZE == kRejectedSize && PCM_LOAM_LOOP_REJECTED_NOT_CONVERGED == kRejectedNotConverged &&
                  PCM_LOAM_LOOP_REJECTED_FITNESS == kRejectedFitness && PCM_LOAM_LOOP_NONE == kNoLoop,
              "status codes");

extern "C" {

int loop_hook_size_gate(long long n_cur, long long n_prev, long long min_cur, long long min_prev) { return size_gate(n_cur, n_prev, min_cur, min_prev) ? 1 : 0; }
int loop_hook_accept(int converged, double fitness, float threshold) { return accept_status(converged, fitness, threshold); }
void loop_hook_affine_from_pose(const float* pose6, float* T16) { affine_from_pose(pose6, T16); }
void loop_hook_affine_mul(const float* a, const float* b, float* out) { affine_mul(a, b, out); }
void loop_hook_pose_from_affine(const float* T16, float* pose6) { pose_from_affine(T16, pose6); }
void loop_hook_rzryrx(double x, double y, double z, double* R9) { rzryrx(x, y, z, R9); }
void loop_hook_between(const double* from6, const double* to6, double* B16, double* b6) { between(from6, to6, B16, b6); }
void loop_hook_factor(const float* correction, const float* pose_cur, const float* pose_pre, double* from6, double* to6, double* B16, double* b6) {
  loop_factor(correction, pose_cur, pose_pre, from6, to6, B16, b6);
}
// the deliberately wrong composition tWrong * correction (tests: it must NOT match the restatement)
void loop_hook_factor_swapped(const float* correction, const float* pose_cur, const float* pose_pre, double* from6, double* to6, double* B16, double* b6) {
  float tWrong[16], tCorrect[16], pc[6];
  affine_from_pose(pose_cur, tWrong);
  affine_mul(tWrong, correction, tCorrect);
  pose_from_affine(tCorrect, pc);
  for (int k = 0; k < 6; k++) { from6[k] = (double)pc[k]; to6[k] = (double)pose_pre[k]; }
  between(from6, to6, B16, b6);
}
void loop_hook_layout(long* o) {
  o[0] = sizeof(pcm_loam_loop_params); o[1] = offsetof(pcm_loam_loop_params, fitness_threshold); o[2] = offsetof(pcm_loam_loop_params, ndt_epsilon);
  o[3] = offsetof(pcm_loam_loop_params, reserved); o[4] = sizeof(pcm_loam_loop_result); o[5] = offsetof(pcm_loam_loop_result, fitness);
  o[6] = offsetof(pcm_loam_loop_result, correction); o[7] = offsetof(pcm_loam_loop_result, pose_from); o[8] = offsetof(pcm_loam_loop_result, between);
  o[9] = offsetof(pcm_loam_loop_result, between6); o[10] = offsetof(pcm_loam_loop_result, reserved);
}

}  // extern "C"

#ifdef LOAM_LOOP_HOOKS_MAIN
// a 64-bit LCG in [0, 1)
static unsigned long long g_s = 0x9e3779b97f4a7c15ull;
static double rnd() { g_s = g_s * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_s >> 11) / 9007199254740992.0; }

int main() {
  const double kPi = 3.14159265358979323846;
  int n = 0, nan_factors = 0;
  double acc = 0.0;
  for (int t = 0; t < 2000; t++) {
    float pose_cur[6], pose_pre[6], corr_pose[6], C[16];
    for (int k = 0; k < 3; k++) { pose_cur[k] = (float)((rnd() - 0.5) * 2.0 * kPi); pose_pre[k] = (float)((rnd() - 0.5) * 2.0 * kPi); corr_pose[k] = (float)((rnd() - 0.5) * 0.2); }
    for (int k = 3; k < 6; k++) { pose_cur[k] = (float)((rnd() - 0.5) * 200.0); pose_pre[k] = (float)((rnd() - 0.5) * 200.0); corr_pose[k] = (float)((rnd() - 0.5) * 2.0); }
    if (t % 4 == 1) pose_cur[1] = (float)((t % 8 == 1 ? 0.5 : -0.5) * kPi + (rnd() - 0.5) * 2e-3);   // pitch within 1e-3 of +-pi/2
    if (t % 4 == 2) for (int k = 0; k < 6; k++) corr_pose[k] = 0.f;                                   // the identity correction
    if (t % 4 == 3) { for (int k = 0; k < 6; k++) corr_pose[k] = 0.f; corr_pose[2] = (float)((rnd() - 0.5) * kPi); }   // pure yaw
    affine_from_pose(corr_pose, C);
    double from6[6], to6[6], B[16], b6[6];
    loop_factor(C, pose_cur, pose_pre, from6, to6, B, b6);
    bool finite = true;
    for (int k = 0; k < 6; k++) finite = finite && b6[k] == b6[k];
    if (!finite) { nan_factors++; continue; }
    for (int k = 0; k < 6; k++) acc += b6[k];
    for (int k = 0; k < 16; k++) acc += B[k];
    n++;
  }
  if (accept_status(1, 0.29, 0.3f) != kAccepted || accept_status(1, 0.31, 0.3f) != kRejectedFitness || accept_status(0, 0.0, 0.3f) != kRejectedNotConverged) return 1;
  if (!size_gate(300, 1000, 300, 1000) || size_gate(299, 1000, 300, 1000) || size_gate(300, 999, 300, 1000)) return 1;
  printf("loop factors: %d finite, %d with asin outside its domain, checksum %a\n", n, nan_factors, acc);
  return n > 0 ? 0 : 1;
}
#endif
