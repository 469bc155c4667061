// loam_loop.h -- the pose algebra between an accepted loop verification and the pose graph: jueying_slam's performLoopClosure
// (mapOptmization.cpp:645-725) after ndt->align, as plain C++ shared by the host side of pcm_loam_loop_verify (loam_loop.hip) and
// the g++ build of tests/test_loam_loop.py (tests/loam_loop_hooks.cpp), which checks it against the numpy restatement
// (tests/loam_loop_ref.py).  Float where the reference is Eigen::Affine3f, double where it is GTSAM.  Every operation below is
// one IEEE operation in the order written (-ffp-contract=off), so the restatement reproduces it bit for bit.
//
// Pinned where the reference tree cannot pin it (PCL, Eigen and GTSAM are outside it):
//   * sin / cos / atan2 / asin of a float are the double functions rounded to float (loam_step.h's rule for pose_matrix);
//   * the Affine3f product sums a row's three products left to right and adds the translation last;
//   * Rot3::RzRyRx and Pose3::between are restated from their definitions (R = Rz(yaw) Ry(pitch) Rx(roll);
//     between = poseFrom^-1 * poseTo = (Rf^T Rt, Rf^T (tt - tf))), sums left to right;
//   * the (roll, pitch, yaw) of `between` are atan2(R21, R22), atan2(-R20, sqrt(R21^2 + R22^2)), atan2(R10, R00).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LOOP_HD __host__ __device__ inline
#else
#define LOOP_HD inline
#endif

namespace pcm {
namespace loam {
namespace loop {

// status of a verification (pcm_loam_loop_result::status)
constexpr int kAccepted = 0, kRejectedSize = 1, kRejectedNotConverged = 2, kRejectedFitness = 3, kNoLoop = 4;

// :652 the size gates, then :693 `hasConverged() == false || getFitnessScore() > historyKeyframeFitnessScore` (double > float)
LOOP_HD bool size_gate(int64_t n_cur, int64_t n_prev, int64_t min_cur, int64_t min_prev) { return !(n_cur < min_cur || n_prev < min_prev); }
LOOP_HD int accept_status(int converged, double fitness, float threshold) {
  if (!converged) return kRejectedNotConverged;
  if (fitness > (double)threshold) return kRejectedFitness;
  return kAccepted;
}

// sin and cos stay two libm calls: a compiler that sees both of one angle merges them into sincos(), whose last bits are not
// glibc's sin() and cos() bits in every case (measured: 1 ulp apart in about one angle of a hundred).  The volatile copy hides
// that the two arguments are equal.
LOOP_HD double sin_d(double a) { volatile double v = a; return sin(v); }
LOOP_HD double cos_d(double a) { volatile double v = a; return cos(v); }
LOOP_HD float sin_f(float a) { return (float)sin_d((double)a); }
LOOP_HD float cos_f(float a) { return (float)cos_d((double)a); }
LOOP_HD float atan2_f(float y, float x) { return (float)atan2((double)y, (double)x); }
LOOP_HD float asin_f(float a) { return (float)asin((double)a); }

// pclPointToAffine3f = pcl::getTransformation(x, y, z, roll, pitch, yaw): row-major 4 x 4 from (roll, pitch, yaw, x, y, z)
LOOP_HD void affine_from_pose(const float* pose6, float* T) {
  const float A = cos_f(pose6[2]), B = sin_f(pose6[2]), C = cos_f(pose6[1]), D = sin_f(pose6[1]), E = cos_f(pose6[0]), F = sin_f(pose6[0]);
  const float DE = D * E, DF = D * F;
  T[0] = A * C; T[1] = A * DF - B * E; T[2] = B * F + A * DE; T[3] = pose6[3];
  T[4] = B * C; T[5] = A * E + B * DF; T[6] = B * DE - A * F; T[7] = pose6[4];
  T[8] = -D;    T[9] = C * F;          T[10] = C * E;         T[11] = pose6[5];
  T[12] = 0.f;  T[13] = 0.f;           T[14] = 0.f;           T[15] = 1.f;
}

// Eigen::Affine3f a * b (:713 tCorrect = correctionLidarFrame * tWrong): the last row of both is (0, 0, 0, 1)
LOOP_HD void affine_mul(const float* a, const float* b, float* out) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) out[4 * i + j] = a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j] + a[4 * i + 2] * b[8 + j];
    out[4 * i + 3] = a[4 * i] * b[3] + a[4 * i + 1] * b[7] + a[4 * i + 2] * b[11] + a[4 * i + 3];
  }
  out[12] = 0.f; out[13] = 0.f; out[14] = 0.f; out[15] = 1.f;
}

// pcl::getTranslationAndEulerAngles: (roll, pitch, yaw, x, y, z).  asin of a value a rounding step beyond +-1 is NaN, as in PCL.
LOOP_HD void pose_from_affine(const float* T, float* pose6) {
  pose6[3] = T[3]; pose6[4] = T[7]; pose6[5] = T[11];
  pose6[0] = atan2_f(T[9], T[10]);
  pose6[1] = asin_f(-T[8]);
  pose6[2] = atan2_f(T[4], T[0]);
}

// gtsam::Rot3::RzRyRx(x = roll, y = pitch, z = yaw): row-major 3 x 3
LOOP_HD void rzryrx(double x, double y, double z, double* R) {
  const double cx = cos_d(x), sx = sin_d(x), cy = cos_d(y), sy = sin_d(y), cz = cos_d(z), sz = sin_d(z);
  const double ss_ = sx * sy, cs_ = cx * sy, sc_ = sx * cy, cc_ = cx * cy;
  const double c_s = cx * sz, s_s = sx * sz, _cs = cy * sz, _cc = cy * cz;
  const double s_c = sx * cz, c_c = cx * cz, ssc = ss_ * cz, csc = cs_ * cz, sss = ss_ * sz, css = cs_ * sz;
  R[0] = _cc; R[1] = -c_s + ssc; R[2] = s_s + csc;
  R[3] = _cs; R[4] = c_c + sss;  R[5] = -s_c + css;
  R[6] = -sy; R[7] = sc_;        R[8] = cc_;
}

// poseFrom.between(poseTo) for poses given as (roll, pitch, yaw, x, y, z) doubles: row-major 4 x 4 and its six numbers
LOOP_HD void between(const double* from6, const double* to6, double* B16, double* b6) {
  double Rf[9], Rt[9];
  rzryrx(from6[0], from6[1], from6[2], Rf);
  rzryrx(to6[0], to6[1], to6[2], Rt);
  const double d[3] = {to6[3] - from6[3], to6[4] - from6[4], to6[5] - from6[5]};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) B16[4 * i + j] = Rf[i] * Rt[j] + Rf[3 + i] * Rt[3 + j] + Rf[6 + i] * Rt[6 + j];   // Rf^T Rt
    B16[4 * i + 3] = Rf[i] * d[0] + Rf[3 + i] * d[1] + Rf[6 + i] * d[2];
  }
  B16[12] = 0.0; B16[13] = 0.0; B16[14] = 0.0; B16[15] = 1.0;
  b6[0] = atan2(B16[9], B16[10]);
  b6[1] = atan2(-B16[8], sqrt(B16[9] * B16[9] + B16[10] * B16[10]));
  b6[2] = atan2(B16[4], B16[0]);
  b6[3] = B16[3]; b6[4] = B16[7]; b6[5] = B16[11];
}

// :706-725 for one accepted pair.  correction: ndt->getFinalTransformation() row-major; pose_cur / pose_pre: the stored key poses.
// out: tCorrect's six numbers promoted (poseFrom), poseTo, between.
LOOP_HD void loop_factor(const float* correction, const float* pose_cur, const float* pose_pre, double* from6, double* to6, double* B16, double* b6) {
  float tWrong[16], tCorrect[16], pc[6];
  affine_from_pose(pose_cur, tWrong);
  affine_mul(correction, tWrong, tCorrect);
  pose_from_affine(tCorrect, pc);
  for (int k = 0; k < 6; k++) { from6[k] = (double)pc[k]; to6[k] = (double)pose_pre[k]; }   // Rot3::RzRyRx(roll, pitch, yaw), Point3(x, y, z): float -> double
  between(from6, to6, B16, b6);
}

// performSCLoopClosure :817-834 for one accepted pair.  correction: icp.getFinalTransformation() row-major.  out: its six numbers
// promoted (poseFrom, :817-818), poseTo = the identity (:819: Rot3::RzRyRx(0, 0, 0), Point3(0, 0, 0)), between (:834).
LOOP_HD void sc_loop_factor(const float* correction, double* from6, double* to6, double* B16, double* b6) {
  float pc[6];
  pose_from_affine(correction, pc);
  for (int k = 0; k < 6; k++) { from6[k] = (double)pc[k]; to6[k] = 0.0; }
  between(from6, to6, B16, b6);
}

}  // namespace loop
}  // namespace loam
}  // namespace pcm
