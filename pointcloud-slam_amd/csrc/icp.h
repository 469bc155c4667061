// icp.h -- the rules of point-to-point ICP (PCM_MODEL_ICP, include/pcm_amd.h) as plain C++ shared by the kernels of icp.hip and the
// g++ build of tests/test_icp.py (tests/icp_hooks.cpp), which checks them against the numpy restatement (tests/icp_ref.py).
//
// pcl::IterativeClosestPoint is not in the reference tree (jueying_slam/src/mapOptmization.cpp:768-779 calls it).  The rules below
// restate PCL 1.10's IterativeClosestPoint::computeTransformation and DefaultConvergenceCriteria::hasConverged from memory and are
// this library's definition.  The closed-form step is in the tree: PCL's TransformationEstimationSVD is
// Eigen's umeyama without scaling, E = fast_gicp/thirdparty/Eigen/Eigen/src/Geometry/Umeyama.h:118-158.
//
//   R1  the pose F is a double 4 x 4; a source point s goes through Ff = float(F) as m0*x + (m1*y + (m2*z + m3)), in float, no
//       contraction (k_fitness's order).  Nothing is written back to the cloud: every iteration transforms the ORIGINAL source by
//       the whole pose -- the one deliberate departure from PCL, which transforms the cloud and composes increments in float.
//   R2  the pair of c = Ff s is its exact nearest target point q; d2 = (ex*ex + ey*ey) + ez*ez in float; kept when
//       (double)d2 <= max_sq, max_sq = min(max_correspondence_distance^2, DBL_MAX) (inclusive); a non-finite c has no pair.
//   R3  fewer than 3 pairs: stop, not converged, F as it was.
//   R4  sums over the kept pairs in double: sum c, sum q, sum q c^T, sum d2; sigma = sum q c^T / N - qm cm^T (E:129 with the means
//       taken out of the raw moments), JacobiSVD (dev_linalg.h), S = diag(1, 1, +-1) with -1 when det(U) det(V) < 0 (E:137-140),
//       R = U S V^T (E:143), t = qm - R cm (E:157-158).  F <- [R t] F in double.
//   R5  convergence, in this order, mse = sum d2 / N of this iteration's pairs:
//         k >= max_iterations                                   -> converged (PCL counts the cap as convergence: kept)
//         0.5 (trace R - 1) >= rot_thr and |t|^2 <= transformation_epsilon
//                                                               -> converged (the epsilon meets the SQUARED translation: kept)
//         |mse - prev_mse| < mse_absolute                       -> converged
//         |mse - prev_mse| / prev_mse < euclidean_fitness_epsilon -> converged
//       else prev_mse = mse.  rot_thr = rotation_epsilon > 0 ? rotation_epsilon : 1 - transformation_epsilon.
// Every operation is one IEEE operation in the order written (-ffp-contract=off).
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "dev_linalg.h"

namespace pcm {
namespace icp {

// pcm_icp_info::stop_reason
constexpr int kStopNone = 0, kStopIterations = 1, kStopTransform = 2, kStopAbsMse = 3, kStopRelMse = 4, kStopNoCorrespondences = 5;
// values of a sum row: sum c (3), sum q (3), sum q c^T (9, row-major: q index first), sum d2, count
constexpr int kSums = 17;
constexpr int kChunk = 8;   // iterations queued between two waits of the host

struct Params {
  int32_t max_iterations;
  double max_sq;      // R2
  double transformation_epsilon, rot_thr, euclidean_fitness_epsilon, mse_absolute;
};

PCM_LA double max_sq_of(double max_correspondence_distance) {
  const double m2 = max_correspondence_distance * max_correspondence_distance;
  return m2 < DBL_MAX ? m2 : DBL_MAX;   // also turns a NaN into DBL_MAX; pcm_icp_set_params refuses one
}
PCM_LA double rot_thr_of(double rotation_epsilon, double transformation_epsilon) { return rotation_epsilon > 0.0 ? rotation_epsilon : 1.0 - transformation_epsilon; }

// R1: the float view of the pose, then one point through it
PCM_LA void pose_to_float(const double* F, float* m) {
  for (int a = 0; a < 12; a++) m[a] = (float)F[a];
}
PCM_LA void transform_point(const float* m, float x, float y, float z, float* c) {
  for (int a = 0; a < 3; a++) c[a] = m[a * 4 + 0] * x + (m[a * 4 + 1] * y + (m[a * 4 + 2] * z + m[a * 4 + 3]));
}
// R2
PCM_LA float sq_dist(const float* q, const float* c) {
  const float ex = q[0] - c[0], ey = q[1] - c[1], ez = q[2] - c[2];
  return (ex * ex + ey * ey) + ez * ez;
}
PCM_LA bool keep_pair(float d2, double max_sq) { return (double)d2 <= max_sq; }

// one pair's contribution to a sum row
PCM_LA void pair_terms(const float* c, const float* q, float d2, double* v) {
  const double cd[3] = {(double)c[0], (double)c[1], (double)c[2]}, qd[3] = {(double)q[0], (double)q[1], (double)q[2]};
  for (int a = 0; a < 3; a++) { v[a] = cd[a]; v[3 + a] = qd[a]; }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) v[6 + a * 3 + b] = qd[a] * cd[b];
  v[15] = (double)d2;
  v[16] = 1.0;
}

PCM_LA double det3(const double* M) {
  return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// R4: the rigid step of one sum row with N = s[16] >= 3: R row-major 3 x 3, t.  Returns S(2): 1 or -1.
PCM_LA int umeyama_step(const double* s, double* R, double* t) {
  const double N = s[16];
  double cm[3], qm[3], sigma[9], U[9], W[3], V[9];
  for (int a = 0; a < 3; a++) { cm[a] = s[a] / N; qm[a] = s[3 + a] / N; }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) sigma[a * 3 + b] = s[6 + a * 3 + b] / N - qm[a] * cm[b];
  jacobi_svd<3>(sigma, U, W, V);
  const double s2 = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) R[a * 3 + b] = (U[a * 3 + 0] * V[b * 3 + 0] + U[a * 3 + 1] * V[b * 3 + 1]) + (U[a * 3 + 2] * s2) * V[b * 3 + 2];
  for (int a = 0; a < 3; a++) t[a] = qm[a] - ((R[a * 3 + 0] * cm[0] + R[a * 3 + 1] * cm[1]) + R[a * 3 + 2] * cm[2]);
  return s2 < 0.0 ? -1 : 1;
}

// F <- [R t; 0 0 0 1] F, row-major 4 x 4 doubles (the last row of F is kept)
PCM_LA void compose(const double* R, const double* t, double* F) {
  double out[12];
  for (int a = 0; a < 3; a++)
    for (int j = 0; j < 4; j++) out[a * 4 + j] = ((R[a * 3 + 0] * F[j] + R[a * 3 + 1] * F[4 + j]) + R[a * 3 + 2] * F[8 + j]) + t[a] * F[12 + j];
  for (int a = 0; a < 12; a++) F[a] = out[a];
}

// R5: the stop reason after iteration k (1-based) whose step was (R, t) and whose pairs had the mean squared distance mse, or
// kStopNone; *prev_mse is updated when the loop goes on
PCM_LA int convergence(const Params& P, int k, const double* R, const double* t, double mse, double* prev_mse) {
  if (k >= P.max_iterations) return kStopIterations;
  const double cos_angle = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double t2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
  if (cos_angle >= P.rot_thr && t2 <= P.transformation_epsilon) return kStopTransform;
  const double diff = fabs(mse - *prev_mse);
  if (diff < P.mse_absolute) return kStopAbsMse;
  if (diff / *prev_mse < P.euclidean_fitness_epsilon) return kStopRelMse;
  *prev_mse = mse;
  return kStopNone;
}

// What the loop carries from one iteration to the next; the device keeps one in its state block.
struct Loop {
  double F[16];
  double prev_mse;
  double mse;            // of the last iteration that had >= 3 pairs
  double num_pairs;      // N of the last iteration that ran
  int32_t iterations;    // completed ones
  int32_t converged;
  int32_t stop;          // kStop*
  int32_t done;
};

PCM_LA void loop_begin(Loop* L, const float* guess) {
  for (int a = 0; a < 16; a++) L->F[a] = (double)guess[a];
  L->prev_mse = DBL_MAX;
  L->mse = 0.0;
  L->num_pairs = 0.0;
  L->iterations = 0; L->converged = 0; L->stop = kStopNone; L->done = 0;
}

// R3-R5 for the sum row of one iteration
PCM_LA void loop_step(const Params& P, const double* s, Loop* L) {
  L->num_pairs = s[16];
  if (s[16] < 3.0) { L->converged = 0; L->stop = kStopNoCorrespondences; L->done = 1; return; }
  double R[9], t[3];
  umeyama_step(s, R, t);
  compose(R, t, L->F);
  L->iterations += 1;
  L->mse = s[15] / s[16];
  const int stop = convergence(P, L->iterations, R, t, L->mse, &L->prev_mse);
  if (stop != kStopNone) { L->converged = 1; L->stop = stop; L->done = 1; }
}

// performSCLoopClosure's factor (mapOptmization.cpp:817-834): poseFrom = getTranslationAndEulerAngles(correction) promoted,
// poseTo = the identity; the algebra itself is loam_loop.h's (pose_from_affine, between)
constexpr float kScNoiseVariance = 0.5f;   // :822 robustNoiseScore
constexpr double kScCauchyK = 1.0;         // :827 Cauchy::Create(1)

}  // namespace icp
}  // namespace pcm
