// loam_step.h -- the per-point arithmetic and the serial LM step of jueying_slam's LOAM scan-to-map optimisation
// (LIO-SAM style edge / plane features), host + device.
//
// Reference: jueying_slam/src/mapOptmization.cpp (paths relative to src/ of the reference tree)
//   pose -> matrix               trans2Affine3f :487-490 (pcl::getTransformation), pointAssociateToMap :439-445
//   edge (corner) coefficient    cornerOptimization :1255-1347
//   plane (surf) coefficient     surfOptimization   :1349-1419
//   Jacobian row, LM step        LMOptimization     :1442-1558
//   localisation fitness         localization.cpp :689-693, :790-794, :1003-1022
// The kernels of loam.hip call these functions per lane (edge_coeff / plane_coeff / jacobian_row) and once per context
// (loam_step); tests/test_loam_step.py compiles this header with g++ and checks it against the numpy restatement
// (tests/loam_ref.py).  Every float operation below is one IEEE operation in the order written (-ffp-contract=off);
// the 6x6 solve and the eigen-decompositions use only +, -, *, / and sqrt in double, so host and device agree bit for bit
// on them.  pose_matrix is the exception: it rounds the double sin / cos of the device library (ocml) or of the host's libm
// to float, and the two are not guaranteed to agree in the last double bit, so a pose matrix can differ in rare cases.
// DESIGN.md section 9 lists what is pinned and which rules replace OpenCV / FLANN where the reference is not.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "plane_fit.h"

#if defined(__HIPCC__)
#define LOAM_HD __host__ __device__ inline
#else
#define LOAM_HD inline
#endif

namespace pcm {
namespace loam {

// ---- reduction layout: one partial row per 64-lane workgroup -------------------------------------------------------------
constexpr int kSumAtA = 0;        // 21: upper triangle of A^T A, row-major (0,0) (0,1) .. (0,5) (1,1) .. (5,5)
constexpr int kSumAtB = 21;       // 6
constexpr int kSumCorner = 27;    // selected corner rows
constexpr int kSumSurf = 28;      // selected surf rows
constexpr int kSumFitC = 29;      // sum of sqDis[0] over corner features with sqDis[0] <= 1
constexpr int kSumFitCN = 30;     //   their number
constexpr int kSumFitS = 31;
constexpr int kSumFitSN = 32;
constexpr int kSums = 33;
constexpr int kLanes = 64;        // features per workgroup of the correspondence pass (one wave)
constexpr int kMinRows = 50;      // LMOptimization: laserCloudSelNum < 50 -> no update  :1455-1458

// device state of one context between the launches of an optimisation (read back once at the end)
struct LoamState {
  float x[6];       // transformTobeMapped: roll, pitch, yaw, x, y, z
  float T[12];      // trans2Affine3f(x), rows 0..2 of the 4x4, row-major
  float trig[6];    // srx crx sry cry srz crz of LMOptimization :1445-1450
  double P[36];     // matP of iteration 0 (row-major)
  double eig[6];    // eigenvalues of A^T A at iteration 0, descending
  double fit[2];    // corner / surf fitness of the last pass
  int32_t iter;     // loop iterations run
  int32_t done;
  int32_t converged;
  int32_t degenerate;
  int32_t n_corner, n_surf;   // selected rows of the last pass
  int32_t pad[2];
};

struct StepParams {
  int32_t iter_num;
  int32_t pad;
  double rot_conv_deg;    // deltaR threshold [deg]
  double trans_conv_cm;   // deltaT threshold [cm]
  double degeneracy;      // eignThre
};

// ---- correctly rounded float division / square root (the device's default float division is not) -----------------------
LOAM_HD float divf(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}
LOAM_HD float sqrtf_rn(float v) { return sqrtf(v); }

// ---- pose -------------------------------------------------------------------------------------------------------------
// pcl::getTransformation(x, y, z, roll, pitch, yaw) in float: R = Rz(yaw) Ry(pitch) Rx(roll).  PCL is not in the reference tree:
// the expression order is PCL's common/impl/eigen.hpp as published (unpinned).  sin / cos: the double function rounded to float
// (std::sin(float) of the reference is not pinned either; a correctly rounded float value is what it approximates).
LOAM_HD float sinf_of(float a) { return (float)sin((double)a); }
LOAM_HD float cosf_of(float a) { return (float)cos((double)a); }

LOAM_HD void pose_matrix(const float (&x)[6], float (&T)[12], float (&trig)[6]) {
  const float A = cosf_of(x[2]), B = sinf_of(x[2]), C = cosf_of(x[1]), D = sinf_of(x[1]), E = cosf_of(x[0]), F = sinf_of(x[0]);
  const float DE = D * E, DF = D * F;
  T[0] = A * C; T[1] = A * DF - B * E; T[2] = B * F + A * DE; T[3] = x[3];
  T[4] = B * C; T[5] = A * E + B * DF; T[6] = B * DE - A * F; T[7] = x[4];
  T[8] = -D;    T[9] = C * F;          T[10] = C * E;         T[11] = x[5];
  // LMOptimization :1445-1450: srx = sin(x[1]), crx = cos(x[1]), sry = sin(x[2]), cry = cos(x[2]), srz = sin(x[0]), crz = cos(x[0])
  trig[0] = D; trig[1] = C; trig[2] = B; trig[3] = A; trig[4] = F; trig[5] = E;
}

// pointAssociateToMap :439-445
LOAM_HD void to_map(const float (&T)[12], float px, float py, float pz, float (&q)[3]) {
  for (int a = 0; a < 3; a++) q[a] = T[a * 4 + 0] * px + T[a * 4 + 1] * py + T[a * 4 + 2] * pz + T[a * 4 + 3];
}

// squared distance of the 5-NN search: (dx^2 + dy^2) + dz^2 in float (FLANN's L2 sums the dimensions in order)
LOAM_HD float dist2(float ax, float ay, float az, const float (&q)[3]) {
  const float dx = ax - q[0], dy = ay - q[1], dz = az - q[2];
  return dx * dx + dy * dy + dz * dz;
}

// ---- symmetric eigen-decomposition (cyclic Jacobi, double) ------------------------------------------------------------
// Replaces cv::eigen (not in the reference tree).  Rotations in the fixed order (0,1), (0,2), .., (N-2,N-1); an off-diagonal
// entry below 1e-18 (|a_pp| + |a_qq|) is set to zero instead of rotated; sweeps end when one rotates nothing (at most 64).
// Out: w descending (ties keep index order), E row k = eigenvector of w[k] (cv::eigen's layout).
template <int N>
LOAM_HD void sym_eigen(const double* Ain, double* w, double* E) {
  double a[N][N], v[N][N];
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) { a[i][j] = Ain[i * N + j]; v[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 64; sweep++) {
    bool rotated = false;
    for (int p = 0; p < N - 1; p++) {
      for (int q = p + 1; q < N; q++) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double app = a[p][p], aqq = a[q][q];
        if (fabs(apq) <= 1e-18 * (fabs(app) + fabs(aqq))) { a[p][q] = 0.0; a[q][p] = 0.0; continue; }
        const double theta = (aqq - app) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; k++) {
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; k++) {
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
        a[p][q] = 0.0; a[q][p] = 0.0;
        for (int k = 0; k < N; k++) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
        rotated = true;
      }
    }
    if (!rotated) break;
  }
  bool used[N];
  for (int i = 0; i < N; i++) used[i] = false;
  for (int k = 0; k < N; k++) {
    int best = -1;
    for (int i = 0; i < N; i++)
      if (!used[i] && (best < 0 || a[i][i] > a[best][best])) best = i;
    used[best] = true;
    w[k] = a[best][best];
    for (int j = 0; j < N; j++) E[k * N + j] = v[j][best];
  }
}

// ---- 6x6 solve (Householder QR, double) ---------------------------------------------------------------------------------
// Replaces cv::solve(matAtA, matAtB, matX, DECOMP_QR) (:1510).  A zero pivot gives a zero component.
LOAM_HD void solve6_qr(const double* Ain, const double* bin, double* x) {
  double A[6][6], b[6], v[6];
  for (int i = 0; i < 6; i++) { b[i] = bin[i]; for (int j = 0; j < 6; j++) A[i][j] = Ain[i * 6 + j]; }
  for (int k = 0; k < 6; k++) {
    double nrm2 = 0.0;
    for (int i = k; i < 6; i++) nrm2 += A[i][k] * A[i][k];
    const double nrm = sqrt(nrm2);
    if (nrm == 0.0) continue;
    const double alpha = A[k][k] > 0.0 ? -nrm : nrm;
    double vtv = 0.0;
    for (int i = k; i < 6; i++) { v[i] = i == k ? A[k][k] - alpha : A[i][k]; vtv += v[i] * v[i]; }
    if (vtv == 0.0) continue;
    for (int j = k; j < 6; j++) {
      double dot = 0.0;
      for (int i = k; i < 6; i++) dot += v[i] * A[i][j];
      const double f = (2.0 * dot) / vtv;
      for (int i = k; i < 6; i++) A[i][j] -= f * v[i];
    }
    double dot = 0.0;
    for (int i = k; i < 6; i++) dot += v[i] * b[i];
    const double f = (2.0 * dot) / vtv;
    for (int i = k; i < 6; i++) b[i] -= f * v[i];
  }
  for (int i = 5; i >= 0; i--) {
    double s = b[i];
    for (int j = i + 1; j < 6; j++) s -= A[i][j] * x[j];
    x[i] = A[i][i] != 0.0 ? s / A[i][i] : 0.0;
  }
}

// ---- per-point coefficients ---------------------------------------------------------------------------------------------
// A feature's coefficient: (coeff.x, coeff.y, coeff.z, coeff.intensity) of the reference; `selected` = the *Flag[i] it sets.
struct Coeff {
  float x, y, z, w;
  bool selected;
};

// cornerOptimization :1273-1343 on the 5 neighbours (ascending distance, rows of nx/ny/nz) of the map-frame point q.
// The caller has checked sqDis[4] < 1.  cv::eigen of the float covariance: sym_eigen<3> in double, rounded to float.
LOAM_HD Coeff edge_coeff(const float (&nx)[5], const float (&ny)[5], const float (&nz)[5], const float (&q)[3]) {
  Coeff r{0.f, 0.f, 0.f, 0.f, false};
  float cx = 0.f, cy = 0.f, cz = 0.f;
  for (int j = 0; j < 5; j++) { cx += nx[j]; cy += ny[j]; cz += nz[j]; }
  cx = divf(cx, 5.f); cy = divf(cy, 5.f); cz = divf(cz, 5.f);
  float a11 = 0.f, a12 = 0.f, a13 = 0.f, a22 = 0.f, a23 = 0.f, a33 = 0.f;
  for (int j = 0; j < 5; j++) {
    const float ax = nx[j] - cx, ay = ny[j] - cy, az = nz[j] - cz;
    a11 += ax * ax; a12 += ax * ay; a13 += ax * az;
    a22 += ay * ay; a23 += ay * az;
    a33 += az * az;
  }
  a11 = divf(a11, 5.f); a12 = divf(a12, 5.f); a13 = divf(a13, 5.f); a22 = divf(a22, 5.f); a23 = divf(a23, 5.f); a33 = divf(a33, 5.f);
  const double M[9] = {a11, a12, a13, a12, a22, a23, a13, a23, a33};
  double w[3], E[9];
  sym_eigen<3>(M, w, E);
  const float l0 = (float)w[0], l1 = (float)w[1];
  if (!(l0 > 3.f * l1)) return r;
  const float v0 = (float)E[0], v1 = (float)E[1], v2 = (float)E[2];
  const float x0 = q[0], y0 = q[1], z0 = q[2];
  // cx + 0.1 * v: evaluated in double, stored to float (:1311-1316)
  const float x1 = (float)((double)cx + 0.1 * (double)v0), y1 = (float)((double)cy + 0.1 * (double)v1), z1 = (float)((double)cz + 0.1 * (double)v2);
  const float x2 = (float)((double)cx - 0.1 * (double)v0), y2 = (float)((double)cy - 0.1 * (double)v1), z2 = (float)((double)cz - 0.1 * (double)v2);
  // the three components of (p0 - p1) x (p0 - p2), as the reference spells them
  const float u = (x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1);
  const float v = (x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1);
  const float t = (y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1);
  const float a012 = sqrtf_rn(u * u + v * v + t * t);
  const float l12 = sqrtf_rn((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2));
  const float la = divf(divf((y1 - y2) * u + (z1 - z2) * v, a012), l12);
  const float lb = divf(divf(-((x1 - x2) * u - (z1 - z2) * t), a012), l12);
  const float lc = divf(divf(-((x1 - x2) * v + (y1 - y2) * t), a012), l12);
  const float ld2 = divf(a012, l12);
  const float s = (float)(1.0 - 0.9 * (double)fabsf(ld2));
  r.x = s * la; r.y = s * lb; r.z = s * lc; r.w = s * ld2;
  r.selected = (double)s > 0.1;
  return r;
}

// surfOptimization :1376-1415: float 5x3 ColPivHouseholderQR solve of A x = -1 (plane_fit.h, the restatement esti_plane uses),
// normalised with a float 1 / |x|; the weight divides by the fourth root of |q|^2 of the MAP-frame point (a reference quirk kept).
LOAM_HD Coeff plane_coeff(const float (&nx)[5], const float (&ny)[5], const float (&nz)[5], const float (&q)[3]) {
  Coeff r{0.f, 0.f, 0.f, 0.f, false};
  float A[3][5], sol[3];
  for (int j = 0; j < 5; j++) { A[0][j] = nx[j]; A[1][j] = ny[j]; A[2][j] = nz[j]; }
  colpiv_qr_solve<float, 5>(A, sol);
  float pa = sol[0], pb = sol[1], pc = sol[2], pd = 1.f;
  const float ps = sqrtf_rn(pa * pa + pb * pb + pc * pc);
  pa = divf(pa, ps); pb = divf(pb, ps); pc = divf(pc, ps); pd = divf(pd, ps);
  for (int j = 0; j < 5; j++) {
    if ((double)fabsf(pa * nx[j] + pb * ny[j] + pc * nz[j] + pd) > 0.2) return r;
  }
  const float pd2 = pa * q[0] + pb * q[1] + pc * q[2] + pd;
  const float rn = sqrtf_rn(sqrtf_rn(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]));
  const float s = (float)(1.0 - 0.9 * (double)fabsf(pd2) / (double)rn);
  r.x = s * pa; r.y = s * pb; r.z = s * pc; r.w = s * pd2;
  r.selected = (double)s > 0.1;
  return r;
}

// One row of matA / matB (:1469-1504): the body-frame point and the coefficient in the reference's permuted frame
// (x, y, z -> y, z, x), columns arz, arx, ary, coeff.z, coeff.x, coeff.y (= original c.x, c.y, c.z), b = -intensity.
LOAM_HD void jacobian_row(const float (&trig)[6], float bx, float by, float bz, const Coeff& c, float (&row)[7]) {
  const float srx = trig[0], crx = trig[1], sry = trig[2], cry = trig[3], srz = trig[4], crz = trig[5];
  const float px = by, py = bz, pz = bx;       // pointOri in the permuted frame
  const float cx = c.y, cy = c.z, cz = c.x;    // coeff in the permuted frame
  const float arx = (crx * sry * srz * px + crx * crz * sry * py - srx * sry * pz) * cx
                  + (-srx * srz * px - crz * srx * py - crx * pz) * cy
                  + (crx * cry * srz * px + crx * cry * crz * py - cry * srx * pz) * cz;
  const float ary = ((cry * srx * srz - crz * sry) * px + (sry * srz + cry * crz * srx) * py + crx * cry * pz) * cx
                  + ((-cry * crz - srx * sry * srz) * px + (cry * srz - crz * srx * sry) * py - crx * sry * pz) * cz;
  const float arz = ((crz * srx * sry - cry * srz) * px + (-cry * crz - srx * sry * srz) * py) * cx
                  + (crx * crz * px - crx * srz * py) * cy
                  + ((sry * srz + cry * crz * srx) * px + (crz * sry - cry * srx * srz) * py) * cz;
  row[0] = arz; row[1] = arx; row[2] = ary;
  row[3] = cz; row[4] = cx; row[5] = cy;
  row[6] = -c.w;
}

// ---- the serial step after one pass (LMOptimization :1442-1558 + the loop of scan2MapOptimization :1572-1584) -----------
// sums: the fixed-order total of the pass's partial rows.  Fitness as localization.cpp:1003-1022 (taken at every pass: the
// value left is that of the last iteration run).
LOAM_HD void loam_step(LoamState& s, const double* sums, const StepParams& p) {
  s.n_corner = (int32_t)sums[kSumCorner];
  s.n_surf = (int32_t)sums[kSumSurf];
  s.fit[0] = sums[kSumFitCN] > 1.0 ? sums[kSumFitC] / sums[kSumFitCN] : DBL_MAX;
  s.fit[1] = sums[kSumFitSN] > 1.0 ? sums[kSumFitS] / sums[kSumFitSN] : DBL_MAX;
  const int iter_count = s.iter;
  s.iter = iter_count + 1;
  if (s.n_corner + s.n_surf >= kMinRows) {
    double AtA[36], AtB[6], x[6];
    int t = 0;
    for (int i = 0; i < 6; i++)
      for (int j = i; j < 6; j++) { AtA[i * 6 + j] = sums[kSumAtA + t]; AtA[j * 6 + i] = sums[kSumAtA + t]; t++; }
    for (int i = 0; i < 6; i++) AtB[i] = sums[kSumAtB + i];
    solve6_qr(AtA, AtB, x);
    if (iter_count == 0) {
      double E[36], E2[36];
      sym_eigen<6>(AtA, s.eig, E);
      for (int k = 0; k < 36; k++) E2[k] = E[k];
      s.degenerate = 0;
      for (int i = 5; i >= 0; i--) {
        if (s.eig[i] < p.degeneracy) {
          for (int j = 0; j < 6; j++) E2[i * 6 + j] = 0.0;
          s.degenerate = 1;
        } else {
          break;
        }
      }
      // matP = matV^-1 matV2; the rows of matV are orthonormal, so matV^-1 = matV^T
      for (int r = 0; r < 6; r++)
        for (int c = 0; c < 6; c++) {
          double acc = 0.0;
          for (int k = 0; k < 6; k++) acc += E[k * 6 + r] * E2[k * 6 + c];
          s.P[r * 6 + c] = acc;
        }
    }
    if (s.degenerate) {
      double y[6];
      for (int r = 0; r < 6; r++) {
        double acc = 0.0;
        for (int c = 0; c < 6; c++) acc += s.P[r * 6 + c] * x[c];
        y[r] = acc;
      }
      for (int r = 0; r < 6; r++) x[r] = y[r];
    }
    float xf[6];
    for (int k = 0; k < 6; k++) { xf[k] = (float)x[k]; s.x[k] += xf[k]; }
    // pcl::rad2deg(float) = alpha * 57.29578f; pow(float, 2) is the exact double square; sqrt in double, stored to float
    const float r0 = xf[0] * 57.29578f, r1 = xf[1] * 57.29578f, r2 = xf[2] * 57.29578f;
    const float t0 = xf[3] * 100.f, t1 = xf[4] * 100.f, t2 = xf[5] * 100.f;
    const float dR = (float)sqrt((double)r0 * (double)r0 + (double)r1 * (double)r1 + (double)r2 * (double)r2);
    const float dT = (float)sqrt((double)t0 * (double)t0 + (double)t1 * (double)t1 + (double)t2 * (double)t2);
    pose_matrix(s.x, s.T, s.trig);
    if ((double)dR < p.rot_conv_deg && (double)dT < p.trans_conv_cm) { s.converged = 1; s.done = 1; }
  }
  if (s.iter >= p.iter_num) s.done = 1;
}

LOAM_HD void init_state(LoamState& s, const float* x6) {
  for (int k = 0; k < 6; k++) s.x[k] = x6[k];
  pose_matrix(s.x, s.T, s.trig);
  for (int k = 0; k < 36; k++) s.P[k] = 0.0;
  for (int k = 0; k < 6; k++) s.eig[k] = 0.0;
  s.fit[0] = s.fit[1] = DBL_MAX;
  s.iter = 0; s.done = 0; s.converged = 0; s.degenerate = 0;
  s.n_corner = s.n_surf = 0;
  s.pad[0] = s.pad[1] = 0;
}

}  // namespace loam
}  // namespace pcm
