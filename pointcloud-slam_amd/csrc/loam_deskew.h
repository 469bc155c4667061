// loam_deskew.h -- motion compensation of a spinning-LiDAR scan in front of the LOAM features (jueying_slam's deskewInfo /
// deskewPoint), host + device.  DESIGN.md section 34.
//
// Reference (paths relative to jueying_slam/src of the reference tree):
//   gate                         deskewInfo        imageProjection.cpp:483-499, new_localization.cpp:1733-1749
//   rotation table               imuDeskewInfo     imageProjection.cpp:501-558, new_localization.cpp:1751-1805
//   translation table            odomDeskewInfo    imageProjection.cpp:560-642, new_localization.cpp:1807-1886
//   table look-up                findRotation / findPosition   imageProjection.cpp:644-702, new_localization.cpp:1888-1946
//   the point                    deskewPoint       new_localization.cpp:1948-1977 (the live form: pointTime = timeScanCur + relTime;
//                                                  imageProjection.cpp:704-733 passes the relative time alone and is the identity)
//   call site                    projectPointCloud imageProjection.cpp:777-782
//   Affine3f inverse / product   Eigen/src/Geometry/Transform.h:1236-1247, :1511-1512; Matrix3f inverse Eigen/src/LU/InverseImpl.h:125-176
// The kernels of loam_features.hip call deskew_find / deskew_point per owner point and deskew_start once per frame;
// tests/test_loam_deskew.py compiles this header with g++ and checks it against the numpy restatement (tests/loam_deskew_ref.py).
// Every float and double operation below is one IEEE operation in the order written (-ffp-contract=off); sin / cos are
// loam_step.h's (the double function rounded to float), which is the one place host and device may differ in a last bit.
#pragma once

#include <math.h>
#include <stdint.h>

#include "dev_linalg.h"
#include "loam_step.h"

namespace pcm {
namespace loam {

// the reference's arrays are imuFrequency (500) long and overflow beyond; a table here holds at most this many entries
constexpr int kDeskewMaxEntries = 1024;

// ---- table look-up -------------------------------------------------------------------------------------------------------
// A table is n = cur + 1 entries (cur = imuPointerCur / OdomPointerCur after the closing decrement), in arrival order: the
// times need not increase.
//
// imuPointerFront of findRotation :648-655 (OdomPointerFront of findPosition :678-685): the first j < cur with t < time[j], else cur.
LOAM_HD int deskew_front_linear(const double* time, int cur, double t) {
  int front = 0;
  while (front < cur) {
    if (t < time[front]) break;
    ++front;
  }
  return front;
}

// pmax[j] = max(time[0..j]) (a NaN time never raises it; before any number it is -inf).
inline void deskew_prefix_max(const double* time, int n, double* pmax) {
  double m = -INFINITY;
  for (int j = 0; j < n; j++) {
    if (time[j] > m) m = time[j];
    pmax[j] = m;
  }
}

// The same index by binary search over the prefix maximum.  Proof: let P(j) = (t < pmax[j]) and j* the first j with
// t < time[j*].  pmax[j*] >= time[j*] > t, so P(j*) holds.  For j < j* every time[i], i <= j, is <= t or NaN, so pmax[j] <= t
// and P(j) fails.  pmax never decreases, so P is false up to j* - 1 and true from j* on: the first j < cur with P(j) is the
// first j < cur with t < time[j], and when there is none both give cur.  A NaN t fails every comparison on both sides.
LOAM_HD int deskew_front_pmax(const double* pmax, int cur, double t) {
  int lo = 0, hi = cur;   // the answer is in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t < pmax[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The branch and the blend of findRotation :657-670 / findPosition :687-700 at `front`: double ratios, the double blend
// assigned to float.
LOAM_HD void deskew_blend(const double* time, const double* vx, const double* vy, const double* vz, int front, double t, float (&out)[3]) {
  if (t > time[front] || front == 0) {
    out[0] = (float)vx[front];
    out[1] = (float)vy[front];
    out[2] = (float)vz[front];
  } else {
    const int back = front - 1;
    const double ratioFront = (t - time[back]) / (time[front] - time[back]);
    const double ratioBack = (time[front] - t) / (time[front] - time[back]);
    out[0] = (float)(vx[front] * ratioFront + vx[back] * ratioBack);
    out[1] = (float)(vy[front] * ratioFront + vy[back] * ratioBack);
    out[2] = (float)(vz[front] * ratioFront + vz[back] * ratioBack);
  }
}

// One table as the device reads it: five rows of n doubles (prefix maximum, time, x, y, z).  n == 0: no table, the value is 0
// (odomDeskewInfo returns before it writes, :572-576, and the tables were zeroed after the last scan, :785-795).
struct DeskewTable {
  const double* rows;
  int32_t n;
  LOAM_HD const double* pmax() const { return rows; }
  LOAM_HD const double* time() const { return rows + n; }
  LOAM_HD const double* v(int a) const { return rows + (size_t)(2 + a) * n; }
};

LOAM_HD void deskew_find(const DeskewTable& tb, double t, float (&out)[3]) {
  if (tb.n <= 0) { out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; return; }
  const int front = deskew_front_pmax(tb.pmax(), tb.n - 1, t);
  deskew_blend(tb.time(), tb.v(0), tb.v(1), tb.v(2), front, t, out);
}

// findRotation / findPosition as written (the linear scan), on separate arrays: what the tests hold deskew_find against
inline void deskew_find_linear(const double* time, const double* vx, const double* vy, const double* vz, int n, double t, float (&out)[3]) {
  if (n <= 0) { out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; return; }
  deskew_blend(time, vx, vy, vz, deskew_front_linear(time, n - 1, t), t, out);
}

// ---- the transform -------------------------------------------------------------------------------------------------------
// pcl::getTransformation(posX, posY, posZ, rotX, rotY, rotZ) :1963 / :1967, rows 0..2 of the 4x4
LOAM_HD void deskew_pose(const float (&rot)[3], const float (&pos)[3], float (&T)[12]) {
  const float x[6] = {rot[0], rot[1], rot[2], pos[0], pos[1], pos[2]};
  float trig[6];
  pose_matrix(x, T, trig);
}

// Affine3f::inverse() with its default hint Affine (:1963): the linear part through Matrix3f::inverse(), then
// translation = (-linear) * t, which rounds like -(linear * t)
LOAM_HD void deskew_inverse(const float (&T)[12], float (&I)[12]) {
  const float m[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
  float inv[9];
  inv3<float>(m, inv);
  for (int r = 0; r < 3; r++) {
    I[r * 4 + 0] = inv[r * 3 + 0]; I[r * 4 + 1] = inv[r * 3 + 1]; I[r * 4 + 2] = inv[r * 3 + 2];
    I[r * 4 + 3] = -((inv[r * 3 + 0] * T[3] + inv[r * 3 + 1] * T[7]) + inv[r * 3 + 2] * T[11]);
  }
}

// transStartInverse of the first point that reaches deskewPoint (firstPointFlag, :1961-1965)
LOAM_HD void deskew_start(const float (&rot)[3], const float (&pos)[3], float (&start_inv)[12]) {
  float T[12];
  deskew_pose(rot, pos, T);
  deskew_inverse(T, start_inv);
}

// transBt = transStartInverse * transFinal (:1968; Transform.h:1511-1512: linear = L1 L2, translation = L1 t2 + t1, coefficient
// sums left to right) and the point (:1971-1973)
LOAM_HD void deskew_point(const float (&start_inv)[12], const float (&rot)[3], const float (&pos)[3], float px, float py, float pz, float (&q)[3]) {
  float F[12], B[12];
  deskew_pose(rot, pos, F);
  for (int r = 0; r < 3; r++) {
    const float a = start_inv[r * 4 + 0], b = start_inv[r * 4 + 1], c = start_inv[r * 4 + 2];
    for (int k = 0; k < 3; k++) B[r * 4 + k] = (a * F[k] + b * F[4 + k]) + c * F[8 + k];
    B[r * 4 + 3] = ((a * F[3] + b * F[7]) + c * F[11]) + start_inv[r * 4 + 3];
  }
  for (int r = 0; r < 3; r++) q[r] = B[r * 4 + 0] * px + B[r * 4 + 1] * py + B[r * 4 + 2] * pz + B[r * 4 + 3];
}

// ---- the table builder (host) --------------------------------------------------------------------------------------------
struct DeskewImu { double t, gyro[3]; };    // a sensor_msgs::Imu after imuConverter: stamp, angular_velocity
struct DeskewOdom { double t, xyz[3]; };    // a nav_msgs::Odometry: stamp, pose.pose.position

enum DeskewBuild { kDeskewReady = 0, kDeskewWaiting = 1, kDeskewTooMany = 2 };

struct DeskewTables {
  int32_t imu_skipped, odom_skipped;   // the leading pops (:505-511, :564-570): what the caller pops from its own queues
  int32_t n_imu, n_odom;               // table entries (imuPointerCur + 1, OdomPointerCur + 1); 0: no table
  int32_t imu_available;               // cloudInfo.imuAvailable
  int32_t odom_available;              // cloudInfo.odomAvailable
  int32_t odom_deskew;                 // odomDeskewFlag
  int32_t start_odom;                  // index of startOdomMsg in the caller's queue as given (:580-588), -1 without one
};

// deskewInfo with both of its callees.  time_scan_next = +inf is new_localization.cpp's form: no `back < timeScanNext` gate
// (:1738) and no `> timeScanNext + 0.01` break.  The tables hold kDeskewMaxEntries entries each; imu_tab / odom_tab are
// four rows of `cap` doubles (time, x, y, z).  kDeskewWaiting: the gate failed, nothing is popped and nothing written.
inline DeskewBuild deskew_tables(double time_scan_cur, double time_scan_next, const DeskewImu* imu, int n_imu, const DeskewOdom* odom, int n_odom,
                                 double* imu_tab, double* odom_tab, int cap, DeskewTables* out) {
  DeskewTables r = {0, 0, 0, 0, 0, 0, 0, -1};
  *out = r;
  const bool open_end = isinf(time_scan_next) && time_scan_next > 0.0;
  if (n_imu <= 0 || imu[0].t > time_scan_cur || (!open_end && imu[n_imu - 1].t < time_scan_next)) return kDeskewWaiting;
  double *it = imu_tab, *ix = imu_tab + cap, *iy = imu_tab + 2 * (size_t)cap, *iz = imu_tab + 3 * (size_t)cap;
  double *ot = odom_tab, *ox = odom_tab + cap, *oy = odom_tab + 2 * (size_t)cap, *oz = odom_tab + 3 * (size_t)cap;
  // imuDeskewInfo
  int s = 0;
  while (s < n_imu && imu[s].t < time_scan_cur - 0.01) s++;
  r.imu_skipped = s;
  int cur = 0;
  for (int i = s; i < n_imu; i++) {
    const double t = imu[i].t;
    if (t > time_scan_next + 0.01) break;
    if (cur >= cap) return kDeskewTooMany;
    if (cur == 0) {
      ix[0] = 0; iy[0] = 0; iz[0] = 0; it[0] = t;
      ++cur;
      continue;
    }
    const double timeDiff = t - it[cur - 1];
    ix[cur] = ix[cur - 1] + imu[i].gyro[0] * timeDiff;
    iy[cur] = iy[cur - 1] + imu[i].gyro[1] * timeDiff;
    iz[cur] = iz[cur - 1] + imu[i].gyro[2] * timeDiff;
    it[cur] = t;
    ++cur;
  }
  r.n_imu = cur;              // the closing --imuPointerCur leaves cur - 1: the entries are 0 .. cur - 1
  r.imu_available = cur - 1 > 0 ? 1 : 0;
  // odomDeskewInfo
  s = 0;
  while (s < n_odom && odom[s].t < time_scan_cur - 0.01) s++;
  r.odom_skipped = s;
  if (s < n_odom && !(odom[s].t > time_scan_cur)) {
    for (int i = s; i < n_odom; i++) {
      r.start_odom = i;
      if (odom[i].t < time_scan_cur) continue;
      break;
    }
    r.odom_available = 1;
    cur = 0;
    double x0 = 0, y0 = 0, z0 = 0;
    for (int i = s; i < n_odom; i++) {
      const double t = odom[i].t;
      if (t > time_scan_next + 0.01) break;
      if (cur >= cap) return kDeskewTooMany;
      if (cur == 0) {
        x0 = odom[i].xyz[0]; y0 = odom[i].xyz[1]; z0 = odom[i].xyz[2];
        ox[0] = 0; oy[0] = 0; oz[0] = 0; ot[0] = t;
        ++cur;
        continue;
      }
      ox[cur] = odom[i].xyz[0] - x0;
      oy[cur] = odom[i].xyz[1] - y0;
      oz[cur] = odom[i].xyz[2] - z0;
      ot[cur] = t;
      ++cur;
    }
    r.n_odom = cur;
    r.odom_deskew = cur - 1 > 0 ? 1 : 0;
  }
  *out = r;
  return kDeskewReady;
}

}  // namespace loam
}  // namespace pcm
