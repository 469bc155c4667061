// loam_sc.h -- Scan Context arithmetic of jueying_slam (src/Scancontext.cpp, include/Scancontext.h) and the ring-key metric of
// its nanoflann search (include/nanoflann.hpp:274-298), as plain C++ that the device kernels (loam_sc.hip) and the host share.
// tests/test_loam_sc.py compiles this header with g++ (tests/loam_sc_hooks.cpp) and checks it bit for bit against the numpy
// restatement (tests/loam_sc_ref.py).  Every operation below is one IEEE operation in the order written (-ffp-contract=off).
//
// A descriptor is num_ring x num_sector, column-major (ring fastest: the layout of the reference's Eigen::MatrixXd), stored as
// float: every entry is a float z (or 0), all arithmetic on it is double.
//
// Pinned where the reference tree cannot pin it:
//   * the means and norms of the keys, the dot products of distDirectSC and the norm of fastAlignUsingVkey are double sums in
//     index order (Eigen's vectorised reductions have no pinned order);
//   * a NaN angle (x = y = 0) is sector 1 (the reference casts NaN to int: INT_MIN on x86-64, clamped to 1);
//   * the ring-key candidates come in ascending (d2, index); the shift set is its sorted set of distinct values.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "loam_step.h"     // LOAM_HD
#include "loam_submap.h"   // KeyPose

namespace pcm {
namespace loam {

constexpr int kScMaxRing = 64, kScMaxSector = 360, kScMaxCandidates = 64;
constexpr float kScNoPoint = -1000.0f;   // makeScancontext's NO_POINT

struct ScShape {
  int num_ring, num_sector;
  double lidar_height, max_radius;
};

LOAM_HD bool sc_finite(float v) { return v == v && v <= 3.402823466e38f && v >= -3.402823466e38f; }

// xy2theta (Scancontext.cpp:23-36): float quotient, double atan, double degrees, rounded to float once
LOAM_HD float sc_theta(float x, float y) {
  const double k = 180.0 / M_PI;
  if ((x >= 0) & (y >= 0)) return (float)(k * atan((double)(y / x)));
  if ((x < 0) & (y >= 0)) return (float)(180.0 - k * atan((double)(y / (-x))));
  if ((x < 0) & (y < 0)) return (float)(180.0 + k * atan((double)(y / x)));
  return (float)(360.0 - k * atan((double)((-y) / x)));
}

// one point of makeScancontext (:166-179): false when the point is skipped, else its bin (0-based) and z + LIDAR_HEIGHT
LOAM_HD bool sc_point_bin(float x, float y, float z, const ScShape& sh, int* ring, int* sector, float* zp) {
  if (!sc_finite(x) || !sc_finite(y) || !sc_finite(z)) return false;
  *zp = (float)((double)z + sh.lidar_height);
  const float range = sqrtf(x * x + y * y);
  const float angle = sc_theta(x, y);
  if ((double)range > sh.max_radius) return false;
  const double fr = ceil(((double)range / sh.max_radius) * (double)sh.num_ring);
  int r = (int)fr;
  if (r > sh.num_ring) r = sh.num_ring;
  if (r < 1) r = 1;
  int s = 1;
  if (angle == angle) {
    const double fs = ceil(((double)angle / 360.0) * (double)sh.num_sector);
    s = (int)fs;
    if (s > sh.num_sector) s = sh.num_sector;
    if (s < 1) s = 1;
  }
  *ring = r - 1;
  *sector = s - 1;
  return true;
}

// a bin's maximum (started from NO_POINT, strict <) to its descriptor entry: NO_POINT -> 0, and one zero for both signs
LOAM_HD float sc_bin_value(float mx) { return (mx == kScNoPoint || mx == 0.0f) ? 0.0f : mx; }

// makeRingkeyFromScancontext + eig2stdvec: mean of row r, rounded to float
LOAM_HD float sc_ring_key(const float* desc, int R, int S, int r) {
  double sum = 0.0;
  for (int s = 0; s < S; s++) sum += (double)desc[(size_t)s * R + r];
  return (float)(sum / (double)S);
}

// makeSectorkeyFromScancontext: mean of column s; *norm = the column's Euclidean norm
LOAM_HD double sc_sector_key(const float* desc, int R, int s, double* norm) {
  double sum = 0.0, sq = 0.0;
  const float* col = desc + (size_t)s * R;
  for (int r = 0; r < R; r++) { const double v = (double)col[r]; sum += v; sq += v * v; }
  *norm = sqrt(sq);
  return sum / (double)R;
}

// nanoflann L2_Adaptor<float>::evalMetric for an accepted point
LOAM_HD float sc_ring_d2(const float* a, const float* b, int R) {
  float result = 0.0f;
  int d = 0;
  for (; d + 3 < R; d += 4) {
    const float d0 = a[d] - b[d], d1 = a[d + 1] - b[d + 1], d2 = a[d + 2] - b[d + 2], d3 = a[d + 3] - b[d + 3];
    result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
  }
  for (; d < R; d++) { const float d0 = a[d] - b[d]; result += d0 * d0; }
  return result;
}

// circshift(_mat, shift) column j is column (j - shift) mod S of _mat
LOAM_HD int sc_src_col(int j, int shift, int S) { int c = j - shift; if (c < 0) c += S; return c; }

// fastAlignUsingVkey's norm for one shift (:99-103)
LOAM_HD double sc_shift_norm(const double* v1, const double* v2, int S, int shift) {
  double sq = 0.0;
  for (int j = 0; j < S; j++) { const double d = v1[j] - v2[sc_src_col(j, shift, S)]; sq += d * d; }
  return sqrt(sq);
}

// SEARCH_RADIUS (:123)
LOAM_HD int sc_search_radius(double search_ratio, int S) { return (int)round(0.5 * search_ratio * (double)S); }

// whether `shift` is in shift_idx_search_space (:124-130)
LOAM_HD bool sc_in_window(int shift, int argmin, int radius, int S) {
  int d = shift - argmin;
  if (d < 0) d += S;
  return d <= radius || S - d <= radius;
}

// one column pair of distDirectSC (:75-84): false when the pair is not counted
LOAM_HD bool sc_col_sim(const float* c1, const float* c2, int R, double n1, double n2, double* sim) {
  if ((n1 == 0) | (n2 == 0)) return false;
  double dot = 0.0;
  for (int r = 0; r < R; r++) dot += (double)c1[r] * (double)c2[r];
  *sim = dot / (n1 * n2);
  return true;
}

// detectLoopClosureID's yaw (:339): nn_align * PC_UNIT_SECTORANGLE rounded to deg2rad's float argument
LOAM_HD float sc_yaw(int nn_align, int S) {
  const float deg = (float)((double)nn_align * (360.0 / (double)S));
  return (float)((double)deg * M_PI / 180.0);
}

// ---- host only: the whole of distanceBtnScanContext / detectLoopClosureDistance, composed of the pieces above ----
struct ScView {   // one stored descriptor
  const float* desc;
  const double* skey;
  const double* norm;
};

inline int sc_fast_align(const double* v1, const double* v2, int S) {
  int arg = 0;
  double best = 10000000;
  for (int sh = 0; sh < S; sh++) {
    const double n = sc_shift_norm(v1, v2, S, sh);
    if (n < best) { arg = sh; best = n; }
  }
  return arg;
}

inline double sc_dist_direct(const ScView& a, const ScView& b, int R, int S, int shift) {
  int eff = 0;
  double sum = 0.0;
  for (int j = 0; j < S; j++) {
    const int c = sc_src_col(j, shift, S);
    double sim;
    if (!sc_col_sim(a.desc + (size_t)j * R, b.desc + (size_t)c * R, R, a.norm[j], b.norm[c], &sim)) continue;
    sum = sum + sim;
    eff = eff + 1;
  }
  return 1.0 - sum / (double)eff;
}

inline double sc_distance(const ScView& a, const ScView& b, int R, int S, double search_ratio, int* shift_out) {
  const int arg = sc_fast_align(a.skey, b.skey, S);
  const int radius = sc_search_radius(search_ratio, S);
  int best_shift = 0;
  double best = 10000000;
  for (int sh = 0; sh < S; sh++) {
    if (!sc_in_window(sh, arg, radius, S)) continue;
    const double d = sc_dist_direct(a, b, R, S, sh);
    if (d < best) { best_shift = sh; best = d; }
  }
  *shift_out = best_shift;
  return best;
}

// detectLoopClosureDistance (mapOptmization.cpp:843-880) without the loopIndexContainer test: the key poses with z = 1.1f,
// neighbours of the last one with d2 < r2 in ascending (d2, index) (loam_submap.h's radius rule), the first that is older
// than time_diff and more than 10 key frames back.  Returns the key frame, or -1.
inline int select_loop_distance(const KeyPose* kp, int K, float radius, double time_diff, double time_cur) {
  if (K <= 0) return -1;
  struct Near { float d2; int32_t id; };
  std::vector<Near> near;
  const float r2 = radius * radius;
  const int cur = K - 1;
  for (int i = 0; i < K; i++) {
    const float dx = kp[i].x - kp[cur].x, dy = kp[i].y - kp[cur].y, dz = 1.1f - 1.1f;
    const float d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < r2) near.push_back({d2, (int32_t)i});
  }
  std::sort(near.begin(), near.end(), [](const Near& a, const Near& b) { return a.d2 != b.d2 ? a.d2 < b.d2 : a.id < b.id; });
  for (const Near& n : near)
    if (fabs(kp[n.id].time - time_cur) > time_diff && cur - n.id > 10) return n.id;
  return -1;
}

}  // namespace loam
}  // namespace pcm
