// octo_map.h -- arithmetic of octomap_server's 3D occupancy map (src/tool/octomap_server/src/OctomapServer.cpp: insertCloudCallback,
// insertScan, publishAll, handlePreNodeTraversal, update2DMap, isSpeckleNode) and of map_saver's bytes as plain C++ that the device
// kernels (octo_map.hip) and the host share.  tests/test_octo_map.py compiles this header with g++ (tests/octo_map_hooks.cpp) and
// checks it against the Python restatement (tests/octo_map_ref.py).  Every operation below is one IEEE operation in the order
// written (-ffp-contract=off).
//
// The octomap library under OctomapServer.cpp (OcTree, computeRayKeys, updateNode) is not in the reference tree.  Its rules are
// restated here and are this library's own:
//   * key = (int)floor((double)coord / res) + 32768, valid iff 0 <= key < 65536 on every axis; centre = (key - 32768 + 0.5) * res;
//   * points are floats; norm = (float)sqrt((double)((x * x + y * y) + z * z)); truncation = o + (p - o) / norm * max_range in float;
//   * the ray walk is Amanatides and Woo in double on float origin and direction, with octomap's tie rule, stop rules and a hard
//     step bound |dkx| + |dky| + |dkz| + 3 (a ray that reaches it is rejected);
//   * a ray that is rejected marks nothing: octo_ray walks twice, first without the callback;
//   * cells live at the finest level only (pruning merges equal children and changes no output built here);
//   * the projection's geometry is computed in double throughout (octomap's point3d is float);
//   * isSpeckleNode is applied at the finest level (the reference's depth test `== m_treeDepth + 1` never holds, so its filter is
//     dead code); a neighbour outside the key range counts as absent.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define OCTO_HD __host__ __device__ inline
#else
#define OCTO_HD inline
#endif

namespace pcm {
namespace octo {

constexpr int kKeyOrigin = 32768;   // tree_max_val of a 16-level tree
constexpr int kKeyEnd = 65536;
enum { kRayOk = 0, kRayRejected = 1, kRayBound = 2 };
// what insertScan does with a point
enum { kSkipMinRange = 0, kEndNone = 1, kEndOccupied = 2, kEndFree = 3 };

// the rules of one map as the kernels read them
struct OctoRules {
  double res, max_range, min_range, occ_min_z, occ_max_z;
  float hit, miss, clamp_min, clamp_max;   // log-odds
  float lo[3], hi[3];                      // pointcloud_min / max as PassThrough limits (floats)
};

OCTO_HD bool octo_finite(float v) { return v == v && v <= 3.402823466e38f && v >= -3.402823466e38f; }

// a double limit as the float PassThrough::setFilterLimits takes: rounded once, beyond FLT_MAX an infinity
OCTO_HD float octo_limit(double v) {
  if (v > 3.4028234663852886e38) return INFINITY;
  if (v < -3.4028234663852886e38) return -INFINITY;
  return (float)v;
}

// (float)log(p / (1 - p)) (host: libm's log in double)
inline float octo_logodds(double p) { return (float)log(p / (1 - p)); }

OCTO_HD bool octo_key_d(double c, double res, int* k) {
  const double f = floor(c / res);
  if (!(f >= -32768.0 && f < 32768.0)) return false;   // also a NaN
  *k = (int)f + kKeyOrigin;
  return true;
}
OCTO_HD bool octo_key(float c, double res, int* k) { return octo_key_d((double)c, res, k); }
OCTO_HD bool octo_key3(const float p[3], double res, int k[3]) {
  const bool a = octo_key(p[0], res, &k[0]), b = octo_key(p[1], res, &k[1]), c = octo_key(p[2], res, &k[2]);
  return a && b && c;
}
OCTO_HD double octo_coord(int k, double res) { return ((double)(k - kKeyOrigin) + 0.5) * res; }
OCTO_HD uint64_t octo_pack(int kx, int ky, int kz) { return ((uint64_t)kx << 32) | ((uint64_t)ky << 16) | (uint64_t)kz; }
OCTO_HD void octo_unpack(uint64_t p, int k[3]) { k[0] = (int)(p >> 32) & 0xffff; k[1] = (int)(p >> 16) & 0xffff; k[2] = (int)p & 0xffff; }

OCTO_HD float octo_norm(float dx, float dy, float dz) {
  const float s = (dx * dx + dy * dy) + dz * dz;
  return (float)sqrt((double)s);
}

// sensor_to_world (row-major 4x4, rows 0..2 used): this project's float transformPointCloud
OCTO_HD void octo_transform(const float* m, const float p[3], float q[3]) {
  for (int a = 0; a < 3; a++) q[a] = m[a * 4 + 0] * p[0] + m[a * 4 + 1] * p[1] + m[a * 4 + 2] * p[2] + m[a * 4 + 3];
}

OCTO_HD bool octo_in_window(const float q[3], const OctoRules& R) {
  return R.lo[0] <= q[0] && q[0] <= R.hi[0] && R.lo[1] <= q[1] && q[1] <= R.hi[1] && R.lo[2] <= q[2] && q[2] <= R.hi[2];
}

OCTO_HD void octo_truncate(const float o[3], const float p[3], float n, float max_range, float e[3]) {
  for (int a = 0; a < 3; a++) e[a] = o[a] + ((p[a] - o[a]) / n) * max_range;
}

// insertScan :373-439 for one point: the ray's end and what becomes of the end key
OCTO_HD int octo_point_rule(const float o[3], const float p[3], bool ground, double max_range, double min_range, float e[3], bool* truncated) {
  const float n = octo_norm(p[0] - o[0], p[1] - o[1], p[2] - o[2]);
  *truncated = false;
  e[0] = p[0]; e[1] = p[1]; e[2] = p[2];
  if (min_range > 0 && (double)n < min_range) return kSkipMinRange;
  if (ground) {
    if (max_range > 0.0 && (double)n > max_range) { octo_truncate(o, p, n, (float)max_range, e); *truncated = true; }
    return kEndNone;
  }
  if (max_range < 0.0 || (double)n <= max_range) return kEndOccupied;
  octo_truncate(o, p, n, (float)max_range, e);
  *truncated = true;
  return kEndFree;
}

// computeRayKeys: f(k) for the origin's key and every key up to, not including, the end's.  *steps: iterations of the walk.
template <class F>
OCTO_HD int octo_walk(const float o[3], const float e[3], double res, F&& f, int* steps) {
  int ko[3], ke[3];
  *steps = 0;
  if (!octo_key3(o, res, ko) || !octo_key3(e, res, ke)) return kRayRejected;
  if (ko[0] == ke[0] && ko[1] == ke[1] && ko[2] == ke[2]) return kRayOk;
  f(ko);
  const float d[3] = {e[0] - o[0], e[1] - o[1], e[2] - o[2]};
  const float n = octo_norm(d[0], d[1], d[2]);
  int step[3];
  double tmax[3], tdelta[3];
  int bound = 3;
  for (int a = 0; a < 3; a++) {
    const float dir = d[a] / n;
    step[a] = dir > 0.0f ? 1 : dir < 0.0f ? -1 : 0;
    if (step[a] != 0) {
      tmax[a] = (octo_coord(ko[a], res) + (double)step[a] * 0.5 * res - (double)o[a]) / (double)dir;
      tdelta[a] = res / fabs((double)dir);
    } else {
      tmax[a] = DBL_MAX;
      tdelta[a] = DBL_MAX;
    }
    bound += ke[a] > ko[a] ? ke[a] - ko[a] : ko[a] - ke[a];
  }
  int k[3] = {ko[0], ko[1], ko[2]};
  for (;;) {
    if (*steps == bound) return kRayBound;
    *steps += 1;
    const int dim = tmax[0] < tmax[1] ? (tmax[0] < tmax[2] ? 0 : 2) : (tmax[1] < tmax[2] ? 1 : 2);
    k[dim] += step[dim];
    tmax[dim] += tdelta[dim];
    if (k[dim] < 0 || k[dim] >= kKeyEnd) return kRayRejected;
    if (k[0] == ke[0] && k[1] == ke[1] && k[2] == ke[2]) break;
    const double m = tmax[0] < tmax[1] ? (tmax[0] < tmax[2] ? tmax[0] : tmax[2]) : (tmax[1] < tmax[2] ? tmax[1] : tmax[2]);
    if (m > (double)n) break;
    f(k);
  }
  return kRayOk;
}

// the ray as insertScan uses it: nothing is reported unless the whole ray is valid
template <class F>
OCTO_HD int octo_ray(const float o[3], const float e[3], double res, F&& f) {
  int steps;
  const int rc = octo_walk(o, e, res, [](const int*) {}, &steps);
  if (rc != kRayOk) return rc;
  return octo_walk(o, e, res, f, &steps);
}

// updateNode's value
OCTO_HD float octo_update(float v, float d, float clamp_min, float clamp_max) {
  v = v + d;
  if (v < clamp_min) v = clamp_min;
  if (v > clamp_max) v = clamp_max;
  return v;
}
OCTO_HD bool octo_occupied(float v) { return v >= 0.0f; }   // occ_prob_thres_log = (float)log(0.5 / 0.5)

// publishAll :540, :611: the cell's z extent against occupancy_min_z / occupancy_max_z
OCTO_HD bool octo_in_z(int kz, const OctoRules& R) {
  const double z = octo_coord(kz, R.res), half = R.res / 2.0;
  return z + half > R.occ_min_z && z - half < R.occ_max_z;
}

// map_saver.cpp:77-83
OCTO_HD unsigned char octo_pgm_byte(int value) {
  if (value >= 0 && value <= 25) return 254;
  if (value >= 65) return 0;
  return 205;
}

// splitmix64's finaliser: where a packed key starts probing
OCTO_HD uint64_t octo_hash(uint64_t x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// handlePreNodeTraversal :951-999 at full depth, from the key box of all known cells
struct OctoGeom {
  int min_key[2];          // m_paddedMinKey
  int width, height;
  double origin_x, origin_y, resolution;
  double metric_min[3], metric_max[3];
};
OCTO_HD bool octo_grid_geometry(const int kmin[3], const int kmax[3], double res, double min_x_size, double min_y_size, OctoGeom* g) {
  double mn[3], mx[3];
  for (int a = 0; a < 3; a++) {
    mn[a] = octo_coord(kmin[a], res) - res / 2.0;
    mx[a] = octo_coord(kmax[a], res) + res / 2.0;
    g->metric_min[a] = mn[a];
    g->metric_max[a] = mx[a];
  }
  const double hx = 0.5 * min_x_size, hy = 0.5 * min_y_size;
  mn[0] = mn[0] < -hx ? mn[0] : -hx;
  mx[0] = mx[0] > hx ? mx[0] : hx;
  mn[1] = mn[1] < -hy ? mn[1] : -hy;
  mx[1] = mx[1] > hy ? mx[1] : hy;
  int lo[3], hi[3];
  for (int a = 0; a < 3; a++)
    if (!octo_key_d(mn[a], res, &lo[a]) || !octo_key_d(mx[a], res, &hi[a])) return false;
  g->min_key[0] = lo[0]; g->min_key[1] = lo[1];
  g->width = hi[0] - lo[0] + 1;
  g->height = hi[1] - lo[1] + 1;
  g->resolution = res;
  g->origin_x = octo_coord(lo[0], res) - res * 0.5;
  g->origin_y = octo_coord(lo[1], res) - res * 0.5;
  return true;
}

}  // namespace octo
}  // namespace pcm
