// occ_map.h -- arithmetic of jueying_slam's 2D occupancy mapping tool (src/tool/occupancy_mapping: getScan, processScan, TraceLine,
// ConvertWorld2GridIndex, getGridMap, saveMap) as plain C++ that the device kernels (occ_map.hip) and the host share.
// tests/test_occ_map.py compiles this header with g++ (tests/occ_map_hooks.cpp) and checks it bit for bit against the numpy
// restatement (tests/occ_map_ref.py).  Every operation below is one IEEE operation in the order written (-ffp-contract=off).
//
// Pinned where the reference tree cannot pin it, or deliberately different:
//   * hypot / atan2 of two floats are the float overloads; the range is (float)sqrt((double)x * x + (double)y * y): the products
//     are exact, so this is one rounding to double, a correctly rounded sqrt and one rounding to float, the same bits on the
//     host and on the device (it is also what glibc's hypotf evaluates);
//   * a point with a non-finite coordinate is skipped (the reference casts a NaN angle to int: undefined);
//   * a cell index is int(v / resolution): truncation towards zero, so the cells -0 and +0 are one cell of double width;
//   * a cell's value comes from its two integer counters, logit = (double)n_occ * log_occ + (double)n_free * log_free, not from
//     a sum in visit order, and the reference's test 1 / (1 + exp(-logit)) * 100 >= 50 is decided as logit > kOccLogitEdge,
//     which is that expression under a correctly rounded exp (occ_cell_value);
//   * the origin is (double)min_index * resolution, one product (the reference adds two products whose split depends on how
//     its quadtree grew);
//   * the grid is a dense rectangle of at most kOccMaxCells cells; counters are uint32 and wrap after 2^32 updates of one cell.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define OCC_HD __host__ __device__ inline
#else
#define OCC_HD inline
#endif

namespace pcm {
namespace occ {

constexpr uint64_t kOccMaxCells = 1ull << 28;       // hard cap of the dense rectangle (2 GiB of counters)
constexpr uint32_t kOccMaxBeams = 1u << 20;         // beams of a virtual scan (angle_increment >= 6e-6)
constexpr double kOccMaxIndex = 1073741824.0;       // |v / resolution| of every pose coordinate +- (max_radius + 0.1) stays below 2^30
// 1 / (1 + exp(-logit)) * 100 >= 50 holds exactly when fl(1 + fl(exp(-logit))) <= 2, i.e. exp(-logit) rounds to at most 1 + 2^-52,
// i.e. (exp correctly rounded) logit > -1.5 * 2^-52
constexpr double kOccLogitEdge = -3.3306690738754696e-16;

struct OccParams {
  double min_z, max_z, angle_increment, min_range, max_range, log_occ, log_free, resolution, max_radius;
  int fill_with_white, use_nan;
};

struct OccRect {   // allocated cells [x0, x0 + w) x [y0, y0 + h)
  long long x0, y0, w, h;
};

OCC_HD bool occ_finite(float v) { return v == v && v <= 3.402823466e38f && v >= -3.402823466e38f; }

// getScan: beam_size
OCC_HD uint32_t occ_beam_size(double angle_increment) { return (uint32_t)ceil((3.1415927 - (-3.1415927)) / angle_increment); }

// the value every beam starts from (laser_scan_output.ranges is float)
OCC_HD float occ_range_init(double max_range) { return (float)(max_range + 1); }

OCC_HD float occ_hypot(float x, float y) { return (float)sqrt((double)x * (double)x + (double)y * (double)y); }

// one point of getScan: false when it does not reach a beam, else the beam and the candidate range
OCC_HD bool occ_point_beam(float x, float y, float z, const OccParams& P, uint32_t beam_size, uint32_t* beam, float* range) {
  if (!occ_finite(x) || !occ_finite(y) || !occ_finite(z)) return false;
  if (!((double)z >= P.min_z && (double)z <= P.max_z)) return false;
  const float r = occ_hypot(x, y);
  const float angle = atan2f(y, x);
  const int index = (int)(((double)angle - (-3.1415927)) / P.angle_increment);
  if (!(index >= 0 && (uint32_t)index < beam_size)) return false;
  if (!((double)r >= P.min_range && (double)r <= P.max_range)) return false;
  *beam = (uint32_t)index;
  *range = r;
  return true;
}

// a beam's minimum to its published range: NaN outside [min_range, max_range]
OCC_HD float occ_beam_range(float r, const OccParams& P) {
  if ((double)r > P.max_range || (double)r < P.min_range) return nanf("");
  return r;
}

OCC_HD double occ_beam_angle(uint32_t i, double angle_increment) { return angle_increment * (double)i + angle_increment / 2 - M_PI; }

// processScan's rules for one beam: false = skipped; else the distance to trace, whether the end cell is hit and whether the
// line is traced
OCC_HD bool occ_beam_dist(float range, const OccParams& P, double* dist, bool* hit, bool* trace) {
  double d = (double)range;
  if (!(d == d) || d > 1.7976931348623157e308) {
    if (!(d == d) && P.use_nan) d = P.max_radius + 0.1; else return false;
  }
  if (d > P.max_radius) d = P.max_radius + 0.1;
  *dist = d;
  *hit = d <= P.max_radius;
  *trace = d <= P.max_radius || P.fill_with_white != 0;
  return true;
}

// ConvertWorld2GridIndex for one axis (the caller keeps |v / resolution| below kOccMaxIndex)
OCC_HD int occ_cell(double v, double resolution) { return (int)(v / resolution); }

OCC_HD void occ_end_cell(double dist, double angle, double yaw, double px, double py, double resolution, int* cx, int* cy) {
  const double laser_x = dist * cos(yaw + angle);
  const double laser_y = dist * sin(yaw + angle);
  *cx = occ_cell(laser_x + px, resolution);
  *cy = occ_cell(laser_y + py, resolution);
}

// TraceLine: f(x, y) for every cell of the line from (x0, y0) towards (x1, y1) in the reference's order, the end cell left out
template <typename F>
OCC_HD void occ_trace_line(int x0, int y0, int x1, int y1, F&& f) {
  const int x_end = x1, y_end = y1;
  const bool steep = fabs(((double)y1 * 1.0 - (double)y0 * 1.0) / ((double)x1 * 1.0 - (double)x0 * 1.0)) >= 1;
  if (steep) { int t = x0; x0 = y0; y0 = t; t = x1; x1 = y1; y1 = t; }
  if (x0 > x1) { int t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; }
  const int delta_x = x1 - x0;
  const int delta_y = y1 > y0 ? y1 - y0 : y0 - y1;
  int error = 0;
  int y = y0;
  const int ystep = y0 < y1 ? 1 : -1;
  for (int x = x0; x <= x1; x++) {
    const int px = steep ? y : x, py = steep ? x : y;
    error += delta_y;
    if (2 * error >= delta_x) { y += ystep; error -= delta_x; }
    if (px == x_end && py == y_end) continue;
    f(px, py);
  }
}

// position of a cell in the allocation, or -1 when it lies outside (the caller counts it and drops it)
OCC_HD long long occ_slot(int ix, int iy, const OccRect& R) {
  const long long cx = (long long)ix - R.x0, cy = (long long)iy - R.y0;
  if (cx < 0 || cy < 0 || cx >= R.w || cy >= R.h) return -1;
  return cy * R.w + cx;
}

OCC_HD double occ_logit(uint32_t n_occ, uint32_t n_free, double log_occ, double log_free) {
  const double a = (double)n_occ * log_occ;
  const double b = (double)n_free * log_free;
  return a + b;
}

// getGridMap's value of a cell: -1 unknown, else 100 / 0.  `exists`: the cell the map was initialised at (it is a node of the
// reference's tree from the start, with logit 0, whether or not a scan touches it).
OCC_HD int occ_cell_value(uint32_t n_occ, uint32_t n_free, bool exists, double log_occ, double log_free) {
  if (n_occ == 0 && n_free == 0 && !exists) return -1;
  return occ_logit(n_occ, n_free, log_occ, log_free) > kOccLogitEdge ? 100 : 0;
}

// saveMap's byte of a value
OCC_HD unsigned char occ_pgm_byte(int value) {
  if (value >= 0 && value <= 25) return 254;
  if (value >= 65) return 0;
  return 205;
}

// ---- host only ----
// the literal expression of getGridMap (libm's exp): what occ_cell_value is shown equal to in tests/test_occ_map.py
inline int occ_value_literal(double logit) {
  double prob = 1.0 / (1.0 + exp(-1.0 * logit));
  prob = prob * 100.0;
  return prob >= 50 ? (int)100.1 : (int)0.1;
}

// the cells a scan at (px, py) can touch, with one cell of slack: false when an index would leave +-2^30
inline bool occ_pose_rect(double px, double py, const OccParams& P, long long* lo_x, long long* hi_x, long long* lo_y, long long* hi_y) {
  const double reach = P.max_radius + 0.1;
  const double v[4] = {(px - reach) / P.resolution, (px + reach) / P.resolution, (py - reach) / P.resolution, (py + reach) / P.resolution};
  for (int k = 0; k < 4; k++)
    if (!(v[k] > -kOccMaxIndex && v[k] < kOccMaxIndex)) return false;
  *lo_x = (long long)floor(v[0]) - 1; *hi_x = (long long)ceil(v[1]) + 1;
  *lo_y = (long long)floor(v[2]) - 1; *hi_y = (long long)ceil(v[3]) + 1;
  return true;
}

}  // namespace occ
}  // namespace pcm
