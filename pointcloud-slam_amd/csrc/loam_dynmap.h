// loam_dynmap.h -- the host logic of jueying_slam's localisation map (include/dynamic_map.h, localization.cpp:229-315,
// new_localization.cpp:454-514): which area tiles are loaded around a pose (is_in_area / create_pcd), when they are reloaded
// (dynamic_load_map_run) and the window that dynamic_load_map's pcl::PassThrough filters cut out of them on every frame.  Plain
// C++17: the API layer (loam_dynmap.hip) runs it on the host, tests/test_loam_dynmap.py compiles it with g++ and checks it against
// the numpy restatement (tests/loam_dynmap_ref.py).  Every float operation below is one IEEE operation in the order written
// (-ffp-contract=off).
//
// Pinned where the reference tree cannot pin it (pcl::PassThrough is not in it):
//   * setFilterLimits takes floats: a limit is the double expression pose -/+ max_range * 1.1 rounded once to float;
//   * a point passes iff lo <= v && v <= hi in float (both ends inclusive, a NaN never passes);
//   * a point with any non-finite coordinate is dropped whatever the window says (deviation: PassThrough reads one field).
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define PCM_DM_HD __host__ __device__
#else
#define PCM_DM_HD
#endif

namespace pcm {
namespace loam {

// dynamic_map.h:16-25 without the path
struct Area {
  double x_min, y_min, z_min, x_max, y_max, z_max;
};

// dynamic_map.h:114-117: inclusive, in double, z never tested
inline bool is_in_area(double x, double y, const Area& area, double m) {
  return ((area.x_min - m) <= x && x <= (area.x_max + m) && (area.y_min - m) <= y && y <= (area.y_max + m));
}

// create_pcd (dynamic_map.h:129-156): the areas of one list that hold (p_x, p_y) with the margin, in list order; the position
// and the margin arrive as floats (const float&, float margin) and are promoted by the call.  margin < 0: every area
// (localization.cpp:229-242 loads the whole list once).
inline std::vector<int32_t> select_areas(const Area* areas, int n, float p_x, float p_y, float margin) {
  std::vector<int32_t> sel;
  for (int i = 0; i < n; i++)
    if (margin < 0.f || is_in_area(p_x, p_y, areas[i], margin)) sel.push_back((int32_t)i);
  return sel;
}

// last_loadMap before the first load (localization.cpp:249)
constexpr float kNeverLoaded = -999999.0f;

// dynamic_load_map_run (localization.cpp:295-300): float differences of pose[3..5], the float sum of their squares left to right,
// a float square root, compared with the int area_size converted to float
inline bool need_load(const float pose[6], const float last_load[6], int32_t area_size) {
  const float distance_x = pose[3] - last_load[3];
  const float distance_y = pose[4] - last_load[4];
  const float distance_z = pose[5] - last_load[5];
  const float load_distance = sqrtf(distance_x * distance_x + distance_y * distance_y + distance_z * distance_z);
  return load_distance > (float)area_size;
}

// pass.setFilterLimits(pose - max_range * 1.1, pose + max_range * 1.1) (localization.cpp:261,269): float - float * double
inline void crop_limits(float pose_v, float max_range, float* lo, float* hi) {
  *lo = (float)((double)pose_v - (double)max_range * 1.1);
  *hi = (float)((double)pose_v + (double)max_range * 1.1);
}

struct CropWindow {
  float x_lo, x_hi, y_lo, y_hi;
  int32_t crop_x;   // 0: the y window alone (what localization.cpp:259-273 computes), 1: x and y
};

// the window of one frame; margin < 0: dynamic_load_map does nothing, the whole map is the target (infinite limits)
inline CropWindow crop_window(const float pose[6], float max_range, int32_t margin, int32_t crop_x) {
  CropWindow w;
  if (margin < 0) {
    w.x_lo = w.y_lo = -INFINITY;
    w.x_hi = w.y_hi = INFINITY;
  } else {
    crop_limits(pose[3], max_range, &w.x_lo, &w.x_hi);
    crop_limits(pose[4], max_range, &w.y_lo, &w.y_hi);
  }
  w.crop_x = crop_x ? 1 : 0;
  return w;
}

PCM_DM_HD inline bool dm_finite(float v) {
  union { float f; uint32_t u; } b;
  b.f = v;
  return (b.u & 0x7f800000u) != 0x7f800000u;
}

// 1: kept, 0: outside the window, 2: dropped for a non-finite coordinate
PCM_DM_HD inline int crop_class(float x, float y, float z, const CropWindow& w) {
  if (!(dm_finite(x) && dm_finite(y) && dm_finite(z))) return 2;
  if (!(w.y_lo <= y && y <= w.y_hi)) return 0;
  if (w.crop_x && !(w.x_lo <= x && x <= w.x_hi)) return 0;
  return 1;
}

}  // namespace loam
}  // namespace pcm
