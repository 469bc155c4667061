// lidar_handlers.h -- arithmetic of jueying_lio's PointCloudPreprocess handlers for sensor_msgs::PointCloud2 clouds
// (src/jueying_lio/src/pointcloud_preprocess.cc: LivoxHandler :89-118, Oust64Handler :120-149, VelodyneHandler :151-227,
// RslidarHandler :229-305), as plain C++ that the device kernels (lidar_handlers.hip) and the host share.
// tests/test_lidar_handlers.py compiles this header with g++ (tests/lidar_handlers_hooks.cpp) and checks it bit for bit against
// the per-point Python restatement (tests/lidar_handlers_ref.py).  Every operation below is one IEEE operation in the order
// written (-ffp-contract=off).
//
// The yaw path of the Velodyne and RoboSense handlers (last point's time not > 0) carries time_last[ring] through the cloud:
//   b = float((yaw <= yaw_fp ? yaw_fp - yaw : yaw_fp - yaw + 360.0) / 3.61);  f = b < time_last ? float(double(b) + 360.0 / 3.61) : b
// As a function of time_last a point is g(x) = x > b ? hi : lo (LhFn); the ring's first point is the constant 0.  Two of them
// compose into a third of the same form, (g2 o g1)(x) = x > b1 ? g2(hi1) : g2(lo1), and that is function composition evaluated
// literally, so any grouping of a chain gives the same bits (lh_compose); the serial loop is the left fold.
//
// Pinned where the reference has undefined behaviour, or deliberately different:
//   * n == 0 gives n_out = 0 (the reference reads points[-1]);
//   * a ring >= num_scans on the yaw path fails the call (the reference writes past its vectors); num_scans > 256,
//     point_filter_num < 1 and a record too short for its offsets are refused;
//   * yaw_first / yaw_end (:172-180) and yaw_last are dead code and are not restated; the loop's constant is 57.2957;
//   * padding of an output record is zero and its fourth float is 1.0f (PCL's constructors do the same).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pcm_amd.h"

#if defined(__HIPCC__)
#define LH_HD __host__ __device__ inline
#else
#define LH_HD inline
#endif

namespace pcm {
namespace lidar {

constexpr size_t kLhMaxPoints = (size_t)1 << 27;   // input points of one call

// what the kernels and the host loop need of a cloud (device or host pointer alike)
struct LhView {
  const char* base;
  uint32_t n, stride, xoff, ioff, toff, roff;
  int32_t type, time_kind, ring_kind, num_scans;
  uint32_t pfn;
  float time_scale;
  double blind2;   // blind_ * blind_, a double product
};

// a point of the yaw path as a function of time_last: x > b ? hi : lo
struct LhFn { float b, lo, hi; };

LH_HD float lh_load_f32(const char* p) { float f; memcpy(&f, p, 4); return f; }
// a double that is only 4-byte aligned in its record
LH_HD double lh_load_f64(const char* p) {
  uint32_t w[2];
  memcpy(&w[0], p, 4); memcpy(&w[1], p + 4, 4);
  double d;
  memcpy(&d, w, 8);
  return d;
}
// the time field widened to double (exact for every kind)
LH_HD double lh_time(const LhView& V, const char* rec) {
  if (V.time_kind == PCM_LIDAR_TIME_DOUBLE) return lh_load_f64(rec + V.toff);
  if (V.time_kind == PCM_LIDAR_TIME_UINT32) { uint32_t u; memcpy(&u, rec + V.toff, 4); return (double)u; }
  return (double)lh_load_f32(rec + V.toff);
}
LH_HD uint32_t lh_ring(const LhView& V, const char* rec) {
  const uint8_t* r = reinterpret_cast<const uint8_t*>(rec + V.roff);
  return V.ring_kind == PCM_LIDAR_RING_UINT16 ? (uint32_t)r[0] | ((uint32_t)r[1] << 8) : (uint32_t)r[0];
}
LH_HD bool lh_uses_yaw_path(int type) { return type == PCM_LIDAR_VELODYNE || type == PCM_LIDAR_RSLIDAR; }
// given_offset_time_  :168, :246 (Ouster and Livox clouds always carry times)
LH_HD bool lh_given_time(const LhView& V) {
  if (!lh_uses_yaw_path(V.type) || V.n == 0) return true;
  return lh_time(V, V.base + (size_t)(V.n - 1) * V.stride) > 0;
}

// curvature [ms] of a point that carries its time  :114, :145, :193, :271; t0 = time of point 0
LH_HD float lh_curvature_given(const LhView& V, const char* rec, double t0) {
  const double t = lh_time(V, rec);
  if (V.type == PCM_LIDAR_OUSTER) return (float)(t / 1e6);
  if (V.type == PCM_LIDAR_VELODYNE) {
    if (V.time_kind == PCM_LIDAR_TIME_FLOAT) return lh_load_f32(rec + V.toff) * V.time_scale;   // a float product
    return (float)(t * (double)V.time_scale);
  }
  return (float)((t - t0) * (double)V.time_scale);
}

// float products, float sums left to right
LH_HD float lh_range2(float x, float y, float z) { return (x * x + y * y) + z * z; }
// the candidate test and the blind test  :98-103, :129-134 (equality kept), :221-222, :299-300 (strict)
LH_HD bool lh_keep(const LhView& V, uint32_t i, float x, float y, float z) {
  if (i % V.pfn != 0) return false;
  const double r2 = (double)lh_range2(x, y, z);
  if (V.type == PCM_LIDAR_OUSTER || V.type == PCM_LIDAR_LIVOX_STD) return !(r2 < V.blind2);
  return r2 > V.blind2;
}

// :197, :275
LH_HD double lh_yaw(float x, float y) { return atan2((double)y, (double)x) * 57.2957; }
// :209-213, :287-291 (omega_l = 3.61)
LH_HD float lh_b(double yaw, double yaw_fp) { return (float)((yaw <= yaw_fp ? yaw_fp - yaw : (yaw_fp - yaw) + 360.0) / 3.61); }
// :215, :293
LH_HD float lh_wrapped(float b) { return (float)((double)b + 360.0 / 3.61); }

LH_HD LhFn lh_fn_first() { return LhFn{0.f, 0.f, 0.f}; }
LH_HD LhFn lh_fn_point(float b) { return LhFn{b, b, lh_wrapped(b)}; }
LH_HD float lh_apply(const LhFn& g, float x) { return x > g.b ? g.hi : g.lo; }   // b < time_last, the literal comparison
// first f, then g
LH_HD LhFn lh_compose(const LhFn& f, const LhFn& g) { return LhFn{f.b, lh_apply(g, f.lo), lh_apply(g, f.hi)}; }

// sort key of a curvature: unsigned order = float order, -0.0 and 0.0 equal
LH_HD uint32_t lh_time_key(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if (f == 0.0f) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

LH_HD void lh_record(float x, float y, float z, float intensity, float curvature, float* o) {
  o[0] = x; o[1] = y; o[2] = z; o[3] = 1.0f;
  o[4] = 0.f; o[5] = 0.f; o[6] = 0.f; o[7] = 0.f;
  o[8] = intensity; o[9] = curvature; o[10] = 0.f; o[11] = 0.f;
}

inline void lh_default_desc(int type, pcm_lidar_desc* d) {
  memset(d, 0, sizeof(*d));
  d->type = type;
  d->stride_bytes = 32; d->xyz_offset_bytes = 0; d->intensity_offset_bytes = 16;
  d->ring_kind = PCM_LIDAR_RING_UINT16;
  switch (type) {
    case PCM_LIDAR_VELODYNE:    // velodyne_ros::Point, config/velodyne.yaml
      d->time_kind = PCM_LIDAR_TIME_FLOAT; d->time_offset_bytes = 20; d->ring_offset_bytes = 24;
      d->num_scans = 16; d->blind = 0.5; d->time_scale = 1e3f; d->point_filter_num = 1;
      break;
    case PCM_LIDAR_RSLIDAR:     // rslidar_ros::Point, config/rslidar.yaml
      d->time_kind = PCM_LIDAR_TIME_DOUBLE; d->time_offset_bytes = 24; d->ring_offset_bytes = 20;
      d->num_scans = 16; d->blind = 0.5; d->time_scale = 1000.f; d->point_filter_num = 1;
      break;
    case PCM_LIDAR_LIVOX_STD:   // livox_ros::Point (tag @20, line @21 are not read), config/livox.yaml
      d->time_kind = PCM_LIDAR_TIME_DOUBLE; d->time_offset_bytes = 24; d->ring_offset_bytes = 21; d->ring_kind = PCM_LIDAR_RING_UINT8;
      d->num_scans = 6; d->blind = 0.1; d->time_scale = 1000.f; d->point_filter_num = 2;
      break;
    case PCM_LIDAR_OUSTER:      // ouster_ros::Point, config/ouster64.yaml
      d->stride_bytes = 48;
      d->time_kind = PCM_LIDAR_TIME_UINT32; d->time_offset_bytes = 20; d->ring_offset_bytes = 26; d->ring_kind = PCM_LIDAR_RING_UINT8;
      d->num_scans = 64; d->blind = 4.0; d->time_scale = 1e-3f; d->point_filter_num = 3;
      break;
    default: break;
  }
}

// nullptr, or why the descriptor is refused
inline const char* lh_check_desc(const pcm_lidar_desc* d) {
  if (!d) return "null descriptor";
  if (d->type != PCM_LIDAR_VELODYNE && d->type != PCM_LIDAR_OUSTER && d->type != PCM_LIDAR_RSLIDAR && d->type != PCM_LIDAR_LIVOX_STD) return "unknown LiDAR type";
  if (d->time_kind != PCM_LIDAR_TIME_FLOAT && d->time_kind != PCM_LIDAR_TIME_DOUBLE && d->time_kind != PCM_LIDAR_TIME_UINT32) return "unknown time kind";
  if (d->ring_kind != PCM_LIDAR_RING_UINT8 && d->ring_kind != PCM_LIDAR_RING_UINT16) return "unknown ring kind";
  if (d->num_scans < 0 || d->num_scans > PCM_LIDAR_MAX_SCANS) return "num_scans must be in [0, 256]";
  if (d->point_filter_num < 1) return "point_filter_num must be >= 1";
  const size_t s = d->stride_bytes;
  if (s < 12 || s > 4096 || (s % 4) != 0) return "stride must be a multiple of 4 in [12, 4096]";
  if ((d->xyz_offset_bytes % 4) != 0 || (d->intensity_offset_bytes % 4) != 0 || (d->time_offset_bytes % 4) != 0) return "x, intensity and time offsets must be multiples of 4";
  const size_t tsize = d->time_kind == PCM_LIDAR_TIME_DOUBLE ? 8 : 4, rsize = d->ring_kind == PCM_LIDAR_RING_UINT16 ? 2 : 1;
  if (d->xyz_offset_bytes > s || d->xyz_offset_bytes + 12 > s || d->intensity_offset_bytes > s || d->intensity_offset_bytes + 4 > s || d->time_offset_bytes > s ||
      d->time_offset_bytes + tsize > s)
    return "the record is too short for its offsets";
  if (lh_uses_yaw_path(d->type) && (d->ring_offset_bytes > s || d->ring_offset_bytes + rsize > s)) return "the record is too short for its offsets";
  return nullptr;
}

inline LhView lh_view(const pcm_lidar_desc& d, const void* base, size_t n) {
  LhView V;
  V.base = static_cast<const char*>(base);
  V.n = (uint32_t)n; V.stride = (uint32_t)d.stride_bytes; V.xoff = (uint32_t)d.xyz_offset_bytes; V.ioff = (uint32_t)d.intensity_offset_bytes;
  V.toff = (uint32_t)d.time_offset_bytes; V.roff = (uint32_t)d.ring_offset_bytes;
  V.type = d.type; V.time_kind = d.time_kind; V.ring_kind = d.ring_kind; V.num_scans = d.num_scans;
  V.pfn = (uint32_t)d.point_filter_num; V.time_scale = d.time_scale;
  V.blind2 = d.blind * d.blind;
  return V;
}

// The handler on host memory, the reference's serial loop.  out: capacity records of 12 floats; *n_out counts every kept point,
// also those past the capacity.  *bad_rings: points of the yaw path whose ring is >= num_scans (they are skipped; the caller fails
// the call when there is one).
inline void lh_filter_host(const LhView& V, float* out, size_t capacity, size_t* n_out, int* given, uint32_t* bad_rings) {
  *n_out = 0; *bad_rings = 0;
  *given = lh_given_time(V) ? 1 : 0;
  if (V.n == 0) return;
  const double t0 = lh_time(V, V.base);
  bool is_first[PCM_LIDAR_MAX_SCANS];
  double yaw_fp[PCM_LIDAR_MAX_SCANS];
  float time_last[PCM_LIDAR_MAX_SCANS];
  for (int r = 0; r < PCM_LIDAR_MAX_SCANS; r++) { is_first[r] = true; yaw_fp[r] = 0.0; time_last[r] = 0.f; }
  size_t m = 0;
  for (uint32_t i = 0; i < V.n; i++) {
    const char* rec = V.base + (size_t)i * V.stride;
    const float x = lh_load_f32(rec + V.xoff), y = lh_load_f32(rec + V.xoff + 4), z = lh_load_f32(rec + V.xoff + 8);
    float curv;
    if (*given) {
      curv = lh_curvature_given(V, rec, t0);
    } else {
      const uint32_t layer = lh_ring(V, rec);
      if (layer >= (uint32_t)V.num_scans) { (*bad_rings)++; continue; }
      const double yaw = lh_yaw(x, y);
      if (is_first[layer]) {
        yaw_fp[layer] = yaw; is_first[layer] = false; time_last[layer] = 0.0f;
        continue;
      }
      curv = lh_b(yaw, yaw_fp[layer]);
      if (curv < time_last[layer]) curv = lh_wrapped(curv);
      time_last[layer] = curv;
    }
    if (!lh_keep(V, i, x, y, z)) continue;
    if (m < capacity) lh_record(x, y, z, lh_load_f32(rec + V.ioff), curv, out + 12 * m);
    m++;
  }
  *n_out = m;
}

}  // namespace lidar
}  // namespace pcm
