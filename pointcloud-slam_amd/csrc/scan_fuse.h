// scan_fuse.h -- arithmetic of jueying_slam's scan producers in front of imageProjection, as plain C++ that the device kernels
// (scan_fuse.hip) and the host share: the LiDAR + depth-camera fusion node (src/tool/integrate_points/src/fusion_lidar_camera.cpp)
// and the vendor-record converters (src/tool/rs_to_velodyne/src/rs_to_velodyne.cpp, src/tool/hesai_to_velodyne/src/
// hesai_to_velodyne.cpp: the same loops over another record).  tests/test_scan_fuse.py compiles this header with g++
// (tests/scan_fuse_hooks.cpp) and checks it byte for byte against the numpy restatement (tests/scan_fuse_ref.py).  Every operation
// below is one IEEE operation in the order written (-ffp-contract=off).
//
// Pinned where the reference tree cannot pin it, or deliberately different:
//   * `double dist = sqrt(x * x + y * y + z * z)` on float members (fusion_lidar_camera.cpp:232): the file includes <math.h> and is
//     C++, where <math.h> declares the overloads of <cmath> in the global namespace ([depr.c.headers]); the argument is a float,
//     so overload resolution takes sqrt(float).  dist = (double)sqrtf((x * x + y * y) + z * z), the sum in float;
//   * `new_point.z / dist` is float / double: the float is widened, one double division; asin and the product are double;
//   * the pitch table has 52 entries and int(round(pitch + 40)) reaches 52 for 11.5 <= pitch < 12: the reference reads past its
//     array.  Here an index outside the table gives the "otherwise" ring and is counted (n_pitch_index_clamped);
//   * an organised XYZI cloud whose height is neither 16 nor 128 leaves `ring` uninitialised in the reference (:311-315); here
//     it is refused (scan_check_args), as is a ring table shorter than the rule can reach;
//   * padding bytes of an output record are zero and its fourth float is 1.0f (PCL's constructors do the same).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pcm_amd.h"

#if defined(__HIPCC__)
#define SCAN_HD __host__ __device__ inline
#else
#define SCAN_HD inline
#endif

namespace pcm {
namespace scan {

constexpr uint32_t kScanMaxPoints = 1u << 27;      // input points of one call (4 GiB of output records)
constexpr uint32_t kScanMaxTable = 1u << 16;       // entries of one ring table

enum DropClass { kKeep = 0, kNan = 1, kDepthFiltered = 2 };

// what the kernels and the host loop need of one segment (device or host pointers alike)
struct SegView {
  const char* base;
  const uint16_t* table;    // LIDAR_XYZI: the ring table, already cast to uint16 as the assignment to `ring` does
  uint32_t start;           // first index of the segment in the concatenated input
  uint32_t n;
  uint32_t stride, ioff, roff, toff;
  int32_t kind, itype;
  uint32_t ring_mod;        // LIDAR_XYZI: 1: table[id % divisor], 0: table[id / divisor]
  uint32_t divisor;
  uint32_t vec16;           // records and base are 16-byte aligned: x y z in one 16-byte load
  float depth_time;         // DEPTH: float(dt_sec * 1.0 + dt_nsec / 1000000000.0)
  double T[12];             // DEPTH: camera_T[0..2], [4..6], [8..10], [12..14]
};

struct FuseRule {
  double depth_filter, pitch_scale, pitch_min, pitch_max, pitch_offset;
  const uint16_t* pitch_table;
  int32_t pitch_len;
  uint16_t ring_below, ring_otherwise;
  float depth_intensity;
  int32_t layout;
};

// has_nan  fusion_lidar_camera.cpp:94-109, rs_to_velodyne.cpp:56-66 (Inf passes)
SCAN_HD bool scan_has_nan(float x, float y, float z) { return x != x || y != y || z != z; }

// the test at the head of each loop: :120 / :302 (LiDAR), :218 (depth: float z against the double depth_filter)
SCAN_HD int scan_drop_class(int kind, float x, float y, float z, double depth_filter) {
  if (scan_has_nan(x, y, z)) return kNan;
  if (kind == PCM_SCAN_DEPTH && ((double)z > depth_filter && depth_filter >= 0)) return kDepthFiltered;
  return kKeep;
}

// a double that is only 4-byte aligned in its record
SCAN_HD double scan_load_double(const char* p) {
  uint32_t w[2] = {*reinterpret_cast<const uint32_t*>(p), *reinterpret_cast<const uint32_t*>(p + 4)};
  double d;
  memcpy(&d, w, 8);
  return d;
}

SCAN_HD float scan_intensity(const char* rec, uint32_t ioff, int itype) {
  if (itype == PCM_SCAN_INTENSITY_UINT8) return (float)*reinterpret_cast<const uint8_t*>(rec + ioff);
  return *reinterpret_cast<const float*>(rec + ioff);
}

// float(timestamp[i] - timestamp[0])  rs_to_velodyne.cpp:143, fusion_lidar_camera.cpp:130
SCAN_HD float scan_lidar_time(double ts, double ts0) { return (float)(ts - ts0); }

// the ring of point `id` of an organised cloud  rs_to_velodyne.cpp:96-100, fusion_lidar_camera.cpp:311-315
SCAN_HD uint32_t scan_position_index(uint32_t id, uint32_t ring_mod, uint32_t divisor) { return ring_mod ? id % divisor : id / divisor; }

// fusion_lidar_camera.cpp:221-228: doubles, left to right, one rounding to float
SCAN_HD void scan_depth_transform(float x, float y, float z, const double* T, float* o) {
  const double X = (double)x, Y = (double)y, Z = (double)z;
  o[0] = (float)(((X * T[0] + Y * T[3]) + Z * T[6]) + T[9]);
  o[1] = (float)(((X * T[1] + Y * T[4]) + Z * T[7]) + T[10]);
  o[2] = (float)(((X * T[2] + Y * T[5]) + Z * T[8]) + T[11]);
}

// :232-233
SCAN_HD double scan_pitch(float ox, float oy, float oz, double scale) {
  const float s = (ox * ox + oy * oy) + oz * oz;
  const double dist = (double)sqrtf(s);
  return asin((double)oz / dist) * scale;
}

// :236-253 with the clamp; *clamped is set when the index left the table
SCAN_HD uint16_t scan_pitch_ring(double pitch, const FuseRule& R, bool* clamped) {
  if (pitch >= R.pitch_min && pitch < R.pitch_max) {
    const double r = round(pitch + R.pitch_offset);
    if (!(r >= 0.0 && r < (double)R.pitch_len)) { *clamped = true; return R.ring_otherwise; }
    return R.pitch_table[(int)r];
  }
  if (pitch < R.pitch_min) return R.ring_below;
  return R.ring_otherwise;
}

// :258
inline float scan_depth_time(int dt_sec, int dt_nsec) { return (float)((double)dt_sec * 1.0 + (double)dt_nsec / 1000000000.0); }

SCAN_HD uint32_t scan_float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the 32-byte record as 8 words
SCAN_HD void scan_pack(int layout, float x, float y, float z, float intensity, uint16_t ring, float time, uint32_t* w) {
  w[0] = scan_float_bits(x); w[1] = scan_float_bits(y); w[2] = scan_float_bits(z); w[3] = 0x3f800000u;
  w[4] = scan_float_bits(intensity);
  w[5] = layout == PCM_SCAN_OUT_XYZI ? 0u : (uint32_t)ring;
  w[6] = layout == PCM_SCAN_OUT_XYZIRT ? scan_float_bits(time) : 0u;
  w[7] = 0u;
}

// the record of a kept point: `rec` its input record, id its index in the segment, (x, y, z) already loaded
SCAN_HD void scan_point_record(const SegView& S, const FuseRule& R, const char* rec, uint32_t id, float x, float y, float z, uint32_t* w, bool* clamped) {
  if (S.kind == PCM_SCAN_DEPTH) {
    float o[3];
    scan_depth_transform(x, y, z, S.T, o);
    const uint16_t ring = scan_pitch_ring(scan_pitch(o[0], o[1], o[2], R.pitch_scale), R, clamped);
    scan_pack(R.layout, o[0], o[1], o[2], R.depth_intensity, ring, S.depth_time, w);
    return;
  }
  const float intensity = scan_intensity(rec, S.ioff, S.itype);
  if (S.kind == PCM_SCAN_LIDAR_XYZIRT) {
    const uint16_t ring = *reinterpret_cast<const uint16_t*>(rec + S.roff);
    const float time = scan_lidar_time(scan_load_double(rec + S.toff), scan_load_double(S.base + S.toff));
    scan_pack(R.layout, x, y, z, intensity, ring, time, w);
    return;
  }
  scan_pack(R.layout, x, y, z, intensity, S.table[scan_position_index(id, S.ring_mod, S.divisor)], 0.f, w);
}

// ---- host only ----
// the argument rules of pcm_scan_fuse that need no device: nullptr when they hold, else the reason
inline const char* scan_check_args(const pcm_scan_segment* segs, int n_segs, const pcm_scan_fuse_params* P) {
  if (!segs || n_segs < 1) return "at least one segment";
  if (n_segs > PCM_SCAN_MAX_SEGMENTS) return "at most 8 segments";
  if (P->output_layout != PCM_SCAN_OUT_XYZI && P->output_layout != PCM_SCAN_OUT_XYZIR && P->output_layout != PCM_SCAN_OUT_XYZIRT) return "unknown output layout";
  if (P->ring_below < 0 || P->ring_below > 65535 || P->ring_otherwise < 0 || P->ring_otherwise > 65535) return "fallback rings must fit a uint16";
  uint64_t total = 0;
  bool depth = false;
  for (int s = 0; s < n_segs; s++) {
    const pcm_scan_segment& g = segs[s];
    if (g.kind != PCM_SCAN_LIDAR_XYZIRT && g.kind != PCM_SCAN_LIDAR_XYZI && g.kind != PCM_SCAN_DEPTH) return "unknown segment kind";
    if (g.memory != PCM_MEM_HOST && g.memory != PCM_MEM_DEVICE) return "memory must be PCM_MEM_HOST or PCM_MEM_DEVICE";
    if (!g.points && g.n) return "null point buffer";
    if (g.stride_bytes < 12 || (g.stride_bytes % 4) != 0 || g.stride_bytes > 65536) return "stride must be a multiple of 4 in [12, 65536]";
    if (((uintptr_t)g.points % 4) != 0) return "point records must be 4-byte aligned";
    total += g.n;
    if (g.n > kScanMaxPoints || total > kScanMaxPoints) return "too many points";
    if (g.kind == PCM_SCAN_DEPTH) { depth = depth || g.n > 0; continue; }
    if (g.intensity_type != PCM_SCAN_INTENSITY_FLOAT && g.intensity_type != PCM_SCAN_INTENSITY_UINT8) return "unknown intensity type";
    const size_t isz = g.intensity_type == PCM_SCAN_INTENSITY_FLOAT ? 4 : 1;
    if (g.intensity_offset_bytes + isz > g.stride_bytes || (g.intensity_offset_bytes % isz) != 0) return "intensity offset outside the record or misaligned";
    if (g.kind == PCM_SCAN_LIDAR_XYZIRT) {
      if (g.ring_offset_bytes + 2 > g.stride_bytes || (g.ring_offset_bytes % 2) != 0) return "ring offset outside the record or misaligned";
      if (g.timestamp_offset_bytes + 8 > g.stride_bytes || (g.timestamp_offset_bytes % 4) != 0) return "timestamp offset outside the record or misaligned";
      continue;
    }
    if (g.width < 1 || g.height < 1) return "an organised cloud needs width and height";
    int rule = g.ring_rule;
    if (rule == PCM_SCAN_RING_BY_HEIGHT) {
      if (g.height == 16) rule = PCM_SCAN_RING_DIV_WIDTH;
      else if (g.height == 128) rule = PCM_SCAN_RING_MOD_HEIGHT;
      else return "height is neither 16 nor 128: the reference leaves the ring of such a cloud unset";
    }
    if (rule != PCM_SCAN_RING_DIV_WIDTH && rule != PCM_SCAN_RING_MOD_HEIGHT) return "unknown ring rule";
    if ((!g.ring_table && g.n) || g.ring_table_len < 0 || (uint32_t)g.ring_table_len > kScanMaxTable) return "ring table missing or too long";
    if (g.n) {   // the largest index the rule reaches
      const uint64_t reach = rule == PCM_SCAN_RING_DIV_WIDTH ? (g.n - 1) / (uint64_t)g.width : (g.n < (uint64_t)g.height ? g.n - 1 : (uint64_t)g.height - 1);
      if (reach >= (uint64_t)g.ring_table_len) return "ring table too short for this cloud";
    }
  }
  if (depth) {
    if (!P->pitch_ring_table || P->pitch_ring_table_len < 1 || (uint32_t)P->pitch_ring_table_len > kScanMaxTable) return "depth segments need the pitch ring table";
    if (!(P->pitch_min == P->pitch_min) || !(P->pitch_max == P->pitch_max) || !(P->pitch_scale == P->pitch_scale) || !(P->pitch_offset == P->pitch_offset) ||
        !(P->depth_filter == P->depth_filter))
      return "NaN parameter";
  }
  return nullptr;
}

inline void scan_default_params(pcm_scan_fuse_params* p) {
  memset(p, 0, sizeof(*p));
  p->depth_filter = 1.8;            // config/fusion_param.yaml
  p->pitch_scale = 28.6478897565;   // fusion_lidar_camera.cpp:233
  p->pitch_min = -40; p->pitch_max = 12; p->pitch_offset = 40.0;   // :236-237
  p->ring_below = 47; p->ring_otherwise = 51;                       // :245, :253
  p->depth_intensity = 100;         // :229
  p->output_layout = PCM_SCAN_OUT_XYZIRT;
}

// the view of a checked segment; `base` / `table` are where the reader will find the records and the uint16 table
inline SegView scan_view(const pcm_scan_segment& g, const char* base, const uint16_t* table, uint32_t start) {
  SegView v;
  memset(&v, 0, sizeof(v));
  v.base = base; v.table = table; v.start = start; v.n = (uint32_t)g.n;
  v.stride = (uint32_t)g.stride_bytes; v.ioff = (uint32_t)g.intensity_offset_bytes; v.roff = (uint32_t)g.ring_offset_bytes; v.toff = (uint32_t)g.timestamp_offset_bytes;
  v.kind = g.kind; v.itype = g.intensity_type;
  if (g.kind == PCM_SCAN_LIDAR_XYZI) {
    const bool mod = g.ring_rule == PCM_SCAN_RING_MOD_HEIGHT || (g.ring_rule == PCM_SCAN_RING_BY_HEIGHT && g.height == 128);
    v.ring_mod = mod ? 1u : 0u;
    v.divisor = (uint32_t)(mod ? g.height : g.width);
  } else {
    v.divisor = 1u;
  }
  v.vec16 = ((uintptr_t)base % 16) == 0 && (g.stride_bytes % 16) == 0 ? 1u : 0u;
  if (g.kind == PCM_SCAN_DEPTH) {
    v.depth_time = scan_depth_time(g.dt_sec, g.dt_nsec);
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 3; c++) v.T[r * 3 + c] = g.T[r * 4 + c];
  }
  return v;
}

inline FuseRule scan_rule(const pcm_scan_fuse_params& P, const uint16_t* pitch_table) {
  FuseRule R;
  R.depth_filter = P.depth_filter; R.pitch_scale = P.pitch_scale; R.pitch_min = P.pitch_min; R.pitch_max = P.pitch_max; R.pitch_offset = P.pitch_offset;
  R.pitch_table = pitch_table; R.pitch_len = P.pitch_ring_table_len;
  R.ring_below = (uint16_t)P.ring_below; R.ring_otherwise = (uint16_t)P.ring_otherwise;
  R.depth_intensity = P.depth_intensity; R.layout = P.output_layout;
  return R;
}

// counters -> the result struct (n_kept, offsets, n_out); nan[s] / filtered[s] per segment
inline void scan_fill_result(const pcm_scan_segment* segs, int n_segs, const uint32_t* nan, const uint32_t* filtered, uint32_t clamped, pcm_scan_fuse_result* res) {
  memset(res, 0, sizeof(*res));
  uint32_t off = 0;
  for (int s = 0; s < n_segs; s++) {
    pcm_scan_segment_counts& c = res->seg[s];
    c.n_in = (uint32_t)segs[s].n; c.n_nan = nan[s]; c.n_depth_filtered = filtered[s];
    c.n_kept = c.n_in - c.n_nan - c.n_depth_filtered;
    c.out_offset = off;
    off += c.n_kept;
  }
  res->n_out = off;
  res->n_pitch_index_clamped = clamped;
}

// The whole operator on host memory: what the device computes, as one serial loop (the reference's own shape).  Records past
// `capacity` are not written.  Returns PCM_OK, or PCM_ERR_INVALID_ARGUMENT with *why set.
inline int scan_fuse_host(const pcm_scan_segment* segs, int n_segs, const pcm_scan_fuse_params* P, uint32_t* out, size_t capacity, pcm_scan_fuse_result* res,
                          const char** why) {
  *why = scan_check_args(segs, n_segs, P);
  if (*why) return PCM_ERR_INVALID_ARGUMENT;
  uint16_t* ptab = nullptr;
  if (P->pitch_ring_table) {
    ptab = new uint16_t[P->pitch_ring_table_len > 0 ? P->pitch_ring_table_len : 1];
    for (int k = 0; k < P->pitch_ring_table_len; k++) ptab[k] = (uint16_t)P->pitch_ring_table[k];
  }
  const FuseRule R = scan_rule(*P, ptab);
  uint32_t nan[PCM_SCAN_MAX_SEGMENTS] = {0}, filtered[PCM_SCAN_MAX_SEGMENTS] = {0}, clamped = 0;
  size_t m = 0;
  for (int s = 0; s < n_segs; s++) {
    const pcm_scan_segment& g = segs[s];
    uint16_t* tab = nullptr;
    if (g.kind == PCM_SCAN_LIDAR_XYZI && g.ring_table) {
      tab = new uint16_t[g.ring_table_len > 0 ? g.ring_table_len : 1];
      for (int k = 0; k < g.ring_table_len; k++) tab[k] = (uint16_t)g.ring_table[k];
    }
    const SegView S = scan_view(g, static_cast<const char*>(g.points), tab, 0);
    for (uint32_t id = 0; id < S.n; id++) {
      const char* rec = S.base + (size_t)id * S.stride;
      const float* p = reinterpret_cast<const float*>(rec);
      const int cls = scan_drop_class(S.kind, p[0], p[1], p[2], R.depth_filter);
      if (cls == kNan) { nan[s]++; continue; }
      if (cls == kDepthFiltered) { filtered[s]++; continue; }
      uint32_t w[8];
      bool cl = false;
      scan_point_record(S, R, rec, id, p[0], p[1], p[2], w, &cl);
      if (cl) clamped++;
      if (m < capacity) memcpy(out + 8 * m, w, 32);
      m++;
    }
    delete[] tab;
  }
  delete[] ptab;
  scan_fill_result(segs, n_segs, nan, filtered, clamped, res);
  if (m > capacity) { *why = "output buffer too small"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

}  // namespace scan
}  // namespace pcm
