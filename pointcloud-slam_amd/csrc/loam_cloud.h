// loam_cloud.h -- jueying_slam's cachePointCloud: from the driver's organised cloud to the node's laserCloudIn, host + device
// (include/pcm_amd.h, pcm_loam_cloud_prepare / pcm_loam_frame_begin_cloud[_batch]).
//
// Reference (paths relative to jueying_slam of the reference tree):
//   lidar types                  elidar_type                 include/utility.h:116-121
//   the 48-byte record           PointXYZIRT                 src/imageProjection.cpp:7-19 (uint8 intensity, double timestamp, uint16 ring)
//   the 32-byte record           PointXYZIRT                 src/new_localization.cpp:26-38 (float intensity, uint16 ring, float time)
//   NaN removal                  myremoveNaNFromPointCloud   src/imageProjection.cpp:211-256
//   Velodyne                     cachePointCloud             src/imageProjection.cpp:277-320, src/new_localization.cpp:1566-1609
//                                (not dense, or no ring field: ROS_ERROR + ros::shutdown, :280-303)
//   loop bounds                  h < height-1, w < width-1   src/imageProjection.cpp:326-327 (:347-348, :367-368, :384-385, :442-443, :459-460):
//                                the last row and the last column are never written
//   rslidar_16 ring              h<8?h:15-(h-8)              src/imageProjection.cpp:328, src/new_localization.cpp:1618
//   rslidar_16 time              h*2.8*1e-6+w*55.5*1e-6      src/imageProjection.cpp:349, src/new_localization.cpp:1639
//   rslidar_ruby ring            h                           src/imageProjection.cpp:369, src/new_localization.cpp:1659
//   rslidar_ruby time            3.236*((((h+1)%64==0?64:(h+1)%64)-1)/4.f) * 1e-6 + w * 55.552 * 1e-6
//                                                            src/imageProjection.cpp:386, src/new_localization.cpp:1676
//   rslidar_32 ring              h                           src/imageProjection.cpp:444, src/new_localization.cpp:1695 (run when
//                                deskewFlag == -1 || ringFlag == -1, :437 / :1692: the caller's synth_ring)
//   rslidar_32 time              (w*55.52+h%16*2.88+1.44*float(h/16))*1e-6   src/imageProjection.cpp:461, src/new_localization.cpp:1712
//   NaN removal call             is_dense == false           src/imageProjection.cpp:356-361, :393-397, :469-473
// myPassThrough (src/imageProjection.cpp:182-209) has no call site and is not here.  The static ringFlag / deskewFlag of the node
// (time synthesis on the first frame only) are the caller's: synth_ring / synth_time say what this call does.
//
// cloud_record is the one place a record is made: k_lc_write (loam_cloud.hip) calls it per kept point, and
// tests/test_loam_cloud.py compiles this header with g++ and holds it against the per-point restatement of tests/loam_cloud_ref.py.
// The time formulas are evaluated as written: int operands converted to double, every operation one IEEE operation in the
// order of the C++ expression (-ffp-contract=off), the division of the ruby formula and the two float() casts in float.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pcm_amd.h"

#if defined(__HIPCC__)
#define LC_HD __host__ __device__ inline
#else
#define LC_HD inline
#endif

namespace pcm {
namespace loam {

constexpr size_t kCloudMaxPoints = 0x3fffffffull;   // what the front end takes
constexpr size_t kCloudMaxStep = 65536;
constexpr uint32_t kCloudAbsent = 0xffffffffu;

LC_HD bool cloud_is_robosense(int type) {
  return type == PCM_LOAM_LIDAR_RSLIDAR_RUBY || type == PCM_LOAM_LIDAR_RSLIDAR_16 || type == PCM_LOAM_LIDAR_RSLIDAR_32;
}
LC_HD uint32_t cloud_record_bytes(int kind) { return kind == PCM_LOAM_CLOUD_MAPPING ? 48u : 32u; }
LC_HD uint32_t cloud_record_ring_offset(int kind) { return kind == PCM_LOAM_CLOUD_MAPPING ? 32u : 20u; }
LC_HD uint32_t cloud_record_time_offset(int) { return 24u; }
LC_HD int cloud_record_time_kind(int kind) { return kind == PCM_LOAM_CLOUD_MAPPING ? PCM_LOAM_TIME_DOUBLE : PCM_LOAM_TIME_FLOAT; }
LC_HD int cloud_record_intensity_kind(int kind) { return kind == PCM_LOAM_CLOUD_MAPPING ? PCM_LOAM_INTENSITY_UINT8 : PCM_LOAM_INTENSITY_FLOAT; }

// the two loops' bounds (:326-327): int h < height-1, int w < width-1 for height, width >= 1
LC_HD bool cloud_in_loops(uint32_t h, uint32_t w, uint32_t height, uint32_t width) { return h + 1u < height && w + 1u < width; }

// the int expression assigned to the uint16 ring (:328, :369, :444)
LC_HD uint16_t cloud_ring(int type, int h) {
  const int r = type == PCM_LOAM_LIDAR_RSLIDAR_16 ? (h < 8 ? h : 15 - (h - 8)) : h;
  return (uint16_t)r;
}

// the double expression assigned to the time field (:349, :386, :461); a RoboSense type
LC_HD double cloud_time(int type, int h, int w) {
  if (type == PCM_LOAM_LIDAR_RSLIDAR_16) return (double)h * 2.8 * 1e-6 + (double)w * 55.5 * 1e-6;
  if (type == PCM_LOAM_LIDAR_RSLIDAR_RUBY) {
    const int k = (h + 1) % 64 == 0 ? 64 : (h + 1) % 64;
    const float q = (float)(k - 1) / 4.f;
    return 3.236 * (double)q * 1e-6 + (double)w * 55.552 * 1e-6;
  }
  const float s = (float)(h / 16);
  return (((double)w * 55.52 + (double)(h % 16) * 2.88) + 1.44 * (double)s) * 1e-6;
}

// an organised cloud as the kernels read it
struct CloudView {
  const char* base;
  uint32_t n, width, height, step;
  uint32_t xoff, ioff, roff, toff;   // roff / toff: kCloudAbsent without the field
  int32_t type, kind, synth_ring, synth_time;
  int32_t dense;                     // nothing is dropped: is_dense != 0 (Velodyne is dense or refused)
};

// A record begins at base + i * step: 4-byte aligned when step is a multiple of 4, else 2-byte aligned (the base is 4-byte
// aligned, step even).  No load crosses its own alignment: a word that is not 4-byte aligned is read as two halves.
LC_HD uint32_t cloud_ld16(const char* p) { return (uint32_t)*reinterpret_cast<const uint16_t*>(p); }
LC_HD uint32_t cloud_ld32(const char* p) {
  if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) return *reinterpret_cast<const uint32_t*>(p);
  return cloud_ld16(p) | (cloud_ld16(p + 2) << 16);
}
LC_HD bool cloud_finite_bits(uint32_t w) { return (w & 0x7f800000u) != 0x7f800000u; }   // std::isfinite of the float
// pcl_isfinite of x, y and z (:236-238)
LC_HD bool cloud_finite(const CloudView& V, const char* rec) {
  return cloud_finite_bits(cloud_ld32(rec + V.xoff)) && cloud_finite_bits(cloud_ld32(rec + V.xoff + 4)) && cloud_finite_bits(cloud_ld32(rec + V.xoff + 8));
}

// Record i of the cloud as the words of the output record: 12 (48 bytes) or 8 (32 bytes), every padding byte zero.
LC_HD void cloud_record(const CloudView& V, const char* rec, uint32_t i, uint32_t* o) {
  const uint32_t h = i / V.width, w = i - h * V.width;
  const bool in_loops = cloud_is_robosense(V.type) && cloud_in_loops(h, w, V.height, V.width);
  o[0] = cloud_ld32(rec + V.xoff);
  o[1] = cloud_ld32(rec + V.xoff + 4);
  o[2] = cloud_ld32(rec + V.xoff + 8);
  o[3] = 0x3f800000u;   // PCL_ADD_POINT4D: data[3] = 1.0f
  uint32_t ring = V.roff != kCloudAbsent ? cloud_ld16(rec + V.roff) : 0u;
  if (V.synth_ring && in_loops) ring = cloud_ring(V.type, (int)h);
  const bool synth_time = V.synth_time && in_loops;
  const double t = synth_time ? cloud_time(V.type, (int)h, (int)w) : 0.0;
  if (V.kind == PCM_LOAM_CLOUD_MAPPING) {
    uint32_t lo = 0u, hi = 0u;
    if (synth_time) {
      uint64_t b;
      memcpy(&b, &t, 8);
      lo = (uint32_t)b; hi = (uint32_t)(b >> 32);
    } else if (V.toff != kCloudAbsent) {
      lo = cloud_ld32(rec + V.toff); hi = cloud_ld32(rec + V.toff + 4);
    }
    o[4] = (uint32_t)*reinterpret_cast<const uint8_t*>(rec + V.ioff);
    o[5] = 0u;
    o[6] = lo; o[7] = hi;
    o[8] = ring;
    o[9] = 0u; o[10] = 0u; o[11] = 0u;
  } else {
    uint32_t tb = 0u;
    if (synth_time) {
      const float tf = (float)t;   // the double expression assigned to `float time`: one rounding
      memcpy(&tb, &tf, 4);
    } else if (V.toff != kCloudAbsent) {
      tb = cloud_ld32(rec + V.toff);
    }
    o[4] = cloud_ld32(rec + V.ioff);
    o[5] = ring;
    o[6] = tb;
    o[7] = 0u;
  }
}

// ---- the descriptor ------------------------------------------------------------------------------------------------------------
// null: the descriptor is usable; else what is wrong with it
inline const char* cloud_check_desc(const pcm_loam_cloud_desc* d) {
  if (!d) return "null cloud descriptor";
  if (d->lidar_type != PCM_LOAM_LIDAR_VELODYNE && !cloud_is_robosense(d->lidar_type)) return "lidar_type must be one of PCM_LOAM_LIDAR_*";
  if (d->record_kind != PCM_LOAM_CLOUD_MAPPING && d->record_kind != PCM_LOAM_CLOUD_LOCALIZATION) return "record_kind must be PCM_LOAM_CLOUD_MAPPING or PCM_LOAM_CLOUD_LOCALIZATION";
  if ((uint64_t)d->height * (uint64_t)d->width > kCloudMaxPoints) return "cloud too large";
  if (d->point_step < 12 || d->point_step > kCloudMaxStep || (d->point_step % 2) != 0) return "point_step must be an even number of bytes in [12, 65536]";
  const size_t step = d->point_step;
  if (d->xyz_offset_bytes > step || d->xyz_offset_bytes + 12 > step) return "x, y, z lie past point_step";
  if ((d->xyz_offset_bytes % 4) != 0) return "the offset of x is not a multiple of 4 (misaligned field)";
  if (d->intensity_kind != cloud_record_intensity_kind(d->record_kind))
    return "intensity_kind is not the record's (uint8 for PCM_LOAM_CLOUD_MAPPING, float for PCM_LOAM_CLOUD_LOCALIZATION); no conversion is defined";
  const size_t isize = d->intensity_kind == PCM_LOAM_INTENSITY_FLOAT ? 4 : 1;
  if (d->intensity_offset_bytes > step || d->intensity_offset_bytes + isize > step) return "the intensity lies past point_step";
  if ((d->intensity_offset_bytes % isize) != 0) return "the offset of the float intensity is not a multiple of 4 (misaligned field)";
  if (d->ring_offset_bytes != PCM_LOAM_FIELD_ABSENT) {
    if (d->ring_kind != PCM_LOAM_RING_UINT16) return "ring_kind must be PCM_LOAM_RING_UINT16";
    if (d->ring_offset_bytes > step || d->ring_offset_bytes + 2 > step) return "the ring lies past point_step";
    if ((d->ring_offset_bytes % 2) != 0) return "the offset of the ring is not a multiple of 2 (misaligned field)";
  }
  if (d->time_offset_bytes != PCM_LOAM_FIELD_ABSENT) {
    if (d->time_kind != cloud_record_time_kind(d->record_kind))
      return "time_kind is not the record's (double for PCM_LOAM_CLOUD_MAPPING, float for PCM_LOAM_CLOUD_LOCALIZATION); no conversion is defined";
    const size_t tsize = d->time_kind == PCM_LOAM_TIME_DOUBLE ? 8 : 4;
    if (d->time_offset_bytes > step || d->time_offset_bytes + tsize > step) return "the time field lies past point_step";
    if ((d->time_offset_bytes % 4) != 0) return "the offset of the time field is not a multiple of 4 (misaligned field)";
  }
  if (d->lidar_type == PCM_LOAM_LIDAR_VELODYNE) {
    if (!d->is_dense) return "Velodyne: point cloud is not in dense format, please remove NaN points first";
    if (d->ring_offset_bytes == PCM_LOAM_FIELD_ABSENT) return "Velodyne: point cloud ring channel not available";
    if (d->synth_ring || d->synth_time) return "Velodyne: the reference synthesises neither ring nor time";
  }
  return nullptr;
}

// the reference's own struct of the node as the message's layout
inline void cloud_default_desc(int lidar_type, int record_kind, pcm_loam_cloud_desc* d) {
  memset(d, 0, sizeof(*d));
  d->point_step = cloud_record_bytes(record_kind);
  d->xyz_offset_bytes = 0;
  d->intensity_offset_bytes = 16;
  d->ring_offset_bytes = cloud_record_ring_offset(record_kind);
  d->time_offset_bytes = cloud_record_time_offset(record_kind);
  d->intensity_kind = cloud_record_intensity_kind(record_kind);
  d->ring_kind = PCM_LOAM_RING_UINT16;
  d->time_kind = cloud_record_time_kind(record_kind);
  d->is_dense = 1;
  d->lidar_type = lidar_type;
  d->record_kind = record_kind;
  d->synth_ring = (lidar_type == PCM_LOAM_LIDAR_RSLIDAR_16 || lidar_type == PCM_LOAM_LIDAR_RSLIDAR_RUBY) ? 1 : 0;   // :328, :369 run on every frame
  d->synth_time = 0;
}

// the descriptor has passed cloud_check_desc
inline CloudView cloud_view(const pcm_loam_cloud_desc& d, const void* base) {
  CloudView V;
  V.base = static_cast<const char*>(base);
  V.n = d.height * d.width; V.width = d.width; V.height = d.height; V.step = (uint32_t)d.point_step;
  V.xoff = (uint32_t)d.xyz_offset_bytes; V.ioff = (uint32_t)d.intensity_offset_bytes;
  V.roff = d.ring_offset_bytes == PCM_LOAM_FIELD_ABSENT ? kCloudAbsent : (uint32_t)d.ring_offset_bytes;
  V.toff = d.time_offset_bytes == PCM_LOAM_FIELD_ABSENT ? kCloudAbsent : (uint32_t)d.time_offset_bytes;
  V.type = d.lidar_type; V.kind = d.record_kind;
  const bool rs = cloud_is_robosense(d.lidar_type);
  V.synth_ring = rs && d.synth_ring ? 1 : 0;
  V.synth_time = rs && d.synth_time ? 1 : 0;
  V.dense = d.is_dense ? 1 : 0;
  return V;
}

// what the call reports besides the counts
inline void cloud_fill_flags(const pcm_loam_cloud_desc& d, pcm_loam_cloud_result* r) {
  const bool rs = cloud_is_robosense(d.lidar_type);
  r->ring_synthesised = rs && d.synth_ring ? 1 : 0;
  r->time_synthesised = rs && d.synth_time ? 1 : 0;
  r->time_available = (d.time_offset_bytes != PCM_LOAM_FIELD_ABSENT || r->time_synthesised) ? 1 : 0;
}

}  // namespace loam
}  // namespace pcm
