// lio_outputs.h -- the host bookkeeping of the jueying_lio frame outputs and the saved map (lio_outputs.hip): where the records of the
// current frame lie and who has taken their memory since, the pose of the last ObsModel call, the chunk counter of
// LaserMapping::PublishFrameWorld (jueying_lio/src/laser_mapping.cc:776-791) and the growth rule of the log.  No HIP here: the
// whole header is exercised by a stand-alone host program (tests/lio_outputs_hooks.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace pcm {
namespace lio_out {

constexpr size_t kInRecord = 48;    // pcl::PointXYZINormal: x, y, z at 0, intensity at 32, curvature at 36
constexpr size_t kInIntensity = 32;
constexpr size_t kOutRecord = 16;   // x, y, z, intensity

// The records pcm_lio_frame_begin / pcm_lio_frame_begin_cloud left in the frame arena: scan_undistort_ (dense) and scan_down_body_
// (down, in the order of the caller's scan).  They live until the next call that takes the arena; that call's name is kept for
// the refusal text.  A context that never ran a frame, or whose source came from pcm_set_source, holds no frame.
struct FrameRecord {
  const char* dense = nullptr;
  const char* down = nullptr;
  size_t n_dense = 0, n_down = 0;
  bool valid = false;
  const char* taken_by = nullptr;   // a string literal: the call that invalidated the record (null: there never was a frame)

  void set(const char* dense_records, size_t nd, const char* down_records, size_t ns) {
    dense = dense_records; n_dense = nd; down = down_records; n_down = ns;
    valid = true; taken_by = nullptr;
  }
  // any call that takes the arena, or replaces the source: the frame's records are gone
  void take(const char* who) {
    if (valid) taken_by = who;
    valid = false;
    dense = down = nullptr; n_dense = n_down = 0;
  }
};

// the float pose of the last ObsModel call (pcm::LioPose::q_wl, t_wl): what the default semantics' 81 pd2^2 test is evaluated at
struct LastObs {
  float q_wl[4] = {0.f, 0.f, 0.f, 1.f};
  float t_wl[3] = {0.f, 0.f, 0.f};
  bool valid = false;
  void set(const float* q, const float* t) {
    for (int a = 0; a < 4; a++) q_wl[a] = q[a];
    for (int a = 0; a < 3; a++) t_wl[a] = t[a];
    valid = true;
  }
};

// scan_wait_num / pcd_index_ of laser_mapping.cc:779-790.  The reference writes the chunk and clears the cloud itself; here the
// append reports the chunk and the caller downloads and clears (clear() = pcl_wait_save_->clear(); scan_wait_num = 0).  A caller
// that does not clear gets the next index on the next append, like a reference whose clear() was skipped.
struct MapCounter {
  uint64_t frames_appended = 0;
  int32_t scan_wait_num = 0;
  int32_t pcd_index = 0;
  int32_t chunk_ready = 0;   // of the last append

  // one `*pcl_wait_save_ += *laserCloudWorld`; points_after: the size of the log behind it
  void append(uint64_t points_after, int pcd_save_interval) {
    frames_appended++;
    if (scan_wait_num < INT32_MAX) scan_wait_num++;
    chunk_ready = 0;
    if (points_after > 0 && pcd_save_interval > 0 && scan_wait_num >= pcd_save_interval) {   // :781
      pcd_index++;
      chunk_ready = 1;
    }
  }
  void clear() { scan_wait_num = 0; chunk_ready = 0; }
};

// capacity of the log that holds `need` records: the growth of reserve_target (x 1.5 + 1024), never below the need.
// 0: `need` records cannot be addressed (size_t overflow of the byte count).
inline size_t grow_capacity(size_t cap, size_t need) {
  if (need > (SIZE_MAX / kOutRecord)) return 0;
  if (need <= cap) return cap;
  size_t grown = cap + cap / 2 + 1024;
  if (grown < cap || grown > SIZE_MAX / kOutRecord) grown = SIZE_MAX / kOutRecord;
  return grown > need ? grown : need;
}

// slice [first, first + count) of a log of n records
inline bool slice_ok(size_t n, size_t first, size_t count) { return first <= n && count <= n - first; }

}  // namespace lio_out
}  // namespace pcm
