// lio_outputs.hip -- the last block of LaserMapping::Run (jueying_lio/src/laser_mapping.cc:361-385) on the device: the frame's
// registered cloud in the world frame (PublishFrameWorld :747-792), in the IMU body frame (PublishFrameBody :794-808), the
// effective points (PublishFrameEffectWorld :810-823), and the saved map pcl_wait_save_ (:776-791, Finish :887-900) as a grow-only
// device log of (x, y, z, intensity) records.  The inputs are the 48-byte PointXYZINormal records the frame entry points left in
// the frame arena (lio_outputs.h: FrameRecord); every transform runs in double with Eigen's _transformVector operation order
// (qrot_d, pcm_device.h) and casts each coordinate to float like `po->x = p_global(0)` (:860-862).
//
// Access pattern: one lane per point.  A lane reads the two 16-byte quarters of its record that hold x, y, z and the intensity
// (bytes 0..15 and 32..47) and writes one 16-byte record, so a wave's stores are 1 KiB contiguous and its loads touch 3 KiB
// contiguous; the unused middle quarter shares its 128-byte lines with the used ones, so staging whole records through LDS would
// fetch the same lines and add a barrier.  The append stores non-temporally: the log is written once and read back much later.
#include "pcm_core.h"
#include "dev_scratch.h"
#include "linearize_common.h"
#include "lio_outputs.h"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace pcm {
namespace {

using lio_out::kInIntensity;
using lio_out::kInRecord;

#define CHECK_CTX(c)                                                   \
  do {                                                                 \
    if (!(c)) return PCM_ERR_INVALID_ARGUMENT;                         \
    if ((c)->device < 0) return PCM_ERR_HIP;                           \
  } while (0)

struct MapLog {   // pcl_wait_save_ and its counters; the context's lio_map sub-state
  DevBuf<float4> pts{"saved map log"};
  size_t n = 0;
  uint64_t growths = 0;   // allocations of the log, the first included
  lio_out::MapCounter ctr;
};

// offset_R_L_I * p + offset_T_L_I   laser_mapping.cc:879
__device__ inline void lidar_to_imu(const LioStateD& s, const float4& p, double (&v)[3]) {
  const double vb[3] = {(double)p.x, (double)p.y, (double)p.z};
  qrot_d(s.off_R, vb, v);
  for (int a = 0; a < 3; a++) v[a] += s.off_T[a];
}
// rot * (offset_R_L_I * p + offset_T_L_I) + pos   laser_mapping.cc:857-858, 868-869
__device__ inline void body_to_world(const LioStateD& s, const float4& p, float (&w)[3]) {
  double v1[3], v2[3];
  lidar_to_imu(s, p, v1);
  qrot_d(s.rot, v1, v2);
  for (int a = 0; a < 3; a++) w[a] = (float)(v2[a] + s.pos[a]);
}

template <bool NT>
__device__ inline void put(float4* dst, const float4& v) {
  if (NT) __builtin_nontemporal_store((pcm_v4f){v.x, v.y, v.z, v.w}, (PCM_GLOBAL pcm_v4f*)dst);
  else gstore4(dst, v);
}

// WORLD: PointBodyToWorld(const PointType*, ...) :855-864; else PointBodyLidarToIMU :877-885.  NT: the destination is the log.
template <bool WORLD, bool NT>
__global__ void __launch_bounds__(256) k_lio_cloud(const char* __restrict__ recs, size_t n, LioStateD s, float4* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const char* r = recs + i * kInRecord;
  const float4 p = gload4(reinterpret_cast<const float4*>(r));
  const float4 q = gload4(reinterpret_cast<const float4*>(r + kInIntensity));   // intensity, curvature, padding
  float w[3];
  if (WORLD) {
    body_to_world(s, p, w);
  } else {
    double v[3];
    lidar_to_imu(s, p, v);
    for (int a = 0; a < 3; a++) w[a] = (float)v[a];
  }
  put<NT>(out + i, make_float4(w[0], w[1], w[2], q.x));
}

// flag[o] = the point contributed a row to the last ObsModel call, o = its place in the caller's scan.
// Default semantics: a plane is stored for it (planes[i], NaN = none) and |p_body| > 81 pd2^2 at the pose of that call -- the
// search kernel's own functions (linearize_common.h).  `scan` is what that kernel read: the re-ordered scan carries o in w.
__global__ void __launch_bounds__(256) k_effect_flags(const float4* __restrict__ scan, const float4* __restrict__ planes, uint32_t n, lio_out::LastObs L, int reordered,
                                                       uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 p = gload4(scan + i);
  float q[3], res = 0.f;
  lio_world_point(L.q_wl, L.t_wl, p, q);
  const bool sel = lio_row_selected(gload4(planes + i), q, lio_body_norm(p), res);
  flag[reordered ? __float_as_uint(p.w) : i] = sel ? 1u : 0u;
}
// PCM_FLAG_LIO_REFERENCE_SEMANTICS: point_selected_surf_[i] as the call left it
__global__ void __launch_bounds__(256) k_effect_flags_ref(const float2* __restrict__ aux, uint32_t n, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  flag[i] = aux[i].y != 0.f ? 1u : 0u;
}
// corr_pts_ in scan order (:645-653) through PointBodyToWorld(const V3F&, ...) :866-875: intensity = |z| of the float just written
__global__ void __launch_bounds__(256) k_effect_scatter(const char* __restrict__ recs, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint32_t n, LioStateD s,
                                                         float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const float4 p = gload4(reinterpret_cast<const float4*>(recs + (size_t)i * kInRecord));
  float w[3];
  body_to_world(s, p, w);
  gstore4(out + pos[i], make_float4(w[0], w[1], w[2], fabsf(w[2])));
}

// PassThrough on z, setFilterLimitsNegative(false): finite x, y, z and z_min <= z <= z_max
__global__ void __launch_bounds__(256) k_z_flags(const float4* __restrict__ pts, size_t n, float z_min, float z_max, uint32_t* __restrict__ flag) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = gload4(pts + i);
  const bool fin = fabsf(p.x) < __builtin_inff() && fabsf(p.y) < __builtin_inff() && fabsf(p.z) < __builtin_inff();
  flag[i] = fin && p.z >= z_min && p.z <= z_max ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_compact(const float4* __restrict__ pts, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, size_t n, float4* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !flag[i]) return;
  gstore4(out + pos[i], gload4(pts + i));
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

// the frame's records, or the refusal: PCM_ERR_NO_INPUT and the call that took them
int need_frame(pcm_ctx* c, const char* who) {
  if (c->lio_frame.valid) return PCM_OK;
  c->err = std::string(who) + ": the context holds no frame records (pcm_lio_frame_begin / pcm_lio_frame_begin_cloud)";
  if (c->lio_frame.taken_by) c->err += std::string("; ") + c->lio_frame.taken_by + " has taken them since";
  return PCM_ERR_NO_INPUT;
}

bool direct_out(void* out, int memory) { return memory == PCM_MEM_DEVICE && (reinterpret_cast<uintptr_t>(out) & 15u) == 0; }

int check_out(pcm_ctx* c, const char* who, int memory, size_t* n) {
  if (!n) { c->err = std::string(who) + ": null count"; return PCM_ERR_INVALID_ARGUMENT; }
  *n = 0;
  if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  return PCM_OK;
}
int too_small(pcm_ctx* c, const char* who, size_t cap, size_t need) {
  char buf[160];
  std::snprintf(buf, sizeof buf, "%s: the output buffer holds %zu records, the result has %zu", who, cap, need);
  c->err = buf;
  return PCM_ERR_INVALID_ARGUMENT;
}
// m records from the device array d to the caller's buffer (d == out: the kernel wrote in place), then wait: the buffer is the caller's again
int deliver(pcm_ctx* c, const float4* d, size_t m, void* out, int memory) {
  if (m && static_cast<const void*>(d) != out)
    PCM_HIPCK(c, hipMemcpyAsync(out, d, sizeof(float4) * m, memory == PCM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

// world (dense or not) and body clouds
template <bool WORLD>
int frame_cloud(pcm_ctx* c, const char* who, const pcm_lio_state* st, int dense, void* out, size_t cap, int memory, size_t* n) {
  CHECK_CTX(c);
  if (!st) { c->err = std::string(who) + ": null state"; return PCM_ERR_INVALID_ARGUMENT; }
  int rc = check_out(c, who, memory, n);
  if (rc != PCM_OK) return rc;
  if ((rc = need_frame(c, who)) != PCM_OK) return rc;
  const char* recs = dense ? c->lio_frame.dense : c->lio_frame.down;
  const size_t m = dense ? c->lio_frame.n_dense : c->lio_frame.n_down;
  *n = m;
  if (!out) return PCM_OK;
  if (cap < m) return too_small(c, who, cap, m);
  if (m == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  DevScratch sc(c->stream);
  float4* d = static_cast<float4*>(out);
  if (!direct_out(out, memory) && (rc = sc.take(&d, m, &c->err, "frame cloud staging")) != PCM_OK) return rc;
  k_lio_cloud<WORLD, false><<<blocks_of(m), 256, 0, c->stream>>>(recs, m, state_of(st), d);
  PCM_HIPCK(c, hipGetLastError());
  return deliver(c, d, m, out, memory);
}

MapLog* log_of(pcm_ctx* c) { return c->lio_map.get<MapLog>(); }

void fill_info(const MapLog* M, pcm_lio_map_info* info) {
  std::memset(info, 0, sizeof(*info));
  if (!M) return;
  info->points = M->n; info->capacity = M->pts.cap; info->frames_appended = M->ctr.frames_appended; info->growths = M->growths;
  info->scan_wait_num = M->ctr.scan_wait_num; info->pcd_index = M->ctr.pcd_index; info->chunk_ready = M->ctr.chunk_ready;
}

}  // namespace
}  // namespace pcm

using namespace pcm;

extern "C" {

int pcm_lio_frame_world(pcm_ctx* c, const pcm_lio_state* st, int dense, void* out, size_t capacity_points, int memory, size_t* n) {
  return frame_cloud<true>(c, "pcm_lio_frame_world", st, dense, out, capacity_points, memory, n);
}

int pcm_lio_frame_body(pcm_ctx* c, const pcm_lio_state* st, void* out, size_t capacity_points, int memory, size_t* n) {
  return frame_cloud<false>(c, "pcm_lio_frame_body", st, 1, out, capacity_points, memory, n);
}

int pcm_lio_frame_effect(pcm_ctx* c, const pcm_lio_state* st, void* out, size_t capacity_points, int memory, size_t* n) {
  static const char who[] = "pcm_lio_frame_effect";
  CHECK_CTX(c);
  if (!st) { c->err = std::string(who) + ": null state"; return PCM_ERR_INVALID_ARGUMENT; }
  int rc = check_out(c, who, memory, n);
  if (rc != PCM_OK) return rc;
  if ((rc = need_frame(c, who)) != PCM_OK) return rc;
  const uint32_t m = (uint32_t)c->src.n;
  const bool ref = (c->cfg.flags & PCM_FLAG_LIO_REFERENCE_SEMANTICS) != 0;
  if (!c->lio_last_obs.valid || m == 0 || m != c->lio_frame.n_down || (ref ? (!c->lio_aux || c->lio_aux_n < m) : !c->planes)) {
    c->err = std::string(who) + ": no ObsModel call (pcm_obs_model / pcm_lio_update) on this frame's scan";
    return PCM_ERR_NO_INPUT;
  }
  PCM_HIPCK(c, hipSetDevice(c->device));
  hipStream_t st_ = c->stream;
  DevScratch sc(st_);
  uint32_t *flag = nullptr, *pos = nullptr;
  if ((rc = sc.take(&flag, m, &c->err, "effect flags")) != PCM_OK || (rc = sc.take(&pos, m, &c->err, "effect places")) != PCM_OK) return rc;
  if (ref) {
    k_effect_flags_ref<<<blocks_of(m), 256, 0, st_>>>(c->lio_aux, m, flag);
  } else {
    const bool reordered = c->cfg.sort_source && c->src_sorted;
    k_effect_flags<<<blocks_of(m), 256, 0, st_>>>(reordered ? c->src_order.p : c->src.d_pts, c->planes, m, c->lio_last_obs, reordered ? 1 : 0, flag);
  }
  PCM_HIPCK(c, hipGetLastError());
  if ((rc = scratch_exclusive_scan(sc, &c->err, flag, pos, (size_t)m)) != PCM_OK) return rc;
  uint32_t tails[2] = {0, 0};
  PCM_HIPCK(c, hipMemcpyAsync(&tails[0], flag + (m - 1), 4, hipMemcpyDeviceToHost, st_));
  PCM_HIPCK(c, hipMemcpyAsync(&tails[1], pos + (m - 1), 4, hipMemcpyDeviceToHost, st_));
  PCM_HIPCK(c, hipStreamSynchronize(st_));
  const size_t k = (size_t)tails[0] + tails[1];
  *n = k;
  if (!out) return PCM_OK;
  if (capacity_points < k) return too_small(c, who, capacity_points, k);
  if (k == 0) return PCM_OK;
  float4* d = static_cast<float4*>(out);
  if (!direct_out(out, memory) && (rc = sc.take(&d, k, &c->err, "effect cloud staging")) != PCM_OK) return rc;
  k_effect_scatter<<<blocks_of(m), 256, 0, st_>>>(c->lio_frame.down, flag, pos, m, state_of(st), d);
  PCM_HIPCK(c, hipGetLastError());
  return deliver(c, d, k, out, memory);
}

// `*pcl_wait_save_ += *laserCloudWorld` and the chunk counter  laser_mapping.cc:776-791
int pcm_lio_map_append(pcm_ctx* c, const pcm_lio_state* st, int dense, int pcd_save_interval, pcm_lio_map_info* info) {
  static const char who[] = "pcm_lio_map_append";
  CHECK_CTX(c);
  if (!st) { c->err = std::string(who) + ": null state"; return PCM_ERR_INVALID_ARGUMENT; }
  if (info) std::memset(info, 0, sizeof(*info));
  int rc = need_frame(c, who);
  if (rc != PCM_OK) return rc;
  PCM_HIPCK(c, hipSetDevice(c->device));
  MapLog* M = c->lio_map.get_or_create<MapLog>();
  if (!M) { c->err = std::string(who) + ": out of host memory"; return PCM_ERR_INTERNAL; }
  const char* recs = dense ? c->lio_frame.dense : c->lio_frame.down;
  const size_t m = dense ? c->lio_frame.n_dense : c->lio_frame.n_down;
  const size_t need = M->n + m;
  const size_t cap = need < M->n ? 0 : lio_out::grow_capacity(M->pts.cap, need);
  if (cap == 0 && need != 0) { c->err = std::string(who) + ": the log cannot hold that many records"; return PCM_ERR_OUT_OF_RANGE; }
  if (need > M->pts.cap || !M->pts.p) {
    if ((rc = M->pts.reserve_keep(c, need, cap, M->n)) != PCM_OK) return rc;
    M->growths++;
  }
  if (m) {   // straight to the tail of the log, behind everything queued on the stream
    k_lio_cloud<true, true><<<blocks_of(m), 256, 0, c->stream>>>(recs, m, state_of(st), M->pts.p + M->n);
    PCM_HIPCK(c, hipGetLastError());
  }
  M->n = need;
  M->ctr.append(M->n, pcd_save_interval);
  if (info) fill_info(M, info);
  return PCM_OK;
}

int pcm_lio_map_info_get(pcm_ctx* c, pcm_lio_map_info* info) {
  CHECK_CTX(c);
  if (!info) { c->err = "pcm_lio_map_info_get: null info"; return PCM_ERR_INVALID_ARGUMENT; }
  fill_info(log_of(c), info);
  return PCM_OK;
}

int pcm_lio_map_get(pcm_ctx* c, size_t first, size_t count, void* out, int memory) {
  CHECK_CTX(c);
  if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  const MapLog* M = log_of(c);
  if (!lio_out::slice_ok(M ? M->n : 0, first, count)) { c->err = "pcm_lio_map_get: the slice does not lie inside the log"; return PCM_ERR_INVALID_ARGUMENT; }
  if (count == 0) return PCM_OK;
  if (!out) { c->err = "pcm_lio_map_get: null output buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  return deliver(c, M->pts.p + first, count, out, memory);
}

// pcl_wait_save_->clear(); scan_wait_num = 0   laser_mapping.cc:788-789.  The buffer stays.
int pcm_lio_map_clear(pcm_ctx* c) {
  CHECK_CTX(c);
  if (MapLog* M = log_of(c)) { M->n = 0; M->ctr.clear(); }
  return PCM_OK;
}

// Finish (laser_mapping.cc:887-900) followed by pcd2map (src/tool/pcd2map/src/pcd2map.cpp:60-72): VoxelGrid, then PassThrough on z
int pcm_lio_map_export(pcm_ctx* c, float leaf_size, double z_min, double z_max, void* out, size_t capacity_points, int memory, size_t* n) {
  static const char who[] = "pcm_lio_map_export";
  CHECK_CTX(c);
  int rc = check_out(c, who, memory, n);
  if (rc != PCM_OK) return rc;
  if (!(leaf_size >= 0.f)) { c->err = std::string(who) + ": leaf_size must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  const MapLog* M = log_of(c);
  const size_t N = M ? M->n : 0;
  const bool window = z_min <= z_max;   // false for NaN limits too
  if (N == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if (!(leaf_size > 0.f) && !window) {   // the log as it is
    *n = N;
    if (!out) return PCM_OK;
    if (capacity_points < N) return too_small(c, who, capacity_points, N);
    return deliver(c, M->pts.p, N, out, memory);
  }
  DevScratch sc(st);
  const float4* cur = M->pts.p;
  size_t m = N;
  if (leaf_size > 0.f) {
    if (N > 0x7fffffffull) { c->err = std::string(who) + ": VoxelGridLarge takes at most 2^31 - 1 points"; return PCM_ERR_OUT_OF_RANGE; }
    float4* cells = nullptr;
    if ((rc = sc.take(&cells, N, &c->err, "export cells")) != PCM_OK) return rc;
    pcm_voxel_large_result r{};
    if ((rc = pcm_voxel_downsample_large(c, M->pts.p, N, sizeof(float4), PCM_MEM_DEVICE, leaf_size, cells, N, &r)) != PCM_OK) return rc;
    cur = cells; m = (size_t)r.cells;
  }
  if (!window || m == 0) {
    *n = m;
    if (!out) return PCM_OK;
    if (capacity_points < m) return too_small(c, who, capacity_points, m);
    return deliver(c, cur, m, out, memory);
  }
  if (m > 0xffffffffull) { c->err = std::string(who) + ": the z window takes at most 2^32 - 1 records"; return PCM_ERR_OUT_OF_RANGE; }
  uint32_t *flag = nullptr, *pos = nullptr;
  if ((rc = sc.take(&flag, m, &c->err, "export flags")) != PCM_OK || (rc = sc.take(&pos, m, &c->err, "export places")) != PCM_OK) return rc;
  // the limits as floats that keep the double comparison: z >= z_min  <=>  z >= the smallest float >= z_min, and the mirror image
  float lo = (float)z_min, hi = (float)z_max;
  if ((double)lo < z_min) lo = std::nextafterf(lo, INFINITY);
  if ((double)hi > z_max) hi = std::nextafterf(hi, -INFINITY);
  k_z_flags<<<blocks_of(m), 256, 0, st>>>(cur, m, lo, hi, flag);
  PCM_HIPCK(c, hipGetLastError());
  if ((rc = scratch_exclusive_scan(sc, &c->err, flag, pos, m)) != PCM_OK) return rc;
  uint32_t tails[2] = {0, 0};
  PCM_HIPCK(c, hipMemcpyAsync(&tails[0], flag + (m - 1), 4, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipMemcpyAsync(&tails[1], pos + (m - 1), 4, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipStreamSynchronize(st));
  const size_t k = (size_t)tails[0] + tails[1];
  *n = k;
  if (!out) return PCM_OK;
  if (capacity_points < k) return too_small(c, who, capacity_points, k);
  if (k == 0) return PCM_OK;
  float4* d = static_cast<float4*>(out);
  if (!direct_out(out, memory) && (rc = sc.take(&d, k, &c->err, "export staging")) != PCM_OK) return rc;
  k_compact<<<blocks_of(m), 256, 0, st>>>(cur, flag, pos, m, d);
  PCM_HIPCK(c, hipGetLastError());
  return deliver(c, d, k, out, memory);
}

}  // extern "C"
