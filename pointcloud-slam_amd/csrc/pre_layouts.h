// pre_layouts.h -- where every pre-processing operator and entry point keeps what in the memory it works out of: one layout
// function each over a carver (arena_carver.h), the only place that memory is described.  Run over a null base a layout is the
// operator's *_scratch_bytes or the size the entry point reserves; run over the real base it is the carve.  The size of a rocPRIM
// temporary comes in as a number.  Host code, no HIP header (tests/arena_carver_check.cpp pins every offset and total).
// The VoxelGrid's arrays are vg::work_carve (voxel_grid.h).
#pragma once

#include <cstdint>

#include "arena_carver.h"
#include "lidar_handlers.h"

namespace pcm {

// ---- operators -------------------------------------------------------------------------------------------------------------------
struct LivoxScratch { uint32_t *flag, *pos; void* tmp; };   // keep flags, their exclusive scan, the scan's temporary
inline LivoxScratch livox_layout(ArenaCarver& a, size_t n, size_t scan_tmp_bytes) {
  LivoxScratch S;
  S.flag = a.take<uint32_t>(n);
  S.pos = a.take<uint32_t>(n);
  S.tmp = a.take<char>(scan_tmp_bytes);
  return S;
}

struct LhScratch {
  uint32_t *small, *first_idx, *flag, *pos, *val, *val_s;
  double* yaw;
  uint8_t *key, *key_s;
  float *curv, *after;
  lidar::LhFn* tot;
  void *scan_tmp, *sort_tmp;
};
// the arrays of one handler call of n points in workgroups of `block`
inline LhScratch lidar_filter_layout(ArenaCarver& a, size_t n, size_t block, size_t scan_tmp_bytes, size_t sort_tmp_bytes) {
  LhScratch S;
  const size_t n1 = n ? n : 1, nb = (n1 + block - 1) / block;
  S.small = a.take<uint32_t>(64);
  S.first_idx = a.take<uint32_t>(PCM_LIDAR_MAX_SCANS);
  S.flag = a.take<uint32_t>(n1);
  S.pos = a.take<uint32_t>(n1);
  S.scan_tmp = a.take<char>(scan_tmp_bytes);
  S.yaw = a.take<double>(n1);
  S.val = a.take<uint32_t>(n1);
  S.val_s = a.take<uint32_t>(n1);
  S.key = a.take<uint8_t>(n1);
  S.key_s = a.take<uint8_t>(n1);
  S.curv = a.take<float>(n1);
  S.tot = a.take<lidar::LhFn>(nb);
  S.after = a.take<float>(nb);
  S.sort_tmp = a.take<char>(sort_tmp_bytes);
  return S;
}

struct TimeSortScratch { uint32_t *key, *key_s, *val, *val_s; void* tmp; };
inline TimeSortScratch lidar_time_sort_layout(ArenaCarver& a, size_t m, size_t sort_tmp_bytes) {
  TimeSortScratch S;
  const size_t m1 = m ? m : 1;
  S.key = a.take<uint32_t>(m1);
  S.key_s = a.take<uint32_t>(m1);
  S.val = a.take<uint32_t>(m1);
  S.val_s = a.take<uint32_t>(m1);
  S.tmp = a.take<char>(sort_tmp_bytes);
  return S;
}

// VoxelGridLarge: the tables of a level, for up to cap pieces; [2]: this level's and the next one's
constexpr uint32_t kVlBoxBlocks = 2048;   // workgroups of a box pass (they stride over the points)
struct VlTables {
  unsigned int* mm[2];   // [cap][6] ordered-int boxes, min then max
  uint32_t* fin[2];      // [cap] 1: a leaf piece, its box is final
  uint32_t* flag;        // [cap] 1: cut at this level (what the scan reads)
  uint32_t* before;      // [cap] cuts before the piece
  int32_t* axis;         // [cap]
  float* mid;            // [cap]
  unsigned int* part;    // [kVlBoxBlocks][6] partial boxes of the first level
  uint32_t* status;      // [0] cuts, [1] first stuck piece, [2] first piece that would pass the depth cap, [3] free; [4..8) fold_boxes' zeros
  void* tmp; size_t tmp_bytes;
};
inline VlTables vl_tables_layout(ArenaCarver& a, size_t cap, size_t scan_tmp_bytes) {
  VlTables T{};
  for (int b = 0; b < 2; b++) T.mm[b] = a.take<unsigned int>(6 * cap);
  for (int b = 0; b < 2; b++) T.fin[b] = a.take<uint32_t>(cap);
  T.flag = a.take<uint32_t>(cap);
  T.before = a.take<uint32_t>(cap);
  T.axis = a.take<int32_t>(cap);
  T.mid = a.take<float>(cap);
  T.part = a.take<unsigned int>(6 * kVlBoxBlocks);
  T.status = a.take<uint32_t>(8);
  T.tmp_bytes = scan_tmp_bytes;
  T.tmp = a.take<char>(scan_tmp_bytes);
  return T;
}
// VoxelGridLarge's per-point memory: [piece ids | a copy of a host cloud]
struct VlPoints { uint32_t* id; const void* cloud; };
template <class S> VlPoints vl_points_layout(S& a, size_t n, int memory, const void* points, size_t stride) {
  VlPoints L;
  L.id = a.template take<uint32_t>(n);
  L.cloud = a.in(memory, points, n * stride);
  return L;
}

// the LOAM front end's batch workspace for B frames: [staged clouds | owner | row counts | row offsets | members | corner picks |
// corner counts | cells of stage 1 | cells of stage 2 | the VoxelGrid's arrays, shared by the two stages]
struct LfBatch {
  uint32_t *owner, *rowcnt, *roff;
  int32_t *member, *cpick, *ccnt;
  void *cells1, *cells2;   // float4 each
  char* vg;
};
// pts[i]: where frame i's cloud is read
template <class S> LfBatch loam_batch_layout(S& a, int B, int memory, const void* const* points, const size_t* n_points, size_t stride, const void** pts, size_t cap, int n_scan, int ppr,
                                             size_t N1, size_t N2, size_t vg_bytes) {
  LfBatch L;
  for (int i = 0; i < B; i++) pts[i] = a.in(memory, points[i], n_points[i] * stride);
  L.owner = a.template take<uint32_t>(cap * B);
  L.rowcnt = a.template take<uint32_t>((size_t)n_scan * B);
  L.roff = a.template take<uint32_t>((size_t)(n_scan + 1) * B);
  L.member = a.template take<int32_t>(cap * B);
  L.cpick = a.template take<int32_t>((size_t)n_scan * ppr * B);
  L.ccnt = a.template take<int32_t>((size_t)n_scan * B);
  L.cells1 = a.template take<char>(16 * N1);
  L.cells2 = a.template take<char>(16 * N2);
  L.vg = a.template take<char>(vg_bytes);
  return L;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
// pcm_voxel_downsample, pcm_livox_filter, pcm_lidar_filter: [staged input | staged output | scratch of the operator]
struct FilterArena { const void* src; void* dst; void* scratch; };
template <class S> FilterArena filter_layout(S& a, int memory, const void* in, size_t in_bytes, int out_memory, void* out, size_t out_bytes, size_t scratch_bytes) {
  FilterArena L;
  L.src = a.in(memory, in, in_bytes);
  L.dst = a.out(out_memory, out, out_bytes);
  L.scratch = a.template take<char>(scratch_bytes);
  return L;
}

// pcm_undistort: [IMU poses | staged points]
struct UndistortArena { pcm_imu_pose* poses; void* pts; };
template <class S> UndistortArena undistort_layout(S& a, const pcm_imu_pose* poses, int npose, int memory, void* points, size_t bytes) {
  UndistortArena L;
  L.poses = a.upload(a.template take<pcm_imu_pose>((size_t)npose), poses, sizeof(pcm_imu_pose) * (size_t)npose);
  L.pts = const_cast<void*>(a.in(memory, points, bytes));
  return L;
}

// pcm_lio_frame_begin: [raw message | filtered records | down-sampled records | IMU poses | scratch of the operators]
// pcm_lio_frame_begin_cloud: [raw cloud | filtered records, later the down-sampled ones | time-sorted records | IMU poses | scratch]
// n 48-byte records in each of rec[0], rec[1]; the raw block is the only host -> device copy of the frame.  raw_always: the block
// is there for a device cloud as well (the Livox entry)
struct FrameArena { const void* raw; char* rec[2]; pcm_imu_pose* poses; void* scratch; };
template <class S> FrameArena frame_layout(S& a, int memory, const void* points, size_t raw_bytes, bool raw_always, size_t n, int npose, std::initializer_list<size_t> operator_scratch) {
  FrameArena L;
  L.raw = a.in(memory, points, raw_bytes);
  if (raw_always && memory != PCM_MEM_HOST) (void)a.template take<char>(raw_bytes);
  L.rec[0] = a.template take<char>(n * 48);
  L.rec[1] = a.template take<char>(n * 48);
  L.poses = a.template take<pcm_imu_pose>((size_t)(npose > 1 ? npose : 1));
  L.scratch = a.take_largest(operator_scratch);
  return L;
}

// pcm_scan_fuse's scratch: [counters | pitch table, ring table of every LiDAR segment | workgroup counts | workgroup offsets |
// rocPRIM's temporary] for nb workgroups; tables of uint16, contiguous from pitch_tab to kept (one upload)
struct ScanScratch { uint32_t* ctr; uint16_t* pitch_tab; uint16_t* seg_tab[PCM_SCAN_MAX_SEGMENTS]; uint32_t *kept, *off; void* tmp; };
inline ScanScratch scan_scratch_layout(ArenaCarver& a, size_t n_counters, const pcm_scan_segment* segs, int n_segs, const pcm_scan_fuse_params& P, size_t nb, size_t scan_tmp_bytes) {
  ScanScratch L{};
  L.ctr = a.take<uint32_t>(n_counters);
  L.pitch_tab = a.take<uint16_t>(P.pitch_ring_table ? (size_t)P.pitch_ring_table_len : 0);
  for (int s = 0; s < n_segs; s++)
    if (segs[s].kind == PCM_SCAN_LIDAR_XYZI) L.seg_tab[s] = a.take<uint16_t>((size_t)segs[s].ring_table_len);
  L.kept = a.take<uint32_t>(nb + 1);
  L.off = a.take<uint32_t>(nb + 1);
  L.tmp = a.take<char>(scan_tmp_bytes);
  return L;
}
// ... and its staged host segments: base[s] = where segment s is read
template <class S> void scan_input_layout(S& a, const pcm_scan_segment* segs, int n_segs, const void** base) {
  for (int s = 0; s < n_segs; s++) base[s] = a.in(segs[s].memory, segs[s].points, segs[s].n * segs[s].stride_bytes);
}

// pcm_loam_cloud_prepare / pcm_loam_frame_begin_cloud[_batch]'s scratch for the B clouds of a call, nb workgroups of non-dense
// clouds together: [workgroup counts | workgroup offsets (one more than counts: the total) | kept count per cloud | rocPRIM's temporary]
struct LoamCloudScratch { uint32_t *kept, *off, *info; void* tmp; };
inline LoamCloudScratch loam_cloud_scratch_layout(ArenaCarver& a, size_t nb, size_t B, size_t scan_tmp_bytes) {
  LoamCloudScratch L;
  L.kept = a.take<uint32_t>(nb + 1);
  L.off = a.take<uint32_t>(nb + 1);
  L.info = a.take<uint32_t>(B);
  L.tmp = a.take<char>(scan_tmp_bytes);
  return L;
}
// ... and its staged host clouds: base[i] = where cloud i is read
template <class S> void loam_cloud_input_layout(S& a, int B, int memory, const void* const* data, const size_t* bytes, const void** base) {
  for (int i = 0; i < B; i++) base[i] = a.in(memory, data[i], bytes[i]);
}

// pcm_gicp_bfgs_set_correspondences: [source | target | source indices | target indices | Mahalanobis rows]
struct BfgsStaging { const void *src, *tgt; const int32_t *idx_src, *idx_tgt; const float* maha; };
template <class S> BfgsStaging bfgs_staging_layout(S& a, int memory, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride, const int32_t* idx_src, const int32_t* idx_tgt,
                                                   size_t m, const float* maha) {
  BfgsStaging L;
  L.src = a.in(memory, src, n_src * stride);
  L.tgt = a.in(memory, tgt, n_tgt * stride);
  L.idx_src = static_cast<const int32_t*>(a.in(memory, idx_src, m * 4));
  L.idx_tgt = static_cast<const int32_t*>(a.in(memory, idx_tgt, m * 4));
  L.maha = static_cast<const float*>(a.in(memory, maha, n_src * 64));
  return L;
}

}  // namespace pcm
