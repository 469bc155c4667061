// loam_device.h -- what the LOAM scan-to-map kernels (loam.hip) and their host side (loam_api.hip) share, and what the LOAM
// operators share among themselves: the context check, the stores, the target's owner, the point arena.
#pragma once

#include <algorithm>

#include "host_util.h"
#include "loam_step.h"
#include "pcm_device.h"

namespace pcm {
namespace loam {

// one context of a (batched) LOAM optimisation, as the kernels read it
struct LoamDesc {
  TargetView map[2];       // [0] corner map, [1] surf map; pts.w = the point's index in the caller's cloud (raw bits)
  const float4* feats;     // body-frame features: n_c corner features, then n_s surf features
  uint32_t n_c, n_s;
  LoamState* st;
  double* partials;        // [cdiv(n_c + n_s, kLanes)][kSums]
  float4* coeff_out;       // parity hook: (coeff.xyz, intensity) per feature, x = NaN when not selected; nullptr: off
  int32_t* nn_out;         // parity hook: [feature][5] caller indices of the neighbours with d2 <= 1 (-1 pads); nullptr: off
  double* sums_out;        // parity hook: the step kernel exports the summed row instead of stepping; nullptr: step
  float x0[6];             // initial pose (roll, pitch, yaw, x, y, z)
  int32_t pad[2];
};

__host__ __device__ inline uint32_t num_blocks(uint32_t n) { return (n + kLanes - 1) / kLanes; }

// loam.hip
void launch_tag_input_index(hipStream_t stream, float4* pts, const uint32_t* order, uint32_t n);
void launch_init(hipStream_t stream, const LoamDesc* d_descs, int n);
// one iteration of every context still running: the correspondence pass, then the step kernel
void launch_round(hipStream_t stream, const LoamDesc* d_descs, int n, uint32_t max_blocks, const StepParams& p);

// loam_api.hip: the front end (loam_features.hip) writes the context's source features in place: room for n features, then
// the counts once they are on the device (the same state pcm_loam_set_source leaves)
int loam_source_reserve(pcm_ctx* c, size_t n, float4** feats);
void loam_source_commit(pcm_ctx* c, uint32_t n_c, uint32_t n_s);

// what every pcm_loam_* entry point asks first: a context, a usable device, PCM_MODEL_LOAM.  The operators answer another model
// with different codes and texts, and callers may depend on them: each passes its own.
inline int loam_check_ctx(pcm_ctx* c, int not_loam, const char* not_loam_msg) {
  if (!c) return PCM_ERR_INVALID_ARGUMENT;
  if (c->device < 0) return PCM_ERR_HIP;
  if (c->cfg.model != PCM_MODEL_LOAM) { c->err = not_loam_msg; return not_loam; }
  return PCM_OK;
}

// loam_api.hip: who wrote the context's two target clouds.  The key-frame submap (loam_submap.hip) and the map-tile crop
// (loam_dynmap.hip) write them in place: room for the clouds (the owner falls back to the caller, as after a real
// pcm_loam_set_target), then their sizes and the writer once they are known (the state pcm_loam_set_target leaves, grids not built
// yet: the next align builds them).  Each keeps its result only while loam_target_view still names it the owner, so neither
// mistakes the other's target for the one it left.
enum class TargetOwner { caller, submap, dynmap };
int loam_target_reserve(pcm_ctx* c, size_t n_corner, size_t n_surf, float4** corner, float4** surf);
void loam_target_commit(pcm_ctx* c, uint32_t n_corner, uint32_t n_surf, TargetOwner owner);
// the target clouds in caller order; false: there is no target, or `owner` did not write it
bool loam_target_view(pcm_ctx* c, TargetOwner owner, const float4** corner, uint32_t* n_corner, const float4** surf, uint32_t* n_surf);
// the current source as PointXYZI pieces: feats (xyz, w = index), and the intensity either as whole records (xyzi, the front
// end's output) or as one float per feature (inten); both null: intensity 0.  Returns 0, 1 without a source, 2 when the source
// came from the front end and its output has been rewritten since (pcm_loam_extract_features on the same context, a failed frame).
int loam_source_view(pcm_ctx* c, const float4** feats, uint32_t* n_c, uint32_t* n_s, const float4** xyzi, const float** inten);
// The stores of a context: the key frames and submap workspace (loam_submap.hip), the Scan Context descriptors (loam_sc.hip), the
// map tiles and crop workspace (loam_dynmap.hip), the loop verifier (loam_loop.hip).  The context's LOAM state owns the holders,
// each of those files its type.  loam_store: the store, made on first use when `create`; null: none yet, or out of host memory.
enum class LoamStore { key, sc, dyn, loop };
SubState* loam_store_holder(pcm_ctx* c, LoamStore which);   // null: the LOAM state itself could not be allocated
template <class T> T* loam_store(pcm_ctx* c, LoamStore which, bool create) {
  SubState* h = loam_store_holder(c, which);
  return !h ? nullptr : create ? h->get_or_create<T>() : h->get<T>();
}
// loam_check_ctx, then the store (the texts: no LOAM state, no store; both for want of host memory)
template <class T> int loam_check_store(pcm_ctx* c, const char* not_loam_msg, LoamStore which, T** out, bool create = true, const char* oom_msg = "out of host memory",
                                        const char* store_oom_msg = "out of host memory") {
  *out = nullptr;
  const int rc = loam_check_ctx(c, PCM_ERR_INVALID_ARGUMENT, not_loam_msg);
  if (rc != PCM_OK) return rc;
  SubState* h = loam_store_holder(c, which);
  if (!h) { c->err = oom_msg; return PCM_ERR_INTERNAL; }
  *out = create ? h->get_or_create<T>() : h->get<T>();
  if (!*out && create) { c->err = store_oom_msg; return PCM_ERR_INTERNAL; }
  return PCM_OK;
}
// a grow-only array of points a store appends to (what: its name in an error text)
struct Arena {
  DevBuf<float4> d;
  size_t n = 0;
  explicit Arena(const char* what) : d(what) {}
  // room for `extra` more points; growth copies device to device.  The first allocation holds at least 65 536 points.
  int reserve(pcm_ctx* c, size_t extra) { return d.reserve_keep(c, n + extra, std::max<size_t>(n + extra, d.cap + d.cap / 2 + 65536), n); }
};
// loam_submap.hip: one stored cloud of a key frame on the device (which: 0 corner, 1 surf; false: no such key frame), and the host
// mirror of the key poses (returns K)
bool loam_keyframe_cloud(pcm_ctx* c, int key, int which, const float4** pts, uint32_t* n);
bool loam_keyframe_pose(pcm_ctx* c, int key, float pose6[6]);   // roll, pitch, yaw, x, y, z as stored
struct KeyPose;
int loam_keyposes(pcm_ctx* c, const KeyPose** kp);
// loam_submap.hip: queues the near-key-frame cloud of (key, search_num, wrt_key, leaf) -- pcm_loam_submap_near's cloud, bit for
// bit -- on the context's stream into workspace `slot` (0 or 1) and does not wait.  Once the stream has drained, h_small[0] is
// the number of points at pts and h_small[2] says whether the leaf index overflowed; pts == nullptr: the selected clouds are
// empty.  An empty store and bad arguments: PCM_ERR_INVALID_ARGUMENT.  loam_near_waited: the caller has drained the stream.
struct NearCloud { const float4* pts; uint32_t n_in; const uint32_t* h_small; };
int loam_near_queue(pcm_ctx* c, int slot, int key, int search_num, int wrt_key, float leaf, NearCloud* out);
void loam_near_waited(pcm_ctx* c);

// loam_features.hip: pieces of the segmented VoxelGrid that do not depend on where the elements live
struct SvWork {
  uint64_t* keys; uint64_t* keys_s; uint32_t* vals; uint32_t* vals_s;   // [N]; after sv_sort_cells vals holds the first sorted element of every cell
  uint32_t* head; uint32_t* slot;                                      // [N]
  uint32_t* scnt; uint32_t* sfirst;                                    // [nseg] cells per segment, first cell of the segment
  uint32_t* nc;                                                        // [0] cells, [1] valid elements (zeroed by the caller)
  void* tmp; size_t tmp_bytes; void* tmp2; size_t tmp2_bytes;          // rocprim scratch (sv_temp_bytes)
};
void sv_temp_bytes(size_t n, size_t* sort_bytes, size_t* scan_bytes);
void sv_clear(hipStream_t st, unsigned int* mm, uint32_t* scnt, uint32_t nseg);
int sv_sort_cells(pcm_ctx* c0, hipStream_t st, const SvWork& W, uint32_t N, uint32_t nseg);
// gen: bumps whenever the output array is rewritten
bool loam_features_last_out(pcm_ctx* c, const float4** out, uint32_t* n_c, uint32_t* n_s, uint64_t* gen);

#if defined(__HIPCC__)
// inverse of pcm_device.h's f2ord, branch-free (the select form crashes this compiler's instruction selection when followed by float arithmetic)
__device__ inline float ord2f(unsigned int o) { const unsigned int m = (unsigned int)((int)o >> 31); return __uint_as_float(o ^ (~m | 0x80000000u)); }

// 64-lane butterfly reductions (every lane ends with the result).  The double sum adds in this fixed order, so its bits do not
// depend on the schedule; linearize_common.h's DPP reductions are another order and stay apart.
__device__ inline uint32_t wave_min_u32(uint32_t v) {
  for (int off = 32; off >= 1; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return v;
}
__device__ inline uint32_t wave_max_u32(uint32_t v) {
  for (int off = 32; off >= 1; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return v;
}
__device__ inline uint32_t wave_sum_u32(uint32_t v) {
  for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
  return v;
}
__device__ inline uint64_t wave_min_u64(uint64_t v) {
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}
__device__ inline double wave_sum_f64(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// a lane's point into the bounding box of its segment (mm: 6 ordered-int words per segment, min then max)
__device__ inline void sv_wave_minmax(bool valid, uint32_t seg, const float4& pt, unsigned int* __restrict__ mm) {
  unsigned int lo[3], hi[3];
  const float c[3] = {pt.x, pt.y, pt.z};
  for (int a = 0; a < 3; a++) { lo[a] = valid ? f2ord(c[a]) : 0xffffffffu; hi[a] = valid ? f2ord(c[a]) : 0u; }
  // one atomic per wave when every valid lane shares the segment
  const uint64_t vm = __ballot(valid);
  if (vm == 0) return;
  const int l0 = __ffsll((unsigned long long)vm) - 1;
  const uint32_t s0 = (uint32_t)__shfl((int)seg, l0, 64);
  const bool same = __ballot(valid && seg != s0) == 0;
  if (same) {
    for (int off = 32; off >= 1; off >>= 1)
      for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], (unsigned int)__shfl_xor((int)lo[a], off, 64)); hi[a] = max(hi[a], (unsigned int)__shfl_xor((int)hi[a], off, 64)); }
    if ((threadIdx.x & 63) == 0)
      for (int a = 0; a < 3; a++) { atomicMin(&mm[6 * s0 + a], lo[a]); atomicMax(&mm[6 * s0 + 3 + a], hi[a]); }
  } else if (valid) {
    for (int a = 0; a < 3; a++) { atomicMin(&mm[6 * seg + a], lo[a]); atomicMax(&mm[6 * seg + 3 + a], hi[a]); }
  }
}

// the box of pcl::VoxelGrid from a segment's min / max: b = {min_b x, y, z, divb_mul[1], divb_mul[2], state} (state 0: empty or no
// leaf, 1: index overflow, 2: valid).  The products are formed in double: exact, as a valid box has fewer than 2^31 cells.
// Returns whether the index overflows.
__device__ inline bool sv_box(const unsigned int* __restrict__ mm, float leaf, long long* __restrict__ b) {
  b[5] = 0;
  if (mm[0] == 0xffffffffu) return false;   // empty segment
  if (!(leaf > 0.f)) return false;
  const float inv = 1.0f / leaf;
  float mn[3], mx[3];
  for (int a = 0; a < 3; a++) { mn[a] = ord2f(mm[a]); mx[a] = ord2f(mm[3 + a]); }
  double cells = 1.0;
  for (int a = 0; a < 3; a++) cells *= trunc((double)((mx[a] - mn[a]) * inv)) + 1.0;   // int64_t((max - min) * inv) + 1, max >= min
  const bool over = cells > 2147483647.0;
  int mb[3], xb[3];
  for (int a = 0; a < 3; a++) { mb[a] = (int)floorf(mn[a] * inv); xb[a] = (int)floorf(mx[a] * inv); }
  const double div0 = (double)xb[0] - (double)mb[0] + 1.0, div1 = (double)xb[1] - (double)mb[1] + 1.0;
  b[0] = mb[0]; b[1] = mb[1]; b[2] = mb[2];
  b[3] = over ? 0 : (long long)div0;
  b[4] = over ? 0 : (long long)(div0 * div1);
  b[5] = over ? 1 : 2;
  return over;
}

// linear leaf index of a point in a valid box
__device__ inline uint64_t sv_cell(const float4& pt, float leaf, const long long* __restrict__ b) {
  const float inv = 1.0f / leaf;
  const int mb0 = (int)b[0], mb1 = (int)b[1], mb2 = (int)b[2];
  const long long i0 = (long long)(floorf(pt.x * inv) - (float)mb0), i1 = (long long)(floorf(pt.y * inv) - (float)mb1),
                  i2 = (long long)(floorf(pt.z * inv) - (float)mb2);
  return (uint64_t)(i0 + i1 * b[3] + i2 * b[4]);
}
#endif

}  // namespace loam
}  // namespace pcm
