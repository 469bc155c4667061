// loam_device.h -- what the LOAM scan-to-map kernels (loam.hip) and their host side (loam_api.hip) share, and what the LOAM
// operators share among themselves: the context check, the stores, the target's owner, the point arena.
#pragma once

#include <algorithm>

#include "host_util.h"
#include "loam_step.h"
#include "pcm_device.h"
#include "table_search.h"

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
// loam_submap.hip: the caller of pcm_loam_map_export / pcm_loam_global_map with a device buffer has drained the stream
void loam_export_waited(pcm_ctx* c);

// loam_dynmap.hip: what the tile builder (loam_tiles.hip) hands the map-tile store.  One tile: its box, its index pair and its
// points, which are cells [first, first + n) of its list's cloud.  loam_tiles_replace empties both lists and the selection as
// pcm_loam_tile_clear does and stores the new tiles; the clouds (device memory, n_cells[m] points) are copied into the arenas on the
// context's stream, device to device, and may be released in stream order on return.  A failure leaves the store as it was.
// loam_tiles_writable: PCM_OK when the context is the only holder of its tile store, else PCM_ERR_UNSUPPORTED with a text that names
// `call` (pcm_loam_tile_share; a shared store is immutable).  The builder asks before any device work; loam_tiles_replace asks again.
struct BuiltTile { double box[6]; int32_t ix, iy; uint32_t first, n; };
int loam_tiles_writable(pcm_ctx* c, const char* call);
int loam_tiles_replace(pcm_ctx* c, const BuiltTile* const tiles[2], const size_t n_tiles[2], const float4* const cells[2], const size_t n_cells[2]);

// loam_features.hip: the context's last front-end features.  gen: bumps whenever the output array is rewritten
bool loam_features_last_out(pcm_ctx* c, const float4** out, uint32_t* n_c, uint32_t* n_s, uint64_t* gen);

}  // namespace loam
}  // namespace pcm
