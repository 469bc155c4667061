// loam_submap.hip -- LOAM key-frame store and surrounding-key-frame submap on the device (include/pcm_amd.h, pcm_loam_keyframe_*,
// pcm_loam_submap_*, pcm_loam_global_* and pcm_loam_map_export): jueying_slam's saveKeyFramesAndFactor clouds (mapOptmization.cpp:1779-1846), correctPoses (:1886-1917),
// extractSurroundingKeyFrames (:1153-1230), transformPointCloud (:447-470) and loopFindNearKeyframes (:972-1018).
//
// Store: one growing float4 arena (x, y, z, intensity; body frame) for the corner clouds of all key frames and one for the surf
// clouds, per-key-frame offsets and counts on the host, the 3 x 4 float pose matrices on the device.  A matrix is loam_step.h's
// pose_matrix evaluated on the HOST when a pose is added or replaced (48 bytes uploaded): the device transform is then
// contraction-free float arithmetic that a test can check bit for bit, whereas the device library's sin / cos need not agree with
// libm in the last bit.
// Submap: the selection runs on the host (loam_submap.h; microseconds); its entry table (arena offset, first output position,
// matrix) is uploaded, k_sm_gather transforms and concatenates the selected clouds and reduces their bounding boxes, and the two
// VoxelGrids run as one segmented pass (segment 0 corner, 1 surf) through voxel_grid.h's segmented pipeline, the one the front end
// (loam_features.hip) runs.  The averaged cells are written
// straight into the context's two target clouds (loam_target_reserve / loam_target_commit); no float atomics anywhere, so two
// updates of the same state give the same bits.
// laserCloudMapContainer (the reference's cache of transformed clouds) never changes a result and is not kept: when the selection,
// the poses and the leaves equal those of the previous update the call does nothing at all, which is the common case at LiDAR rate.
// Near-key-frame cloud (pcm_loam_submap_near, pcm_loam_submap_near_dev and the clouds pcm_loam_loop_verify feeds its NDT with):
// one path, queue_near -- pcm_loam_submap_near is pcm_loam_submap_near_dev with a host buffer.  It is the update's pass with one
// segment, bit for bit (tests/golden/loam_near_parent.json holds the clouds of the two-segment pass it replaced), through
// voxel_grid.h's single-segment pipeline: 32-bit keys (half the radix passes; the sort stays stable, so a cell's run keeps its
// input order and its sum its bits), fewer launches; without a leaf the gather writes the result itself.
// Global map and saved map (pcm_loam_global_map, pcm_loam_map_export; publishGlobalMap :547-590 and the clouds of :524-542): the
// near pass on publishGlobalMap's selection (select_global) in a workspace of its own whose per-point arrays live for one call,
// with a gather that leaves one partial bounding box per workgroup instead of atomics per wave (k_gm_gather, vg::fold_boxes; the
// same bits); the export is that gather alone, writing transformPointCloud's values as they are.  DESIGN.md section 20.
// The two passes share the entry table (build_entries), the gather and the workspace type, and run voxel_grid.h's two pipelines
// on purpose: the update sorts 64-bit (segment, leaf) keys, the near pass 32-bit keys.  One pipeline for both would change the
// number of radix passes of one of them, and with it its speed.
#include "host_util.h"
#include "loam_device.h"
#include "loam_submap.h"
#include "voxel_grid.h"

#include <chrono>
#include <cstring>
#include <vector>

using namespace pcm;
using namespace pcm::loam;

namespace {

// one cloud of one selected key frame: points [src, src + count) of an arena go to output positions [first, first + count)
struct SmEntry {
  uint32_t src;     // first point in its arena
  uint32_t first;   // first output position (ascending over the table; an empty entry shares it with its successor)
  uint32_t mat;     // key frame whose pose matrix applies
  uint32_t flags;   // bit 0: surf arena, bit 1: VoxelGrid segment 1
};

// One lane per point of the concatenated selection.  The lane finds its entry by a binary search over the first positions: the
// trip count is the same in every lane (it depends on the table size only) and a key frame's cloud holds thousands of points, so
// nearly every wave reads one entry and one matrix (wave-uniform addresses, served by one cache line); the arena read and the
// output write are contiguous 16-byte accesses per lane.  transformPointCloud :462-466: T(r,0) x + T(r,1) y + T(r,2) z + T(r,3),
// left to right in float (built with -ffp-contract=off), intensity copied.
// kDirect (the near pass without a leaf): every point is its own cell, and the mean of one value v is
// (float)((0.0 + (double)v) / 1.0): v itself with a negative zero turned positive, which v + 0.0f is as well; the lane writes that
// to the result and nothing else runs.
// point gg < N of the concatenated selection under its key frame's matrix; *flags = its entry's
__device__ __forceinline__ float4 sm_point(const float4* __restrict__ corner_arena, const float4* __restrict__ surf_arena, const float* __restrict__ mats,
                                           const SmEntry* __restrict__ ent, uint32_t n_ent, uint32_t gg, uint32_t* flags) {
  const SmEntry e = ent[table_row_of(&ent->first, sizeof(SmEntry) / 4, n_ent, gg)];   // never an empty entry: the last row at or before gg
  const float4* __restrict__ arena = (e.flags & 1u) ? surf_arena : corner_arena;
  const float4 p = arena[(size_t)e.src + (gg - e.first)];
  const float* __restrict__ T = mats + 12 * (size_t)e.mat;
  float4 q;
  q.x = T[0] * p.x + T[1] * p.y + T[2] * p.z + T[3];
  q.y = T[4] * p.x + T[5] * p.y + T[6] * p.z + T[7];
  q.z = T[8] * p.x + T[9] * p.y + T[10] * p.z + T[11];
  q.w = p.w;
  *flags = e.flags;
  return q;
}

template <bool kDirect>
__global__ void __launch_bounds__(256) k_sm_gather(const float4* __restrict__ corner_arena, const float4* __restrict__ surf_arena, const float* __restrict__ mats,
                                                   const SmEntry* __restrict__ ent, uint32_t n_ent, uint32_t N, float4* __restrict__ out,
                                                   unsigned int* __restrict__ mm) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = g < N;
  uint32_t flags;
  const float4 q = sm_point(corner_arena, surf_arena, mats, ent, n_ent, valid ? g : N - 1, &flags);
  if (kDirect) {
    if (valid) out[g] = make_float4(q.x + 0.0f, q.y + 0.0f, q.z + 0.0f, q.w + 0.0f);
  } else {
    if (valid) out[g] = q;
    vg::wave_minmax(valid, (flags >> 1) & 1u, q, mm);
  }
}

// The gather of the global pass (pcm_loam_global_map, pcm_loam_map_export): k_sm_gather's points, at most kGmBlocks workgroups
// striding over them.  kBox: no atomics -- every lane keeps the box of its points in registers, a butterfly folds the wave's, LDS
// the workgroup's four, and the workgroup stores one partial box (6 ordered words, min then max) that vg::fold_boxes folds into
// the words the key kernel reads.  Min and max are exact in any order, so box, keys and cells are k_sm_gather<false>'s bit for bit.
// !kBox (the export): transformPointCloud's value as it is -- no + 0.0f, a negative zero stays negative -- and nothing else.
constexpr unsigned kGmBlocks = 2048;

template <bool kBox>
__global__ void __launch_bounds__(256) k_gm_gather(const float4* __restrict__ corner_arena, const float4* __restrict__ surf_arena, const float* __restrict__ mats,
                                                   const SmEntry* __restrict__ ent, uint32_t n_ent, uint32_t N, float4* __restrict__ out,
                                                   unsigned int* __restrict__ part) {
  unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  // N < 2^31 and a stride of at most 2^19: base does not wrap
  for (uint32_t base = blockIdx.x * 256u; base < N; base += gridDim.x * 256u) {
    const uint32_t g = base + threadIdx.x;
    if (g >= N) continue;
    uint32_t flags;
    const float4 q = sm_point(corner_arena, surf_arena, mats, ent, n_ent, g, &flags);
    out[g] = q;
    if (kBox) {
      const float c[3] = {q.x, q.y, q.z};
      for (int a = 0; a < 3; a++) { const unsigned int o = f2ord(c[a]); lo[a] = min(lo[a], o); hi[a] = max(hi[a], o); }
    }
  }
  if (!kBox) return;
  vg::fold_block_box(lo, hi, part + 6 * blockIdx.x);
}

// What the totals of a pass look like on the host (vg::Work::small): [0] cells, [1] valid elements, [2] index overflow; the update
// reads on: [4..5] cells per segment, [6..7] first cell of the segment.
constexpr int kNearWords = 3, kUpdateWords = vg::Work::kSmallWords + 4;

// the update's elements: N gathered points, the first n0 of them segment 0 (corner), the others segment 1 (surf).  The cells of
// segment 0 go to out0, those of segment 1 to out1, each in leaf-index order.
struct UpdateElems {
  static constexpr int kFields = 4;
  const float4* in; uint32_t N, n0; float leaf0, leaf1;
  uint32_t* small; float4* out0; float4* out1;
  __device__ int fields() const { return 4; }
  __device__ float4 fetch(uint32_t g, uint32_t) const { return in[g]; }
  __device__ bool slot(uint32_t, uint32_t j, uint32_t* g) const { *g = j; return j < N; }
  __device__ vg::Elem elem(uint32_t, uint32_t j) const { return vg::Elem{true, j >= n0 ? 1u : 0u, j, in[j]}; }
  __device__ float leaf(uint32_t seg) const { return seg ? leaf1 : leaf0; }
  __device__ void overflow(uint32_t) const { small[2] = 1u; }   // every writer stores 1
  __device__ void put(uint32_t cell, const float (&m)[kFields]) const {
    const uint32_t n_seg0 = small[vg::Work::kSmallWords];
    const float4 r = make_float4(m[0], m[1], m[2], m[3]);
    if (cell < n_seg0) out0[cell] = r; else out1[cell - n_seg0] = r;
  }
};

// the near and global passes' elements: one segment, every point counts, the cells go to one array
struct NearElems {
  static constexpr int kFields = 4;
  const float4* in; float4* out;
  __device__ int fields() const { return 4; }
  __device__ float4 fetch(uint32_t g, uint32_t) const { return in[g]; }
  __device__ bool point(uint32_t g, float4* pt) const { *pt = in[g]; return true; }
  __device__ void put(uint32_t cell, const float (&m)[kFields]) const { out[cell] = make_float4(m[0], m[1], m[2], m[3]); }
};

// the context's LOAM source as PointXYZI: corner features to dst_c, surf features to dst_s
__global__ void k_sm_store_source(const float4* __restrict__ feats, const float4* __restrict__ xyzi, const float* __restrict__ inten, uint32_t n_c, uint32_t n_s,
                                  float4* __restrict__ dst_c, float4* __restrict__ dst_s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_c + n_s) return;
  float4 p;
  if (xyzi) p = xyzi[i];
  else { p = feats[i]; p.w = inten ? inten[i] : 0.f; }
  if (i < n_c) dst_c[i] = p; else dst_s[i - n_c] = p;
}

// device workspace of one gather + VoxelGrid pass.  The update pass (segmented) sorts 64-bit keys and keeps the cell heads, two
// boxes and the totals of two segments; its cells go to the context's target.  The near pass sorts 32-bit keys and owns a cell
// array.  The near pass has two workspaces, so that the two clouds of a loop verification are in flight together.
// The global pass (one_shot) is the near pass on a selection of up to 2^31 points: its per-point arrays are sized exactly, hold
// only what the call at hand needs and are released when it returns; the entry table and the partial boxes of its gather (a few
// bytes per key frame) stay.
struct SmWork {
  DevBuf<char> buf;
  DevBuf<SmEntry> ent{"key-frame entry table"};
  DevBuf<unsigned int> part{"partial boxes"};   // one_shot: [kGmBlocks][6]
  size_t n_cap = 0;
  float4* d_in = nullptr;        // inside buf (sm_carve): the gathered points
  float4* d_cells = nullptr;     //                          the pass's own cells
  vg::Work grid{};               // the VoxelGrid's arrays, inside buf
  PinnedBuf<uint32_t> h_small;
  PinnedBuf<SmEntry> h_ent;      // staging of the entry table
  bool in_flight = false;        // the last near pass was left without a wait: its staging is not free yet
  bool one_shot = false;

  float4* in() const { return d_in; }
  float4* cells() const { return d_cells; }
};

// buf's layout: [gathered points | own cells | the VoxelGrid's Work].  Over a null base the size query, over buf.p the carve.
struct SmCarve { float4* in; float4* cells; char* grid; size_t bytes; };
SmCarve sm_carve(char* base, size_t n_in, size_t n_cells, size_t grid_bytes) {
  ArenaCarver a(base);
  SmCarve c;
  c.in = a.take<float4>(n_in);
  c.cells = a.take<float4>(n_cells);
  c.grid = a.take<char>(grid_bytes);
  c.bytes = a.used();
  return c;
}

// room for N points and n_ent entries; keys of key_bytes each.  segmented: the head and box arrays and the second segment exist.
// sorted: the arrays of the VoxelGrid exist (a one-shot pass without a leaf has none); own_cells: the cell array does.
int ensure_work(pcm_ctx* c, SmWork* W, size_t N, size_t n_ent, size_t key_bytes, bool segmented, bool sorted, bool own_cells) {
  const size_t words = segmented ? kUpdateWords : kNearWords;
  int rc = W->h_small.reserve(c, words, words);
  if (rc != PCM_OK) return rc;
  if (n_ent > W->h_ent.cap && (rc = W->h_ent.reserve(c, n_ent, n_ent + n_ent / 2 + 16)) != PCM_OK) return rc;
  if ((rc = W->ent.reserve(c, n_ent, W->h_ent.cap)) != PCM_OK) return rc;
  if (W->one_shot && (rc = W->part.reserve(c, 6 * kGmBlocks, 6 * kGmBlocks)) != PCM_OK) return rc;
  if (W->buf && N <= W->n_cap) return PCM_OK;
  if (!sorted && !own_cells) return PCM_OK;   // nothing per point
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  W->buf.release();   // the layout below is for the new sizes alone
  W->n_cap = 0;
  const size_t nc = W->one_shot ? N : N + N / 4 + 1024, ns = sorted ? nc : 0;
  const size_t nseg = segmented ? 2 : 0, n_cells = own_cells ? nc : 1;
  size_t vg_bytes = 0;
  (void)vg::work_layout(nullptr, ns, key_bytes, nseg, &vg_bytes);
  const size_t bytes = sm_carve(nullptr, ns, n_cells, vg_bytes).bytes;
  if ((rc = W->buf.reserve(c, bytes, bytes)) != PCM_OK) return rc;
  const SmCarve at = sm_carve(W->buf.p, ns, n_cells, vg_bytes);
  W->d_in = at.in; W->d_cells = at.cells;
  W->grid = vg::work_layout(at.grid, ns, key_bytes, nseg, &vg_bytes);
  W->n_cap = nc;
  return PCM_OK;
}

// the per-point arrays of a one-shot workspace go when the call returns (hipFree waits for what is queued on them)
struct OneShot {
  SmWork* W;
  ~OneShot() { W->buf.release(); W->n_cap = 0; }
};

struct KeyFrame {
  float pose[6];   // roll, pitch, yaw, x, y, z
  double time;
  size_t off_c, off_s;
  uint32_t n_c, n_s;
};

struct KeyStore {
  std::vector<KeyFrame> kf;
  std::vector<KeyPose> kp;   // what the selection reads
  Arena arena[2] = {Arena("key-frame arena"), Arena("key-frame arena")};   // corner, surf
  DevBuf<float> mats{"key-frame matrices"};   // [K][12]
  uint64_t gen = 1;          // bumps whenever a key frame or a pose changes
  SmWork upd;                // pcm_loam_submap_update
  SmWork ndev[2];            // near clouds: [0] pcm_loam_submap_near, pcm_loam_submap_near_dev and slot 0 of loam_near_queue, [1] slot 1
  SmWork glob;               // pcm_loam_global_map, pcm_loam_map_export: one_shot
  KeyStore() { glob.one_shot = true; }
  // the last update
  bool last_valid = false;
  uint64_t last_gen = 0;
  float last_leaf[2] = {0.f, 0.f};
  std::vector<int32_t> last_keys;
  pcm_loam_submap_result last{};
};

int check_ctx_sm(pcm_ctx* c, KeyStore** ks) {
  return loam_check_store(c, "pcm_loam_keyframe_* / pcm_loam_submap_* need a context created with PCM_MODEL_LOAM", LoamStore::key, ks);
}

void host_matrix(const float* pose6, float* T12) {
  float x[6], T[12], trig[6];
  for (int k = 0; k < 6; k++) x[k] = pose6[k];
  pose_matrix(x, T, trig);
  for (int k = 0; k < 12; k++) T12[k] = T[k];
}

int upload_matrices(pcm_ctx* c, KeyStore* S, size_t first, size_t n) {
  const size_t K = S->kf.size();
  if (12 * K > S->mats.cap || !S->mats) {
    int rc = S->mats.reserve_keep(c, 12 * K, 12 * (K + K / 2 + 256), 0);
    if (rc != PCM_OK) return rc;
    first = 0; n = K;   // a fresh array gets every matrix
  }
  if (n == 0) return PCM_OK;
  std::vector<float> T(12 * n);
  for (size_t i = 0; i < n; i++) host_matrix(S->kf[first + i].pose, T.data() + 12 * i);
  PCM_HIPCK(c, hipMemcpyAsync(S->mats + 12 * first, T.data(), sizeof(float) * 12 * n, hipMemcpyHostToDevice, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

// rows whose `first` holds their count get their first output position
void entry_positions(SmEntry* ent, size_t rows) {
  uint32_t first = 0;
  for (size_t r = 0; r < rows; r++) { const uint32_t n = ent[r].first; ent[r].first = first; first += n; }
}

// The entry table of `keys`, two rows per key frame, into ent.  wrt_key < 0: every key frame under its own pose; else all under
// wrt_key's.  interleaved (near): corner, surf, corner, surf, ... in one segment; else (update) all corner clouds, then all surf
// clouds as segment 1.
void build_entries(const KeyStore* S, const std::vector<int32_t>& keys, int wrt_key, bool interleaved, SmEntry* ent) {
  const size_t E = keys.size();
  for (size_t i = 0; i < E; i++) {
    const KeyFrame& k = S->kf[(size_t)keys[i]];
    const uint32_t mat = wrt_key < 0 ? (uint32_t)keys[i] : (uint32_t)wrt_key;
    ent[interleaved ? 2 * i : i] = SmEntry{(uint32_t)k.off_c, k.n_c, mat, 0u};                           // first: the count for now
    ent[interleaved ? 2 * i + 1 : E + i] = SmEntry{(uint32_t)k.off_s, k.n_s, mat, interleaved ? 1u : 3u};
  }
  entry_positions(ent, 2 * E);
}

// corner and surf points of `keys`; more than 2^31 - 1 together: PCM_ERR_OUT_OF_RANGE
int count_points(pcm_ctx* c, const KeyStore* S, const std::vector<int32_t>& keys, uint64_t* n_c, uint64_t* n_s) {
  *n_c = *n_s = 0;
  for (int32_t k : keys) { *n_c += S->kf[(size_t)k].n_c; *n_s += S->kf[(size_t)k].n_s; }
  if (*n_c + *n_s > 0x7fffffffull) { c->err = "the selected key frames hold more than 2^31 points"; return PCM_ERR_OUT_OF_RANGE; }
  return PCM_OK;
}

// the update's pass: gather + segmented VoxelGrid of W->h_ent[0..n_ent): N points, the first n0 of them segment 0.  Cells of
// segment 0 -> out0, of segment 1 -> out1; the counts and the overflow flag come back through W->h_small.
int run_pass(pcm_ctx* c, KeyStore* S, SmWork* W, size_t n_ent, uint32_t N, uint32_t n0, float leaf0, float leaf1, float4* out0, float4* out1) {
  hipStream_t st = c->stream;
  SmEntry* d_ent = W->ent;
  const vg::Work& V = W->grid;
  PCM_HIPCK(c, hipMemcpyAsync(d_ent, W->h_ent, sizeof(SmEntry) * n_ent, hipMemcpyHostToDevice, st));
  vg::clear(st, V);
  k_sm_gather<false><<<(N + 255) / 256, 256, 0, st>>>(S->arena[0].d, S->arena[1].d, S->mats, d_ent, (uint32_t)n_ent, N, W->in(), V.mm);
  PCM_HIPCK(c, hipGetLastError());
  const int rc = vg::seg_cells(&c->err, st, UpdateElems{W->in(), N, n0, leaf0, leaf1, V.small, out0, out1}, 1u, N, N, V);
  if (rc != PCM_OK) return rc;
  PCM_HIPCK(c, hipMemcpyAsync(W->h_small, V.small, sizeof(uint32_t) * kUpdateWords, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipStreamSynchronize(st));
  return PCM_OK;
}

int check_sparams(pcm_ctx* c, const pcm_loam_submap_params& p) {
  if (!(p.search_radius > 0.f) || !finite_f_3e38(p.search_radius)) { c->err = "search_radius must be a positive number"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.keypose_density > 0.f) || !finite_f_3e38(p.keypose_density)) { c->err = "keypose_density must be a positive number"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.corner_leaf >= 0.f) || !(p.surf_leaf >= 0.f) || !finite_f_3e38(p.corner_leaf) || !finite_f_3e38(p.surf_leaf)) {
    c->err = "corner_leaf and surf_leaf must be >= 0 (0: no down-sampling)"; return PCM_ERR_INVALID_ARGUMENT;
  }
  if (!(p.recent_window_s == p.recent_window_s)) { c->err = "recent_window_s must be a number"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

// the arguments of a near cloud for a store of K key frames; K == 0 passes once search_num and leaf are sound (the entries then
// decide what an empty store means)
int check_near_args(pcm_ctx* c, int K, int key, int search_num, int wrt_key, float leaf, const char* who) {
  if (search_num < 0) { c->err = "search_num must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(leaf >= 0.f) || !finite_f_3e38(leaf)) { c->err = "leaf must be >= 0 (0: no down-sampling)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (K == 0) return PCM_OK;
  if (key < 0 || key >= K) { c->err = std::string(who) + ": key outside [0, K)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (wrt_key >= K) { c->err = std::string(who) + ": wrt_key outside [0, K)"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

// Queues the near cloud of `keys` (N >= 1 points) on the context's stream and does not wait.  leaf > 0: the cells go to `dst` (room
// for N; null: the workspace's cell array) and the totals to W->h_small once the stream has drained.  leaf == 0: the N points go
// to dst and W->h_small holds the count at once.  *where = the array written.
int queue_near(pcm_ctx* c, KeyStore* S, SmWork* W, const std::vector<int32_t>& keys, int wrt_key, float leaf, uint32_t N, float4* dst, float4** where) {
  hipStream_t st = c->stream;
  const size_t E = 2 * keys.size();
  int rc = ensure_work(c, W, N, E, sizeof(uint32_t), false, !W->one_shot || leaf > 0.f, !W->one_shot || !dst);
  if (rc != PCM_OK) return rc;
  if (W->in_flight) { PCM_HIPCK(c, hipStreamSynchronize(st)); W->in_flight = false; }
  build_entries(S, keys, wrt_key, true, W->h_ent);
  SmEntry* d_ent = W->ent;
  if (!dst) dst = W->cells();
  *where = dst;
  W->in_flight = true;
  PCM_HIPCK(c, hipMemcpyAsync(d_ent, W->h_ent, sizeof(SmEntry) * E, hipMemcpyHostToDevice, st));
  const unsigned nb = (N + 255) / 256;
  if (!(leaf > 0.f)) {
    k_sm_gather<true><<<nb, 256, 0, st>>>(S->arena[0].d, S->arena[1].d, S->mats, d_ent, (uint32_t)E, N, dst, nullptr);
    PCM_HIPCK(c, hipGetLastError());
    W->h_small[0] = N; W->h_small[1] = N; W->h_small[2] = 0u;
    return PCM_OK;
  }
  const vg::Work& V = W->grid;
  if (W->one_shot) {
    const unsigned gb = std::min(nb, kGmBlocks);
    k_gm_gather<true><<<gb, 256, 0, st>>>(S->arena[0].d, S->arena[1].d, S->mats, d_ent, (uint32_t)E, N, W->in(), W->part);
    vg::fold_boxes(st, W->part, gb, V);
  } else {
    vg::clear(st, V);
    k_sm_gather<false><<<nb, 256, 0, st>>>(S->arena[0].d, S->arena[1].d, S->mats, d_ent, (uint32_t)E, N, W->in(), V.mm);
  }
  if ((rc = vg::single_cells(&c->err, st, NearElems{W->in(), dst}, N, leaf, V)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipMemcpyAsync(W->h_small, V.small, sizeof(uint32_t) * kNearWords, hipMemcpyDeviceToHost, st));
  return PCM_OK;
}

// The near cloud of `keys` (N >= 1 points) through workspace W into the caller's host or device buffer of cap points; `who` in
// the error texts.  *n_out is set before a "capacity too small" error.
int emit_near(pcm_ctx* c, KeyStore* S, SmWork* W, const char* who, const std::vector<int32_t>& keys, int wrt_key, float leaf, uint32_t N, void* out, size_t cap,
              int memory, size_t* n_out) {
  int rc = PCM_OK;
  const std::string too_small = std::string(who) + ": capacity too small (the count is set)";
  const bool counted = !(leaf > 0.f);   // without a leaf the count is known before anything runs
  if (counted) {
    if (n_out) *n_out = N;
    if (N > cap || !out) { c->err = too_small; return PCM_ERR_INVALID_ARGUMENT; }
  }
  PCM_HIPCK(c, hipSetDevice(c->device));
  // a device buffer with room for every input point takes the result in place
  const bool in_place = memory == PCM_MEM_DEVICE && out && cap >= N && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  float4* where = nullptr;
  if ((rc = queue_near(c, S, W, keys, wrt_key, leaf, N, in_place ? static_cast<float4*>(out) : nullptr, &where)) != PCM_OK) return rc;
  size_t m = N;
  if (!counted) {
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the count has to come back
    W->in_flight = false;
    if (W->h_small[2]) { c->err = "leaf size too small for the extent of the cloud (index overflow)"; return PCM_ERR_OUT_OF_RANGE; }
    m = W->h_small[0];
    if (n_out) *n_out = m;
    if (m > cap || (!out && m)) { c->err = too_small; return PCM_ERR_INVALID_ARGUMENT; }
  }
  if (in_place || m == 0) return PCM_OK;
  if (memory == PCM_MEM_DEVICE) {
    PCM_HIPCK(c, hipMemcpyAsync(out, where, sizeof(float4) * m, hipMemcpyDeviceToDevice, c->stream));
    W->in_flight = true;
    return PCM_OK;
  }
  PCM_HIPCK(c, hipMemcpyAsync(out, where, sizeof(float4) * m, hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  W->in_flight = false;
  return PCM_OK;
}

// pcm_loam_submap_near (memory = PCM_MEM_HOST) and pcm_loam_submap_near_dev, `who` in the error texts
int near_cloud(pcm_ctx* c, const char* who, int key, int search_num, int wrt_key, float leaf, void* out, size_t cap, int memory, size_t* n_out) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  if (n_out) *n_out = 0;
  if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  const int K = (int)S->kf.size();
  if ((rc = check_near_args(c, K, key, search_num, wrt_key, leaf, who)) != PCM_OK) return rc;
  if (K == 0) return PCM_OK;   // nothing to assemble
  const std::vector<int32_t> keys = select_near(K, key, search_num);
  uint64_t n_c = 0, n_s = 0;
  if ((rc = count_points(c, S, keys, &n_c, &n_s)) != PCM_OK) return rc;
  const uint32_t N = (uint32_t)(n_c + n_s);
  if (N == 0) return PCM_OK;
  return emit_near(c, S, &S->ndev[0], who, keys, wrt_key, leaf, N, out, cap, memory, n_out);
}

int check_gparams(pcm_ctx* c, const pcm_loam_global_params& p) {
  if (!(p.search_radius > 0.f) || !finite_f_3e38(p.search_radius)) { c->err = "search_radius must be a positive number"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.keypose_density > 0.f) || !finite_f_3e38(p.keypose_density)) { c->err = "keypose_density must be a positive number"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.leaf >= 0.f) || !finite_f_3e38(p.leaf)) { c->err = "leaf must be >= 0 (0: no down-sampling)"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

// publishGlobalMap's selection on the store (K >= 1); an overflow of the pose grid: PCM_ERR_OUT_OF_RANGE
int global_selection(pcm_ctx* c, const KeyStore* S, const pcm_loam_global_params& p, SubmapSelection* sel) {
  *sel = select_global(S->kp.data(), (int)S->kf.size(), p.search_radius, p.keypose_density);
  if (sel->status == 0) return PCM_OK;
  c->err = "keypose_density too small for the extent of the key poses (index overflow)";
  return PCM_ERR_OUT_OF_RANGE;
}

// the entry table of pcm_loam_map_export: one row per cloud, in the order the reference concatenates them
size_t export_entries(const KeyStore* S, int which, int first, int n, SmEntry* ent) {
  size_t r = 0;
  for (int arena = which == 1 ? 1 : 0; arena <= (which == 0 ? 0 : 1); arena++)
    for (int i = first; i < first + n; i++) {
      const KeyFrame& k = S->kf[(size_t)i];
      ent[r++] = arena ? SmEntry{(uint32_t)k.off_s, k.n_s, (uint32_t)i, 1u} : SmEntry{(uint32_t)k.off_c, k.n_c, (uint32_t)i, 0u};   // first: the count for now
    }
  entry_positions(ent, r);
  return r;
}

}  // namespace

namespace pcm {
namespace loam {
bool loam_keyframe_cloud(pcm_ctx* c, int key, int which, const float4** pts, uint32_t* n) {
  const KeyStore* S = loam_store<KeyStore>(c, LoamStore::key, false);
  if (!S || key < 0 || (size_t)key >= S->kf.size()) return false;
  const KeyFrame& k = S->kf[(size_t)key];
  *pts = S->arena[which ? 1 : 0].d + (which ? k.off_s : k.off_c);
  *n = which ? k.n_s : k.n_c;
  return true;
}

bool loam_keyframe_pose(pcm_ctx* c, int key, float pose6[6]) {
  const KeyStore* S = loam_store<KeyStore>(c, LoamStore::key, false);
  if (!S || key < 0 || (size_t)key >= S->kf.size()) return false;
  for (int a = 0; a < 6; a++) pose6[a] = S->kf[(size_t)key].pose[a];
  return true;
}

int loam_keyposes(pcm_ctx* c, const KeyPose** kp) {
  const KeyStore* S = loam_store<KeyStore>(c, LoamStore::key, false);
  *kp = S ? S->kp.data() : nullptr;
  return S ? (int)S->kf.size() : 0;
}
int loam_near_queue(pcm_ctx* c, int slot, int key, int search_num, int wrt_key, float leaf, NearCloud* out) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  out->pts = nullptr; out->n_in = 0; out->h_small = nullptr;
  const int K = (int)S->kf.size();
  if (K == 0) { c->err = "the key-frame store is empty"; return PCM_ERR_INVALID_ARGUMENT; }
  if ((rc = check_near_args(c, K, key, search_num, wrt_key, leaf, "pcm_loam_loop_verify")) != PCM_OK) return rc;
  const std::vector<int32_t> keys = select_near(K, key, search_num);
  uint64_t n_c = 0, n_s = 0;
  if ((rc = count_points(c, S, keys, &n_c, &n_s)) != PCM_OK) return rc;
  const uint32_t N = (uint32_t)(n_c + n_s);
  if (N == 0) return PCM_OK;   // every selected cloud is empty
  PCM_HIPCK(c, hipSetDevice(c->device));
  SmWork* W = &S->ndev[slot ? 1 : 0];
  float4* where = nullptr;
  if ((rc = queue_near(c, S, W, keys, wrt_key, leaf, N, nullptr, &where)) != PCM_OK) return rc;
  out->pts = where; out->n_in = N; out->h_small = W->h_small;
  return PCM_OK;
}

void loam_near_waited(pcm_ctx* c) {
  KeyStore* S = loam_store<KeyStore>(c, LoamStore::key, false);
  if (S) S->ndev[0].in_flight = S->ndev[1].in_flight = false;
}

void loam_export_waited(pcm_ctx* c) {
  KeyStore* S = loam_store<KeyStore>(c, LoamStore::key, false);
  if (S) S->glob.in_flight = false;
}
}  // namespace loam
}  // namespace pcm

extern "C" {

void pcm_loam_default_submap_params(pcm_loam_submap_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->search_radius = 50.0f;     // utility.h:282
  p->keypose_density = 1.0f;    // utility.h:283
  p->corner_leaf = 0.2f;        // utility.h:271
  p->surf_leaf = 0.2f;          // utility.h:272
  p->recent_window_s = 10.0;    // mapOptmization.cpp:1174
}

int pcm_loam_keyframe_add(pcm_ctx* c, const float pose6[6], double time, const void* corner, size_t n_corner, const void* surf, size_t n_surf, size_t stride,
                          int memory) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  if (!pose6) { c->err = "null pose"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int k = 0; k < 6; k++) if (!finite_f_3e38(pose6[k])) { c->err = "the pose must be finite"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(time == time)) { c->err = "the time must be a number"; return PCM_ERR_INVALID_ARGUMENT; }
  const bool from_source = !corner && !surf;
  const float4* feats = nullptr; const float4* xyzi = nullptr; const float* inten = nullptr;
  uint32_t sc = 0, ss = 0;
  if (from_source) {
    const int sv = loam_source_view(c, &feats, &sc, &ss, &xyzi, &inten);
    if (sv == 1) { c->err = "pcm_loam_keyframe_add without clouds needs a LOAM source (pcm_loam_frame_begin / pcm_loam_set_source)"; return PCM_ERR_NO_INPUT; }
    if (sv != 0) {
      c->err = "pcm_loam_keyframe_add without clouds: the front end has processed another frame on this context since pcm_loam_frame_begin "
               "(pcm_loam_extract_features or a failed frame), so the source's intensities are gone; add the key frame before that, or pass the clouds";
      return PCM_ERR_NO_INPUT;
    }
    n_corner = sc; n_surf = ss;
  } else {
    if ((!corner && n_corner) || (!surf && n_surf)) { c->err = "null point buffer"; return PCM_ERR_INVALID_ARGUMENT; }
    if (stride < 3 * sizeof(float) || (stride % sizeof(float)) != 0) { c->err = "stride must be a multiple of 4 and >= 12 bytes"; return PCM_ERR_INVALID_ARGUMENT; }
    if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  }
  if (n_corner > 0x3fffffffull || n_surf > 0x3fffffffull || S->arena[0].n + n_corner > 0xffffffffull || S->arena[1].n + n_surf > 0xffffffffull) {
    c->err = "key-frame store too large"; return PCM_ERR_INVALID_ARGUMENT;
  }
  PCM_HIPCK(c, hipSetDevice(c->device));
  if ((rc = S->arena[0].reserve(c, n_corner)) != PCM_OK || (rc = S->arena[1].reserve(c, n_surf)) != PCM_OK) return rc;
  float4* dc = S->arena[0].d + S->arena[0].n;
  float4* ds = S->arena[1].d + S->arena[1].n;
  if (from_source) {
    const uint32_t n = (uint32_t)(n_corner + n_surf);
    if (n) {
      k_sm_store_source<<<(n + 255) / 256, 256, 0, c->stream>>>(feats, xyzi, inten, (uint32_t)n_corner, (uint32_t)n_surf, dc, ds);
      PCM_HIPCK(c, hipGetLastError());
    }
  } else {
    if ((rc = load_xyzw_rows(c, corner, n_corner, stride, memory, true, dc)) != PCM_OK) return rc;
    if ((rc = load_xyzw_rows(c, surf, n_surf, stride, memory, true, ds)) != PCM_OK) return rc;
  }
  KeyFrame k{};
  for (int a = 0; a < 6; a++) k.pose[a] = pose6[a];
  k.time = time;
  k.off_c = S->arena[0].n; k.off_s = S->arena[1].n;
  k.n_c = (uint32_t)n_corner; k.n_s = (uint32_t)n_surf;
  S->kf.push_back(k);
  S->kp.push_back(KeyPose{pose6[3], pose6[4], pose6[5], time});
  rc = upload_matrices(c, S, S->kf.size() - 1, 1);   // synchronises: the caller may reuse its buffers on return
  if (rc != PCM_OK) { S->kf.pop_back(); S->kp.pop_back(); return rc; }
  S->arena[0].n += n_corner;
  S->arena[1].n += n_surf;
  S->gen++;
  return PCM_OK;
}

int pcm_loam_keyframe_set_poses(pcm_ctx* c, int first, int n, const float* pose6) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  const long long K = (long long)S->kf.size();
  if (first < 0 || n < 0 || (long long)first + n > K) { c->err = "pcm_loam_keyframe_set_poses: first + n exceeds the number of key frames"; return PCM_ERR_INVALID_ARGUMENT; }
  if (n == 0) return PCM_OK;
  if (!pose6) { c->err = "null poses"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int i = 0; i < 6 * n; i++) if (!finite_f_3e38(pose6[i])) { c->err = "the poses must be finite"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  for (int i = 0; i < n; i++) {
    KeyFrame& k = S->kf[(size_t)(first + i)];
    for (int a = 0; a < 6; a++) k.pose[a] = pose6[6 * i + a];
    KeyPose& q = S->kp[(size_t)(first + i)];
    q.x = k.pose[3]; q.y = k.pose[4]; q.z = k.pose[5];
  }
  S->gen++;
  return upload_matrices(c, S, (size_t)first, (size_t)n);
}

int pcm_loam_keyframe_count(pcm_ctx* c) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  return (int)S->kf.size();
}

int pcm_loam_keyframe_clear(pcm_ctx* c) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  S->kf.clear(); S->kp.clear();
  S->arena[0].n = S->arena[1].n = 0;   // the arenas keep their memory
  S->gen++;
  S->last_valid = false;
  return PCM_OK;
}

int pcm_loam_keyframe_get(pcm_ctx* c, int key, float* corner, size_t cap_corner, float* surf, size_t cap_surf, size_t* n_corner, size_t* n_surf) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  if (n_corner) *n_corner = 0;
  if (n_surf) *n_surf = 0;
  if (key < 0 || (size_t)key >= S->kf.size()) { c->err = "pcm_loam_keyframe_get: key outside [0, K)"; return PCM_ERR_INVALID_ARGUMENT; }
  const KeyFrame& k = S->kf[(size_t)key];
  if (n_corner) *n_corner = k.n_c;
  if (n_surf) *n_surf = k.n_s;
  if ((corner && cap_corner < k.n_c) || (surf && cap_surf < k.n_s)) { c->err = "pcm_loam_keyframe_get: capacity too small (the counts are set)"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  if (corner && k.n_c) PCM_HIPCK(c, hipMemcpyAsync(corner, S->arena[0].d + k.off_c, sizeof(float4) * k.n_c, hipMemcpyDeviceToHost, c->stream));
  if (surf && k.n_s) PCM_HIPCK(c, hipMemcpyAsync(surf, S->arena[1].d + k.off_s, sizeof(float4) * k.n_s, hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

int pcm_loam_submap_update(pcm_ctx* c, const pcm_loam_submap_params* params, double time_cur, pcm_loam_submap_result* result) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  if (!result) { c->err = "null result"; return PCM_ERR_INVALID_ARGUMENT; }
  pcm_loam_submap_params p;
  if (params) p = *params; else pcm_loam_default_submap_params(&p);
  if ((rc = check_sparams(c, p)) != PCM_OK) return rc;
  if (!(time_cur == time_cur)) { c->err = "time_cur must be a number"; return PCM_ERR_INVALID_ARGUMENT; }
  std::memset(result, 0, sizeof(*result));
  const int K = (int)S->kf.size();
  if (K == 0) return PCM_OK;   // extractSurroundingKeyFrames :1226
  SubmapSelection sel = select_surrounding(S->kp.data(), K, p.search_radius, p.keypose_density, time_cur, p.recent_window_s);
  pcm_loam_submap_result r{};
  r.num_keyframes = K;
  r.num_near = sel.num_near;
  if (sel.status != 0) {
    r.status = PCM_ERR_OUT_OF_RANGE;
    *result = r;
    c->err = "keypose_density too small for the extent of the key poses (index overflow)";
    return PCM_ERR_OUT_OF_RANGE;
  }
  r.num_pose_leaves = sel.num_pose_leaves;
  r.num_selected = (int32_t)sel.keys.size();
  r.num_skipped = sel.num_skipped;
  const float4 *tc = nullptr, *ts = nullptr;
  uint32_t tnc = 0, tns = 0;
  if (S->last_valid && S->last_gen == S->gen && S->last_leaf[0] == p.corner_leaf && S->last_leaf[1] == p.surf_leaf && S->last_keys == sel.keys &&
      loam_target_view(c, TargetOwner::submap, &tc, &tnc, &ts, &tns)) {
    // same key frames in the same order under the same poses and leaves: the maps are the ones the context already holds
    r.num_corner_in = S->last.num_corner_in; r.num_surf_in = S->last.num_surf_in;
    r.num_corner_map = S->last.num_corner_map; r.num_surf_map = S->last.num_surf_map;
    r.rebuilt = 0;
    r.status = PCM_OK;
    *result = r;
    return PCM_OK;
  }
  PCM_HIPCK(c, hipSetDevice(c->device));
  S->last_valid = false;
  const size_t E = sel.keys.size();
  uint64_t n_c = 0, n_s = 0;
  if ((rc = count_points(c, S, sel.keys, &n_c, &n_s)) != PCM_OK) return rc;
  float4 *out_c = nullptr, *out_s = nullptr;
  if ((rc = loam_target_reserve(c, (size_t)n_c, (size_t)n_s, &out_c, &out_s)) != PCM_OK) return rc;
  r.num_corner_in = (int32_t)n_c; r.num_surf_in = (int32_t)n_s;
  const uint32_t N = (uint32_t)(n_c + n_s);
  if ((rc = ensure_work(c, &S->upd, N, 2 * E, sizeof(uint64_t), true, true, false)) != PCM_OK) return rc;
  if (N > 0) {
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the pinned staging of an earlier pass is free again
    build_entries(S, sel.keys, -1, false, S->upd.h_ent);
    if ((rc = run_pass(c, S, &S->upd, 2 * E, N, (uint32_t)n_c, p.corner_leaf, p.surf_leaf, out_c, out_s)) != PCM_OK) return rc;
    if (S->upd.h_small[2]) {
      r.status = PCM_ERR_OUT_OF_RANGE;
      *result = r;
      c->err = "leaf size too small for the extent of the submap (index overflow)";
      return PCM_ERR_OUT_OF_RANGE;
    }
    r.num_corner_map = (int32_t)S->upd.h_small[vg::Work::kSmallWords];
    r.num_surf_map = (int32_t)S->upd.h_small[vg::Work::kSmallWords + 1];
  }
  loam_target_commit(c, (uint32_t)r.num_corner_map, (uint32_t)r.num_surf_map, TargetOwner::submap);
  r.rebuilt = 1;
  r.status = PCM_OK;
  S->last_valid = true;
  S->last_gen = S->gen;
  S->last_leaf[0] = p.corner_leaf; S->last_leaf[1] = p.surf_leaf;
  S->last_keys = std::move(sel.keys);
  S->last = r;
  *result = r;
  return PCM_OK;
}

int pcm_loam_submap_near(pcm_ctx* c, int key, int search_num, int wrt_key, float leaf, float* out, size_t cap, size_t* n_out) {
  return near_cloud(c, "pcm_loam_submap_near", key, search_num, wrt_key, leaf, out, cap, PCM_MEM_HOST, n_out);
}

int pcm_loam_submap_near_dev(pcm_ctx* c, int key, int search_num, int wrt_key, float leaf, void* out, size_t cap, int memory, size_t* n_out) {
  return near_cloud(c, "pcm_loam_submap_near_dev", key, search_num, wrt_key, leaf, out, cap, memory, n_out);
}

void pcm_loam_default_global_params(pcm_loam_global_params* p) {
  if (!p) return;
  p->search_radius = 1000.0f;   // utility.h:293
  p->keypose_density = 10.0f;   // utility.h:294
  p->leaf = 1.0f;               // utility.h:295
}

int pcm_loam_global_keys(pcm_ctx* c, const pcm_loam_global_params* params, int32_t* keys, size_t cap, size_t* n) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_global_params p;
  if (params) p = *params; else pcm_loam_default_global_params(&p);
  if ((rc = check_gparams(c, p)) != PCM_OK) return rc;
  if (n) *n = 0;
  if (S->kf.empty()) return PCM_OK;
  SubmapSelection sel;
  if ((rc = global_selection(c, S, p, &sel)) != PCM_OK) return rc;
  if (n) *n = sel.keys.size();
  if (sel.keys.size() > cap || (!keys && !sel.keys.empty())) { c->err = "pcm_loam_global_keys: capacity too small (the count is set)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!sel.keys.empty()) std::memcpy(keys, sel.keys.data(), sizeof(int32_t) * sel.keys.size());
  return PCM_OK;
}

int pcm_loam_global_map(pcm_ctx* c, const pcm_loam_global_params* params, void* out, size_t cap, int memory, pcm_loam_global_result* result) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_global_params p;
  if (params) p = *params; else pcm_loam_default_global_params(&p);
  if ((rc = check_gparams(c, p)) != PCM_OK) return rc;
  if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  pcm_loam_global_result r{};
  if (result) *result = r;
  if (S->kf.empty()) return PCM_OK;   // publishGlobalMap :552
  SubmapSelection sel;
  if ((rc = global_selection(c, S, p, &sel)) != PCM_OK) return rc;
  r.num_near = sel.num_near; r.num_pose_leaves = sel.num_pose_leaves; r.num_skipped = sel.num_skipped; r.num_used = (int32_t)sel.keys.size();
  if (result) *result = r;
  uint64_t n_c = 0, n_s = 0;
  if ((rc = count_points(c, S, sel.keys, &n_c, &n_s)) != PCM_OK) return rc;
  r.points_in = n_c + n_s;
  if (result) *result = r;
  if (r.points_in == 0) return PCM_OK;
  OneShot release{&S->glob};
  size_t m = 0;
  rc = emit_near(c, S, &S->glob, "pcm_loam_global_map", sel.keys, -1, p.leaf, (uint32_t)r.points_in, out, cap, memory, &m);
  r.points_out = m;
  if (result) *result = r;
  return rc;
}

int pcm_loam_map_export(pcm_ctx* c, int which, int first, int n, void* out, size_t cap, int memory, size_t* n_out) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  if (which < 0 || which > 2) { c->err = "pcm_loam_map_export: which must be 0 (corner), 1 (surf) or 2 (corner then surf)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  if (first < 0 || n < 0 || (long long)first + n > (long long)S->kf.size()) { c->err = "pcm_loam_map_export: first + n exceeds the number of key frames"; return PCM_ERR_INVALID_ARGUMENT; }
  if (n_out) *n_out = 0;
  uint64_t total = 0;
  for (int i = first; i < first + n; i++) total += (which != 1 ? S->kf[(size_t)i].n_c : 0u) + (uint64_t)(which != 0 ? S->kf[(size_t)i].n_s : 0u);
  if (total > 0x7fffffffull) { c->err = "the key frames hold more than 2^31 points: export them in parts"; return PCM_ERR_OUT_OF_RANGE; }
  const uint32_t N = (uint32_t)total;
  if (n_out) *n_out = N;
  if (N == 0) return PCM_OK;
  if (N > cap || !out) { c->err = "pcm_loam_map_export: capacity too small (the count is set)"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  SmWork* W = &S->glob;
  OneShot release{W};
  const bool in_place = memory == PCM_MEM_DEVICE && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const size_t E = (size_t)n * (which == 2 ? 2 : 1);
  if ((rc = ensure_work(c, W, N, E, sizeof(uint32_t), false, false, !in_place)) != PCM_OK) return rc;
  if (W->in_flight) { PCM_HIPCK(c, hipStreamSynchronize(c->stream)); W->in_flight = false; }
  export_entries(S, which, first, n, W->h_ent);
  float4* dst = in_place ? static_cast<float4*>(out) : W->cells();
  W->in_flight = true;
  PCM_HIPCK(c, hipMemcpyAsync(W->ent, W->h_ent, sizeof(SmEntry) * E, hipMemcpyHostToDevice, c->stream));
  k_gm_gather<false><<<std::min((N + 255) / 256, kGmBlocks), 256, 0, c->stream>>>(S->arena[0].d, S->arena[1].d, S->mats, W->ent, (uint32_t)E, N, dst, nullptr);
  PCM_HIPCK(c, hipGetLastError());
  if (in_place) return PCM_OK;
  PCM_HIPCK(c, hipMemcpyAsync(out, dst, sizeof(float4) * N, memory == PCM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  if (memory == PCM_MEM_HOST) { PCM_HIPCK(c, hipStreamSynchronize(c->stream)); W->in_flight = false; }
  return PCM_OK;
}

int pcm_loam_global_gather_ms(pcm_ctx* c, const pcm_loam_global_params* params, int variant, float* ms, uint32_t* box6, size_t* workspace_bytes,
                              float* workspace_ms) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_global_params p;
  if (params) p = *params; else pcm_loam_default_global_params(&p);
  if ((rc = check_gparams(c, p)) != PCM_OK) return rc;
  if ((variant != 0 && variant != 1) || !ms) { c->err = "pcm_loam_global_gather_ms: variant must be 0 or 1 and ms not null"; return PCM_ERR_INVALID_ARGUMENT; }
  if (S->kf.empty()) { c->err = "the key-frame store is empty"; return PCM_ERR_INVALID_ARGUMENT; }
  SubmapSelection sel;
  if ((rc = global_selection(c, S, p, &sel)) != PCM_OK) return rc;
  uint64_t n_c = 0, n_s = 0;
  if ((rc = count_points(c, S, sel.keys, &n_c, &n_s)) != PCM_OK) return rc;
  const uint32_t N = (uint32_t)(n_c + n_s);
  if (N == 0) { c->err = "the selected key frames are empty"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  SmWork* W = &S->glob;
  OneShot release{W};
  const size_t E = 2 * sel.keys.size();
  using Clock = std::chrono::steady_clock;
  const Clock::time_point t0 = Clock::now();
  if ((rc = ensure_work(c, W, N, E, sizeof(uint32_t), false, true, false)) != PCM_OK) return rc;
  const Clock::time_point t1 = Clock::now();
  if (workspace_bytes) *workspace_bytes = W->buf.cap;
  PCM_HIPCK(c, hipStreamSynchronize(st));
  W->in_flight = false;
  build_entries(S, sel.keys, -1, true, W->h_ent);
  PCM_HIPCK(c, hipMemcpyAsync(W->ent, W->h_ent, sizeof(SmEntry) * E, hipMemcpyHostToDevice, st));
  unsigned int* mm = W->grid.mm;
  const unsigned nb = (N + 255) / 256, gb = std::min(nb, kGmBlocks);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  PCM_HIPCK(c, hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); c->err = "hipEventCreate failed"; return PCM_ERR_HIP; }
  hipError_t e = hipEventRecord(e0, st);
  if (variant == 0) {
    vg::clear(st, W->grid);
    k_sm_gather<false><<<nb, 256, 0, st>>>(S->arena[0].d, S->arena[1].d, S->mats, W->ent, (uint32_t)E, N, W->in(), mm);
  } else {
    k_gm_gather<true><<<gb, 256, 0, st>>>(S->arena[0].d, S->arena[1].d, S->mats, W->ent, (uint32_t)E, N, W->in(), W->part);
    vg::fold_boxes(st, W->part, gb, W->grid);
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(e1, st);
  if (e == hipSuccess && box6) e = hipMemcpyAsync(box6, mm, 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipEventElapsedTime(ms, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  PCM_HIPCK(c, e);
  const Clock::time_point t2 = Clock::now();
  W->buf.release();   // the stream is idle: what OneShot would do, timed
  if (workspace_ms) *workspace_ms = std::chrono::duration<float, std::milli>((t1 - t0) + (Clock::now() - t2)).count();
  return PCM_OK;
}

int pcm_loam_submap_info(pcm_ctx* c, int32_t* keys, float* corner_in, float* surf_in, float* corner_map, float* surf_map) {
  KeyStore* S = nullptr;
  int rc = check_ctx_sm(c, &S);
  if (rc != PCM_OK) return rc;
  const float4 *tc = nullptr, *ts = nullptr;
  uint32_t tnc = 0, tns = 0;
  if (!S->last_valid || !loam_target_view(c, TargetOwner::submap, &tc, &tnc, &ts, &tns)) { c->err = "pcm_loam_submap_info: the context's target is not the result of pcm_loam_submap_update"; return PCM_ERR_NO_INPUT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  if (keys && !S->last_keys.empty()) std::memcpy(keys, S->last_keys.data(), sizeof(int32_t) * S->last_keys.size());
  const size_t n_c = (size_t)S->last.num_corner_in, n_s = (size_t)S->last.num_surf_in;
  if (corner_in && n_c) PCM_HIPCK(c, hipMemcpyAsync(corner_in, S->upd.in(), sizeof(float4) * n_c, hipMemcpyDeviceToHost, c->stream));
  if (surf_in && n_s) PCM_HIPCK(c, hipMemcpyAsync(surf_in, S->upd.in() + n_c, sizeof(float4) * n_s, hipMemcpyDeviceToHost, c->stream));
  if (corner_map && tnc) PCM_HIPCK(c, hipMemcpyAsync(corner_map, tc, sizeof(float4) * tnc, hipMemcpyDeviceToHost, c->stream));
  if (surf_map && tns) PCM_HIPCK(c, hipMemcpyAsync(surf_map, ts, sizeof(float4) * tns, hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

}  // extern "C"
