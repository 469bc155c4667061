// loam_dynmap.hip -- localisation map tiles and the per-frame crop on the device (include/pcm_amd.h, pcm_loam_tile_* and
// pcm_loam_dynmap_*): jueying_slam's area tiles (include/dynamic_map.h:16-156), dynamic_load_map_run (localization.cpp:281-315,
// new_localization.cpp:480-514) and dynamic_load_map (localization.cpp:256-280, new_localization.cpp:454-478).
//
// Store: one growing float4 arena (x, y, z, intensity; map frame) for the tiles of the corner list and one for those of the surf
// list, per-tile offset, count and Area on the host.  Load: the selection runs on the host (loam_dynmap.h; microseconds) and
// moves no points.  Crop: the selected tiles' entry table (arena offset, first position in the concatenation) is uploaded and
// the concatenation is compacted through the frame's window in three steps that keep the order:
//   k_dm_count    one lane per point, 256 points per workgroup (a workgroup never straddles the two lists): the predicate, a
//                 ballot and a popcount per wave, one count per workgroup;
//   k_dm_scan_*   exclusive scan of the workgroup counts: 256 counts per scan block, then the block totals in one workgroup;
//   k_dm_scatter  the predicate again, the lane's rank from the ballot, the whole 16-byte record to its place in the context's
//                 corner or surf target cloud (loam_target_reserve / loam_target_commit).
// The only atomic is the integer counter of dropped non-finite points: no output position depends on the schedule, so two crops
// of one state give the same bits.  When selection, limits and crop_x equal those of the last crop and the target is still its
// result, the call does nothing at all (a standing robot, the relocalisation branch's second scan2MapOptimization).
#include "host_util.h"
#include "loam_device.h"
#include "loam_dynmap.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace pcm;
using namespace pcm::loam;

namespace {

constexpr uint32_t kDmBlock = 256;   // points per workgroup of k_dm_count / k_dm_scatter
constexpr uint32_t kDmChunk = 256;   // workgroup counts per scan block

// the points [src, src + n) of an arena are positions [first, first + n) of the concatenation (n = the next entry's first - first)
struct DmEntry {
  uint32_t src;     // first point in its arena
  uint32_t first;   // first position (ascending over the table; no entry is empty)
  uint32_t flags;   // bit 0: surf arena
  uint32_t pad;
};

// small: [0] corner points kept, [1] points kept, [2] non-finite points dropped
constexpr int kSmallWords = 4;

// the workgroup's lane -> its position g in the concatenation (corner workgroups first: b < nb0 covers [0, n0), the rest
// [n0, N)), its record and the record's class.  The entry is found by a binary search over the first positions whose trip count
// depends on the table size alone; a tile holds thousands of points, so nearly every wave reads one entry.  An idle lane reads
// the last record of its own list (in bounds) and is class 0.
__device__ inline int dm_fetch(const float4* __restrict__ corner_arena, const float4* __restrict__ surf_arena, const DmEntry* __restrict__ ent, uint32_t n_ent,
                               uint32_t nb0, uint32_t n0, uint32_t N, const CropWindow& w, float4* p, bool* seg1) {
  const uint32_t b = blockIdx.x;
  *seg1 = b >= nb0;
  const uint32_t g = *seg1 ? n0 + (b - nb0) * kDmBlock + threadIdx.x : b * kDmBlock + threadIdx.x;
  const uint32_t end = *seg1 ? N : n0;
  const bool valid = g < end;
  const uint32_t gg = valid ? g : end - 1;
  uint32_t lo = 0, hi = n_ent;   // ent[lo].first <= gg < ent[hi].first (ent[n_ent].first taken as N)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ent[mid].first <= gg) lo = mid; else hi = mid;
  }
  const DmEntry e = ent[lo];
  const float4* __restrict__ arena = (e.flags & 1u) ? surf_arena : corner_arena;
  *p = arena[(size_t)e.src + (gg - e.first)];
  return valid ? crop_class(p->x, p->y, p->z, w) : 0;
}

__global__ void __launch_bounds__(kDmBlock) k_dm_count(const float4* __restrict__ corner_arena, const float4* __restrict__ surf_arena,
                                                       const DmEntry* __restrict__ ent, uint32_t n_ent, uint32_t nb0, uint32_t n0, uint32_t N, CropWindow w,
                                                       uint32_t* __restrict__ counts, uint32_t* __restrict__ small) {
  __shared__ uint32_t wk[kDmBlock / 64], wn[kDmBlock / 64];
  float4 p;
  bool seg1;
  const int cls = dm_fetch(corner_arena, surf_arena, ent, n_ent, nb0, n0, N, w, &p, &seg1);
  const uint64_t km = __ballot(cls == 1), nm = __ballot(cls == 2);
  if ((threadIdx.x & 63) == 0) { wk[threadIdx.x >> 6] = (uint32_t)__popcll(km); wn[threadIdx.x >> 6] = (uint32_t)__popcll(nm); }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t k = 0, n = 0;
    for (uint32_t i = 0; i < kDmBlock / 64; i++) { k += wk[i]; n += wn[i]; }
    counts[blockIdx.x] = k;
    if (n) atomicAdd(&small[2], n);   // an integer sum: the same in every order
  }
}

// exclusive scan of one value per lane over a workgroup of kDmChunk lanes; *total: the sum, in every lane
__device__ inline uint32_t dm_block_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t x = v;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)x, off, 64);
    if (lane >= (uint32_t)off) x += t;
  }
  if (lane == 63) sh[wv] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t i = 0; i < kDmChunk / 64; i++) { if (i < wv) before += sh[i]; all += sh[i]; }
  __syncthreads();   // sh is free for the next call
  *total = all;
  return before + x - v;
}

// counts[i] -> the sum of the counts before i inside its scan block; chunk_tot[block] = the block's sum
__global__ void __launch_bounds__(kDmChunk) k_dm_scan_chunks(uint32_t* __restrict__ counts, uint32_t nb, uint32_t* __restrict__ chunk_tot) {
  __shared__ uint32_t sh[kDmChunk / 64];
  const uint32_t i = blockIdx.x * kDmChunk + threadIdx.x;
  uint32_t total;
  const uint32_t ex = dm_block_scan(i < nb ? counts[i] : 0u, sh, &total);
  if (i < nb) counts[i] = ex;
  if (threadIdx.x == 0) chunk_tot[blockIdx.x] = total;
}

// one workgroup: chunk_off[c] = the sum of the scan-block totals before c; small[1] = all points kept, small[0] = those of the
// corner workgroups (the offset of workgroup nb0)
__global__ void __launch_bounds__(kDmChunk) k_dm_scan_tops(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ chunk_tot, uint32_t nchunks, uint32_t nb,
                                                           uint32_t nb0, uint32_t* __restrict__ chunk_off, uint32_t* __restrict__ small) {
  __shared__ uint32_t sh[kDmChunk / 64];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nchunks; base += kDmChunk) {
    const uint32_t i = base + threadIdx.x;
    uint32_t total;
    const uint32_t ex = dm_block_scan(i < nchunks ? chunk_tot[i] : 0u, sh, &total);
    if (i < nchunks) {
      chunk_off[i] = carry + ex;
      if (nb0 < nb && i == nb0 / kDmChunk) small[0] = carry + ex + counts[nb0];
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    small[1] = carry;
    if (nb0 >= nb) small[0] = carry;   // no surf workgroup
  }
}

__global__ void __launch_bounds__(kDmBlock) k_dm_scatter(const float4* __restrict__ corner_arena, const float4* __restrict__ surf_arena,
                                                         const DmEntry* __restrict__ ent, uint32_t n_ent, uint32_t nb0, uint32_t n0, uint32_t N, CropWindow w,
                                                         const uint32_t* __restrict__ counts, const uint32_t* __restrict__ chunk_off,
                                                         const uint32_t* __restrict__ small, float4* __restrict__ out0, float4* __restrict__ out1) {
  __shared__ uint32_t wk[kDmBlock / 64];
  float4 p;
  bool seg1;
  const int cls = dm_fetch(corner_arena, surf_arena, ent, n_ent, nb0, n0, N, w, &p, &seg1);
  const uint64_t km = __ballot(cls == 1);
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) wk[wv] = (uint32_t)__popcll(km);
  __syncthreads();
  if (cls != 1) return;
  uint32_t off = chunk_off[blockIdx.x / kDmChunk] + counts[blockIdx.x];
  for (uint32_t i = 0; i < wv; i++) off += wk[i];
  off += (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
  if (seg1) out1[off - small[0]] = p; else out0[off] = p;
}

struct Tile {
  Area box;
  size_t off;
  uint32_t n;
  int32_t ix = 0, iy = 0;   // the index pair of a tile pcm_loam_tiles_build cut; 0, 0 for one the caller added
};

struct DynStore {
  std::vector<Tile> tiles[2];   // corner list, surf list
  Arena arena[2] = {Arena("map-tile arena"), Arena("map-tile arena")};
  // the selection of the last load
  bool loaded = false;
  std::vector<int32_t> sel[2];
  uint64_t sel_gen = 0;
  float last_load[6] = {kNeverLoaded, kNeverLoaded, kNeverLoaded, kNeverLoaded, kNeverLoaded, kNeverLoaded};
  // crop workspace
  DevBuf<char> buf{"map-crop workspace"};
  size_t nb_cap = 0, ent_cap = 0;
  size_t o_counts = 0, o_tot = 0, o_off = 0, o_small = 0, o_ent = 0;
  PinnedBuf<uint32_t> h_small;
  PinnedBuf<DmEntry> h_ent;
  // the last crop
  bool last_valid = false;
  uint64_t last_gen = 0;
  CropWindow last_w{};
  pcm_loam_dynmap_crop_result last{};
};

int check_ctx_dm(pcm_ctx* c, DynStore** ds) {
  return loam_check_store(c, "pcm_loam_tile_* / pcm_loam_dynmap_* need a context created with PCM_MODEL_LOAM", LoamStore::dyn, ds);
}

int check_dparams(pcm_ctx* c, const pcm_loam_dynmap_params* params, const float* pose6, pcm_loam_dynmap_params* p) {
  if (params) *p = *params; else pcm_loam_default_dynmap_params(p);
  if (!(p->max_range >= 0.f) || !finite_f(p->max_range)) { c->err = "max_range must be a number >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!pose6) { c->err = "null pose"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int k = 0; k < 6; k++) if (!finite_f(pose6[k])) { c->err = "the pose must be finite"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

int ensure_work(pcm_ctx* c, DynStore* S, size_t nb, size_t n_ent) {
  int rc = S->h_small.reserve(c, kSmallWords, kSmallWords);
  if (rc != PCM_OK) return rc;
  if (n_ent > S->h_ent.cap && (rc = S->h_ent.reserve(c, n_ent, n_ent + n_ent / 2 + 16)) != PCM_OK) return rc;
  if (S->buf && nb <= S->nb_cap && n_ent <= S->ent_cap) return PCM_OK;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  S->buf.release();   // the layout below is for the new sizes alone
  S->nb_cap = S->ent_cap = 0;
  const size_t bc = nb + nb / 4 + 256, ec = S->h_ent.cap, cc = (bc + kDmChunk - 1) / kDmChunk;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t r = o; o += up256(bytes); return r; };
  S->o_counts = take(4 * bc);
  S->o_tot = take(4 * cc);
  S->o_off = take(4 * cc);
  S->o_small = take(4 * kSmallWords);
  S->o_ent = take(sizeof(DmEntry) * ec);
  if ((rc = S->buf.reserve(c, o, o)) != PCM_OK) return rc;
  S->nb_cap = bc; S->ent_cap = ec;
  return PCM_OK;
}

// both lists and the selection; the arenas keep their memory
void clear_tiles(DynStore* S) {
  for (int m = 0; m < 2; m++) {
    S->tiles[m].clear();
    S->sel[m].clear();
    S->arena[m].n = 0;
  }
  S->loaded = false;
  S->sel_gen++;
  S->last_valid = false;
  for (int k = 0; k < 6; k++) S->last_load[k] = kNeverLoaded;
}

bool same_window(const CropWindow& a, const CropWindow& b) {
  // float equality: the limits are finite or the two infinities of margin < 0, never NaN
  return a.x_lo == b.x_lo && a.x_hi == b.x_hi && a.y_lo == b.y_lo && a.y_hi == b.y_hi && a.crop_x == b.crop_x;
}

}  // namespace

namespace pcm {
namespace loam {
int loam_tiles_replace(pcm_ctx* c, const BuiltTile* const tiles[2], const size_t n_tiles[2], const float4* const cells[2], const size_t n_cells[2]) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  for (int m = 0; m < 2; m++) {
    if (n_cells[m] > 0xffffffffull || n_tiles[m] > 0x7fffffffull) { c->err = "map-tile store too large"; return PCM_ERR_OUT_OF_RANGE; }
    // room first, so that a failed allocation leaves both lists whole (growth keeps the stored points)
    Arena& A = S->arena[m];
    if (n_cells[m] > A.n && (rc = A.reserve(c, n_cells[m] - A.n)) != PCM_OK) return rc;
  }
  for (int m = 0; m < 2; m++) {
    try { S->tiles[m].reserve(n_tiles[m]); } catch (...) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  }
  clear_tiles(S);
  for (int m = 0; m < 2; m++) {
    Arena& A = S->arena[m];
    if (n_cells[m]) PCM_HIPCK(c, hipMemcpyAsync(A.d.p, cells[m], sizeof(float4) * n_cells[m], hipMemcpyDeviceToDevice, c->stream));
    for (size_t t = 0; t < n_tiles[m]; t++) {
      const BuiltTile& b = tiles[m][t];
      Tile T;
      T.box = Area{b.box[0], b.box[1], b.box[2], b.box[3], b.box[4], b.box[5]};
      T.off = b.first; T.n = b.n; T.ix = b.ix; T.iy = b.iy;
      S->tiles[m].push_back(T);
    }
    A.n = n_cells[m];
  }
  return PCM_OK;
}
}  // namespace loam
}  // namespace pcm

extern "C" {

void pcm_loam_default_dynmap_params(pcm_loam_dynmap_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_range = 150.0f;   // utility.h:224
  p->margin = -1;          // utility.h:186
  p->area_size = -1;       // utility.h:185
  p->crop_x = 0;           // localization.cpp:259-273 as it behaves
}

int pcm_loam_tile_add(pcm_ctx* c, int which, const double box[6], const void* points, size_t n, size_t stride, int memory) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (which != 0 && which != 1) { c->err = "which must be 0 (corner list) or 1 (surf list)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!box) { c->err = "null box"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int k = 0; k < 6; k++) if (!(box[k] == box[k])) { c->err = "the box must hold numbers"; return PCM_ERR_INVALID_ARGUMENT; }
  if ((rc = check_point_records(c, points, n, stride, memory, 0x3fffffffull)) != PCM_OK) return rc;
  Arena& A = S->arena[which];
  if (A.n + n > 0xffffffffull || S->tiles[which].size() >= 0x7fffffffull) { c->err = "map-tile store too large"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  if ((rc = A.reserve(c, n)) != PCM_OK) return rc;
  if ((rc = load_xyzw_rows(c, points, n, stride, memory, true, A.d + A.n)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the caller may reuse its buffer on return
  Tile t;
  t.box = Area{box[0], box[1], box[2], box[3], box[4], box[5]};
  t.off = A.n;
  t.n = (uint32_t)n;
  S->tiles[which].push_back(t);
  A.n += n;
  return (int)S->tiles[which].size() - 1;
}

int pcm_loam_tile_count(pcm_ctx* c, int which) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (which != 0 && which != 1) { c->err = "which must be 0 (corner list) or 1 (surf list)"; return PCM_ERR_INVALID_ARGUMENT; }
  return (int)S->tiles[which].size();
}

int pcm_loam_tile_clear(pcm_ctx* c) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  clear_tiles(S);
  return PCM_OK;
}

int pcm_loam_tile_info(pcm_ctx* c, int which, int index, double box[6], int32_t ixy[2], size_t* n_points) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (which != 0 && which != 1) { c->err = "which must be 0 (corner list) or 1 (surf list)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (index < 0 || (size_t)index >= S->tiles[which].size()) { c->err = "pcm_loam_tile_info: index outside [0, tiles of the list)"; return PCM_ERR_INVALID_ARGUMENT; }
  const Tile& T = S->tiles[which][(size_t)index];
  if (box) { box[0] = T.box.x_min; box[1] = T.box.y_min; box[2] = T.box.z_min; box[3] = T.box.x_max; box[4] = T.box.y_max; box[5] = T.box.z_max; }
  if (ixy) { ixy[0] = T.ix; ixy[1] = T.iy; }
  if (n_points) *n_points = T.n;
  return PCM_OK;
}

int pcm_loam_tile_get(pcm_ctx* c, int which, int index, void* out, size_t capacity, int memory, size_t* n) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (n) *n = 0;
  if (which != 0 && which != 1) { c->err = "which must be 0 (corner list) or 1 (surf list)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  if (index < 0 || (size_t)index >= S->tiles[which].size()) { c->err = "pcm_loam_tile_get: index outside [0, tiles of the list)"; return PCM_ERR_INVALID_ARGUMENT; }
  const Tile& T = S->tiles[which][(size_t)index];
  if (n) *n = T.n;
  if (T.n > capacity || (!out && T.n)) { c->err = "pcm_loam_tile_get: capacity too small (the count is set)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (T.n == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  PCM_HIPCK(c, hipMemcpyAsync(out, S->arena[which].d + T.off, sizeof(float4) * T.n, memory == PCM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

int pcm_loam_dynmap_need_load(pcm_ctx* c, const pcm_loam_dynmap_params* params, const float pose6[6]) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_dynmap_params p;
  if ((rc = check_dparams(c, params, pose6, &p)) != PCM_OK) return rc;
  return need_load(pose6, S->last_load, p.area_size) ? 1 : 0;
}

int pcm_loam_dynmap_load(pcm_ctx* c, const pcm_loam_dynmap_params* params, const float pose6[6], pcm_loam_dynmap_load_result* result) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_dynmap_params p;
  if ((rc = check_dparams(c, params, pose6, &p)) != PCM_OK) return rc;
  pcm_loam_dynmap_load_result r;
  std::memset(&r, 0, sizeof(r));
  bool changed = !S->loaded;
  for (int m = 0; m < 2; m++) {
    std::vector<Area> areas(S->tiles[m].size());
    for (size_t i = 0; i < areas.size(); i++) areas[i] = S->tiles[m][i].box;
    // create_pcd(transformTobeMapped[3], transformTobeMapped[4], areas, dir, margin): the int margin becomes a float there
    std::vector<int32_t> sel = select_areas(areas.data(), (int)areas.size(), pose6[3], pose6[4], (float)p.margin);
    if (sel != S->sel[m]) changed = true;
    S->sel[m] = std::move(sel);
  }
  if (changed) S->sel_gen++;
  S->loaded = true;
  for (int k = 0; k < 6; k++) S->last_load[k] = pose6[k];
  r.num_corner_tiles = (int32_t)S->tiles[0].size();
  r.num_surf_tiles = (int32_t)S->tiles[1].size();
  r.num_corner_selected = (int32_t)S->sel[0].size();
  r.num_surf_selected = (int32_t)S->sel[1].size();
  for (int32_t t : S->sel[0]) r.num_corner_points += S->tiles[0][(size_t)t].n;
  for (int32_t t : S->sel[1]) r.num_surf_points += S->tiles[1][(size_t)t].n;
  r.generation = S->sel_gen;
  r.changed = changed ? 1 : 0;
  if (result) *result = r;
  return PCM_OK;
}

int pcm_loam_dynmap_crop(pcm_ctx* c, const pcm_loam_dynmap_params* params, const float pose6[6], pcm_loam_dynmap_crop_result* result) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (!result) { c->err = "null result"; return PCM_ERR_INVALID_ARGUMENT; }
  pcm_loam_dynmap_params p;
  if ((rc = check_dparams(c, params, pose6, &p)) != PCM_OK) return rc;
  std::memset(result, 0, sizeof(*result));
  if (!S->loaded) { c->err = "pcm_loam_dynmap_crop before pcm_loam_dynmap_load"; return PCM_ERR_NO_INPUT; }
  const CropWindow w = crop_window(pose6, p.max_range, p.margin, p.crop_x);
  const float4 *tc = nullptr, *ts = nullptr;
  uint32_t tnc = 0, tns = 0;
  if (S->last_valid && S->last_gen == S->sel_gen && same_window(S->last_w, w) && loam_target_view(c, TargetOwner::dynmap, &tc, &tnc, &ts, &tns)) {
    // the same tiles through the same window: the target is the one the context already holds
    *result = S->last;
    result->rebuilt = 0;
    return PCM_OK;
  }
  PCM_HIPCK(c, hipSetDevice(c->device));
  S->last_valid = false;
  uint64_t n0 = 0, n1 = 0;
  size_t E = 0;
  for (int32_t t : S->sel[0]) { n0 += S->tiles[0][(size_t)t].n; E += S->tiles[0][(size_t)t].n ? 1 : 0; }
  for (int32_t t : S->sel[1]) { n1 += S->tiles[1][(size_t)t].n; E += S->tiles[1][(size_t)t].n ? 1 : 0; }
  if (n0 + n1 > 0x7fffffffull) { c->err = "the selected tiles hold more than 2^31 points"; return PCM_ERR_OUT_OF_RANGE; }
  float4 *out_c = nullptr, *out_s = nullptr;
  if ((rc = loam_target_reserve(c, (size_t)n0, (size_t)n1, &out_c, &out_s)) != PCM_OK) return rc;
  pcm_loam_dynmap_crop_result r;
  std::memset(&r, 0, sizeof(r));
  r.num_corner_in = (int32_t)n0; r.num_surf_in = (int32_t)n1;
  r.x_lo = w.x_lo; r.x_hi = w.x_hi; r.y_lo = w.y_lo; r.y_hi = w.y_hi;
  const uint32_t N = (uint32_t)(n0 + n1);
  if (N > 0) {
    const uint32_t nb0 = (uint32_t)((n0 + kDmBlock - 1) / kDmBlock), nb = nb0 + (uint32_t)((n1 + kDmBlock - 1) / kDmBlock);
    const uint32_t nchunks = (nb + kDmChunk - 1) / kDmChunk;
    if ((rc = ensure_work(c, S, nb, E)) != PCM_OK) return rc;
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the pinned staging of an earlier crop is free again
    uint32_t first = 0;
    size_t e = 0;
    for (int m = 0; m < 2; m++)
      for (int32_t t : S->sel[m]) {
        const Tile& T = S->tiles[m][(size_t)t];
        if (T.n == 0) continue;   // an empty tile contributes nothing
        S->h_ent[e++] = DmEntry{(uint32_t)T.off, first, (uint32_t)m, 0u};
        first += T.n;
      }
    hipStream_t st = c->stream;
    char* b = S->buf.p;
    uint32_t* counts = reinterpret_cast<uint32_t*>(b + S->o_counts);
    uint32_t* chunk_tot = reinterpret_cast<uint32_t*>(b + S->o_tot);
    uint32_t* chunk_off = reinterpret_cast<uint32_t*>(b + S->o_off);
    uint32_t* small = reinterpret_cast<uint32_t*>(b + S->o_small);
    DmEntry* d_ent = reinterpret_cast<DmEntry*>(b + S->o_ent);
    PCM_HIPCK(c, hipMemcpyAsync(d_ent, S->h_ent, sizeof(DmEntry) * E, hipMemcpyHostToDevice, st));
    PCM_HIPCK(c, hipMemsetAsync(small, 0, sizeof(uint32_t) * kSmallWords, st));
    k_dm_count<<<nb, kDmBlock, 0, st>>>(S->arena[0].d, S->arena[1].d, d_ent, (uint32_t)E, nb0, (uint32_t)n0, N, w, counts, small);
    k_dm_scan_chunks<<<nchunks, kDmChunk, 0, st>>>(counts, nb, chunk_tot);
    k_dm_scan_tops<<<1, kDmChunk, 0, st>>>(counts, chunk_tot, nchunks, nb, nb0, chunk_off, small);
    k_dm_scatter<<<nb, kDmBlock, 0, st>>>(S->arena[0].d, S->arena[1].d, d_ent, (uint32_t)E, nb0, (uint32_t)n0, N, w, counts, chunk_off, small, out_c, out_s);
    PCM_HIPCK(c, hipGetLastError());
    PCM_HIPCK(c, hipMemcpyAsync(S->h_small, small, sizeof(uint32_t) * kSmallWords, hipMemcpyDeviceToHost, st));
    PCM_HIPCK(c, hipStreamSynchronize(st));
    const uint32_t k0 = S->h_small[0], k = S->h_small[1];
    if (k0 > n0 || k < k0 || k - k0 > n1) { c->err = "pcm_loam_dynmap_crop: inconsistent counts"; return PCM_ERR_INTERNAL; }
    r.num_corner = (int32_t)k0;
    r.num_surf = (int32_t)(k - k0);
    r.num_nonfinite = (int32_t)S->h_small[2];
  }
  loam_target_commit(c, (uint32_t)r.num_corner, (uint32_t)r.num_surf, TargetOwner::dynmap);
  r.rebuilt = 1;
  r.status = PCM_OK;
  S->last_valid = true;
  S->last_gen = S->sel_gen;
  S->last_w = w;
  S->last = r;
  *result = r;
  return PCM_OK;
}

int pcm_loam_dynmap_info(pcm_ctx* c, int32_t* corner_tiles, int32_t* surf_tiles, float* corner, float* surf) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (!S->loaded) { c->err = "pcm_loam_dynmap_info before pcm_loam_dynmap_load"; return PCM_ERR_NO_INPUT; }
  if (corner_tiles && !S->sel[0].empty()) std::memcpy(corner_tiles, S->sel[0].data(), sizeof(int32_t) * S->sel[0].size());
  if (surf_tiles && !S->sel[1].empty()) std::memcpy(surf_tiles, S->sel[1].data(), sizeof(int32_t) * S->sel[1].size());
  if (!corner && !surf) return PCM_OK;
  const float4 *tc = nullptr, *ts = nullptr;
  uint32_t tnc = 0, tns = 0;
  if (!S->last_valid || !loam_target_view(c, TargetOwner::dynmap, &tc, &tnc, &ts, &tns)) { c->err = "pcm_loam_dynmap_info: the context's target is not the result of pcm_loam_dynmap_crop"; return PCM_ERR_NO_INPUT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  if (corner && tnc) PCM_HIPCK(c, hipMemcpyAsync(corner, tc, sizeof(float4) * tnc, hipMemcpyDeviceToHost, c->stream));
  if (surf && tns) PCM_HIPCK(c, hipMemcpyAsync(surf, ts, sizeof(float4) * tns, hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

int pcm_loam_dynmap_global(pcm_ctx* c, void* out, size_t capacity, size_t* n, int memory) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (n) *n = 0;
  if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  const float4 *tc = nullptr, *ts = nullptr;
  uint32_t tnc = 0, tns = 0;
  if (!S->last_valid || !loam_target_view(c, TargetOwner::dynmap, &tc, &tnc, &ts, &tns)) { c->err = "pcm_loam_dynmap_global: the context's target is not the result of pcm_loam_dynmap_crop"; return PCM_ERR_NO_INPUT; }
  const size_t m = (size_t)tnc + tns;
  if (n) *n = m;
  if (m > capacity || (!out && m)) { c->err = "pcm_loam_dynmap_global: capacity too small (the count is set)"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  const hipMemcpyKind kind = memory == PCM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  float4* dst = static_cast<float4*>(out);
  if (tnc) PCM_HIPCK(c, hipMemcpyAsync(dst, tc, sizeof(float4) * tnc, kind, c->stream));
  if (tns) PCM_HIPCK(c, hipMemcpyAsync(dst + tnc, ts, sizeof(float4) * tns, kind, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

}  // extern "C"
