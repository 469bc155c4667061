// neighbour_lists.hip -- per-voxel candidate lists of a static submap and k_linearize_lists, the point-to-plane linearize pass that
// reads them (PCM_FLAG_NEIGHBOUR_LISTS).
//
// IVox::GetClosestPoint (/root/reference/src/jueying_lio/include/ivox3d/ivox3d.h:132-204) visits, for a query in voxel u, the
// voxels u + nearby_grids_[g] in list order and every point of each in insertion order.  That candidate sequence depends on u only.
// The tile kernel (kernels.hip) re-derives it per pass -- tile box, brick probes by one wave, the bricks' points staged through LDS,
// a cell grid, 27 per-cell walks in lock-step, five barriers in front of the plane fit -- and its waves spend four fifths of their
// life waiting (the search over a ready-made flat list is 12x cheaper than the cell walk).  For a submap that is
// registered against many times (jueying_slam's localization against one global map; fast_gicp/src/align.cpp:51-104 is no such
// protocol: it clears the target on every iteration and its reuse loop swaps source and target) the sequences are
// built ONCE, with the map: for every voxel of the occupied set dilated by the neighbourhood, the points of its <= 27 neighbour
// voxels in the reference's visit order, contiguous in HBM (27 x 16 B per map point).  The pass is then: voxel of the query ->
// one probe of the list index -> a flat walk of one contiguous run (lanes of a wave mostly share it) -> plane fit -> the shared
// residual / reduction tail.  No LDS staging, no cell grid, no barrier before the reduction; same candidates in the same order
// into the same best_offer: bit-identical planes (tests/test_gpu_neighbour_lists.py).
//
// The list index is an ordinary brick hash (voxel_hash.hip) built from one stand-in point per dilated voxel (its centre), so a
// TargetView serves as the view of the lists: bricks / bmask / bpref give the voxel's rank r, vox_start[r] .. vox_start[r + 1] is
// its run in pts -- which here holds the candidates (w = index of the point in the map's own array).
//
// Compiled with -ffp-contract=off (see kernels.hip).
#include "pcm_device.h"
#include "pcm_host.h"
#include "plane_fit.h"
#include "linearize_common.h"
#include "keyed_best.h"
#include "dev_scratch.h"

#include <algorithm>
#include <cstring>
#include <string>

namespace pcm {

namespace {

constexpr int kKeyBias = 1 << 20;
// A run of candidate points (kind 0) is padded to a multiple of kListTrip entries, so with the array's base aligned (hipMalloc: 256
// bytes) every run starts on a 64-byte boundary and the walk of k_linearize_lists takes whole trips of four 16-byte loads without
// a bounds test.  A pad entry is (+inf, +inf, +inf, id 0xffffffff): for every finite query pad - q = +inf, its square and the sum
// of the squares are +inf (with and without FMA contraction), and best_offer's `d2 < thr` with thr <= max_r2f <= +inf is false.
constexpr uint32_t kListTrip = 4;
constexpr uint32_t kListPadId = 0xffffffffu;
// Trips the keyed walk of k_linearize_lists loads ahead of the one it consumes; the point lists end with as many zeroed trips.
constexpr uint32_t kWalkAhead = 1;

// the key of a list voxel: 3 x 21 bits, biased
__device__ inline uint64_t nl_pack(int x, int y, int z) { return ((uint64_t)(uint32_t)(x + kKeyBias) << 42) | ((uint64_t)(uint32_t)(y + kKeyBias) << 21) | (uint64_t)(uint32_t)(z + kKeyBias); }
__device__ inline void nl_unpack(uint64_t k, int& x, int& y, int& z) {
  x = (int)((k >> 42) & 0x1fffffu) - kKeyBias; y = (int)((k >> 21) & 0x1fffffu) - kKeyBias; z = (int)(k & 0x1fffffu) - kKeyBias;
}

// one key per (occupied voxel, neighbour offset): the voxels a query can sit in and see this voxel.  grid = ceil(nvox / 256)
__global__ void k_nl_keys(const float4* __restrict__ pts, const uint32_t* __restrict__ vox_start, uint32_t nvox, float res, float inv_res, int mode, int nn, uint64_t* __restrict__ keys) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nvox) return;
  const float4 p = pts[vox_start[v]];
  const int cx = voxel_coord(p.x, res, inv_res, mode), cy = voxel_coord(p.y, res, inv_res, mode), cz = voxel_coord(p.z, res, inv_res, mode);   // the map's own convention (Pos2Grid  ivox3d.h:283-286; pclomp: floor(p * inverse_leaf_size))
  const int lim = kKeyBias - 64;
  for (int g = 0; g < nn; g++) {
    const int x = cx - c_nearby[g][0], y = cy - c_nearby[g][1], z = cz - c_nearby[g][2];   // u + nearby[g] = this voxel
    const bool ok = x > -lim && x < lim && y > -lim && y < lim && z > -lim && z < lim;
    keys[(size_t)v * nn + g] = ok ? nl_pack(x, y, z) : ~0ull;
  }
}

__global__ void k_nl_flags(const uint64_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[i] = (keys[i] != ~0ull && (i == 0 || keys[i] != keys[i - 1])) ? 1u : 0u;
}

// the stand-in point of every distinct key: the centre of its voxel (Pos2Grid of it is the voxel again)
__global__ void k_nl_centres(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint32_t n, float res, float shift, float4* __restrict__ out,
                             uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == n - 1) *count = pos[i] + flag[i];
  if (!flag[i]) return;
  int x, y, z;
  nl_unpack(keys[i], x, y, z);
  out[pos[i]] = make_float4(((float)x + shift) * res, ((float)y + shift) * res, ((float)z + shift) * res, 0.f);   // shift: 0 (round) or 0.5 (floor): the voxel's centre
}

// FILL = false: len[r] = candidates of list voxel r, rounded up to a multiple of kListTrip (0 stays 0); FILL = true: copy them and
// fill the rest of the run with kListPad entries.  One lane per list voxel.
// The candidates of list voxel (cx, cy, cz) and their padded number: the build (k_nl_lists) and the update of following lists
// (k_fl_classify / k_fl_rewrite) share it.  FILL: they are written to out[0 ..), pad entries behind them.
template <bool FILL>
__device__ inline uint32_t nl_gather(const TargetView& tg, int nn, int cx, int cy, int cz, float4* __restrict__ out) {
  BrickCursor cur;
  uint32_t n = 0;
  for (int g = 0; g < nn; g++) {   // nearby_grids_ order  ivox3d.h:211-235
    const int v = voxel_rank(tg, cur, cx + c_nearby[g][0], cy + c_nearby[g][1], cz + c_nearby[g][2]);
    if (v < 0) continue;
    uint32_t s, e;
    voxel_run(tg, (uint32_t)v, s, e);
    if (FILL) {
      for (uint32_t k = s; k < e; k++) {   // the voxel's points in insertion order (points_)  ivox3d_node.hpp:158-166
        float4 p = gload4(tg.pts + k);
        p.w = __uint_as_float(k);
        out[n + (k - s)] = p;
      }
    }
    n += e - s;
  }
  const uint32_t padded = (n + (kListTrip - 1u)) & ~(kListTrip - 1u);
  if (FILL) {
    const float inf = __builtin_inff();
    for (uint32_t k = n; k < padded; k++) out[k] = make_float4(inf, inf, inf, __uint_as_float(kListPadId));
  }
  return padded;
}
template <bool FILL>
__global__ void k_nl_lists(const float4* __restrict__ centres, uint32_t nd, TargetView tg, int mode, int nn, uint32_t* __restrict__ len, const uint32_t* __restrict__ start, float4* __restrict__ out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nd) return;
  const float4 c = centres[r];
  const int cx = voxel_coord(c.x, tg.res, tg.inv_res, mode), cy = voxel_coord(c.y, tg.res, tg.inv_res, mode), cz = voxel_coord(c.z, tg.res, tg.inv_res, mode);
  const uint32_t padded = nl_gather<FILL>(tg, nn, cx, cy, cz, FILL ? out + start[r] : nullptr);
  if (!FILL) len[r] = padded;
}

// pclomp NDT: the neighbour LEAVES of every list voxel in the order getNeighborhoodAtPoint{,7,1} / the radius search visit them
// (voxel_grid_covariance_omp_impl.hpp:373-442; the 27 cells as direct_offset orders them, brick_table.h), filtered as far as the filter
// does not depend on the query: DIRECT1/7/27 keep a leaf with >= 6 points; KDTREE (nn = 0) keeps a leaf of the centroid cloud and
// stores its float centroid for the radius test the pass applies per point.  Entry = (centroid xyz or 0, leaf index).
template <bool FILL>
__global__ void k_nl_leaf_lists(const float4* __restrict__ centres, uint32_t nd, TargetView tg, int mode, const PclLeaf* __restrict__ leaves, int nn, uint32_t* __restrict__ len,
                                const uint32_t* __restrict__ start, float4* __restrict__ out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nd) return;
  const float4 c = centres[r];
  const int cx = voxel_coord(c.x, tg.res, tg.inv_res, mode), cy = voxel_coord(c.y, tg.res, tg.inv_res, mode), cz = voxel_coord(c.z, tg.res, tg.inv_res, mode);
  const int nk = nn == 0 ? 27 : nn;
  BrickCursor cur;
  uint32_t n = 0;
  const uint32_t o = FILL ? start[r] : 0u;
  for (int k = 0; k < nk; k++) {
    int ox, oy, oz;
    direct_offset(nk, k, ox, oy, oz);
    const int v = voxel_rank(tg, cur, cx + ox, cy + oy, cz + oz);
    if (v < 0) continue;
    const PclLeaf* L = leaves + v;
    const bool keep = nn == 0 ? L->in_centroids != 0 : L->n >= 6;
    if (!keep) continue;
    if (FILL) out[o + n] = nn == 0 ? make_float4(L->centroid[0], L->centroid[1], L->centroid[2], __int_as_float(v)) : make_float4(0.f, 0.f, 0.f, __int_as_float(v));
    n++;
  }
  if (!FILL) len[r] = n;
}

// fast_gicp NDTCuda / VGICP of the CUDA core (ndt.hip k_ndt): the voxel of every neighbour offset of a list voxel, in the offset order
// of ndt_cuda.cu:35-88 (DIRECT1 / 7 / 27), -1 where the cell is empty -- a fixed row of nO indices per list voxel, so the pass reads
// one row behind one probe instead of probing nO cells one after the other.
__global__ void k_nl_voxel_slots(const float4* __restrict__ centres, uint32_t nd, TargetView tg, int mode, int nO, int32_t* __restrict__ out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nd) return;
  const float4 c = centres[r];
  const int cx = voxel_coord(c.x, tg.res, tg.inv_res, mode), cy = voxel_coord(c.y, tg.res, tg.inv_res, mode), cz = voxel_coord(c.z, tg.res, tg.inv_res, mode);
  BrickCursor cur;
  for (int k = 0; k < nO; k++) {
    int ox, oy, oz;
    direct_offset(nO, k, ox, oy, oz);
    out[(size_t)r * nO + k] = voxel_rank(tg, cur, cx + ox, cy + oy, cz + oz);
  }
}

}  // namespace

TargetView view_of_lists(const NeighbourLists& l) {
  TargetView v = view_of(l.index);
  v.pts = l.pts;
  v.vox_start = l.pooled ? reinterpret_cast<const uint32_t*>(l.rank_rec.p) : l.start.p;   // pooled: (start, length) records, read by k_linearize_lists<.., true> only
  v.num_points = (uint32_t)l.num_candidates;
  return v;
}

// ---------------------------------------------------------------------------
// build_neighbour_lists in stages over one ListBuild (DESIGN.md "Build stages"; as build_target_map, voxel_hash.hip)
// ---------------------------------------------------------------------------
struct ListBuild {
  hipStream_t stream;
  std::string* err;
  const TargetMap& map;
  NeighbourLists* out;
  DevScratch sc;
  int nn;        // the neighbourhood asked for (0: the KDTREE search of pclomp NDT)
  int nset;      // its cells (the SET is the same in the iVox and the pcl order: c_nearby's prefixes)
  size_t nk;     // (voxel, offset) keys
  float4* centres = nullptr;   // a stand-in point per dilated voxel, in key order
  uint32_t nd = 0;             // dilated voxels = lists
  const ListFollow* follow = nullptr;   // the pooled form of following lists
};

// room for `need` bytes?  a quarter of the free memory stays untouched (the caller's next targets, the scratch of the passes)
static int room_for(size_t need, std::string* err) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b - free_b / 4) {
    *err = "neighbour lists: " + std::to_string(need >> 20) + " MiB needed, " + std::to_string(free_b >> 20) + " MiB of device memory free";
    return PCM_ERR_HIP;
  }
  return PCM_OK;
}

// The sorted distinct keys of keys[0 .. n) (~0: no key), as far as the build and the update share them: the keys sorted, a flag on
// the first of every run of equal keys, and the flags' exclusive scan = the place of each head among the distinct keys.  The
// caller compacts the heads its own way: into centres (dilated_voxels), into the keys themselves and their number (dirty_lists).
struct DistinctKeys { uint64_t* sorted = nullptr; uint32_t *flag = nullptr, *pos = nullptr; };
static int distinct_keys(DevScratch& sc, std::string* err, const uint64_t* keys, size_t n, DistinctKeys* out) {
  if (sc.take(&out->sorted, n, err, "list keys, sorted") || sc.take(&out->flag, n, err, "list key heads") || sc.take(&out->pos, n, err, "list key ranks")) return PCM_ERR_HIP;
  if (const int rc = scratch_sort_keys(sc, err, keys, out->sorted, n, 0, 64); rc != PCM_OK) return rc;
  k_nl_flags<<<(unsigned)((n + 255) / 256), 256, 0, sc.stream()>>>(out->sorted, (uint32_t)n, out->flag);
  PCM_HIPCK_ERR(err, hipGetLastError());
  return scratch_exclusive_scan(sc, err, out->flag, out->pos, n);
}

// the dilated occupied set: the distinct keys of every (voxel, offset), one centre per key; their number to the host (one read-back)
static int dilated_voxels(ListBuild& b) {
  const TargetMap& map = b.map;
  const int mode = map.coord_mode;
  const size_t nk = b.nk;
  uint64_t* keys = nullptr;
  uint32_t *d_cnt = nullptr, h_cnt = 0;
  DistinctKeys dk;
  if (b.sc.take(&keys, nk, b.err, "dilation keys") || b.sc.take(&d_cnt, 2, b.err, "dilation count")) return PCM_ERR_HIP;
  k_nl_keys<<<(map.num_voxels + 255) / 256, 256, 0, b.stream>>>(map.pts, map.vox_start, map.num_voxels, map.res, map.inv_res, mode, b.nset, keys);
  PCM_HIPCK_ERR(b.err, hipGetLastError());
  if (const int rc = distinct_keys(b.sc, b.err, keys, nk, &dk); rc != PCM_OK) return rc;
  if (const int rc = b.sc.take(&b.centres, nk, b.err, "dilated voxel centres"); rc != PCM_OK) return rc;   // at most one per key
  k_nl_centres<<<(unsigned)((nk + 255) / 256), 256, 0, b.stream>>>(dk.sorted, dk.flag, dk.pos, (uint32_t)nk, map.res, mode == COORD_ROUND ? 0.f : mode == COORD_FLOOR_MUL ? 0.5f : 1.0f, b.centres, d_cnt);
  PCM_HIPCK_ERR(b.err, hipGetLastError());
  PCM_HIPCK_ERR(b.err, hipMemcpyAsync(&h_cnt, d_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream));
  PCM_HIPCK_ERR(b.err, hipStreamSynchronize(b.stream));
  b.nd = h_cnt;
  if (b.nd == 0) { *b.err = "neighbour lists: empty map"; return PCM_ERR_NO_INPUT; }
  return PCM_OK;
}

// the list index: a brick hash over the stand-in points (one per dilated voxel); its own host syncs
static int list_index(ListBuild& b) {
  if (b.follow) {   // the index of following lists is merged into later (update_neighbour_lists): its point log stays
    if (const int rc = b.out->centres.reserve(b.stream, b.err, b.nd, (size_t)b.nd + b.nd / 4 + 1024); rc != PCM_OK) return rc;
    PCM_HIPCK_ERR(b.err, hipMemcpyAsync(b.out->centres, b.centres, sizeof(float4) * (size_t)b.nd, hipMemcpyDeviceToDevice, b.stream));
    b.centres = b.out->centres;
  }
  if (const int rc = build_target_map(b.stream, b.centres, &b.nd, b.map.res, b.map.coord_mode, &b.out->index, b.err); rc != PCM_OK) return rc;
  if (b.out->index.num_voxels != b.nd || b.out->index.num_points != b.nd) { *b.err = "neighbour lists: index does not hold one voxel per list"; return PCM_ERR_INTERNAL; }
  return PCM_OK;
}

// kind 2: a fixed row of nn voxel indices per list voxel, kept in the `pts` allocation
static int voxel_slot_rows(ListBuild& b) {
  NeighbourLists* out = b.out;
  const uint32_t nd = b.nd;
  const size_t words = (size_t)nd * b.nn, cells = (words + 3) / 4 + 4;
  if (const int rc = out->pts.reserve(b.stream, b.err, cells, cells); rc != PCM_OK) return rc;
  k_nl_voxel_slots<<<(nd + 127) / 128, 128, 0, b.stream>>>(out->index.pts, nd, view_of(b.map), b.map.coord_mode, b.nn, reinterpret_cast<int32_t*>(out->pts.p));
  PCM_HIPCK_ERR(b.err, hipGetLastError());
  PCM_HIPCK_ERR(b.err, hipStreamSynchronize(b.stream));
  out->num_lists = nd;
  out->num_candidates = words;
  out->num_neighbors = b.nn;
  out->kind = 2;
  out->valid = true;
  return PCM_OK;
}

// ---------------------------------------------------------------------------
// Following lists (PCM_FLAG_FOLLOWING_LISTS): the runs in a pool, a (start, length) record per list
// ---------------------------------------------------------------------------
static_assert(list_pool::kTrip == kListTrip && list_pool::kTailTrips == kWalkAhead, "list_pool.h lays the pool out for this walk");

namespace {

// the records of a full build: run r of the contiguous layout belongs to the list whose stand-in point is log entry idx_s[r]
__global__ void k_fl_records(const uint32_t* __restrict__ idx_s, const uint32_t* __restrict__ start, const uint32_t* __restrict__ len, uint32_t nd, uint2* __restrict__ rec,
                             uint32_t* __restrict__ rec_cap, uint2* __restrict__ rank_rec) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nd) return;
  const uint32_t id = idx_s[r];
  const uint2 v = make_uint2(start[r], len[r]);
  rec[id] = v;
  rec_cap[id] = v.y;
  rank_rec[r] = v;
}
// rank -> record, after the ranks or the records changed
__global__ void k_fl_rank_records(const uint32_t* __restrict__ idx_s, const uint2* __restrict__ rec, uint32_t nd, uint2* __restrict__ rank_rec) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < nd) rank_rec[r] = rec[idx_s[r]];
}

__device__ inline void fl_unpack_point_key(uint64_t k, int& x, int& y, int& z) {   // point_key (pcm_device.h) back to the voxel
  const uint64_t bkey = k >> 9;
  const uint32_t li = (uint32_t)(k & 511u);
  x = (((int)(bkey >> 36) - kBrickBias) << kBrickShift) + (int)(li >> 6);
  y = (((int)((bkey >> 18) & 0x3ffff) - kBrickBias) << kBrickShift) + (int)((li >> 3) & 7u);
  z = (((int)(bkey & 0x3ffff) - kBrickBias) << kBrickShift) + (int)(li & 7u);
}

// the dilation of k_nl_keys over the touched voxels: one key per (touched voxel, offset); a touched key equal to its predecessor
// (the batch's keys are sorted: a voxel's points follow one another) or ~0 gives none.  grid = ceil(nt / 256)
__global__ void k_fl_dirty_keys(const uint64_t* __restrict__ touched, uint32_t nt, int nn, uint64_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt) return;
  const uint64_t t = touched[i];
  const bool skip = t == ~0ull || (i > 0 && touched[i - 1] == t);
  int cx = 0, cy = 0, cz = 0;
  fl_unpack_point_key(t, cx, cy, cz);
  const int lim = kKeyBias - 64;
  for (int g = 0; g < nn; g++) {
    const int x = cx - c_nearby[g][0], y = cy - c_nearby[g][1], z = cz - c_nearby[g][2];
    const bool ok = !skip && x > -lim && x < lim && y > -lim && y < lim && z > -lim && z < lim;
    keys[(size_t)i * nn + g] = ok ? nl_pack(x, y, z) : ~0ull;
  }
}
// distinct keys to the front; their number to ctr[kTotDirty]
enum { kTotDirty = 0, kTotNew, kTotRelocEntries, kTotRelocated, kTotInPlace, kTotWasted, kTotLiveAdded, kTotLiveRemoved, kTotBecameEmpty, kTotLeftEmpty, kTotWords = 16 };
__global__ void k_fl_compact(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint32_t n, uint64_t* __restrict__ out, unsigned long long* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == n - 1) ctr[kTotDirty] = pos[i] + flag[i];
  if (flag[i]) out[pos[i]] = keys[i];
}

// What becomes of every dirty list: its new padded length from the updated map, its record in the index as it was before the
// update (none: a new list voxel), and from the two whether it is rewritten in place or placed at the bump pointer (list_pool.h).
// Entries past the dirty count are cleared, so the scans over the whole arrays are the scans over the dirty lists.
struct DirtyList { uint32_t id, start, cap, len; };   // id: ~0 = new; start / cap: the old run; len: the new padded length
__global__ void k_fl_classify(const uint64_t* __restrict__ dirty, uint32_t nk, TargetView tg, int nn, TargetView index, const uint32_t* __restrict__ index_idx, const uint2* __restrict__ rec,
                              const uint32_t* __restrict__ rec_cap, DirtyList* __restrict__ out, uint32_t* __restrict__ newcap, uint32_t* __restrict__ isnew, unsigned long long* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nk) return;
  if (i >= ctr[kTotDirty]) { newcap[i] = 0; isnew[i] = 0; return; }
  int cx, cy, cz;
  nl_unpack(dirty[i], cx, cy, cz);
  DirtyList d;
  d.len = nl_gather<false>(tg, nn, cx, cy, cz, nullptr);
  const int rank = voxel_rank(index, cx, cy, cz);
  d.id = ~0u; d.start = 0; d.cap = 0;
  uint32_t old_len = 0;
  if (rank >= 0) {
    d.id = index_idx[rank];
    const uint2 r = rec[d.id];
    d.start = r.x; old_len = r.y; d.cap = rec_cap[d.id];
  }
  const bool fresh = rank < 0, stay = list_pool::rewrite_in_place(d.len, d.cap);
  const uint32_t cap_new = stay ? 0u : list_pool::grown_capacity(d.len);
  out[i] = d;
  newcap[i] = cap_new;
  isnew[i] = fresh ? 1u : 0u;
  if (fresh) atomicAdd(&ctr[kTotNew], 1ull);
  else if (stay) atomicAdd(&ctr[kTotInPlace], 1ull);
  else { atomicAdd(&ctr[kTotRelocated], 1ull); atomicAdd(&ctr[kTotWasted], (unsigned long long)d.cap); }
  if (cap_new) atomicAdd(&ctr[kTotRelocEntries], (unsigned long long)cap_new);
  if (d.len) atomicAdd(&ctr[kTotLiveAdded], (unsigned long long)d.len);
  if (old_len) atomicAdd(&ctr[kTotLiveRemoved], (unsigned long long)old_len);
  if (d.len == 0 && (fresh || old_len != 0)) atomicAdd(&ctr[kTotBecameEmpty], 1ull);
  if (d.len != 0 && !fresh && old_len == 0) atomicAdd(&ctr[kTotLeftEmpty], 1ull);
}

// The rewrite: a new list voxel gets the next id and its centre goes to the log; a run that does not stay gets its place behind
// the bump pointer; every dirty run is gathered again, the bytes nl_gather<true> would write (k_nl_lists).  One WAVE per dirty list
// (block = kRewriteWaves waves): lane g < nn resolves neighbourhood offset g (c_nearby order) to its voxel's run in the map, a wave
// prefix sum over the run lengths in offset order gives every cell its place, and the 64 lanes copy cell after cell with
// coalesced 16-byte loads and stores (w = the point's index in the map array), then the +inf pad entries up to the whole trip.
// The record, the capacity and a new list voxel's centre are lane 0's.  Every condition in front of the prefix sum is
// wave-uniform, so all 64 lanes take part in it.  A write never passes d.len, the padded length classify reserved room for.
constexpr uint32_t kRewriteWaves = 4;
__global__ void __launch_bounds__(64 * kRewriteWaves) k_fl_rewrite(const uint64_t* __restrict__ dirty, uint32_t nd, TargetView tg, int nn, const DirtyList* __restrict__ lists,
                             const uint32_t* __restrict__ newcap, const uint32_t* __restrict__ reloc_off, const uint32_t* __restrict__ isnew, const uint32_t* __restrict__ new_off,
                             uint32_t first_new_id, uint32_t bump, float res, float4* __restrict__ centres, uint2* __restrict__ rec, uint32_t* __restrict__ rec_cap,
                             float4* __restrict__ pool) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * kRewriteWaves + (threadIdx.x >> 6);   // the same in every lane of a wave
  if (i >= nd) return;
  int cx, cy, cz;
  nl_unpack(dirty[i], cx, cy, cz);
  const DirtyList d = lists[i];
  uint32_t id = d.id, start = d.start, cap = d.cap;
  const bool fresh = isnew[i] != 0;
  if (fresh) id = first_new_id + new_off[i];
  if (!list_pool::rewrite_in_place(d.len, d.cap)) { start = bump + reloc_off[i]; cap = newcap[i]; }
  if (lane == 0) {
    if (fresh) centres[id] = make_float4((float)cx * res, (float)cy * res, (float)cz * res, 0.f);   // COORD_ROUND: k_nl_centres with shift 0
    rec[id] = make_uint2(start, d.len);
    rec_cap[id] = cap;
  }
  if (d.len == 0) return;
  uint32_t s = 0, n = 0;
  if ((int)lane < nn) {   // nearby_grids_ order  ivox3d.h:211-235
    const int v = voxel_rank(tg, cx + c_nearby[lane][0], cy + c_nearby[lane][1], cz + c_nearby[lane][2]);
    if (v >= 0) {
      uint32_t e;
      voxel_run(tg, (uint32_t)v, s, e);
      n = e - s;
    }
  }
  const uint32_t incl = scan_add_wave(n), excl = incl - n;
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  float4* const out = pool + start;
  for (int g = 0; g < nn; g++) {
    const uint32_t sg = (uint32_t)__builtin_amdgcn_readlane((int)s, g), ng = (uint32_t)__builtin_amdgcn_readlane((int)n, g), og = (uint32_t)__builtin_amdgcn_readlane((int)excl, g);
    for (uint32_t k = lane; k < ng; k += 64u) {   // the voxel's points in insertion order (points_)  ivox3d_node.hpp:158-166
      float4 p = gload4(tg.pts + sg + k);
      p.w = __uint_as_float(sg + k);
      if (og + k < d.len) out[og + k] = p;
    }
  }
  const uint32_t padded = (total + (kListTrip - 1u)) & ~(kListTrip - 1u);
  const float inf = __builtin_inff();
  const uint32_t k = total + lane;
  if (lane < kListTrip && k < padded && k < d.len) out[k] = make_float4(inf, inf, inf, __uint_as_float(kListPadId));
}

// parity hook: the pooled runs into contiguous order by rank
__global__ void k_fl_lengths(const uint2* __restrict__ rank_rec, uint32_t nd, uint32_t* __restrict__ len) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r <= nd) len[r] = r < nd ? rank_rec[r].y : 0u;
}
__global__ void k_fl_export(const uint2* __restrict__ rank_rec, const uint32_t* __restrict__ start, uint32_t nd, const float4* __restrict__ pool, float4* __restrict__ out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nd) return;
  const uint2 v = rank_rec[r];
  for (uint32_t k = 0; k < v.y; k++) out[start[r] + k] = pool[v.x + k];
}

}  // namespace

// a list's records hold `n` lists (growth keeps the first `keep`)
static int reserve_records(hipStream_t stream, std::string* err, NeighbourLists* nl, size_t n, size_t keep) {
  const size_t cap = n + n / 4 + 1024;
  if (const int rc = nl->rec.reserve_keep(stream, err, n, cap, keep); rc != PCM_OK) return rc;
  if (const int rc = nl->rec_cap.reserve_keep(stream, err, n, cap, keep); rc != PCM_OK) return rc;
  return nl->rank_rec.reserve(stream, err, n, cap);
}

// the contiguous runs of a full build become the pool's first entries (capacity = length); `len`: their padded lengths by rank
static int pool_the_lists(ListBuild& b, const uint32_t* len) {
  NeighbourLists* out = b.out;
  const uint32_t nd = b.nd;
  if (const int rc = reserve_records(b.stream, b.err, out, nd, 0); rc != PCM_OK) return rc;
  k_fl_records<<<(nd + 255) / 256, 256, 0, b.stream>>>(out->index.idx_s, out->start, len, nd, out->rec, out->rec_cap, out->rank_rec);
  PCM_HIPCK_ERR(b.err, hipGetLastError());
  const size_t tail = (size_t)list_pool::Pool::tail();
  PCM_HIPCK_ERR(b.err, hipMemsetAsync(out->pts + (out->pts.cap - tail), 0, sizeof(float4) * tail, b.stream));   // the kWalkAhead zeroed trips behind the pool's end
  out->pool.built(out->pts.cap, out->num_candidates, nd, 0, b.follow->by_policy);   // no list of a full build is empty: a dilated voxel has an occupied neighbour
  out->pooled = true;
  return PCM_OK;
}

// kinds 0 (points) and 1 (`ndt_leaves`): list lengths -> starts -> candidates; the total length to the host (one read-back)
static int fill_lists(ListBuild& b, const PclLeaf* ndt_leaves, size_t list_entries) {
  NeighbourLists* out = b.out;
  hipStream_t stream = b.stream;
  const TargetMap& map = b.map;
  const uint32_t nd = b.nd;
  const int nn = b.nn, mode = map.coord_mode;
  const bool point_lists = !ndt_leaves;   // runs padded to whole trips (kListTrip)
  // A point list ends with at most kListTrip - 1 pad entries: the 32-bit starts and the memory must hold them too (the scratch of
  // the build is still taken here, so only the lists themselves are asked for)
  const size_t pad_max = point_lists ? (size_t)nd * (kListTrip - 1) : 0;
  if (list_entries + pad_max >= (1ull << 32)) { *b.err = "neighbour lists: map too large"; return PCM_ERR_UNSUPPORTED; }
  if (pad_max)
    if (const int rc = room_for((list_entries + pad_max) * sizeof(float4) + ((size_t)64 << 20), b.err); rc != PCM_OK) return rc;
  if (const int rc = out->start.reserve(stream, b.err, (size_t)nd + 1, (size_t)nd + 1); rc != PCM_OK) return rc;
  uint32_t *len = nullptr, h_total = 0;
  if (b.sc.take(&len, (size_t)nd + 1, b.err, "list lengths")) return PCM_ERR_HIP;
  PCM_HIPCK_ERR(b.err, hipMemsetAsync(len, 0, sizeof(uint32_t) * ((size_t)nd + 1), stream));
  if (ndt_leaves) k_nl_leaf_lists<false><<<(nd + 127) / 128, 128, 0, stream>>>(out->index.pts, nd, view_of(map), mode, ndt_leaves, nn, len, nullptr, nullptr);
  else k_nl_lists<false><<<(nd + 127) / 128, 128, 0, stream>>>(out->index.pts, nd, view_of(map), mode, nn, len, nullptr, nullptr);
  PCM_HIPCK_ERR(b.err, hipGetLastError());
  if (const int rc = scratch_exclusive_scan(b.sc, b.err, len, out->start.p, (size_t)nd + 1); rc != PCM_OK) return rc;
  PCM_HIPCK_ERR(b.err, hipMemcpyAsync(&h_total, out->start + nd, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  PCM_HIPCK_ERR(b.err, hipStreamSynchronize(stream));
  const size_t total = h_total;
  // The starts of the point lists are multiples of kListTrip entries = 64 bytes and DevBuf's hipMalloc returns at least 256-byte
  // aligned memory, so every run starts on a 64-byte boundary; `total` counts the pad entries, so the last trip of the last run
  // ends inside the array.  Zeroed tail: the walk of the leaf lists (pclndt.hip) reads (never uses) up to three entries past a
  // run, the keyed walk of k_linearize_lists loads (never offers) kWalkAhead trips past one.
  const size_t tail = point_lists ? (size_t)kListTrip * kWalkAhead : 4;
  static_assert(kListTrip * kWalkAhead >= 4, "the tail of the point lists is no shorter than that of the leaf lists");
  const size_t alloc = b.follow ? (size_t)list_pool::Pool::capacity_for(total, b.follow->headroom_fraction, b.follow->headroom_min) : total + tail;
  if (alloc >= (1ull << 32)) { *b.err = "neighbour lists: map too large"; return PCM_ERR_UNSUPPORTED; }
  if (const int rc = out->pts.reserve(stream, b.err, alloc, b.follow ? std::min<size_t>(alloc + alloc / 4, 0xfffffff0u) : alloc); rc != PCM_OK) return rc;
  PCM_HIPCK_ERR(b.err, hipMemsetAsync(out->pts + total, 0, sizeof(float4) * tail, stream));
  if (ndt_leaves) k_nl_leaf_lists<true><<<(nd + 127) / 128, 128, 0, stream>>>(out->index.pts, nd, view_of(map), mode, ndt_leaves, nn, nullptr, out->start, out->pts);
  else k_nl_lists<true><<<(nd + 127) / 128, 128, 0, stream>>>(out->index.pts, nd, view_of(map), mode, nn, nullptr, out->start, out->pts);
  PCM_HIPCK_ERR(b.err, hipGetLastError());
  PCM_HIPCK_ERR(b.err, hipStreamSynchronize(stream));
  out->num_lists = nd;
  out->num_candidates = total;
  out->num_neighbors = nn;
  out->kind = ndt_leaves ? 1 : 0;
  out->pooled = false;
  out->stale = false;
  if (b.follow)
    if (const int rc = pool_the_lists(b, len); rc != PCM_OK) return rc;
  out->valid = true;
  return PCM_OK;
}

// Build the lists of `map` for the neighbourhood `nn`, of one of three kinds (NeighbourLists::kind):
//   0  neither `ndt_leaves` nor `voxel_slots`: candidate POINTS of the nn = 1 / 7 / 19 / 27 cells, runs padded to whole trips;
//   1  `ndt_leaves` (pclomp NDT): neighbour LEAVES, nn = 0 for the KDTREE search, else 1 / 7 / 27;
//   2  `voxel_slots` (k_ndt): a fixed row of nn = 1 / 7 / 27 neighbour voxel indices per list voxel.
// Host syncs: the number of dilated voxels, the index build's own, the total list length (kind 2: the end of its one kernel).
int build_neighbour_lists(hipStream_t stream, const TargetMap& map, int nn, NeighbourLists* out, std::string* err, const PclLeaf* ndt_leaves, bool voxel_slots, const ListFollow* follow) {
  out->valid = false;
  out->pooled = false;
  out->stale = false;
  out->generation++;
  if (follow && (ndt_leaves || voxel_slots)) { *err = "neighbour lists: only candidate lists of points follow a target"; return PCM_ERR_INTERNAL; }
  const int mode = map.coord_mode;
  if (!map.valid || (mode != COORD_ROUND && mode != COORD_FLOOR_MUL && mode != COORD_FLOOR_HALF)) { *err = "neighbour lists: unsupported voxel convention"; return PCM_ERR_UNSUPPORTED; }
  if (voxel_slots ? (nn != 1 && nn != 7 && nn != 27) : ndt_leaves ? (nn != 0 && nn != 1 && nn != 7 && nn != 27) : (nn != 1 && nn != 7 && nn != 19 && nn != 27)) { *err = "neighbour lists: unsupported neighbourhood"; return PCM_ERR_INVALID_ARGUMENT; }
  ListBuild b{stream, err, map, out, DevScratch(stream), nn, nn == 0 ? 27 : nn, 0};
  b.follow = follow;
  b.nk = (size_t)map.num_voxels * b.nset;
  if (b.nk >= (1ull << 31) || (size_t)map.num_points * b.nset >= (1ull << 32)) { *err = "neighbour lists: map too large"; return PCM_ERR_UNSUPPORTED; }
  // room for them?  27 x 16 B per map point for the lists (the pad entries of the point lists come on top: fill_lists, once the
  // number of lists is known), ~56 B per (voxel, offset) key while they are built
  const size_t list_entries = (!ndt_leaves && !voxel_slots ? (size_t)map.num_points : (size_t)map.num_voxels) * b.nset;
  int rc = room_for(list_entries * sizeof(float4) + b.nk * 56 + ((size_t)64 << 20), err);
  if (rc == PCM_OK) rc = dilated_voxels(b);
  if (rc == PCM_OK) rc = list_index(b);
  if (rc == PCM_OK) rc = voxel_slots ? voxel_slot_rows(b) : fill_lists(b, ndt_leaves, list_entries);
  if (rc != PCM_OK) out->valid = false;
  return rc;
}

// ---------------------------------------------------------------------------
// update_neighbour_lists in stages over one ListUpdate
// ---------------------------------------------------------------------------
struct ListUpdate {
  hipStream_t stream;
  std::string* err;
  const TargetMap& map;
  NeighbourLists* nl;
  DevScratch sc;
  int nn;
  uint32_t nk;                    // (touched voxel, offset) keys: the most lists an update can dirty
  uint64_t* dirty = nullptr;      // the dirty lists' keys, distinct, ascending; their number is ctr[kTotDirty]
  unsigned long long* ctr = nullptr;   // the update's totals (kTot*), 64-bit sums
  DirtyList* lists = nullptr;
  uint32_t *newcap = nullptr, *reloc_off = nullptr, *isnew = nullptr, *new_off = nullptr;
  list_pool::Totals tot;
};

// stage 1 + 2: the touched voxels dilated by the neighbourhood, sorted, duplicates removed
static int dirty_lists(ListUpdate& u) {
  const uint32_t nt = u.map.touched_n, nk = u.nk;
  uint64_t* keys = nullptr;
  DistinctKeys dk;
  if (u.sc.take(&keys, nk, u.err, "dirty keys") || u.sc.take(&u.dirty, nk, u.err, "dirty lists") || u.sc.take(&u.ctr, kTotWords, u.err, "update totals")) return PCM_ERR_HIP;
  PCM_HIPCK_ERR(u.err, hipMemsetAsync(u.ctr, 0, sizeof(unsigned long long) * kTotWords, u.stream));
  k_fl_dirty_keys<<<(nt + 255) / 256, 256, 0, u.stream>>>(u.map.touched, nt, u.nn, keys);
  PCM_HIPCK_ERR(u.err, hipGetLastError());
  if (const int rc = distinct_keys(u.sc, u.err, keys, nk, &dk); rc != PCM_OK) return rc;
  k_fl_compact<<<(nk + 255) / 256, 256, 0, u.stream>>>(dk.sorted, dk.flag, dk.pos, nk, u.dirty, u.ctr);
  PCM_HIPCK_ERR(u.err, hipGetLastError());
  return PCM_OK;
}

// stage 3 + the first half of 4: new length, old record and the way of every dirty list; where the relocated runs and the new
// lists go (two scans); the totals to the host -- the update's one read-back
static int classify(ListUpdate& u) {
  NeighbourLists* nl = u.nl;
  const uint32_t nk = u.nk;
  if (u.sc.take(&u.lists, nk, u.err, "dirty list records") || u.sc.take(&u.newcap, nk, u.err, "relocated capacities") || u.sc.take(&u.reloc_off, nk, u.err, "relocation offsets")) return PCM_ERR_HIP;
  if (u.sc.take(&u.isnew, nk, u.err, "new list flags") || u.sc.take(&u.new_off, nk, u.err, "new list ids")) return PCM_ERR_HIP;
  if (const int rc = nl->h_totals.reserve(u.stream, u.err, kTotWords, kTotWords); rc != PCM_OK) return rc;
  k_fl_classify<<<(nk + 127) / 128, 128, 0, u.stream>>>(u.dirty, nk, view_of(u.map), u.nn, view_of(nl->index), nl->index.idx_s, nl->rec, nl->rec_cap, u.lists, u.newcap, u.isnew, u.ctr);
  PCM_HIPCK_ERR(u.err, hipGetLastError());
  if (const int rc = scratch_exclusive_scan(u.sc, u.err, u.newcap, u.reloc_off, nk); rc != PCM_OK) return rc;
  if (const int rc = scratch_exclusive_scan(u.sc, u.err, u.isnew, u.new_off, nk); rc != PCM_OK) return rc;
  PCM_HIPCK_ERR(u.err, hipMemcpyAsync(nl->h_totals.p, u.ctr, sizeof(unsigned long long) * kTotWords, hipMemcpyDeviceToHost, u.stream));
  PCM_HIPCK_ERR(u.err, hipStreamSynchronize(u.stream));
  const unsigned long long* h = nl->h_totals.p;
  list_pool::Totals& t = u.tot;
  t.dirty = h[kTotDirty]; t.new_lists = h[kTotNew]; t.reloc_entries = h[kTotRelocEntries]; t.relocated = h[kTotRelocated]; t.in_place = h[kTotInPlace];
  t.wasted_added = h[kTotWasted]; t.live_added = h[kTotLiveAdded]; t.live_removed = h[kTotLiveRemoved]; t.became_empty = h[kTotBecameEmpty]; t.left_empty = h[kTotLeftEmpty];
  return PCM_OK;
}

// stage 4: the dirty runs again from the updated map, in place or behind the bump pointer; the centres of new list voxels to the log
static int rewrite(ListUpdate& u) {
  NeighbourLists* nl = u.nl;
  const size_t n_old = nl->num_lists, n_new = n_old + u.tot.new_lists;
  if (u.tot.new_lists) {
    if (const int rc = nl->centres.reserve_keep(u.stream, u.err, n_new, n_new + n_new / 4 + 1024, n_old); rc != PCM_OK) return rc;
    if (const int rc = reserve_records(u.stream, u.err, nl, n_new, n_old); rc != PCM_OK) return rc;
  }
  if (u.tot.dirty) {
    k_fl_rewrite<<<((uint32_t)u.tot.dirty + kRewriteWaves - 1u) / kRewriteWaves, 64 * kRewriteWaves, 0, u.stream>>>(u.dirty, (uint32_t)u.tot.dirty, view_of(u.map), u.nn, u.lists, u.newcap, u.reloc_off, u.isnew, u.new_off, (uint32_t)n_old,
                                                                 (uint32_t)nl->pool.bump, u.map.res, nl->centres, nl->rec, nl->rec_cap, nl->pts);
    PCM_HIPCK_ERR(u.err, hipGetLastError());
  }
  return PCM_OK;
}

// stage 3, second half: the new list voxels' stand-in points, appended to the log, are merged into the index (build_target_map's
// incremental path; its own host syncs); the ranks shift, so the kernel's rank -> record table is derived again either way
static int merge_index(ListUpdate& u) {
  NeighbourLists* nl = u.nl;
  if (u.tot.new_lists) {
    uint32_t n = nl->num_lists + (uint32_t)u.tot.new_lists;   // <= dirty <= nk < 2^31
    MapBuildOptions opt; opt.n_indexed = nl->index.index_n;
    if (const int rc = build_target_map(u.stream, nl->centres, &n, u.map.res, u.map.coord_mode, &nl->index, u.err, opt); rc != PCM_OK) return rc;
    if (nl->index.num_voxels != n || nl->index.num_points != n) { *u.err = "neighbour lists: index does not hold one voxel per list"; return PCM_ERR_INTERNAL; }
    nl->num_lists = n;
  }
  k_fl_rank_records<<<(nl->num_lists + 255) / 256, 256, 0, u.stream>>>(nl->index.idx_s, nl->rec, nl->num_lists, nl->rank_rec);
  PCM_HIPCK_ERR(u.err, hipGetLastError());
  return PCM_OK;
}

int update_neighbour_lists(hipStream_t stream, const TargetMap& map, NeighbourLists* nl, std::string* err, bool* rebuild) {
  *rebuild = false;
  if (!nl->valid || !nl->pooled || nl->kind != 0 || !map.valid || !map.touched_valid || map.coord_mode != COORD_ROUND) { *rebuild = true; return PCM_OK; }
  if ((size_t)map.touched_n * nl->num_neighbors >= (1ull << 31)) { *rebuild = true; return PCM_OK; }
  if (map.touched_n == 0) { nl->stale = false; return PCM_OK; }
  ListUpdate u{stream, err, map, nl, DevScratch(stream), nl->num_neighbors, map.touched_n * (uint32_t)nl->num_neighbors};
  nl->generation++;
  // nl->time_stages (pcm_set_profiling bit 0): HIP events around the stages, read after the update (one more synchronisation)
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int nev = 0;
  auto mark = [&]() { if (nl->time_stages && nev < 5 && hipEventCreate(&ev[nev]) == hipSuccess) { (void)hipEventRecord(ev[nev], stream); nev++; } };
  for (float& m : nl->stage_ms) m = 0.f;
  mark();
  int rc = dirty_lists(u);
  mark();
  if (rc == PCM_OK) rc = classify(u);
  mark();
  const bool apply = rc == PCM_OK && nl->pool.decide(u.tot) == list_pool::kApply;   // stage 5: nothing was written yet
  if (apply) rc = rewrite(u);
  mark();
  if (apply && rc == PCM_OK) rc = merge_index(u);
  mark();
  if (nev == 5 && rc == PCM_OK && hipEventSynchronize(ev[4]) == hipSuccess) {
    for (int k = 0; k < 4; k++) (void)hipEventElapsedTime(&nl->stage_ms[k], ev[k], ev[k + 1]);
    (void)hipEventElapsedTime(&nl->stage_ms[4], ev[0], ev[4]);
  }
  for (int k = 0; k < nev; k++) (void)hipEventDestroy(ev[k]);
  if (rc == PCM_OK && !apply) { *rebuild = true; return PCM_OK; }
  if (rc != PCM_OK) { nl->valid = false; return rc; }
  nl->pool.apply(u.tot);
  nl->num_candidates = (size_t)nl->pool.bump;
  nl->stale = false;
  return PCM_OK;
}

int export_pooled_lists(hipStream_t stream, const NeighbourLists& nl, std::vector<uint32_t>* starts, DevBuf<float4>* entries, std::string* err) {
  const uint32_t nd = nl.num_lists;
  DevScratch sc(stream);
  uint32_t *len = nullptr, *start = nullptr;
  if (sc.take(&len, (size_t)nd + 1, err, "list lengths") || sc.take(&start, (size_t)nd + 1, err, "list starts")) return PCM_ERR_HIP;
  k_fl_lengths<<<(nd + 256) / 256, 256, 0, stream>>>(nl.rank_rec, nd, len);
  PCM_HIPCK_ERR(err, hipGetLastError());
  if (const int rc = scratch_exclusive_scan(sc, err, len, start, (size_t)nd + 1); rc != PCM_OK) return rc;
  starts->resize((size_t)nd + 1);
  PCM_HIPCK_ERR(err, hipMemcpyAsync(starts->data(), start, sizeof(uint32_t) * ((size_t)nd + 1), hipMemcpyDeviceToHost, stream));
  PCM_HIPCK_ERR(err, hipStreamSynchronize(stream));
  const size_t total = starts->back();
  if (const int rc = entries->reserve(stream, err, total, total); rc != PCM_OK) return rc;
  k_fl_export<<<(nd + 127) / 128, 128, 0, stream>>>(nl.rank_rec, start, nd, nl.pts, entries->p);
  PCM_HIPCK_ERR(err, hipGetLastError());
  PCM_HIPCK_ERR(err, hipStreamSynchronize(stream));
  return PCM_OK;
}

// distance2() of ivox3d_node.hpp:13-16, the operations of best_offer in its order
__device__ inline float list_d2(const float4& mp, const float (&q)[3]) {
  const float dx = mp.x - q[0], dy = mp.y - q[1], dz = mp.z - q[2];
  return dx * dx + dy * dy + dz * dz;
}

// list_d2 for the keyed walk, the same operations in the same order on plain f32 instructions.  Left alone, the SLP vectoriser
// pairs the z and x squares of a candidate (v_pk_add_f32 / v_pk_mul_f32 on (z, x) against (q.z, q.x)): x has to be copied next to z
// first, into the dead w register of its load, one v_mov per candidate and for the carried buffer a second one, behind a wait for
// loads the turn does not need yet; and a packed f32 instruction costs more issue time than the two plain ones it replaces
// ("Padded runs").  An empty statement that takes a square and hands it back issues nothing, and a value
// that comes out of it is no multiply the vectoriser could pair with another.  With contraction off a packed instruction rounds
// each half as the plain one does: same bits.
__device__ inline float walk_plain(float v) {
  asm("" : "+v"(v));
  return v;
}
__device__ inline float walk_d2(const float4& mp, const float (&q)[3]) {
  const float dx = mp.x - q[0], dy = mp.y - q[1], dz = mp.z - q[2];
  return walk_plain(dx * dx) + walk_plain(dy * dy) + walk_plain(dz * dz);
}

// one trip of the keyed walk: its four loads, and its four candidates into the key network in list order
__device__ inline void walk_load(float4 (&c)[kListTrip], const float4* p) {
#pragma unroll
  for (uint32_t j = 0; j < kListTrip; j++) c[j] = gload4(p + j);
}
// PLAIN: the distances by walk_d2 (k_linearize_lists) or by list_d2 as the compiler packs it (lists_knn, see there).
template <bool PLAIN>
__device__ inline void walk_offer(KeyedBest& kb, const float4 (&c)[kListTrip], const float (&q)[3], uint32_t pos) {
  // An empty statement that reads the four w components (the candidates' indices, which the keyed walk does not need): it issues
  // nothing.  Without it the register allocator treats the w register of a load that is still in flight as free, parks a
  // temporary of the running trip in it, and the compiler must then wait for that load before the temporary is written -- a full
  // wait in the middle of the trip the load was issued ahead of.
  asm volatile("" ::"v"(c[0].w), "v"(c[1].w), "v"(c[2].w), "v"(c[3].w));
  float d0, d1, d2, d3;
  if constexpr (PLAIN) { d0 = walk_d2(c[0], q); d1 = walk_d2(c[1], q); d2 = walk_d2(c[2], q); d3 = walk_d2(c[3], q); }
  else { d0 = list_d2(c[0], q); d1 = list_d2(c[1], q); d2 = list_d2(c[2], q); d3 = list_d2(c[3], q); }
  keyed_offer(kb, keyed_pack(d0, pos));
  keyed_offer(kb, keyed_pack(d1, pos + 1));
  keyed_offer(kb, keyed_pack(d2, pos + 2));
  keyed_offer(kb, keyed_pack(d3, pos + 3));
}

// The 5-NN of query q among the candidates of list r, and those candidates again for the fit: bi[j] = index of the j-th best in
// nl.pts (j < bm), bm = min(K, #in range), fp[j] = its entry (the run's first entry beyond bm, never used).  The search of
// k_lio_lists.  It is a copy of the walk inside k_linearize_lists below, statement for statement: called from there it changed that
// kernel's register allocation (88 -> 86 VGPRs, another schedule), and that kernel is the measured one, so the twin stays written
// out.  A change of the walk goes to both -- but for the plain-f32 distances (walk_d2): with them this kernel's allocation goes from
// 96 to 98 registers, four waves per SIMD instead of five, for every placement of the barriers that was built (the peak is in the
// fit and the tail, which keep bi[] and the body point live; held to five waves it spills three dwords).  So the twin walks on
// list_d2 and compiles to the instructions it had.
template <bool POOLED>
__device__ inline void lists_knn(const TargetView& nl, uint32_t r, const float (&q)[3], float max_range_sq, uint32_t (&bi)[K], int& bm, float4 (&fp)[K]) {
  uint32_t s, e;
  if constexpr (POOLED) {
    const unsigned long long run_rec = *(const PCM_GLOBAL unsigned long long*)(reinterpret_cast<const unsigned long long*>(nl.vox_start) + r);   // one 8-byte load
    s = (uint32_t)run_rec; e = s + (uint32_t)(run_rec >> 32);
  } else {
    voxel_run(nl, r, s, e);
  }
  // the voxel's candidates in the reference's visit order, four per trip.  The run is padded to whole trips and starts on a
  // 64-byte boundary (build_neighbour_lists), so e - s is a multiple of four: no bounds test, all four loads under way and all
  // four distances formed before the first offer.  A load past the run's true end is a pad entry (d2 = +inf) and is never
  // among the in-range entries.
  //
  // Keyed walk (keyed_best.h): a run of at most kKeyedMaxRun entries keeps the six smallest (distance, position) keys by a
  // branch-free min / med3 network.  The position `pos` is the same in every lane that is still walking, a scalar.
  bm = 0;
  const uint32_t len = e - s;
  const bool keyed = len <= kKeyedMaxRun;
  KeyedBest kb;
  keyed_init(kb);
  const float4* run = nl.pts + s;
  // Pipelined: the loads of trip pos + kWalkAhead * kListTrip are issued before trip pos is consumed, so they are in flight
  // while the distances and the network of trip pos issue.  No bounds test on them: a trip consumed at pos < len starts at
  // most kWalkAhead trips behind the run's last one, so the furthest entry read is s + len - kListTrip + kWalkAhead * kListTrip
  // + (kListTrip - 1) < e + kWalkAhead * kListTrip <= num_candidates + kWalkAhead * kListTrip, inside the array
  // (build_neighbour_lists keeps kWalkAhead zeroed trips behind the last run; for an empty run s <= num_candidates and the
  // same bound holds for the prologue).  What a load past e brings -- the head of the next run, or the zeroed tail -- belongs
  // to a trip at a position >= len: the loop ends before that trip is consumed, its registers are dropped, nothing of it is
  // offered.  A lane whose run is longer than kKeyedMaxRun loads nothing here: no prologue, and it never enters the loop.
  float4 buf[kWalkAhead + 1][kListTrip];
  if (keyed) {
#pragma unroll
    for (uint32_t u = 0; u < kWalkAhead; u++) walk_load(buf[u], run + u * kListTrip);
  }
  // kWalkAhead + 1 trips per turn, the buffers in fixed roles (no copies): at the top buf[u] holds trip pos + u * kListTrip
  // for u < kWalkAhead; step u loads trip u + kWalkAhead into the buffer that step u - 1 emptied and consumes buf[u].  The
  // turn runs while all its trips are inside the run; the at most kWalkAhead trips left are loaded already.
  uint32_t pos = 0;
  for (; pos + kWalkAhead * kListTrip < (keyed ? len : 0u); pos += (kWalkAhead + 1) * kListTrip) {
#pragma unroll
    for (uint32_t u = 0; u <= kWalkAhead; u++) {
      walk_load(buf[(u + kWalkAhead) % (kWalkAhead + 1)], run + pos + (u + kWalkAhead) * kListTrip);
      walk_offer<false>(kb, buf[u], q, pos + u * kListTrip);
    }
  }
#pragma unroll
  for (uint32_t u = 0; u < kWalkAhead; u++) {
    if (pos + u * kListTrip < (keyed ? len : 0u)) walk_offer<false>(kb, buf[u], q, pos + u * kListTrip);
  }
  uint32_t kpos[kKeyedBest];
  const bool decided = keyed_decode(kb, max_range_sq, kpos, bm) && keyed;
#pragma unroll
  for (int j = 0; j < K; j++) bi[j] = s + kpos[j];
  // An ambiguous lane (ties, near-ties, the range boundary, a run longer than kKeyedMaxRun) repeats its walk with the running
  // list of the other kernels: the same offers in the same visit order.  The wave branches over this when no lane needs it.
  if (!decided) {
    Best best;
    best_init(best, max_range_sq);
    for (uint32_t k = s; k < e; k += kListTrip) {
      const float4 c0 = gload4(nl.pts + k), c1 = gload4(nl.pts + k + 1), c2 = gload4(nl.pts + k + 2), c3 = gload4(nl.pts + k + 3);
      const float d0 = list_d2(c0, q), d1 = list_d2(c1, q), d2 = list_d2(c2, q), d3 = list_d2(c3, q);
      best_offer_d2(best, d0, k, max_range_sq);
      best_offer_d2(best, d1, k + 1, max_range_sq);
      best_offer_d2(best, d2, k + 2, max_range_sq);
      best_offer_d2(best, d3, k + 3, max_range_sq);
    }
    best_finish(best);
    bm = best.m;
#pragma unroll
    for (int j = 0; j < K; j++) bi[j] = best.i[j];
  }
  // The five chosen candidates again, by index, for the fit: all five loads issued back to back ahead of the bm >= KMIN
  // test, one round trip.  (Guarded by `if (j < bm)` the fourth and the fifth load each sat in a branch of its own behind a
  // full wait: three round trips.)  Every lane loads five entries: entry j < bm is its j-th best, any other load reads the
  // run's first entry (address s: inside the array, see above) and its value is replaced by zero -- an index that bm
  // excludes is never formed into an address.
#pragma unroll
  for (int j = 0; j < K; j++) fp[j] = gload4(nl.pts + (j < bm ? bi[j] : s));
}

// ---------------------------------------------------------------------------
// k_linearize_lists: grid (ceil(N / 256), pairs), one scan point per lane
// ---------------------------------------------------------------------------
// POOLED: following lists -- the run of list r is the 8-byte record rank_rec[r] = (start, length) in the pool (the view's vox_start
// points at the records); the walk is the same code.
template <bool WRITE_PLANES, bool POOLED = false>
__global__ void __launch_bounds__(256) k_linearize_lists(const PairDesc* __restrict__ descs, const PairState* __restrict__ states, KernelParams kp) {
  // the tile placement of k_linearize (kernels.hip): neighbouring tiles of a pair share an XCD (they read the same lists)
  uint32_t tile_x = blockIdx.x;
  {
    const uint32_t base = blockIdx.x & ~63u, w = blockIdx.x & 63u;
    if (base + 64u <= gridDim.x) tile_x = base + (w & 7u) * 8u + (w >> 3);
  }
  const int pair = PCM_PAIR_OF(kp, blockIdx.y);
  if (states[pair].mode != MODE_LINEARIZE) return;
  const PairDesc d = descs[pair];
  const uint32_t i = tile_x * 256u + threadIdx.x;
  if (tile_x * 256u >= d.src.num_points) return;
  const bool live = i < d.src.num_points;
  const PoseF P = load_pose(states[pair].x0);
  const TargetView nl = d.nl;
  __shared__ __align__(16) unsigned char s_mem[kReduceLdsBytes];

  float4 pl = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
  float q[3] = {0.f, 0.f, 0.f};
  float pn_body = 0.f;
  if (live) {
    const float4 p = gload4(d.src.pts + i);
    pn_body = pcm_sqrtf_rn(p.x * p.x + p.y * p.y + p.z * p.z);
    transform(P, p, q);
    const float fx = roundf(q[0] * nl.inv_res), fy = roundf(q[1] * nl.inv_res), fz = roundf(q[2] * nl.inv_res);  // Pos2Grid  ivox3d.h:283-286
    const float lim = (float)(kCoordBias - 32);
    if (fabsf(fx) < lim && fabsf(fy) < lim && fabsf(fz) < lim) {   // also false for NaN
      const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
      const int rank = voxel_rank(nl, cx, cy, cz);   // the list index: voxel -> rank of its list
      if (rank >= 0) {
        const uint32_t r = (uint32_t)rank;
        uint32_t s, e;
        if constexpr (POOLED) {
          const unsigned long long run_rec = *(const PCM_GLOBAL unsigned long long*)(reinterpret_cast<const unsigned long long*>(nl.vox_start) + r);   // one 8-byte load
          s = (uint32_t)run_rec; e = s + (uint32_t)(run_rec >> 32);
        } else {
          voxel_run(nl, r, s, e);
        }
        // the voxel's candidates in the reference's visit order, four per trip.  The run is padded to whole trips and starts on a
        // 64-byte boundary (build_neighbour_lists), so e - s is a multiple of four: no bounds test, all four loads under way and all
        // four distances formed before the first offer.  A load past the run's true end is a pad entry (d2 = +inf) and is never
        // among the in-range entries.
        //
        // Keyed walk (keyed_best.h): a run of at most kKeyedMaxRun entries keeps the six smallest (distance, position) keys by a
        // branch-free min / med3 network.  The position `pos` is the same in every lane that is still walking, a scalar.
        uint32_t bi[K];
        int bm = 0;
        const uint32_t len = e - s;
        const bool keyed = len <= kKeyedMaxRun;
        KeyedBest kb;
        keyed_init(kb);
        const float4* run = nl.pts + s;
        // Pipelined: the loads of trip pos + kWalkAhead * kListTrip are issued before trip pos is consumed, so they are in flight
        // while the distances and the network of trip pos issue.  No bounds test on them: a trip consumed at pos < len starts at
        // most kWalkAhead trips behind the run's last one, so the furthest entry read is s + len - kListTrip + kWalkAhead * kListTrip
        // + (kListTrip - 1) < e + kWalkAhead * kListTrip <= num_candidates + kWalkAhead * kListTrip, inside the array
        // (build_neighbour_lists keeps kWalkAhead zeroed trips behind the last run; for an empty run s <= num_candidates and the
        // same bound holds for the prologue).  What a load past e brings -- the head of the next run, or the zeroed tail -- belongs
        // to a trip at a position >= len: the loop ends before that trip is consumed, its registers are dropped, nothing of it is
        // offered.  A lane whose run is longer than kKeyedMaxRun loads nothing here: no prologue, and it never enters the loop.
        float4 buf[kWalkAhead + 1][kListTrip];
        if (keyed) {
#pragma unroll
          for (uint32_t u = 0; u < kWalkAhead; u++) walk_load(buf[u], run + u * kListTrip);
        }
        // kWalkAhead + 1 trips per turn, the buffers in fixed roles (no copies): at the top buf[u] holds trip pos + u * kListTrip
        // for u < kWalkAhead; step u loads trip u + kWalkAhead into the buffer that step u - 1 emptied and consumes buf[u].  The
        // turn runs while all its trips are inside the run; the at most kWalkAhead trips left are loaded already.
        uint32_t pos = 0;
        for (; pos + kWalkAhead * kListTrip < (keyed ? len : 0u); pos += (kWalkAhead + 1) * kListTrip) {
#pragma unroll
          for (uint32_t u = 0; u <= kWalkAhead; u++) {
            walk_load(buf[(u + kWalkAhead) % (kWalkAhead + 1)], run + pos + (u + kWalkAhead) * kListTrip);
            walk_offer<true>(kb, buf[u], q, pos + u * kListTrip);
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < kWalkAhead; u++) {
          if (pos + u * kListTrip < (keyed ? len : 0u)) walk_offer<true>(kb, buf[u], q, pos + u * kListTrip);
        }
        uint32_t kpos[kKeyedBest];
        const bool decided = keyed_decode(kb, kp.max_range_sq, kpos, bm) && keyed;
#pragma unroll
        for (int j = 0; j < K; j++) bi[j] = s + kpos[j];
        // An ambiguous lane (ties, near-ties, the range boundary, a run longer than kKeyedMaxRun) repeats its walk with the running
        // list of the other kernels: the same offers in the same visit order.  The wave branches over this when no lane needs it.
        if (!decided) {
          Best best;
          best_init(best, kp.max_range_sq);
          for (uint32_t k = s; k < e; k += kListTrip) {
            const float4 c0 = gload4(nl.pts + k), c1 = gload4(nl.pts + k + 1), c2 = gload4(nl.pts + k + 2), c3 = gload4(nl.pts + k + 3);
            const float d0 = list_d2(c0, q), d1 = list_d2(c1, q), d2 = list_d2(c2, q), d3 = list_d2(c3, q);
            best_offer_d2(best, d0, k, kp.max_range_sq);
            best_offer_d2(best, d1, k + 1, kp.max_range_sq);
            best_offer_d2(best, d2, k + 2, kp.max_range_sq);
            best_offer_d2(best, d3, k + 3, kp.max_range_sq);
          }
          best_finish(best);
          bm = best.m;
#pragma unroll
          for (int j = 0; j < K; j++) bi[j] = best.i[j];
        }
        // The five chosen candidates again, by index, for the fit: all five loads issued back to back ahead of the bm >= KMIN
        // test, one round trip.  (Guarded by `if (j < bm)` the fourth and the fifth load each sat in a branch of its own behind a
        // full wait: three round trips.)  Every lane loads five entries: entry j < bm is its j-th best, any other load reads the
        // run's first entry (address s: inside the array, see above) and its value is replaced by zero -- an index that bm
        // excludes is never formed into an address.
        float4 fp[K];
#pragma unroll
        for (int j = 0; j < K; j++) fp[j] = gload4(nl.pts + (j < bm ? bi[j] : s));
        if (bm >= KMIN) {   // laser_mapping.cc:619-623
          float px[K], py[K], pz[K];
#pragma unroll
          for (int j = 0; j < K; j++) {
            asm volatile("" ::"v"(fp[j].w));   // see walk_offer
            px[j] = j < bm ? fp[j].x : 0.f; py[j] = j < bm ? fp[j].y : 0.f; pz[j] = j < bm ? fp[j].z : 0.f;
          }
          float4 fit;
          if (esti_plane<true>(px, py, pz, bm, kp.plane_threshold, &fit)) pl = fit;
        }
      }
    }
  }
  residual_and_reduce<WRITE_PLANES>(d, i, tile_x, live, pl, q, pn_body, s_mem);
}

void launch_linearize_lists(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp, int npairs, bool write_planes, bool pooled) {
  dim3 grid((unsigned)kp.tiles_per_pair, (unsigned)npairs);
  if (pooled && write_planes) k_linearize_lists<true, true><<<grid, 256, 0, stream>>>(d_descs, d_states, kp);
  else if (pooled) k_linearize_lists<false, true><<<grid, 256, 0, stream>>>(d_descs, d_states, kp);
  else if (write_planes) k_linearize_lists<true><<<grid, 256, 0, stream>>>(d_descs, d_states, kp);
  else k_linearize_lists<false><<<grid, 256, 0, stream>>>(d_descs, d_states, kp);
}

// ---------------------------------------------------------------------------
// k_lio_lists: the jueying_lio measurement model (LaserMapping::ObsModel) on candidate lists -- what k_linearize<.., LIO>
// (kernels.hip) computes, bit for bit, with the search of k_linearize_lists.  grid (ceil(N / 256), 1), one scan point per lane.
//   world point   lio_world_point / lio_body_norm with the float pose of the descriptor, as the tile kernel
//   search        Pos2Grid -> list index -> lists_knn (keyed walk, running-list fallback); a call that does not match
//                 (converge == false, laser_mapping.cc:616) reads the stored plane and walks nothing
//   fit           esti_plane<true> on the bm >= KMIN neighbours, verdict kept apart for the reference semantics
//   nearest_points_ (d.nn)   positions in the list entry array nl.pts, nearest first, ~0u beyond bm: the entries hold the xyz of
//                 the map's points, so k_map_filter reads them through that array (pcm_map_incremental)
//   tail          lio_row_and_reduce (linearize_common.h)
// POOLED as in k_linearize_lists; LIO_DEV: a round of pcm_lio_update, the converge flag k_iekf_step left in the descriptor.
// ---------------------------------------------------------------------------
template <bool POOLED, bool LIO_DEV>
__global__ void __launch_bounds__(256) k_lio_lists(const PairDesc* __restrict__ descs, const PairState* __restrict__ states, KernelParams kp) {
  uint32_t tile_x = blockIdx.x;
  {
    const uint32_t base = blockIdx.x & ~63u, w = blockIdx.x & 63u;
    if (base + 64u <= gridDim.x) tile_x = base + (w & 7u) * 8u + (w >> 3);
  }
  const int pair = PCM_PAIR_OF(kp, blockIdx.y);
  if (states[pair].mode != MODE_LINEARIZE) return;
  const PairDesc d = descs[pair];
  const uint32_t i = tile_x * 256u + threadIdx.x;
  if (tile_x * 256u >= d.src.num_points) return;
  const bool live = i < d.src.num_points;
  const TargetView nl = d.nl;
  const bool do_search = LIO_DEV ? d.lio.rematch != 0 : kp.lio_rematch != 0;
  __shared__ __align__(16) unsigned char s_mem[kLioReduceLdsBytes];

  float4 p = make_float4(0.f, 0.f, 0.f, 1.f);
  float4 pl = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
  float q[3] = {0.f, 0.f, 0.f};
  float pn_body = 0.f;
  bool ref_fit = false, ref_ok = false;
  if (live) {
    p = gload4(d.src.pts + i);
    pn_body = lio_body_norm(p);
    lio_world_point(d.lio.q_wl, d.lio.t_wl, p, q);
    if (do_search) {
      uint32_t bi[K];
      int bm = 0;
      const float fx = roundf(q[0] * nl.inv_res), fy = roundf(q[1] * nl.inv_res), fz = roundf(q[2] * nl.inv_res);  // Pos2Grid  ivox3d.h:283-286
      const float lim = (float)(kCoordBias - 32);
      if (fabsf(fx) < lim && fabsf(fy) < lim && fabsf(fz) < lim) {   // also false for NaN
        const int rank = voxel_rank(nl, (int)fx, (int)fy, (int)fz);
        if (rank >= 0) {
          float4 fp[K];
          lists_knn<POOLED>(nl, (uint32_t)rank, q, kp.max_range_sq, bi, bm, fp);
          if (bm >= KMIN) {   // laser_mapping.cc:619-623
            float px[K], py[K], pz[K];
#pragma unroll
            for (int j = 0; j < K; j++) {
              asm volatile("" ::"v"(fp[j].w));   // see walk_offer
              px[j] = j < bm ? fp[j].x : 0.f; py[j] = j < bm ? fp[j].y : 0.f; pz[j] = j < bm ? fp[j].z : 0.f;
            }
            float4 fit;
            const bool ok = esti_plane<true>(px, py, pz, bm, kp.plane_threshold, &fit);
            if (kp.lio_ref) { pl = fit; ref_fit = true; ref_ok = ok; }   // plane_coef_[i] is written whatever the verdict (common_lib.h:229-233)
            else if (ok) pl = fit;
            else if (bm < K) { pl.y = fit.y; pl.z = fit.z; pl.w = fit.w; }   // the tile kernel's queued 3- / 4-neighbour fits hand back (NaN, y, z, w)
          }
        }
      }
#pragma unroll
      for (int j = 0; j < K; j++) *(PCM_GLOBAL uint32_t*)(d.nn + (size_t)i * K + j) = j < bm ? bi[j] : ~0u;
    } else {
      pl = gload4(d.planes + (kp.lio_ref == 2 ? __float_as_uint(p.w) : i));   // plane of the previous ObsModel call
    }
  }
  lio_row_and_reduce(d, kp, i, tile_x, live, do_search, p, q, pn_body, pl, ref_fit, ref_ok, s_mem);
}

void launch_lio_lists(hipStream_t stream, const PairDesc* d_descs, const PairState* d_states, const KernelParams& kp, bool pooled, bool dev) {
  dim3 grid((unsigned)kp.tiles_per_pair, 1u);
  if (pooled && dev) k_lio_lists<true, true><<<grid, 256, 0, stream>>>(d_descs, d_states, kp);
  else if (pooled) k_lio_lists<true, false><<<grid, 256, 0, stream>>>(d_descs, d_states, kp);
  else if (dev) k_lio_lists<false, true><<<grid, 256, 0, stream>>>(d_descs, d_states, kp);
  else k_lio_lists<false, false><<<grid, 256, 0, stream>>>(d_descs, d_states, kp);
}

}  // namespace pcm
