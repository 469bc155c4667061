// loam_tiles.hip -- the key-frame map cut into localisation area tiles on the device (include/pcm_amd.h, pcm_loam_tiles_build): what
// a mapping context hands a localisation context.  The tiles follow the layout include/dynamic_map.h:16-156 reads (one cloud per
// area, selected by (x, y)); the reference tree reads area lists and holds no program that writes them, so the rules of the cut
// are this library's (loam_tiles.h).
//
// Two stages with one wait after each; both lists are queued before either wait, so the call waits twice in all:
//   gather     pcm_loam_map_export's pass (which = 2: both lists through one entry table) into the workspace:
//              transformPointCloud's values, bit for bit; then per list (corner, surf)
//   k_tile_keys      a point's tile key (loam_tiles.h); a non-finite point and a point without a tile get key 0 and are counted
//   sort, k_tile_heads, scan, k_tile_distinct      the distinct keys in ascending order, and how many there are
//   [wait: the number of tiles, the two counts -- the tile count sizes the per-segment arrays of the VoxelGrid pass]
//   k_tile_rank      a point's segment = the rank of its key in the distinct keys, by a binary search whose trip count depends on
//                    the tile count alone; the rank is an address only after distinct[rank] == key held (section 13's rule), a
//                    point whose key is not found is dropped and counted (PCM_ERR_INTERNAL)
//   voxel_grid.h's segmented pass with segment = tile: leaf > 0 the pcl::VoxelGrid of the tile's points alone (box from the tile's
//                    own min / max, cells in leaf-index order: pcm_voxel_downsample's bits), leaf == 0 one cell per point in export
//                    order.  Its put() is the scatter: cell c of the sorted (tile, cell) order is point c of the list's cloud.
//   k_tile_stats     count and z range of every tile from the stored cells: a segmented wave reduction (the cells of a tile are
//                    consecutive), then one atomic per wave and tile run -- integer add, min and max on ordered words, exact in any
//                    order, so two builds of one state give the same table
//   [wait: the per-tile table (key, count, z range: 16 bytes per tile) and the totals]
// The tile clouds then go to the arenas pcm_loam_tile_add fills with one device-to-device copy per list (loam_tiles_replace), after
// every check has passed: an error leaves the tile store as it was.
// Workspace: 88 bytes per point of a list -- the gathered point 16, its cell 16, keys and sorted keys 8, head, rank and segment 12,
// the distinct keys 4 (one word per point: the tile count is not known when the array is taken), and the segmented pass's 32
// (64-bit keys twice, values twice, slot, head) -- plus rocPRIM's temporaries and 96 bytes per tile (box words 24, box 48, counts
// 8, table record 16); both lists' workspaces are alive together.  All of it comes from a scoped DevScratch and goes back, in stream order,
// before the call returns.  gfx950.
#include "dev_scratch.h"
#include "host_util.h"
#include "loam_device.h"
#include "loam_tiles.h"
#include "voxel_grid.h"

#include <chrono>
#include <cstring>
#include <vector>

using namespace pcm;
using namespace pcm::loam;

namespace {

constexpr uint32_t kNoTile = 0xffffffffu;   // the segment of a point without a tile

// status words of one list: [0] tiles, [1] points without a tile (index out of range), [2] non-finite points, [3] points whose key
// was not found among the distinct keys, [4] cells whose segment is not a tile
constexpr int kStatusWords = 8;

struct TileRec { uint32_t key, n, z_lo, z_hi; };   // z as ordered words (pcm_device.h f2ord)

__global__ void __launch_bounds__(256) k_tile_keys(const float4* __restrict__ pts, uint32_t N, float tile_size, uint32_t* __restrict__ keys, uint32_t* __restrict__ status) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  const bool in = g < N;
  const float4 p = in ? pts[g] : make_float4(0.f, 0.f, 0.f, 0.f);
  const bool fin = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
  int32_t ix, iy;
  const bool okx = tile_index(p.x, tile_size, &ix), oky = tile_index(p.y, tile_size, &iy);
  const bool tiled = fin && okx && oky;
  if (in) keys[g] = tiled ? tile_key(ix, iy) : kNoTileKey;
  const uint64_t nf = __ballot(in && !fin), far = __ballot(in && fin && !tiled);
  if ((threadIdx.x & 63u) == 0) {   // integer sums: the same in every order
    if (nf) atomicAdd(&status[2], (uint32_t)__popcll(nf));
    if (far) atomicAdd(&status[1], (uint32_t)__popcll(far));
  }
}

__global__ void __launch_bounds__(256) k_tile_heads(const uint32_t* __restrict__ keys_s, uint32_t N, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const uint32_t k = keys_s[i];
  head[i] = (k != kNoTileKey && (i == 0 || keys_s[i - 1] != k)) ? 1u : 0u;
}

// rank[i]: the heads before sorted element i, so a head's rank is its tile's place in [0, tiles) -- below N, the size of `distinct`
__global__ void __launch_bounds__(256) k_tile_distinct(const uint32_t* __restrict__ keys_s, const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank, uint32_t N,
                                                       uint32_t* __restrict__ distinct, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  if (head[i]) distinct[rank[i]] = keys_s[i];
  if (i + 1 == N) status[0] = rank[i] + head[i];
}

__global__ void __launch_bounds__(256) k_tile_rank(const uint32_t* __restrict__ keys, uint32_t N, const uint32_t* __restrict__ distinct, uint32_t T, uint32_t* __restrict__ seg,
                                                   uint32_t* __restrict__ status) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  const bool in = g < N;
  const uint32_t k = in ? keys[g] : kNoTileKey;
  const uint32_t lo = table_row_of(distinct, 1u, T, k);   // T >= 1; row 0 when k lies before the table: the comparison below says so
  const bool found = k != kNoTileKey && distinct[lo] == k;
  if (in) seg[g] = found ? lo : kNoTile;
  const uint64_t lost = __ballot(in && k != kNoTileKey && !found);
  if ((threadIdx.x & 63u) == 0 && lost) atomicAdd(&status[3], (uint32_t)__popcll(lost));
}

__global__ void __launch_bounds__(256) k_tile_table_init(const uint32_t* __restrict__ distinct, uint32_t T, TileRec* __restrict__ table) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < T) table[t] = TileRec{distinct[t], 0u, 0xffffffffu, 0u};
}

// One lane per stored cell.  pos[c] (below N) is the first sorted element of cell c and the upper half of its key the cell's tile;
// the cells are in (tile, cell) order, so the lanes of a tile form a run: lane l folds [l, l + 2^k) of its run in step k, the
// first lane of a run ends with the whole of it inside this wave.
__global__ void __launch_bounds__(256) k_tile_stats(const float4* __restrict__ cells, const uint64_t* __restrict__ keys_s, const uint32_t* __restrict__ pos,
                                                    const uint32_t* __restrict__ small, uint32_t N, uint32_t T, TileRec* __restrict__ table, uint32_t* __restrict__ status) {
  const uint32_t ncells = min(small[0], N);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = blockIdx.x * 256u; base < ncells; base += gridDim.x * 256u) {   // uniform per workgroup
    const uint32_t i = base + threadIdx.x;
    bool valid = i < ncells;
    uint32_t seg = kNoTile;
    if (valid) {
      const uint32_t e = pos[i];
      seg = e < N ? (uint32_t)(keys_s[e] >> 32) : kNoTile;
      if (seg >= T) { valid = false; seg = kNoTile; atomicAdd(&status[4], 1u); }   // cannot happen: the pass numbers cells of tiles only
    }
    const uint32_t o = valid ? f2ord(cells[i].z) : 0u;
    uint32_t z_lo = valid ? o : 0xffffffffu, z_hi = o, cnt = valid ? 1u : 0u;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t s2 = (uint32_t)__shfl_down((int)seg, off, 64), lo2 = (uint32_t)__shfl_down((int)z_lo, off, 64), hi2 = (uint32_t)__shfl_down((int)z_hi, off, 64),
                     c2 = (uint32_t)__shfl_down((int)cnt, off, 64);
      if (lane + (uint32_t)off < 64u && s2 == seg) { z_lo = min(z_lo, lo2); z_hi = max(z_hi, hi2); cnt += c2; }
    }
    const uint32_t before = (uint32_t)__shfl_up((int)seg, 1, 64);
    if (valid && (lane == 0 || before != seg)) {
      atomicAdd(&table[seg].n, cnt);
      atomicMin(&table[seg].z_lo, z_lo);
      atomicMax(&table[seg].z_hi, z_hi);
    }
  }
}

// the elements of the segmented pass: one row, element j = gathered point j, segment = its tile
struct TileElems {
  static constexpr int kFields = 4;
  const float4* in; const uint32_t* seg; uint32_t N; float leaf_size; uint32_t* small; float4* out;
  __device__ int fields() const { return 4; }
  __device__ float4 fetch(uint32_t g, uint32_t) const { return in[g]; }
  __device__ bool slot(uint32_t, uint32_t j, uint32_t* g) const { *g = j; return j < N; }
  __device__ vg::Elem elem(uint32_t, uint32_t j) const {
    const uint32_t s = seg[j];
    return vg::Elem{s != kNoTile, s, j, in[j]};
  }
  __device__ float leaf(uint32_t) const { return leaf_size; }
  __device__ void overflow(uint32_t) const { small[2] = 1u; }   // every writer stores 1
  __device__ void put(uint32_t cell, const float (&m)[kFields]) const { out[cell] = make_float4(m[0], m[1], m[2], m[3]); }
};

// the stages of one list, as pcm_loam_tiles_build_ms reports them
enum { kStAlloc = 0, kStKeys, kStKeySort, kStDistinct, kStRank, kStMinMax, kStCellSort, kStAverage, kStStats, kStages };

// device events at the stage boundaries of a timed build (pcm_loam_tiles_build_ms); an untimed build records nothing
struct StageClock {
  bool on = false;
  hipStream_t st = nullptr;
  std::vector<hipEvent_t> ev;
  std::vector<int> slot;   // ms slot that the span ending at ev[i] belongs to; -1: none (the first event of a sequence)
  ~StageClock() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
  void mark(int s) {
    if (!on) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    ev.push_back(e); slot.push_back(s);
  }
  // after the stream has drained: ms[slot] += the span that ends at each event
  void collect(float* ms) const {
    for (size_t i = 1; i < ev.size(); i++) {
      float t = 0.f;
      if (slot[i] >= 0 && hipEventElapsedTime(&t, ev[i - 1], ev[i]) == hipSuccess) ms[slot[i]] += t;
    }
  }
};

// one list's build
struct ListJob {
  int which = 0;
  float leaf = 0.f;
  uint32_t N = 0, T = 0;
  float4* pts = nullptr; float4* cells = nullptr;
  uint32_t *keys = nullptr, *keys_s = nullptr, *head = nullptr, *rank = nullptr, *distinct = nullptr, *seg = nullptr, *status = nullptr;
  TileRec* table = nullptr;
  vg::Work W{};
  uint32_t h_status[kStatusWords] = {};
  uint32_t h_small[vg::Work::kSmallWords] = {};
  std::vector<TileRec> h_table;
  std::vector<BuiltTile> tiles;
  uint32_t n_cells = 0;
  float alloc_ms = 0.f;   // host time of the workspace requests
};

int check_tparams(pcm_ctx* c, const pcm_loam_tiles_params& p) {
  if (!(p.tile_size > 0.f) || !finite_f(p.tile_size)) { c->err = "tile_size must be a positive number"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.leaf_corner >= 0.f) || !(p.leaf_surf >= 0.f) || !finite_f(p.leaf_corner) || !finite_f(p.leaf_surf)) {
    c->err = "leaf_corner and leaf_surf must be >= 0 (0: no down-sampling)"; return PCM_ERR_INVALID_ARGUMENT;
  }
  return PCM_OK;
}

using HostClock = std::chrono::steady_clock;
float since_ms(HostClock::time_point t0) { return std::chrono::duration<float, std::milli>(HostClock::now() - t0).count(); }

// the per-point arrays of a list (its points, J.pts, are the caller's)
int take_arrays(pcm_ctx* c, DevScratch& sc, ListJob& J) {
  const HostClock::time_point t0 = HostClock::now();
  const size_t N = J.N;
  int rc;
  if ((rc = sc.take(&J.cells, N, &c->err, "tile cells")) != PCM_OK || (rc = sc.take(&J.keys, N, &c->err, "tile keys")) != PCM_OK ||
      (rc = sc.take(&J.keys_s, N, &c->err, "tile keys")) != PCM_OK || (rc = sc.take(&J.head, N, &c->err, "tile heads")) != PCM_OK ||
      (rc = sc.take(&J.rank, N, &c->err, "tile ranks")) != PCM_OK || (rc = sc.take(&J.distinct, N, &c->err, "distinct tile keys")) != PCM_OK ||
      (rc = sc.take(&J.seg, N, &c->err, "tile segments")) != PCM_OK || (rc = sc.take(&J.status, (size_t)kStatusWords, &c->err, "tile status")) != PCM_OK)
    return rc;
  J.alloc_ms += since_ms(t0);
  return PCM_OK;
}

// keys and the distinct keys of the gathered points; queues and does not wait
int queue_keys(pcm_ctx* c, DevScratch& sc, ListJob& J, float tile_size, StageClock& clk) {
  hipStream_t st = c->stream;
  const size_t N = J.N;
  int rc;
  const unsigned nb = (J.N + 255u) / 256u;
  clk.mark(-1);
  PCM_HIPCK(c, hipMemsetAsync(J.status, 0, sizeof(uint32_t) * kStatusWords, st));
  k_tile_keys<<<nb, 256, 0, st>>>(J.pts, J.N, tile_size, J.keys, J.status);
  PCM_HIPCK(c, hipGetLastError());
  clk.mark(kStKeys);
  if ((rc = scratch_sort_keys(sc, &c->err, J.keys, J.keys_s, N, 0, 32)) != PCM_OK) return rc;
  clk.mark(kStKeySort);
  k_tile_heads<<<nb, 256, 0, st>>>(J.keys_s, J.N, J.head);
  PCM_HIPCK(c, hipGetLastError());
  if ((rc = scratch_exclusive_scan(sc, &c->err, J.head, J.rank, N)) != PCM_OK) return rc;
  k_tile_distinct<<<nb, 256, 0, st>>>(J.keys_s, J.head, J.rank, J.N, J.distinct, J.status);
  PCM_HIPCK(c, hipGetLastError());
  clk.mark(kStDistinct);
  PCM_HIPCK(c, hipMemcpyAsync(J.h_status, J.status, sizeof(uint32_t) * kStatusWords, hipMemcpyDeviceToHost, st));
  return PCM_OK;
}

// segments, the VoxelGrid of every tile, the per-tile table; queues and does not wait.  J.T >= 1.
int queue_cells(pcm_ctx* c, DevScratch& sc, ListJob& J, StageClock& clk) {
  hipStream_t st = c->stream;
  int rc;
  size_t work_bytes = 0;
  (void)vg::work_layout(nullptr, J.N, sizeof(uint64_t), J.T, &work_bytes);
  char* work = nullptr;
  const HostClock::time_point t0 = HostClock::now();
  if ((rc = sc.take(&work, work_bytes, &c->err, "tile VoxelGrid arrays")) != PCM_OK || (rc = sc.take(&J.table, (size_t)J.T, &c->err, "tile table")) != PCM_OK) return rc;
  J.alloc_ms += since_ms(t0);
  J.W = vg::work_layout(work, J.N, sizeof(uint64_t), J.T, &work_bytes);
  const unsigned nb = (J.N + 255u) / 256u;
  clk.mark(-1);
  k_tile_rank<<<nb, 256, 0, st>>>(J.keys, J.N, J.distinct, J.T, J.seg, J.status);
  k_tile_table_init<<<(J.T + 255u) / 256u, 256, 0, st>>>(J.distinct, J.T, J.table);
  PCM_HIPCK(c, hipGetLastError());
  clk.mark(kStRank);
  vg::clear(st, J.W);
  TileElems E{J.pts, J.seg, J.N, J.leaf, J.W.small, J.cells};
  if (J.leaf > 0.f) vg::seg_minmax(st, E, 1u, J.N, J.W);
  clk.mark(kStMinMax);
  if ((rc = vg::seg_sort(&c->err, st, E, 1u, J.N, J.N, J.W)) != PCM_OK) return rc;
  clk.mark(kStCellSort);
  if ((rc = vg::seg_average(&c->err, st, E, J.N, J.W)) != PCM_OK) return rc;
  clk.mark(kStAverage);
  k_tile_stats<<<std::min(nb, 2048u), 256, 0, st>>>(J.cells, static_cast<const uint64_t*>(J.W.keys_s), J.W.vals, J.W.small, J.N, J.T, J.table, J.status);
  PCM_HIPCK(c, hipGetLastError());
  clk.mark(kStStats);
  try { J.h_table.resize(J.T); } catch (...) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  PCM_HIPCK(c, hipMemcpyAsync(J.h_table.data(), J.table, sizeof(TileRec) * J.T, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipMemcpyAsync(J.h_small, J.W.small, sizeof(J.h_small), hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipMemcpyAsync(J.h_status, J.status, sizeof(uint32_t) * kStatusWords, hipMemcpyDeviceToHost, st));
  return PCM_OK;
}

// the table of a finished list -> its tiles
int finish_list(pcm_ctx* c, ListJob& J, float tile_size) {
  static const char* const name[2] = {"corner", "surf"};
  if (J.h_small[2]) {
    c->err = std::string("pcm_loam_tiles_build: the leaf is too small for the extent of a ") + name[J.which] + " tile (VoxelGrid index overflow); tiles are not cut as VoxelGridLarge cuts";
    return PCM_ERR_OUT_OF_RANGE;
  }
  if (J.h_status[3] || J.h_status[4]) { c->err = "pcm_loam_tiles_build: a point's tile key was not found among the distinct keys"; return PCM_ERR_INTERNAL; }
  try { J.tiles.resize(J.T); } catch (...) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  uint64_t first = 0;
  for (uint32_t t = 0; t < J.T; t++) {
    const TileRec& r = J.h_table[t];
    if (r.n == 0 || r.key == kNoTileKey || (t && r.key <= J.h_table[t - 1].key)) { c->err = "pcm_loam_tiles_build: inconsistent tile table"; return PCM_ERR_INTERNAL; }
    BuiltTile& b = J.tiles[t];
    b.ix = tile_key_ix(r.key); b.iy = tile_key_iy(r.key);
    tile_box_xy(b.ix, b.iy, tile_size, &b.box[0], &b.box[1], &b.box[3], &b.box[4]);
    b.box[2] = (double)vg::ord2f(r.z_lo); b.box[5] = (double)vg::ord2f(r.z_hi);
    b.first = (uint32_t)first; b.n = r.n;
    first += r.n;
  }
  if (first != J.h_small[0] || first > J.N) { c->err = "pcm_loam_tiles_build: the tile counts do not add up to the cells"; return PCM_ERR_INTERNAL; }
  J.n_cells = (uint32_t)first;
  return PCM_OK;
}

// Everything between the argument checks and the result.  Whatever it queued may still be in flight when it returns an error: the
// caller drains the stream before the scratch and the jobs (pageable targets of the read-backs) go.
int run_build(pcm_ctx* c, DevScratch& sc, ListJob (&job)[2], StageClock (&clk)[2], const pcm_loam_tiles_params& p, int first, int n, const uint64_t (&total)[2],
              pcm_loam_tiles_result* r, float* gather_ms, float* copy_ms) {
  hipStream_t st = c->stream;
  int rc;
  const uint64_t all = total[0] + total[1];
  if (all) {
    // the export pass: both lists through one entry table (which = 2: every corner cloud, then every surf cloud) while the sum
    // fits its 2^31 - 1 limit, else list by list (the second export then waits for the first one's staging)
    const bool one = all <= 0x7fffffffull;
    StageClock& g = clk[0];
    const HostClock::time_point t0 = HostClock::now();
    float4* base = nullptr;
    if (one && (rc = sc.take(&base, (size_t)all, &c->err, "tile points")) != PCM_OK) return rc;
    for (int m = 0; m < 2; m++) {
      if (!job[m].N) continue;
      if (one) job[m].pts = base + (m ? total[0] : 0);
      else if ((rc = sc.take(&job[m].pts, (size_t)job[m].N, &c->err, "tile points")) != PCM_OK) return rc;
    }
    job[0].alloc_ms += since_ms(t0);
    g.mark(-1);
    size_t got = 0;
    if (one) {
      if ((rc = pcm_loam_map_export(c, 2, first, n, base, (size_t)all, PCM_MEM_DEVICE, &got)) != PCM_OK) return rc;   // in place, not waited for
      if (got != all) { c->err = "pcm_loam_tiles_build: the export pass disagrees about the number of points"; return PCM_ERR_INTERNAL; }
    } else {
      for (int m = 0; m < 2; m++) {
        if (!job[m].N) continue;
        if ((rc = pcm_loam_map_export(c, m, first, n, job[m].pts, (size_t)job[m].N, PCM_MEM_DEVICE, &got)) != PCM_OK) return rc;
        if (got != job[m].N) { c->err = "pcm_loam_tiles_build: the export pass disagrees about the number of points"; return PCM_ERR_INTERNAL; }
      }
    }
    g.mark(kStages);   // the gather of both lists
    for (int m = 0; m < 2; m++)
      if (job[m].N && ((rc = take_arrays(c, sc, job[m])) != PCM_OK || (rc = queue_keys(c, sc, job[m], p.tile_size, clk[m])) != PCM_OK)) return rc;
    PCM_HIPCK(c, hipStreamSynchronize(st));   // wait 1: the number of tiles and the two counts
    loam_export_waited(c);
  }
  uint64_t far = 0;
  for (int m = 0; m < 2; m++) {
    if (!job[m].N) continue;
    job[m].T = job[m].h_status[0];
    far += job[m].h_status[1];
    r->num_nonfinite += job[m].h_status[2];
    if (job[m].T > job[m].N) { c->err = "pcm_loam_tiles_build: more tiles than points"; return PCM_ERR_INTERNAL; }
  }
  if (far) {
    c->err = "pcm_loam_tiles_build: a point lies 32768 tiles or more from the origin (tile_size too small for the extent of the map)";
    return PCM_ERR_OUT_OF_RANGE;
  }
  bool queued = false;
  for (int m = 0; m < 2; m++)
    if (job[m].T) {
      if ((rc = queue_cells(c, sc, job[m], clk[m])) != PCM_OK) return rc;
      queued = true;
    }
  if (queued) PCM_HIPCK(c, hipStreamSynchronize(st));   // wait 2: the per-tile tables and the totals
  for (int m = 0; m < 2; m++)
    if (job[m].T && (rc = finish_list(c, job[m], p.tile_size)) != PCM_OK) return rc;
  const BuiltTile* tiles[2] = {job[0].tiles.data(), job[1].tiles.data()};
  const size_t n_tiles[2] = {job[0].tiles.size(), job[1].tiles.size()};
  const float4* cells[2] = {job[0].cells, job[1].cells};
  const size_t n_cells[2] = {job[0].n_cells, job[1].n_cells};
  StageClock& k = clk[1];
  k.mark(-1);
  if ((rc = loam_tiles_replace(c, tiles, n_tiles, cells, n_cells)) != PCM_OK) return rc;
  k.mark(kStages);   // the copies into the arenas
  if (clk[0].on) {
    PCM_HIPCK(c, hipStreamSynchronize(st));
    float g[kStages + 1] = {}, q[kStages + 1] = {};
    clk[0].collect(g); clk[1].collect(q);
    *gather_ms = g[kStages]; *copy_ms = q[kStages];
  }
  r->num_corner_tiles = (int32_t)job[0].tiles.size(); r->num_surf_tiles = (int32_t)job[1].tiles.size();
  r->corner_points_out = job[0].n_cells; r->surf_points_out = job[1].n_cells;
  return PCM_OK;
}

// stage_ms: null, or [2][kStages] + gather + arena copy (pcm_loam_tiles_build_ms)
int build(pcm_ctx* c, const pcm_loam_tiles_params* params, int first, int n, pcm_loam_tiles_result* result, float* stage_ms) {
  int rc = loam_check_ctx(c, PCM_ERR_INVALID_ARGUMENT, "pcm_loam_tiles_build needs a context created with PCM_MODEL_LOAM");
  if (rc != PCM_OK) return rc;
  if ((rc = loam_tiles_writable(c, "pcm_loam_tiles_build")) != PCM_OK) return rc;   // a shared store: refused before any device work
  pcm_loam_tiles_params p;
  if (params) p = *params; else pcm_loam_default_tiles_params(&p);
  if ((rc = check_tparams(c, p)) != PCM_OK) return rc;
  const int K = pcm_loam_keyframe_count(c);
  if (K < 0) return K;
  if (first < 0 || n < 0 || (long long)first + n > (long long)K) { c->err = "pcm_loam_tiles_build: first + n exceeds the number of key frames"; return PCM_ERR_INVALID_ARGUMENT; }
  pcm_loam_tiles_result r;
  std::memset(&r, 0, sizeof(r));
  if (result) *result = r;
  uint64_t total[2] = {0, 0};
  for (int i = first; i < first + n; i++)
    for (int m = 0; m < 2; m++) {
      const float4* q = nullptr;
      uint32_t cnt = 0;
      if (!loam_keyframe_cloud(c, i, m, &q, &cnt)) { c->err = "pcm_loam_tiles_build: no such key frame"; return PCM_ERR_INTERNAL; }
      total[m] += cnt;
    }
  if (total[0] > 0x7fffffffull || total[1] > 0x7fffffffull) { c->err = "pcm_loam_tiles_build: more than 2^31 - 1 points in one list: build the tiles of sub-ranges"; return PCM_ERR_OUT_OF_RANGE; }
  r.corner_points_in = total[0]; r.surf_points_in = total[1];
  PCM_HIPCK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  ListJob job[2];
  StageClock clk[2];
  for (int m = 0; m < 2; m++) {
    job[m].which = m; job[m].leaf = m ? p.leaf_surf : p.leaf_corner; job[m].N = (uint32_t)total[m];
    clk[m].on = stage_ms != nullptr; clk[m].st = st;
  }
  float gather_ms = 0.f, copy_ms = 0.f;
  {
    DevScratch sc(st);   // everything the build takes lives until the end of this block and goes back in stream order
    rc = run_build(c, sc, job, clk, p, first, n, total, &r, &gather_ms, &copy_ms);
    if (rc != PCM_OK) (void)hipStreamSynchronize(st);   // a read-back queued before the error must not land after job[] is gone
  }
  if (rc != PCM_OK) return rc;
  if (stage_ms) {
    for (int m = 0; m < 2; m++) {
      float ms[kStages + 1] = {};
      clk[m].collect(ms);
      ms[kStAlloc] = job[m].alloc_ms;
      for (int s = 0; s < kStages; s++) stage_ms[m * kStages + s] = ms[s];
    }
    stage_ms[2 * kStages] = gather_ms; stage_ms[2 * kStages + 1] = copy_ms;
  }
  if (result) *result = r;
  return PCM_OK;
}

}  // namespace

extern "C" {

void pcm_loam_default_tiles_params(pcm_loam_tiles_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->tile_size = 50.0f;
  p->leaf_corner = 0.2f;   // utility.h:271
  p->leaf_surf = 0.2f;     // utility.h:272
}

int pcm_loam_tiles_build(pcm_ctx* c, const pcm_loam_tiles_params* params, int first, int n, pcm_loam_tiles_result* result) {
  return build(c, params, first, n, result, nullptr);
}

int pcm_loam_tiles_build_ms(pcm_ctx* c, const pcm_loam_tiles_params* params, int first, int n, pcm_loam_tiles_result* result, float* stage_ms) {
  if (c && !stage_ms) { c->err = "pcm_loam_tiles_build_ms: null stage_ms"; return PCM_ERR_INVALID_ARGUMENT; }
  return build(c, params, first, n, result, stage_ms);
}

}  // extern "C"
