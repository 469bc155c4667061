// loam_dynmap.hip -- localisation map tiles and the per-frame crop on the device (include/pcm_amd.h, pcm_loam_tile_* and
// pcm_loam_dynmap_*): jueying_slam's area tiles (include/dynamic_map.h:16-156), dynamic_load_map_run (localization.cpp:281-315,
// new_localization.cpp:480-514) and dynamic_load_map (localization.cpp:256-280, new_localization.cpp:454-478).
//
// Store: one growing float4 arena (x, y, z, intensity; map frame) for the tiles of the corner list and one for those of the surf
// list, per-tile offset, count and Area on the host.  Load: the selection runs on the host (loam_dynmap.h; microseconds) and
// moves no points.  Crop: the selected tiles' entry table (arena offset, first position in the concatenation) is uploaded and
// the concatenation is compacted through the frame's window in three steps that keep the order:
//   count    one lane per point, 256 points per workgroup (a workgroup never straddles the two lists): the predicate, a ballot
//            and a popcount per wave, one count per workgroup;
//   scan     exclusive scan of the workgroup counts: 256 counts per scan block, then the block totals in one workgroup;
//   scatter  the predicate again, the lane's rank from the ballot, the whole 16-byte record to its place in the context's corner
//            or surf target cloud (loam_target_reserve / loam_target_commit).
// The only atomic is the integer counter of dropped non-finite points: no output position depends on the schedule, so two crops
// of one state give the same bits.  When selection, limits and crop_x equal those of the last crop and the target is still its
// result, the call does nothing at all (a standing robot, the relocalisation branch's second scan2MapOptimization).
//
// The store proper (tile tables and arenas: TileStore) is held through a counted reference (loam_dynmap.h, TileHolder): after
// pcm_loam_tile_share several contexts read one store, which is then immutable; the selection, the crop workspace and the record of
// the last crop stay per context.  There is one host path and one kernel set (crop_contexts): the crops of B contexts run in one
// round of launches, and pcm_loam_dynmap_crop is that round with B = 1:
//   k_dm_count_batch / k_dm_scatter_batch   the workgroups of all contexts in one grid; a workgroup finds its context in the
//                 block-prefix table and reads that context's DmBatchDesc, then runs the body of one context;
//   k_dm_scan_chunks                        over the count slices of all contexts, each padded to whole scan blocks;
//   k_dm_scan_tops_batch                    one workgroup per context.
// A context's bits do not depend on who else is in the round.  DESIGN.md sections 14 and 33.
#include "host_util.h"
#include "loam_device.h"
#include "loam_dynmap.h"

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

using namespace pcm;
using namespace pcm::loam;

namespace {

// the points [src, src + n) of an arena are positions [first, first + n) of the concatenation (n = the next entry's first - first)
struct DmEntry {
  uint32_t src;     // first point in its arena
  uint32_t first;   // first position (ascending over the table; no entry is empty)
  uint32_t flags;   // bit 0: surf arena
  uint32_t pad;
};

// small: [0] corner points kept, [1] points kept, [2] non-finite points dropped
constexpr int kSmallWords = 4;

// lane threadIdx.x of a context's workgroup b -> its position g in the concatenation (corner workgroups first: b < nb0 covers
// [0, n0), the rest [n0, N)), its record and the record's class.  The entry is found by the search of table_search.h, whose trip
// count depends on the table size alone; a tile holds thousands of points, so nearly every wave reads one entry.  An idle
// lane reads the last record of its own list (in bounds) and is class 0.
__device__ inline int dm_fetch(const float4* __restrict__ corner_arena, const float4* __restrict__ surf_arena, const DmEntry* __restrict__ ent, uint32_t n_ent,
                               uint32_t b, uint32_t nb0, uint32_t n0, uint32_t N, const CropWindow& w, float4* p, bool* seg1) {
  *seg1 = b >= nb0;
  const uint32_t g = *seg1 ? n0 + (b - nb0) * kDmBlock + threadIdx.x : b * kDmBlock + threadIdx.x;
  const uint32_t end = *seg1 ? N : n0;
  const bool valid = g < end;
  const uint32_t gg = valid ? g : end - 1;
  const DmEntry e = ent[table_row_of(&ent->first, sizeof(DmEntry) / 4, n_ent, gg)];
  const float4* __restrict__ arena = (e.flags & 1u) ? surf_arena : corner_arena;
  *p = arena[(size_t)e.src + (gg - e.first)];
  return valid ? crop_class(p->x, p->y, p->z, w) : 0;
}

// workgroup b of one context: counts[b] = its points kept; its non-finite points are added to small[2]
__device__ inline void dm_count_body(const float4* __restrict__ corner_arena, const float4* __restrict__ surf_arena, const DmEntry* __restrict__ ent, uint32_t n_ent,
                                     uint32_t b, uint32_t nb0, uint32_t n0, uint32_t N, const CropWindow& w, uint32_t* __restrict__ counts,
                                     uint32_t* __restrict__ small) {
  __shared__ uint32_t wk[kDmBlock / 64], wn[kDmBlock / 64];
  float4 p;
  bool seg1;
  const int cls = dm_fetch(corner_arena, surf_arena, ent, n_ent, b, nb0, n0, N, w, &p, &seg1);
  const uint64_t km = __ballot(cls == 1), nm = __ballot(cls == 2);
  if ((threadIdx.x & 63) == 0) { wk[threadIdx.x >> 6] = (uint32_t)__popcll(km); wn[threadIdx.x >> 6] = (uint32_t)__popcll(nm); }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t k = 0, n = 0;
    for (uint32_t i = 0; i < kDmBlock / 64; i++) { k += wk[i]; n += wn[i]; }
    counts[b] = k;
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
__device__ inline void dm_scan_tops_body(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ chunk_tot, uint32_t nchunks, uint32_t nb, uint32_t nb0,
                                         uint32_t* __restrict__ chunk_off, uint32_t* __restrict__ small) {
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

// workgroup b of one context: its kept records to their places in the context's two output clouds
__device__ inline void dm_scatter_body(const float4* __restrict__ corner_arena, const float4* __restrict__ surf_arena, const DmEntry* __restrict__ ent, uint32_t n_ent,
                                       uint32_t b, uint32_t nb0, uint32_t n0, uint32_t N, const CropWindow& w, const uint32_t* __restrict__ counts,
                                       const uint32_t* __restrict__ chunk_off, const uint32_t* __restrict__ small, float4* __restrict__ out0,
                                       float4* __restrict__ out1) {
  __shared__ uint32_t wk[kDmBlock / 64];
  float4 p;
  bool seg1;
  const int cls = dm_fetch(corner_arena, surf_arena, ent, n_ent, b, nb0, n0, N, w, &p, &seg1);
  const uint64_t km = __ballot(cls == 1);
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) wk[wv] = (uint32_t)__popcll(km);
  __syncthreads();
  if (cls != 1) return;
  uint32_t off = chunk_off[b / kDmChunk] + counts[b];
  for (uint32_t i = 0; i < wv; i++) off += wk[i];
  off += (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
  if (seg1) out1[off - small[0]] = p; else out0[off] = p;
}

// ---- the launches: the contexts of one round (a single crop is a round of one) -------------------------------------------------
// one context as the kernels read it; counts, chunk_tot, chunk_off and small point at its own slices (BatchSlice)
struct DmBatchDesc {
  const float4* arena[2];   // the store this context holds
  const DmEntry* ent;       // its entry table
  uint32_t* counts;
  uint32_t* chunk_tot;
  uint32_t* chunk_off;
  uint32_t* small;
  float4* out[2];           // its corner / surf target clouds
  uint32_t n_ent, nb0, nb, n0, N, nchunks;
  CropWindow w;
  uint32_t pad;
};
static_assert(sizeof(DmBatchDesc) % 8 == 0, "descriptors lie in an array");

// Each of the three kernels below exists twice (Descs): with the round's descriptors in memory (DescArray), and for a round of one
// with the descriptor in the kernel arguments (DmBatchDesc), where the workgroup needs neither the block prefix nor a load before
// its first instruction.  The single crop was measured slower than its own earlier kernels without this.
using DescArray = const DmBatchDesc* __restrict__;
__device__ inline const DmBatchDesc& dm_desc(DescArray descs, uint32_t i) { return descs[i]; }
__device__ inline const DmBatchDesc& dm_desc(const DmBatchDesc& one, uint32_t) { return one; }
// workgroup blockIdx.x of the grid -> its context i and its place *b among that context's workgroups
template <class Descs>
__device__ inline uint32_t dm_context(const uint32_t* __restrict__ block0, uint32_t n_ctx, uint32_t* b) {
  if (std::is_same<Descs, DmBatchDesc>::value) { *b = blockIdx.x; return 0u; }
  const uint32_t i = batch_context_of(block0, n_ctx, blockIdx.x);
  *b = blockIdx.x - block0[i];
  return i;
}

// grid: the workgroups of all contexts; block0[i] = the first workgroup of context i
template <class Descs>
__global__ void __launch_bounds__(kDmBlock) k_dm_count_batch(const Descs descs, const uint32_t* __restrict__ block0, uint32_t n_ctx) {
  uint32_t b;
  const DmBatchDesc& D = dm_desc(descs, dm_context<Descs>(block0, n_ctx, &b));
  dm_count_body(D.arena[0], D.arena[1], D.ent, D.n_ent, b, D.nb0, D.n0, D.N, D.w, D.counts, D.small);
}

// grid: one workgroup per context
template <class Descs>
__global__ void __launch_bounds__(kDmChunk) k_dm_scan_tops_batch(const Descs descs) {
  const DmBatchDesc& D = dm_desc(descs, blockIdx.x);
  dm_scan_tops_body(D.counts, D.chunk_tot, D.nchunks, D.nb, D.nb0, D.chunk_off, D.small);
}

template <class Descs>
__global__ void __launch_bounds__(kDmBlock) k_dm_scatter_batch(const Descs descs, const uint32_t* __restrict__ block0, uint32_t n_ctx) {
  uint32_t b;
  const DmBatchDesc& D = dm_desc(descs, dm_context<Descs>(block0, n_ctx, &b));
  dm_scatter_body(D.arena[0], D.arena[1], D.ent, D.n_ent, b, D.nb0, D.n0, D.N, D.w, D.counts, D.chunk_off, D.small, D.out[0], D.out[1]);
}

struct Tile {
  Area box;
  size_t off;
  uint32_t n;
  int32_t ix = 0, iy = 0;   // the index pair of a tile pcm_loam_tiles_build cut; 0, 0 for a tile the caller added
};

// the store proper: what several contexts may hold (immutable while they do)
struct TileStore {
  std::vector<Tile> tiles[2];   // corner list, surf list
  Arena arena[2] = {Arena("map-tile arena"), Arena("map-tile arena")};
  // loam_tiles_replace queued copies into the arenas on its context's stream and did not wait.  Only a sole holder writes, so the
  // stream is that of the one context holding the store; whoever reads the arenas on another stream drains it first.
  bool fill_queued = false;
};

// what a context keeps for itself
struct DynStore {
  TileHolder<TileStore> h;      // the reference to the store, and the selection of the last load
  int device = -1;              // of the context (the last holder frees the arenas with it current)
  // workspace and staging of the rounds this context leads (its own crops among them): crop_carve
  DevBuf<char> bbuf{"map-crop batch workspace"};
  PinnedBuf<char> h_up{"map-crop batch staging"};
  PinnedBuf<uint32_t> h_bsmall{"map-crop batch counters"};
  // the last crop (current while h.s.last_valid)
  uint64_t last_gen = 0;
  CropWindow last_w{};
  pcm_loam_dynmap_crop_result last{};
  // the context goes (pcm_destroy has made the device current and drained the stream)
  ~DynStore() {
    const int dev = device;
    h.let_go([dev] { if (dev >= 0) (void)hipSetDevice(dev); });
  }
};

int check_ctx_dm(pcm_ctx* c, DynStore** ds) {
  const int rc = loam_check_store(c, "pcm_loam_tile_* / pcm_loam_dynmap_* need a context created with PCM_MODEL_LOAM", LoamStore::dyn, ds);
  if (rc != PCM_OK) return rc;
  if (!(*ds)->h.ready()) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  (*ds)->device = c->device;
  return PCM_OK;
}

// What runs before the last reference frees a store: the device current and this context's stream drained (dev_buf.h).  The other
// contexts that held it drained their own streams when they let go, so nothing queued reads it.
auto store_release_hook(pcm_ctx* c) {
  return [c] {
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
  };
}

// the answer of every call that would change a store other contexts read
int refuse_shared_store(pcm_ctx* c, const DynStore* S, const char* call) {
  c->err = std::string(call) + ": the tile store is shared by " + std::to_string(S->h.holders()) +
           " contexts and cannot be changed (pcm_loam_tile_clear gives this context a store of its own)";
  return PCM_ERR_UNSUPPORTED;
}

int check_dparams(pcm_ctx* c, const pcm_loam_dynmap_params* params, const float* pose6, pcm_loam_dynmap_params* p) {
  if (params) *p = *params; else pcm_loam_default_dynmap_params(p);
  if (!(p->max_range >= 0.f) || !finite_f(p->max_range)) { c->err = "max_range must be a number >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!pose6) { c->err = "null pose"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int k = 0; k < 6; k++) if (!finite_f(pose6[k])) { c->err = "the pose must be finite"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

// both lists of a store the caller alone holds; the arenas keep their memory
void empty_store(TileStore& T) {
  for (int m = 0; m < 2; m++) {
    T.tiles[m].clear();
    T.arena[m].n = 0;
  }
}

bool same_window(const CropWindow& a, const CropWindow& b) {
  // float equality: the limits are finite or the two infinities of margin < 0, never NaN
  return a.x_lo == b.x_lo && a.x_hi == b.x_hi && a.y_lo == b.y_lo && a.y_hi == b.y_hi && a.crop_x == b.crop_x;
}

// the crop of this selection through w is what the context's target already holds
bool crop_unchanged(pcm_ctx* c, const DynStore* S, const CropWindow& w) {
  const float4 *tc = nullptr, *ts = nullptr;
  uint32_t tnc = 0, tns = 0;
  return S->h.s.last_valid && S->last_gen == S->h.s.sel_gen && same_window(S->last_w, w) && loam_target_view(c, TargetOwner::dynmap, &tc, &tnc, &ts, &tns);
}

// the points and the non-empty tiles of the selection
void selection_size(const DynStore* S, uint64_t* n0, uint64_t* n1, size_t* E) {
  const TileStore& T = *S->h.ts;
  *n0 = *n1 = 0; *E = 0;
  for (int32_t t : S->h.s.sel[0]) { *n0 += T.tiles[0][(size_t)t].n; *E += T.tiles[0][(size_t)t].n ? 1 : 0; }
  for (int32_t t : S->h.s.sel[1]) { *n1 += T.tiles[1][(size_t)t].n; *E += T.tiles[1][(size_t)t].n ? 1 : 0; }
}

// the selection's entry table; returns the number of rows (selection_size's E)
size_t write_entries(const DynStore* S, DmEntry* ent) {
  const TileStore& T = *S->h.ts;
  uint32_t first = 0;
  size_t e = 0;
  for (int m = 0; m < 2; m++)
    for (int32_t t : S->h.s.sel[m]) {
      const Tile& tile = T.tiles[m][(size_t)t];
      if (tile.n == 0) continue;   // an empty tile contributes nothing
      ent[e++] = DmEntry{(uint32_t)tile.off, first, (uint32_t)m, 0u};
      first += tile.n;
    }
  return e;
}

pcm_loam_dynmap_crop_result crop_record(uint64_t n0, uint64_t n1, const CropWindow& w) {
  pcm_loam_dynmap_crop_result r;
  std::memset(&r, 0, sizeof(r));
  r.num_corner_in = (int32_t)n0; r.num_surf_in = (int32_t)n1;
  r.x_lo = w.x_lo; r.x_hi = w.x_hi; r.y_lo = w.y_lo; r.y_hi = w.y_hi;
  return r;
}

// the counters of a finished crop into its record; false: they contradict the input sizes
bool take_counters(const uint32_t* small, uint64_t n0, uint64_t n1, pcm_loam_dynmap_crop_result* r) {
  const uint32_t k0 = small[0], k = small[1];
  if (k0 > n0 || k < k0 || k - k0 > n1) return false;
  r->num_corner = (int32_t)k0;
  r->num_surf = (int32_t)(k - k0);
  r->num_nonfinite = (int32_t)small[2];
  return true;
}

// the crop's result is the context's target from now on
void commit_crop(pcm_ctx* c, DynStore* S, const CropWindow& w, pcm_loam_dynmap_crop_result* r) {
  loam_target_commit(c, (uint32_t)r->num_corner, (uint32_t)r->num_surf, TargetOwner::dynmap);
  r->rebuilt = 1;
  r->status = PCM_OK;
  S->h.s.last_valid = true;
  S->last_gen = S->h.s.sel_gen;
  S->last_w = w;
  S->last = *r;
}

// one context of a batch that has work for the device
struct BatchJob {
  int i;                 // its place in the call
  pcm_ctx* c;
  DynStore* S;
  CropWindow w;
  uint64_t n0, n1;
  size_t E;
  uint32_t nb0, nb;
  float4* out[2];
  pcm_loam_dynmap_crop_result r;
};

using Carve = CropCarve<DmBatchDesc, DmEntry>;

// the four launches of a round of m contexts over the workspace d
template <class Descs>
void launch_round(hipStream_t st, const Descs descs, const Carve& d, uint32_t m, const BatchLayout& lay) {
  k_dm_count_batch<Descs><<<lay.blocks, kDmBlock, 0, st>>>(descs, d.block0, m);
  k_dm_scan_chunks<<<lay.chunks, kDmChunk, 0, st>>>(d.counts, lay.slots, d.chunk_tot);
  k_dm_scan_tops_batch<Descs><<<m, kDmChunk, 0, st>>>(descs);
  k_dm_scatter_batch<Descs><<<lay.blocks, kDmBlock, 0, st>>>(descs, d.block0, m);
}

// The crops of n contexts in one round of launches on the stream of the first context: the one path of pcm_loam_dynmap_crop
// (n = 1; `one`) and pcm_loam_dynmap_crop_batch.  Host: per context the window and the unchanged short-cut, the target's room, the
// entry table into one pinned block; one upload (descriptors, block prefix, entry tables), one clear (counters and count slices),
// four launches, one read-back of all counters, one wait.  results[i].status and the return value (the first failure's status) are
// the batched call's; a failed allocation names the buffer as the entry point at hand always has.
int crop_contexts(pcm_ctx* const* ctxs, int n, const pcm_loam_dynmap_params* params, const float* poses6, pcm_loam_dynmap_crop_result* results, bool one) {
  pcm_ctx* c0 = ctxs[0];
  DynStore* S0 = nullptr;
  int rc = check_ctx_dm(c0, &S0);
  if (rc != PCM_OK) return rc;
  std::memset(results, 0, sizeof(pcm_loam_dynmap_crop_result) * (size_t)n);
  int worst = PCM_OK;
  auto fail = [&](int i, int status, pcm_ctx* c) {
    results[i].status = status;
    if (c && c != c0) c0->err = c->err;
    if (worst == PCM_OK) worst = status;
  };
  // what every context asks for; nothing is changed yet
  std::vector<BatchJob> jobs;
  std::vector<uint32_t> nbs;
  jobs.reserve((size_t)n); nbs.reserve((size_t)n);
  for (int i = 0; i < n; i++) {
    pcm_ctx* c = ctxs[i];
    DynStore* S = nullptr;
    if ((rc = check_ctx_dm(c, &S)) != PCM_OK) {
      if (!c) c0->err = "pcm_loam_dynmap_crop_batch: null context";
      fail(i, rc, c);
      continue;
    }
    if (c->device != c0->device) { c0->err = "all contexts of a batch must live on one device"; fail(i, PCM_ERR_INVALID_ARGUMENT, nullptr); continue; }
    bool twice = false;
    for (int j = 0; j < i; j++) twice = twice || ctxs[j] == c;
    if (twice) { c0->err = "a context appears twice in the batch"; fail(i, PCM_ERR_INVALID_ARGUMENT, nullptr); continue; }
    pcm_loam_dynmap_params p;
    const float* pose6 = poses6 + 6 * (size_t)i;
    if ((rc = check_dparams(c, params, pose6, &p)) != PCM_OK) { fail(i, rc, c); continue; }
    if (!S->h.s.loaded) { c->err = "pcm_loam_dynmap_crop before pcm_loam_dynmap_load"; fail(i, PCM_ERR_NO_INPUT, c); continue; }
    BatchJob J{};
    J.i = i; J.c = c; J.S = S;
    J.w = crop_window(pose6, p.max_range, p.margin, p.crop_x);
    if (crop_unchanged(c, S, J.w)) {
      // the same tiles through the same window: the target is the one the context already holds
      results[i] = S->last;
      results[i].rebuilt = 0;
      continue;
    }
    selection_size(S, &J.n0, &J.n1, &J.E);
    if (J.n0 + J.n1 > 0x7fffffffull) { c->err = "the selected tiles hold more than 2^31 points"; fail(i, PCM_ERR_OUT_OF_RANGE, c); continue; }
    J.nb0 = (uint32_t)((J.n0 + kDmBlock - 1) / kDmBlock);
    J.nb = J.nb0 + (uint32_t)((J.n1 + kDmBlock - 1) / kDmBlock);
    jobs.push_back(J);
    nbs.push_back(J.nb);
  }
  if (jobs.empty()) return worst;   // nothing for the device: the short-cut does not touch it
  std::vector<BatchSlice> slices(jobs.size());
  BatchLayout lay;
  if (!batch_layout(nbs.data(), (int)nbs.size(), slices.data(), &lay)) {
    c0->err = "pcm_loam_dynmap_crop_batch: the workgroups of the batch do not fit one grid: crop in smaller batches";
    return PCM_ERR_OUT_OF_RANGE;
  }
  PCM_HIPCK(c0, hipSetDevice(c0->device));
  // room for the targets; a context without points is done here.  Those that go on to the device move to the front of jobs.
  uint32_t m = 0;
  size_t E_all = 0;
  for (size_t k = 0; k < jobs.size(); k++) {
    BatchJob& J = jobs[k];
    J.S->h.s.last_valid = false;
    if ((rc = loam_target_reserve(J.c, (size_t)J.n0, (size_t)J.n1, &J.out[0], &J.out[1])) != PCM_OK) { fail(J.i, rc, J.c); continue; }
    J.r = crop_record(J.n0, J.n1, J.w);
    if (J.nb == 0) {
      commit_crop(J.c, J.S, J.w, &J.r);
      results[J.i] = J.r;
      continue;
    }
    if (J.S->h.ts->fill_queued && J.c != c0) {   // copies into this store are queued on its sole holder's stream
      if (hipStreamSynchronize(J.c->stream) != hipSuccess) { J.c->err = "pcm_loam_dynmap_crop_batch: hipStreamSynchronize failed"; fail(J.i, PCM_ERR_HIP, J.c); continue; }
      J.S->h.ts->fill_queued = false;
    }
    E_all += J.E;
    nbs[m] = J.nb;
    jobs[m++] = J;
  }
  if (m == 0) return worst;
  (void)batch_layout(nbs.data(), (int)m, slices.data(), &lay);   // a failed reservation took a context out: a subset of what fitted
  const Carve size = crop_carve<DmBatchDesc, DmEntry>(nullptr, m, E_all, kSmallWords, lay);
  const size_t bytes = size.bytes, up_bytes = size.up_bytes;
  hipStream_t st = c0->stream;
  S0->bbuf.what = one ? "map-crop workspace" : "map-crop batch workspace";
  S0->h_up.what = one ? "pinned buffer" : "map-crop batch staging";
  S0->h_bsmall.what = one ? "pinned buffer" : "map-crop batch counters";
  if ((rc = S0->bbuf.reserve(c0, bytes, bytes + bytes / 2)) != PCM_OK) return rc;
  if ((rc = S0->h_up.reserve(c0, up_bytes, up_bytes + up_bytes / 2)) != PCM_OK) return rc;
  if ((rc = S0->h_bsmall.reserve(c0, (size_t)kSmallWords * m, (size_t)kSmallWords * m)) != PCM_OK) return rc;
  PCM_HIPCK(c0, hipStreamSynchronize(st));   // the pinned staging of an earlier round is free again
  const Carve d = crop_carve<DmBatchDesc, DmEntry>(S0->bbuf.p, m, E_all, kSmallWords, lay);
  const Carve h = crop_carve<DmBatchDesc, DmEntry>(S0->h_up.p, m, E_all, kSmallWords, lay);   // its upload range mirrors d's
  size_t e0 = 0;
  for (uint32_t k = 0; k < m; k++) {
    const BatchJob& J = jobs[k];
    const BatchSlice& sl = slices[k];
    const TileStore& T = *J.S->h.ts;
    DmBatchDesc D;
    std::memset(&D, 0, sizeof(D));
    D.arena[0] = T.arena[0].d; D.arena[1] = T.arena[1].d;
    D.ent = d.ent + e0;
    D.counts = d.counts + sl.slot0;
    D.chunk_tot = d.chunk_tot + sl.chunk0;
    D.chunk_off = d.chunk_off + sl.chunk0;
    D.small = d.small + (size_t)kSmallWords * k;
    D.out[0] = J.out[0]; D.out[1] = J.out[1];
    D.n_ent = (uint32_t)J.E; D.nb0 = J.nb0; D.nb = J.nb; D.n0 = (uint32_t)J.n0; D.N = (uint32_t)(J.n0 + J.n1); D.nchunks = sl.nchunks;
    D.w = J.w;
    h.desc[k] = D;
    h.block0[k] = sl.block0;
    e0 += write_entries(J.S, h.ent + e0);
  }
  PCM_HIPCK(c0, hipMemcpyAsync(d.desc, h.desc, d.up_bytes, hipMemcpyHostToDevice, st));
  PCM_HIPCK(c0, hipMemsetAsync(d.small, 0, d.zero_bytes, st));
  if (m == 1) launch_round<DmBatchDesc>(st, h.desc[0], d, m, lay);   // the descriptor in the kernel arguments
  else launch_round<DescArray>(st, d.desc, d, m, lay);
  PCM_HIPCK(c0, hipGetLastError());
  PCM_HIPCK(c0, hipMemcpyAsync(S0->h_bsmall, d.small, sizeof(uint32_t) * kSmallWords * m, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c0, hipStreamSynchronize(st));
  S0->h.ts->fill_queued = false;
  for (uint32_t k = 0; k < m; k++) {
    BatchJob& J = jobs[k];
    if (!take_counters(S0->h_bsmall + (size_t)kSmallWords * k, J.n0, J.n1, &J.r)) {
      J.c->err = "pcm_loam_dynmap_crop: inconsistent counts";
      fail(J.i, PCM_ERR_INTERNAL, J.c);
      continue;
    }
    commit_crop(J.c, J.S, J.w, &J.r);
    results[J.i] = J.r;
  }
  return worst;
}

}  // namespace

namespace pcm {
namespace loam {
int loam_tiles_writable(pcm_ctx* c, const char* call) {
  DynStore* S = nullptr;
  const int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  return S->h.writable() ? PCM_OK : refuse_shared_store(c, S, call);
}

int loam_tiles_replace(pcm_ctx* c, const BuiltTile* const tiles[2], const size_t n_tiles[2], const float4* const cells[2], const size_t n_cells[2]) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (!S->h.writable()) return refuse_shared_store(c, S, "pcm_loam_tiles_build");
  TileStore& T = *S->h.ts;
  for (int m = 0; m < 2; m++) {
    if (n_cells[m] > 0xffffffffull || n_tiles[m] > 0x7fffffffull) { c->err = "map-tile store too large"; return PCM_ERR_OUT_OF_RANGE; }
    // room first, so that a failed allocation leaves both lists whole (growth keeps the stored points)
    Arena& A = T.arena[m];
    if (n_cells[m] > A.n && (rc = A.reserve(c, n_cells[m] - A.n)) != PCM_OK) return rc;
  }
  for (int m = 0; m < 2; m++) {
    try { T.tiles[m].reserve(n_tiles[m]); } catch (...) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  }
  empty_store(T);
  S->h.s.reset();
  for (int m = 0; m < 2; m++) {
    Arena& A = T.arena[m];
    if (n_cells[m]) {
      PCM_HIPCK(c, hipMemcpyAsync(A.d.p, cells[m], sizeof(float4) * n_cells[m], hipMemcpyDeviceToDevice, c->stream));
      T.fill_queued = true;
    }
    for (size_t t = 0; t < n_tiles[m]; t++) {
      const BuiltTile& b = tiles[m][t];
      Tile tile;
      tile.box = Area{b.box[0], b.box[1], b.box[2], b.box[3], b.box[4], b.box[5]};
      tile.off = b.first; tile.n = b.n; tile.ix = b.ix; tile.iy = b.iy;
      T.tiles[m].push_back(tile);
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
  if (!S->h.writable()) return refuse_shared_store(c, S, "pcm_loam_tile_add");
  TileStore& T = *S->h.ts;
  if (which != 0 && which != 1) { c->err = "which must be 0 (corner list) or 1 (surf list)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!box) { c->err = "null box"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int k = 0; k < 6; k++) if (!(box[k] == box[k])) { c->err = "the box must hold numbers"; return PCM_ERR_INVALID_ARGUMENT; }
  if ((rc = check_point_records(c, points, n, stride, memory, 0x3fffffffull)) != PCM_OK) return rc;
  Arena& A = T.arena[which];
  if (A.n + n > 0xffffffffull || T.tiles[which].size() >= 0x7fffffffull) { c->err = "map-tile store too large"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  if ((rc = A.reserve(c, n)) != PCM_OK) return rc;
  if ((rc = load_xyzw_rows(c, points, n, stride, memory, true, A.d + A.n)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the caller may reuse its buffer on return
  T.fill_queued = false;
  Tile t;
  t.box = Area{box[0], box[1], box[2], box[3], box[4], box[5]};
  t.off = A.n;
  t.n = (uint32_t)n;
  T.tiles[which].push_back(t);
  A.n += n;
  return (int)T.tiles[which].size() - 1;
}

int pcm_loam_tile_count(pcm_ctx* c, int which) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (which != 0 && which != 1) { c->err = "which must be 0 (corner list) or 1 (surf list)"; return PCM_ERR_INVALID_ARGUMENT; }
  return (int)S->h.ts->tiles[which].size();
}

int pcm_loam_tile_clear(pcm_ctx* c) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (S->h.ts.shared()) {   // this context's queued work may read the store it is about to let go of
    PCM_HIPCK(c, hipSetDevice(c->device));
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  }
  if (!S->h.clear_or_detach(store_release_hook(c), empty_store)) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  return PCM_OK;
}

// dst reads src's tile store from now on (pcm_amd.h).  Everything queued into the arenas was queued on src's stream, which is
// drained here: what dst -- and any later holder -- reads through its own stream was complete before this call returned, and
// nothing writes to the store while it has more than one holder.
int pcm_loam_tile_share(pcm_ctx* dst, pcm_ctx* src) {
  if (!dst) return PCM_ERR_INVALID_ARGUMENT;
  if (dst->device < 0) return PCM_ERR_HIP;
  if (!src) { dst->err = "pcm_loam_tile_share: null source context"; return PCM_ERR_INVALID_ARGUMENT; }
  if (src->device < 0) { dst->err = "pcm_loam_tile_share: the source context has no device"; return PCM_ERR_HIP; }
  if (dst == src) { dst->err = "pcm_loam_tile_share: a context cannot share its tile store with itself"; return PCM_ERR_INVALID_ARGUMENT; }
  if (dst->cfg.model != PCM_MODEL_LOAM || src->cfg.model != PCM_MODEL_LOAM) {
    dst->err = "pcm_loam_tile_share: both contexts must be created with PCM_MODEL_LOAM";
    return PCM_ERR_INVALID_ARGUMENT;
  }
  if (dst->device != src->device) { dst->err = "pcm_loam_tile_share: both contexts must live on one device"; return PCM_ERR_INVALID_ARGUMENT; }
  DynStore *D = nullptr, *S = nullptr;
  int rc = check_ctx_dm(dst, &D);
  if (rc != PCM_OK) return rc;
  if ((rc = check_ctx_dm(src, &S)) != PCM_OK) { dst->err = src->err; return rc; }
  PCM_HIPCK(dst, hipSetDevice(src->device));
  PCM_HIPCK(dst, hipStreamSynchronize(src->stream));   // build before read
  S->h.ts->fill_queued = false;
  PCM_HIPCK(dst, hipStreamSynchronize(dst->stream));   // dst's queued crops may read the store it lets go of
  D->h.share_from(S->h, store_release_hook(dst));
  return PCM_OK;
}

int pcm_loam_tile_share_count(pcm_ctx* c) {
  DynStore* S = nullptr;
  const int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  return S->h.holders();
}

int pcm_loam_tile_info(pcm_ctx* c, int which, int index, double box[6], int32_t ixy[2], size_t* n_points) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (which != 0 && which != 1) { c->err = "which must be 0 (corner list) or 1 (surf list)"; return PCM_ERR_INVALID_ARGUMENT; }
  const std::vector<Tile>& tiles = S->h.ts->tiles[which];
  if (index < 0 || (size_t)index >= tiles.size()) { c->err = "pcm_loam_tile_info: index outside [0, tiles of the list)"; return PCM_ERR_INVALID_ARGUMENT; }
  const Tile& T = tiles[(size_t)index];
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
  const std::vector<Tile>& tiles = S->h.ts->tiles[which];
  if (index < 0 || (size_t)index >= tiles.size()) { c->err = "pcm_loam_tile_get: index outside [0, tiles of the list)"; return PCM_ERR_INVALID_ARGUMENT; }
  const Tile& T = tiles[(size_t)index];
  if (n) *n = T.n;
  if (T.n > capacity || (!out && T.n)) { c->err = "pcm_loam_tile_get: capacity too small (the count is set)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (T.n == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  PCM_HIPCK(c, hipMemcpyAsync(out, S->h.ts->arena[which].d + T.off, sizeof(float4) * T.n, memory == PCM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

int pcm_loam_dynmap_need_load(pcm_ctx* c, const pcm_loam_dynmap_params* params, const float pose6[6]) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_dynmap_params p;
  if ((rc = check_dparams(c, params, pose6, &p)) != PCM_OK) return rc;
  return need_load(pose6, S->h.s.last_load, p.area_size) ? 1 : 0;
}

int pcm_loam_dynmap_load(pcm_ctx* c, const pcm_loam_dynmap_params* params, const float pose6[6], pcm_loam_dynmap_load_result* result) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_dynmap_params p;
  if ((rc = check_dparams(c, params, pose6, &p)) != PCM_OK) return rc;
  pcm_loam_dynmap_load_result r;
  std::memset(&r, 0, sizeof(r));
  const TileStore& T = *S->h.ts;
  TileSelection& sel = S->h.s;
  bool changed = !sel.loaded;
  for (int m = 0; m < 2; m++) {
    std::vector<Area> areas(T.tiles[m].size());
    for (size_t i = 0; i < areas.size(); i++) areas[i] = T.tiles[m][i].box;
    // create_pcd(transformTobeMapped[3], transformTobeMapped[4], areas, dir, margin): the int margin becomes a float there
    std::vector<int32_t> s = select_areas(areas.data(), (int)areas.size(), pose6[3], pose6[4], (float)p.margin);
    if (s != sel.sel[m]) changed = true;
    sel.sel[m] = std::move(s);
  }
  if (changed) sel.sel_gen++;
  sel.loaded = true;
  for (int k = 0; k < 6; k++) sel.last_load[k] = pose6[k];
  r.num_corner_tiles = (int32_t)T.tiles[0].size();
  r.num_surf_tiles = (int32_t)T.tiles[1].size();
  r.num_corner_selected = (int32_t)sel.sel[0].size();
  r.num_surf_selected = (int32_t)sel.sel[1].size();
  for (int32_t t : sel.sel[0]) r.num_corner_points += T.tiles[0][(size_t)t].n;
  for (int32_t t : sel.sel[1]) r.num_surf_points += T.tiles[1][(size_t)t].n;
  r.generation = sel.sel_gen;
  r.changed = changed ? 1 : 0;
  if (result) *result = r;
  return PCM_OK;
}

// A round of one.  What this call always answered stays: bad arguments leave *result as it was, every later failure leaves it
// zeroed (the per-context status is the batched call's), the unchanged short-cut returns the last record with rebuilt = 0.
int pcm_loam_dynmap_crop(pcm_ctx* c, const pcm_loam_dynmap_params* params, const float pose6[6], pcm_loam_dynmap_crop_result* result) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  if (!result) { c->err = "null result"; return PCM_ERR_INVALID_ARGUMENT; }
  pcm_loam_dynmap_params p;
  if ((rc = check_dparams(c, params, pose6, &p)) != PCM_OK) return rc;
  if ((rc = crop_contexts(&c, 1, params, pose6, result, true)) != PCM_OK) std::memset(result, 0, sizeof(*result));
  return rc;
}

int pcm_loam_dynmap_crop_batch(pcm_ctx* const* ctxs, int n, const pcm_loam_dynmap_params* params, const float* poses6, pcm_loam_dynmap_crop_result* results) {
  if (!ctxs || n <= 0 || !poses6 || !results) return PCM_ERR_INVALID_ARGUMENT;
  return crop_contexts(ctxs, n, params, poses6, results, false);
}

int pcm_loam_dynmap_info(pcm_ctx* c, int32_t* corner_tiles, int32_t* surf_tiles, float* corner, float* surf) {
  DynStore* S = nullptr;
  int rc = check_ctx_dm(c, &S);
  if (rc != PCM_OK) return rc;
  const TileSelection& sel = S->h.s;
  if (!sel.loaded) { c->err = "pcm_loam_dynmap_info before pcm_loam_dynmap_load"; return PCM_ERR_NO_INPUT; }
  if (corner_tiles && !sel.sel[0].empty()) std::memcpy(corner_tiles, sel.sel[0].data(), sizeof(int32_t) * sel.sel[0].size());
  if (surf_tiles && !sel.sel[1].empty()) std::memcpy(surf_tiles, sel.sel[1].data(), sizeof(int32_t) * sel.sel[1].size());
  if (!corner && !surf) return PCM_OK;
  const float4 *tc = nullptr, *ts = nullptr;
  uint32_t tnc = 0, tns = 0;
  if (!sel.last_valid || !loam_target_view(c, TargetOwner::dynmap, &tc, &tnc, &ts, &tns)) { c->err = "pcm_loam_dynmap_info: the context's target is not the result of pcm_loam_dynmap_crop"; return PCM_ERR_NO_INPUT; }
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
  if (!S->h.s.last_valid || !loam_target_view(c, TargetOwner::dynmap, &tc, &tnc, &ts, &tns)) { c->err = "pcm_loam_dynmap_global: the context's target is not the result of pcm_loam_dynmap_crop"; return PCM_ERR_NO_INPUT; }
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
