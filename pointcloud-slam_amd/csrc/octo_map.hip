// octo_map.hip -- octomap_server's 3D occupancy map and projected 2D map on the device (include/pcm_amd.h, pcm_octo_*):
// insertCloudCallback (OctomapServer.cpp:281-346), insertScan (:357-451), publishAll's projected map and point-cloud centres
// (:497-640, :943-1109) and map_saver's bytes (map_saver.cpp:72-84).  Arithmetic: octo_map.h.  DESIGN.md section 38.
//
// State: one open-addressing table of 32-byte slots keyed by the packed 48-bit key + 1 (0 = empty), claimed with a 64-bit CAS; a
// slot holds the float log-odds, the scan epochs free / occ / seen and the epoch of its last update (0: inserted, never observed).
// k_octo_mark: one ray per lane: transform, windows, range rules, the walk; every key's slot is found or inserted and its free or
// occ epoch raised to the scan's with atomicMax, only after a coherent read shows it older; the lane that raises `seen` appends
// the slot to the touched list.  Nothing is cleared between scans.  k_octo_apply: over the touched list, one hit or one miss per
// cell, counters and key box reduced through LDS into one row per workgroup; k_octo_fold adds the rows to the map's statistics.
// A table that fills up raises a flag (probe loops are bounded by the capacity); apply and fold then do nothing, the host rehashes
// the observed cells into a table of twice the size and marks again under a new epoch.
// k_octo_collect / rocPRIM sort / k_octo_emit: cells or occupied centres sorted by packed key.  k_octo_project: occupied
// columns, then free columns where still unknown; k_octo_pgm: map_saver's bytes.
#include "dev_scratch.h"
#include "host_util.h"
#include "loam_device.h"
#include "octo_map.h"
#include "voxel_grid.h"

#include <algorithm>
#include <chrono>
#include <cstring>

using namespace pcm;
using namespace pcm::octo;

namespace {

struct Slot {
  unsigned long long key;   // packed key + 1; 0: empty
  float v;
  uint32_t fe, oe, seen, ae, pad;
};
static_assert(sizeof(Slot) == 32, "two slots per 64-byte line");

enum { kDropped = 0, kWindow = 1, kMinRange = 2, kTruncated = 3, kRejected = 4, kCallCounters = 5 };
struct Call {   // cleared before every mark pass
  uint32_t overflow, n_touched;
  unsigned long long cnt[kCallCounters];
  unsigned long long touched, new_cells;   // k_octo_fold
};
struct Stats {  // of the map
  uint32_t n_keys, pad;   // claimed slots, observed or not
  unsigned long long cells, occupied, free_cells;
  int32_t kmin[3], kmax[3];
};
struct Back { Call call; Stats stats; };

struct Seg { const float4* pts; uint32_t n; uint32_t ground; };
struct MarkArgs {
  Slot* tab;
  uint32_t mask, cells_cap, epoch, has_T;
  uint32_t* touched;
  Call* call;
  Stats* stats;
  Seg seg[2];
  float o[3];
  float T[12];
  OctoRules R;
};

constexpr unsigned kApplyBlocks = 2048;   // 8 workgroups per CU: the apply pass is a latency-bound gather and scatter
constexpr int kRow = 12;   // dcells, docc, dfree, min xyz, max xyz, pad

__device__ inline uint32_t coherent_u32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline unsigned long long coherent_u64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the slot of key1, inserted when absent and `insert`; -1: absent, or the table is full (flag raised).  h stays below mask + 1.
__device__ inline long long slot_of(Slot* __restrict__ tab, uint32_t mask, unsigned long long key1, bool insert, uint32_t cells_cap, Call* __restrict__ call,
                                    Stats* __restrict__ stats) {
  uint32_t h = (uint32_t)octo_hash(key1) & mask;
  for (uint32_t i = 0; i <= mask; i++) {
    const unsigned long long k = coherent_u64(&tab[h].key);
    if (k == key1) return h;
    if (k == 0ull) {
      if (!insert) return -1;
      const unsigned long long old = atomicCAS(&tab[h].key, 0ull, key1);
      if (old == 0ull) {
        if (atomicAdd(&stats->n_keys, 1u) >= cells_cap) atomicExch(&call->overflow, 1u);
        return h;
      }
      if (old == key1) return h;
    }
    h = (h + 1u) & mask;
  }
  if (insert) atomicExch(&call->overflow, 1u);
  return -1;
}

__device__ inline void mark_key(const MarkArgs& A, const int k[3], bool occ) {
  const long long h = slot_of(A.tab, A.mask, octo_pack(k[0], k[1], k[2]) + 1ull, true, A.cells_cap, A.call, A.stats);
  if (h < 0) return;
  Slot* s = A.tab + h;
  uint32_t* w = occ ? &s->oe : &s->fe;
  if (coherent_u32(w) >= A.epoch) return;
  if (atomicMax(w, A.epoch) >= A.epoch) return;
  if (atomicMax(&s->seen, A.epoch) >= A.epoch) return;
  const uint32_t at = atomicAdd(&A.call->n_touched, 1u);   // uniform address, constant 1: one add per wave instruction
  if (at < A.cells_cap) A.touched[at] = (uint32_t)h; else atomicExch(&A.call->overflow, 1u);
}

// point g of the scan up to its ray: the rule of its end key, or -1 when it casts no ray; f counts what became of it
__device__ inline int prepare_ray(const MarkArgs& A, uint32_t g, float e[3], uint32_t f[kCallCounters]) {
  const int sg = g < A.seg[0].n ? 0 : 1;
  const float4 p4 = A.seg[sg].pts[sg ? g - A.seg[0].n : g];
  const float p[3] = {p4.x, p4.y, p4.z};
  float q[3] = {p[0], p[1], p[2]};
  if (A.has_T) octo_transform(A.T, p, q);
  if (!octo_finite(q[0]) || !octo_finite(q[1]) || !octo_finite(q[2])) { f[kDropped] = 1; return -1; }
  if (!octo_in_window(q, A.R)) { f[kWindow] = 1; return -1; }
  bool truncated;
  const int rule = octo_point_rule(A.o, q, A.seg[sg].ground != 0u, A.R.max_range, A.R.min_range, e, &truncated);
  if (rule == kSkipMinRange) { f[kMinRange] = 1; return -1; }
  f[kTruncated] = truncated ? 1u : 0u;
  return rule;
}

__device__ inline void mark_end(const MarkArgs& A, int rule, int rc, const float e[3]) {
  int ke[3];
  if (rule == kEndOccupied) {
    if (octo_key3(e, A.R.res, ke)) mark_key(A, ke, true);
  } else if (rule == kEndFree && rc == kRayOk) {
    if (octo_key3(e, A.R.res, ke)) mark_key(A, ke, false);
  }
}

__device__ inline void count_points(const MarkArgs& A, const uint32_t f[kCallCounters]) {
  for (int a = 0; a < kCallCounters; a++) {
    const uint32_t s = vg::wave_sum_u32(f[a]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&A.call->cnt[a], (unsigned long long)s);
  }
}

// Once the table has overflowed nothing of the pass counts, and the rays in flight must stop inserting: a probe of a full table
// visits all of it.  The flag is polled once per kPoll keys of a ray.
constexpr uint32_t kPoll = 32;

// one ray per lane.  kDry: the ray is walked once without marking first (octo_ray); false is a measurement variant only, in which a
// rejected ray leaves its marks
template <bool kDry>
__global__ void __launch_bounds__(256) k_octo_mark(MarkArgs A) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t total = A.seg[0].n + A.seg[1].n;
  uint32_t f[kCallCounters] = {0u, 0u, 0u, 0u, 0u};
  if (g < total && coherent_u32(&A.call->overflow) == 0u) {
    float e[3];
    const int rule = prepare_ray(A, g, e, f);
    if (rule > 0) {
      uint32_t n = 0;
      bool stop = false;
      auto put = [&](const int* k) {
        if ((n++ & (kPoll - 1u)) == 0u && coherent_u32(&A.call->overflow) != 0u) stop = true;
        if (!stop) mark_key(A, k, false);
      };
      int steps;
      const int rc = kDry ? octo_ray(A.o, e, A.R.res, put) : octo_walk(A.o, e, A.R.res, put, &steps);
      if (rc != kRayOk) f[kRejected] = 1;
      if (!stop) mark_end(A, rule, rc, e);
    }
  }
  count_points(A, f);
}

// one ray per wave: every lane walks the same ray (uniform control flow), lane i keeps key i of each run of 64 keys, and the run is
// marked by the 64 lanes at once -- 64 probes in flight per wave instruction instead of one per lane at a time
template <bool kDry>
__global__ void __launch_bounds__(256) k_octo_mark_wave(MarkArgs A) {
  const uint32_t ray = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint32_t total = A.seg[0].n + A.seg[1].n;
  uint32_t f[kCallCounters] = {0u, 0u, 0u, 0u, 0u};
  if (ray < total && coherent_u32(&A.call->overflow) == 0u) {
    float e[3];
    const int rule = prepare_ray(A, ray, e, f);
    if (rule > 0) {
      int mine[3] = {0, 0, 0};
      uint32_t cnt = 0;
      bool stop = false;
      auto flush = [&]() {
        if (lane < cnt && !stop) mark_key(A, mine, false);
        if (coherent_u32(&A.call->overflow) != 0u) stop = true;
        cnt = 0;
      };
      auto put = [&](const int* k) {
        if (cnt == lane) { mine[0] = k[0]; mine[1] = k[1]; mine[2] = k[2]; }
        if (++cnt == 64u) flush();
      };
      int steps;
      const int rc = kDry ? octo_ray(A.o, e, A.R.res, put) : octo_walk(A.o, e, A.R.res, put, &steps);
      flush();
      if (rc != kRayOk) f[kRejected] = 1;
      if (lane == 0u && !stop) mark_end(A, rule, rc, e);
    }
    if (lane != 0u)
      for (int a = 0; a < kCallCounters; a++) f[a] = 0u;
  }
  count_points(A, f);
}

// one update per touched cell; row[blockIdx.x] = this workgroup's counter deltas and key box
__global__ void __launch_bounds__(256) k_octo_apply(Slot* __restrict__ tab, const uint32_t* __restrict__ touched, const Call* __restrict__ call, OctoRules R,
                                                    uint32_t epoch, uint32_t cells_cap, int32_t* __restrict__ rows) {
  __shared__ uint32_t s_red[4][9];
  uint32_t dcells = 0, docc = 0, dfree = 0;   // docc, dfree: signed, modulo 2^32
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  const uint32_t n = call->overflow ? 0u : min(call->n_touched, cells_cap);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    Slot* s = tab + touched[i];
    const bool was = s->ae != 0u;
    const float v0 = was ? s->v : 0.0f;
    const float v = octo_update(v0, s->oe == epoch ? R.hit : R.miss, R.clamp_min, R.clamp_max);
    s->v = v;
    s->ae = epoch;
    const bool o1 = octo_occupied(v), o0 = was && octo_occupied(v0), f0 = was && !octo_occupied(v0);
    dcells += was ? 0u : 1u;
    docc += (o1 ? 1u : 0u) - (o0 ? 1u : 0u);
    dfree += (o1 ? 0u : 1u) - (f0 ? 1u : 0u);
    int k[3];
    octo_unpack(s->key - 1ull, k);
    for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], (uint32_t)k[a]); hi[a] = max(hi[a], (uint32_t)k[a]); }
  }
  uint32_t r[9] = {vg::wave_sum_u32(dcells), vg::wave_sum_u32(docc), vg::wave_sum_u32(dfree), vg::wave_min_u32(lo[0]), vg::wave_min_u32(lo[1]), vg::wave_min_u32(lo[2]),
                   vg::wave_max_u32(hi[0]), vg::wave_max_u32(hi[1]), vg::wave_max_u32(hi[2])};
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 9; a++) s_red[wave][a] = r[a];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < 4; w++) {
      for (int a = 0; a < 3; a++) r[a] += s_red[w][a];
      for (int a = 3; a < 6; a++) r[a] = min(r[a], s_red[w][a]);
      for (int a = 6; a < 9; a++) r[a] = max(r[a], s_red[w][a]);
    }
    for (int a = 0; a < 9; a++) rows[blockIdx.x * kRow + a] = (int32_t)r[a];
  }
}

// one wave: the workgroups' rows into the map's statistics
__global__ void __launch_bounds__(64) k_octo_fold(const int32_t* __restrict__ rows, uint32_t nrows, Call* __restrict__ call, Stats* __restrict__ stats) {
  if (call->overflow) return;
  uint32_t sum[3] = {0u, 0u, 0u}, lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (uint32_t i = threadIdx.x; i < nrows; i += 64) {
    const int32_t* r = rows + i * kRow;
    for (int a = 0; a < 3; a++) { sum[a] += (uint32_t)r[a]; lo[a] = min(lo[a], (uint32_t)r[3 + a]); hi[a] = max(hi[a], (uint32_t)r[6 + a]); }
  }
  for (int a = 0; a < 3; a++) { sum[a] = vg::wave_sum_u32(sum[a]); lo[a] = vg::wave_min_u32(lo[a]); hi[a] = vg::wave_max_u32(hi[a]); }
  if (threadIdx.x == 0) {
    call->touched = call->n_touched;
    call->new_cells = sum[0];
    if (call->n_touched != 0u) {
      const bool first = stats->cells == 0ull;
      stats->cells += sum[0];
      stats->occupied += (long long)(int32_t)sum[1];
      stats->free_cells += (long long)(int32_t)sum[2];
      for (int a = 0; a < 3; a++) {
        stats->kmin[a] = first ? (int32_t)lo[a] : min(stats->kmin[a], (int32_t)lo[a]);
        stats->kmax[a] = first ? (int32_t)hi[a] : max(stats->kmax[a], (int32_t)hi[a]);
      }
    }
  }
}

// observed cells of the old table into the new one (which has room for all of them)
__global__ void __launch_bounds__(256) k_octo_rehash(const Slot* __restrict__ src, uint32_t n_src, Slot* __restrict__ dst, uint32_t mask, Call* __restrict__ call,
                                                     Stats* __restrict__ stats) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_src; i += gridDim.x * blockDim.x) {
    const Slot s = src[i];
    if (s.key == 0ull || s.ae == 0u) continue;
    const long long h = slot_of(dst, mask, s.key, true, 0xffffffffu, call, stats);
    if (h < 0) continue;   // cannot happen: the flag is raised and the host reports it
    dst[h].v = s.v;
    dst[h].ae = s.ae;
  }
}

__device__ inline bool occupied_at(const Slot* __restrict__ tab, uint32_t mask, int kx, int ky, int kz) {
  if (kx < 0 || ky < 0 || kz < 0 || kx >= kKeyEnd || ky >= kKeyEnd || kz >= kKeyEnd) return false;
  const long long h = slot_of(const_cast<Slot*>(tab), mask, octo_pack(kx, ky, kz) + 1ull, false, 0u, nullptr, nullptr);
  return h >= 0 && tab[h].ae != 0u && octo_occupied(tab[h].v);
}

// isSpeckleNode :1113-1130
__device__ inline bool is_speckle(const Slot* __restrict__ tab, uint32_t mask, const int k[3]) {
  for (int dz = -1; dz <= 1; dz++)
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++)
        if ((dx | dy | dz) != 0 && occupied_at(tab, mask, k[0] + dx, k[1] + dy, k[2] + dz)) return false;
  return true;
}

// a cell of publishAll's traversal: 2 occupied and published, 1 free and published, 0 neither
__device__ inline int published(const Slot* __restrict__ tab, uint32_t mask, const Slot& s, const OctoRules& R, int filter_speckles, int k[3]) {
  if (s.key == 0ull || s.ae == 0u) return 0;
  octo_unpack(s.key - 1ull, k);
  if (!octo_in_z(k[2], R)) return 0;
  if (!octo_occupied(s.v)) return 1;
  if (filter_speckles && is_speckle(tab, mask, k)) return 0;
  return 2;
}

// mode 0: every observed cell; mode 1: the occupied cells of octomap_point_cloud_centers
__global__ void __launch_bounds__(256) k_octo_collect(const Slot* __restrict__ tab, uint32_t n_slots, int mode, OctoRules R, int filter_speckles,
                                                      unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t cap, uint32_t* __restrict__ count) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += gridDim.x * blockDim.x) {
    const Slot s = tab[i];
    int k[3];
    const bool take = mode == 0 ? (s.key != 0ull && s.ae != 0u) : published(tab, n_slots - 1u, s, R, filter_speckles, k) == 2;
    if (!take) continue;
    const uint32_t at = atomicAdd(count, 1u);
    if (at < cap) { keys[at] = s.key - 1ull; vals[at] = i; }
  }
}

__global__ void __launch_bounds__(256) k_octo_emit(const Slot* __restrict__ tab, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n,
                                                   int mode, double res, int4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int k[3];
  octo_unpack(keys[i], k);
  const float v = tab[vals[i]].v;
  if (mode == 0) out[i] = make_int4(k[0], k[1], k[2], __float_as_int(v));
  else out[i] = make_int4(__float_as_int((float)octo_coord(k[0], res)), __float_as_int((float)octo_coord(k[1], res)), __float_as_int((float)octo_coord(k[2], res)), __float_as_int(v));
}

// update2DMap :1081-1090: pass 0 writes 100 for occupied cells, pass 1 writes 0 for free cells where the grid still says -1
__global__ void __launch_bounds__(256) k_octo_project(const Slot* __restrict__ tab, uint32_t n_slots, OctoRules R, int filter_speckles, int min_kx, int min_ky, int w,
                                                      int h, int pass, int8_t* __restrict__ grid) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += gridDim.x * blockDim.x) {
    const Slot s = tab[i];
    int k[3];
    const int what = published(tab, n_slots - 1u, s, R, pass == 0 ? filter_speckles : 0, k);
    if (what == 0) continue;
    const int cx = k[0] - min_kx, cy = k[1] - min_ky;
    if (cx < 0 || cy < 0 || cx >= w || cy >= h) continue;   // the geometry covers every known cell
    const size_t at = (size_t)cy * (size_t)w + (size_t)cx;
    if (pass == 0) { if (what == 2) grid[at] = 100; }
    else if (what == 1 && grid[at] == -1) grid[at] = 0;
  }
}

__global__ void __launch_bounds__(256) k_octo_pgm(const int8_t* __restrict__ grid, uint32_t w, uint32_t h, unsigned char* __restrict__ pgm) {
  const size_t n = (size_t)w * h;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
    const uint32_t j = (uint32_t)(t / w), i = (uint32_t)(t - (size_t)j * w);
    pgm[(size_t)(h - 1u - j) * w + i] = octo_pgm_byte((int)grid[t]);
  }
}

struct OctoMap {
  bool have_params = false;
  pcm_octo_params P{};
  OctoRules R{};
  DevBuf<Slot> tab{"octomap cell table"};
  uint32_t n_slots = 0, cells_cap = 0;
  DevBuf<uint32_t> touched{"octomap touched list"};
  DevBuf<Slot> tab_next{"octomap cell table"};              // a growth's new table and list until both exist
  DevBuf<uint32_t> touched_next{"octomap touched list"};
  // measurement hook (pcm_octo_debug): mark kernel variant, event timing of the phases of the last insert
  int variant = 0;
  bool timed = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  float phase_ms[4] = {0.f, 0.f, 0.f, 0.f};   // mark, apply + fold, growth (host clock), mark passes
  ~OctoMap() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  DevBuf<int32_t> rows{"octomap apply rows"};
  DevBuf<Back> d_back{"octomap counters"};
  PinnedBuf<Back> h_back{"octomap counters"};
  DevBuf<float4> stage{"octomap staged cloud"};
  DevBuf<int4> out{"octomap output records"};
  uint64_t epoch = 0;
  // the last projection
  bool projected = false;
  OctoGeom G{};
  DevBuf<int8_t> d_grid{"octomap projected grid"};
  DevBuf<unsigned char> d_pgm{"octomap pgm bytes"};
};

int check_ctx_octo(pcm_ctx* c, OctoMap** out, bool need_params) {
  *out = nullptr;
  if (!c) return PCM_ERR_INVALID_ARGUMENT;
  if (c->device < 0) return PCM_ERR_HIP;
  *out = c->octo.get_or_create<OctoMap>();
  if (!*out) { c->err = "the 3D occupancy map could not be allocated (out of host memory)"; return PCM_ERR_INTERNAL; }
  if (need_params && !(*out)->have_params) { c->err = "no 3D occupancy map yet: call pcm_octo_reset first"; return PCM_ERR_NO_INPUT; }
  return PCM_OK;
}

int check_params(pcm_ctx* c, const pcm_octo_params& p) {
  if (!finite_d(p.resolution) || !(p.resolution > 0.0)) { c->err = "resolution must be positive and finite"; return PCM_ERR_INVALID_ARGUMENT; }
  const double pr[4] = {p.prob_hit, p.prob_miss, p.clamp_min, p.clamp_max};
  for (double x : pr) if (!(x > 0.0 && x < 1.0)) { c->err = "prob_hit, prob_miss, clamp_min and clamp_max must lie inside (0, 1)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.clamp_min <= p.clamp_max)) { c->err = "clamp_min must not exceed clamp_max"; return PCM_ERR_INVALID_ARGUMENT; }
  const double w[12] = {p.max_range, p.min_range, p.pointcloud_min_x, p.pointcloud_max_x, p.pointcloud_min_y, p.pointcloud_max_y, p.pointcloud_min_z,
                        p.pointcloud_max_z, p.occupancy_min_z, p.occupancy_max_z, p.min_x_size, p.min_y_size};
  for (double x : w) if (!finite_d(x)) { c->err = "every range, window and size must be finite (+-DBL_MAX switches a window off)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.initial_cells == 0 || p.max_cells < p.initial_cells || p.max_cells > (1ull << 30)) {
    c->err = "1 <= initial_cells <= max_cells <= 2^30 is required"; return PCM_ERR_INVALID_ARGUMENT;
  }
  return PCM_OK;
}

uint32_t slots_for(uint64_t cells) {
  uint64_t s = 1024;
  while (s < 2 * cells) s <<= 1;
  return (uint32_t)s;
}

Back* back_of(OctoMap* M) { return M->h_back.p; }

// the observed cells into a fresh table with room for `cells` (the same size compacts it); waits.  The new table and the new
// touched list are both allocated before anything of the map changes: a failure leaves the map as it was.
int rehash(pcm_ctx* c, OctoMap* M, uint64_t cells) {
  const uint32_t ns = slots_for(cells);
  int rc;
  if ((rc = M->tab_next.reserve(c, ns, ns)) != PCM_OK) return rc;
  if ((rc = M->touched_next.reserve(c, (size_t)cells, (size_t)cells)) != PCM_OK) { M->tab_next.release(); return rc; }
  Slot* nt = M->tab_next;
  hipStream_t st = c->stream;
  hipError_t e = hipMemsetAsync(nt, 0, sizeof(Slot) * (size_t)ns, st);
  if (e == hipSuccess) e = hipMemsetAsync(&M->d_back.p->call, 0, sizeof(Call), st);
  if (e == hipSuccess) e = hipMemsetAsync(&M->d_back.p->stats.n_keys, 0, sizeof(uint32_t), st);
  if (e == hipSuccess && M->tab && M->n_slots) {
    k_octo_rehash<<<std::min<uint32_t>(4096u, (M->n_slots + 255u) / 256u), 256, 0, st>>>(M->tab, M->n_slots, nt, ns - 1u, &M->d_back.p->call, &M->d_back.p->stats);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(M->h_back.p, M->d_back.p, sizeof(Back), hipMemcpyDeviceToHost, st);
  const hipError_t w = hipStreamSynchronize(st);   // also after a failure: nothing queued may still use the new blocks
  if (e == hipSuccess) e = w;
  if (e != hipSuccess || back_of(M)->call.overflow) {
    M->tab_next.release(); M->touched_next.release();
    if (e != hipSuccess) { c->err = std::string("3D occupancy map growth: ") + hipGetErrorString(e); return PCM_ERR_HIP; }
    c->err = "3D occupancy map: the rehash did not fit (internal error)";
    return PCM_ERR_INTERNAL;
  }
  M->tab.swap(M->tab_next);
  M->touched.swap(M->touched_next);
  M->tab_next.release(); M->touched_next.release();   // the old ones; synchronised above
  M->n_slots = ns;
  M->cells_cap = (uint32_t)cells;
  return PCM_OK;
}

int ensure_small(pcm_ctx* c, OctoMap* M) {
  int rc;
  if ((rc = M->h_back.reserve(c, 1, 1)) != PCM_OK) return rc;
  if ((rc = M->rows.reserve(c, kApplyBlocks * kRow, kApplyBlocks * kRow)) != PCM_OK) return rc;
  if (!M->d_back) {
    if ((rc = M->d_back.reserve(c, 1, 1)) != PCM_OK) return rc;
    PCM_HIPCK(c, hipMemsetAsync(M->d_back.p, 0, sizeof(Back), c->stream));
    std::memset(M->h_back.p, 0, sizeof(Back));
  }
  return PCM_OK;
}

// insertScan of two device clouds (float4 rows) under one origin
int insert_device(pcm_ctx* c, OctoMap* M, const Seg seg[2], const float origin[3], const float* T12, pcm_octo_insert_result* res) {
  pcm_octo_insert_result r;
  std::memset(&r, 0, sizeof(r));
  r.points_in = (uint64_t)seg[0].n + seg[1].n;
  auto done = [&](int rc) { r.status = rc; if (res) *res = r; return rc; };
  for (int a = 0; a < 3; a++) if (!finite_f(origin[a])) { c->err = "the sensor origin must be finite"; return done(PCM_ERR_INVALID_ARGUMENT); }
  if (T12) for (int a = 0; a < 12; a++) if (!finite_f(T12[a])) { c->err = "sensor_to_world must be finite"; return done(PCM_ERR_INVALID_ARGUMENT); }
  if (r.points_in == 0) return done(PCM_OK);
  PCM_HIPCK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  M->projected = false;
  for (float& v : M->phase_ms) v = 0.f;
  const uint32_t total = (uint32_t)r.points_in;
  for (;;) {
    MarkArgs A;
    std::memset(&A, 0, sizeof(A));
    A.tab = M->tab; A.mask = M->n_slots - 1u; A.cells_cap = M->cells_cap; A.epoch = (uint32_t)++M->epoch; A.has_T = T12 ? 1u : 0u;
    A.touched = M->touched; A.call = &M->d_back.p->call; A.stats = &M->d_back.p->stats;
    A.seg[0] = seg[0]; A.seg[1] = seg[1];
    for (int a = 0; a < 3; a++) A.o[a] = origin[a];
    if (T12) for (int a = 0; a < 12; a++) A.T[a] = T12[a];
    A.R = M->R;
    if (M->epoch >= 0xfffffff0ull) { c->err = "3D occupancy map: 2^32 mark passes since the reset (reset the map)"; return done(PCM_ERR_OUT_OF_RANGE); }
    hipError_t e = hipMemsetAsync(A.call, 0, sizeof(Call), st);
    if (e != hipSuccess) { c->err = std::string("3D occupancy map: ") + hipGetErrorString(e); return done(PCM_ERR_HIP); }
    const bool timed = M->timed && M->ev[2];
    if (timed) (void)hipEventRecord(M->ev[0], st);
    const unsigned lane_grid = (total + 255u) / 256u, wave_grid = (total + 3u) / 4u;
    switch (M->variant & 3) {
      case 0: k_octo_mark<true><<<lane_grid, 256, 0, st>>>(A); break;
      case 1: k_octo_mark_wave<true><<<wave_grid, 256, 0, st>>>(A); break;
      case 2: k_octo_mark<false><<<lane_grid, 256, 0, st>>>(A); break;
      default: k_octo_mark_wave<false><<<wave_grid, 256, 0, st>>>(A); break;
    }
    if (timed) (void)hipEventRecord(M->ev[1], st);
    k_octo_apply<<<kApplyBlocks, 256, 0, st>>>(M->tab, M->touched, A.call, M->R, A.epoch, M->cells_cap, M->rows);
    k_octo_fold<<<1, 64, 0, st>>>(M->rows, kApplyBlocks, A.call, A.stats);
    if (timed) (void)hipEventRecord(M->ev[2], st);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(M->h_back.p, M->d_back.p, sizeof(Back), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // the one wait of a call without growth
    if (e == hipSuccess && timed) {
      float a = 0.f, b = 0.f;
      if (hipEventElapsedTime(&a, M->ev[0], M->ev[1]) == hipSuccess && hipEventElapsedTime(&b, M->ev[1], M->ev[2]) == hipSuccess) {
        M->phase_ms[0] += a; M->phase_ms[1] += b;
      }
      M->phase_ms[3] += 1.f;
    }
    if (e != hipSuccess) { c->err = std::string("3D occupancy map insert: ") + hipGetErrorString(e); return done(PCM_ERR_HIP); }
    const Back& B = *back_of(M);
    if (!B.call.overflow) {
      r.dropped_nonfinite = B.call.cnt[kDropped]; r.skipped_window = B.call.cnt[kWindow]; r.skipped_min_range = B.call.cnt[kMinRange];
      r.truncated = B.call.cnt[kTruncated]; r.rejected_rays = B.call.cnt[kRejected];
      r.cells_touched = B.call.touched; r.new_cells = B.call.new_cells;
      return done(PCM_OK);
    }
    // the table filled up: nothing was applied.  Twice the room, the observed cells moved, the same scan marked again.
    const bool at_limit = (uint64_t)M->cells_cap >= M->P.max_cells;
    const uint64_t room = at_limit ? M->cells_cap : std::min<uint64_t>(2ull * M->cells_cap, M->P.max_cells);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = rehash(c, M, room);
    M->phase_ms[2] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != PCM_OK) return done(rc);
    if (at_limit) { c->err = "3D occupancy map: the scan needs more than max_cells cells; the map is unchanged"; return done(PCM_ERR_OUT_OF_RANGE); }
    r.table_growths++;
  }
}

template <typename T>
int reserve_half(pcm_ctx* c, DevBuf<T>* b, size_t n) { return b->reserve(c, n, n + n / 2 + 64); }

// the known cells (mode 0) or the occupied centres (mode 1) sorted by packed key into M->out; *n their number (records false: the number alone)
int collect(pcm_ctx* c, OctoMap* M, int mode, size_t* n, bool records = true) {
  *n = 0;
  const Back& B = *back_of(M);
  const size_t cap = mode == 0 ? (size_t)B.stats.cells : (size_t)B.stats.occupied;
  if (cap == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  DevScratch sc(st);
  unsigned long long *k0 = nullptr, *k1 = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr, *count = nullptr;
  int rc;
  if ((rc = sc.take(&k0, cap, &c->err, "octomap keys")) != PCM_OK || (rc = sc.take(&k1, cap, &c->err, "octomap keys")) != PCM_OK ||
      (rc = sc.take(&v0, cap, &c->err, "octomap slots")) != PCM_OK || (rc = sc.take(&v1, cap, &c->err, "octomap slots")) != PCM_OK ||
      (rc = sc.take(&count, 1, &c->err, "octomap count")) != PCM_OK) return rc;
  if ((rc = reserve_half(c, &M->out, cap)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipMemsetAsync(count, 0, sizeof(uint32_t), st));
  k_octo_collect<<<std::min<uint32_t>(4096u, (M->n_slots + 255u) / 256u), 256, 0, st>>>(M->tab, M->n_slots, mode, M->R, M->P.filter_speckles, k0, v0, (uint32_t)cap, count);
  PCM_HIPCK(c, hipGetLastError());
  uint32_t h_count = 0;
  PCM_HIPCK(c, hipMemcpyAsync(&h_count, count, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipStreamSynchronize(st));
  if (h_count > cap) { c->err = "3D occupancy map: more cells than counted (internal error)"; return PCM_ERR_INTERNAL; }
  if (h_count == 0) return PCM_OK;
  if (!records) { *n = h_count; return PCM_OK; }   // the count alone: no sort
  if ((rc = scratch_sort_pairs(sc, &c->err, k0, k1, v0, v1, (size_t)h_count, 0, 48)) != PCM_OK) return rc;
  k_octo_emit<<<(h_count + 255u) / 256u, 256, 0, st>>>(M->tab, k1, v1, h_count, mode, M->R.res, M->out);
  PCM_HIPCK(c, hipGetLastError());
  *n = h_count;
  return PCM_OK;
}

int copy_out(pcm_ctx* c, void* user, const void* dev, size_t bytes, int memory) {
  if (bytes == 0) return PCM_OK;
  PCM_HIPCK(c, hipMemcpyAsync(user, dev, bytes, memory == PCM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

int get_records(pcm_ctx* c, int mode, void* out, size_t capacity, int memory, size_t* n) {
  if (n) *n = 0;
  OctoMap* M = nullptr;
  int rc = check_ctx_octo(c, &M, true);
  if (rc != PCM_OK) return rc;
  if (!n) { c->err = "null count pointer"; return PCM_ERR_INVALID_ARGUMENT; }
  if ((rc = check_memory(c, memory, "memory")) != PCM_OK) return rc;
  if (!out && capacity == 0 && mode == 0) {   // the count alone: the statistics have it
    *n = (size_t)back_of(M)->stats.cells;
    return PCM_OK;
  }
  size_t m = 0;
  if ((rc = collect(c, M, mode, &m, out != nullptr || capacity != 0)) != PCM_OK) return rc;
  *n = m;
  if (capacity < m || (m && !out)) {
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));
    c->err = "capacity too small (the count is returned)";
    return PCM_ERR_INVALID_ARGUMENT;
  }
  if (m == 0) return PCM_OK;
  return copy_out(c, out, M->out, sizeof(int4) * m, memory);
}

int ensure_project(pcm_ctx* c, OctoMap* M) {
  if (M->projected) return PCM_OK;
  std::memset(&M->G, 0, sizeof(M->G));
  M->G.resolution = M->R.res;
  const Back& B = *back_of(M);
  if (B.stats.cells <= 1ull) { M->projected = true; return PCM_OK; }   // publishAll :501
  OctoGeom G;
  if (!octo_grid_geometry(B.stats.kmin, B.stats.kmax, M->R.res, M->P.min_x_size, M->P.min_y_size, &G)) {   // :973-980: no map
    M->projected = true;
    return PCM_OK;
  }
  const size_t m = (size_t)G.width * (size_t)G.height;
  if (m > (1ull << 31)) { c->err = "the projected map would exceed 2^31 cells"; return PCM_ERR_OUT_OF_RANGE; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  int rc;
  if ((rc = reserve_half(c, &M->d_grid, m)) != PCM_OK || (rc = reserve_half(c, &M->d_pgm, m)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipMemsetAsync(M->d_grid, 0xff, m, st));
  const uint32_t grid = std::min<uint32_t>(4096u, (M->n_slots + 255u) / 256u);
  for (int pass = 0; pass < 2; pass++)
    k_octo_project<<<grid, 256, 0, st>>>(M->tab, M->n_slots, M->R, M->P.filter_speckles, G.min_key[0], G.min_key[1], G.width, G.height, pass, M->d_grid);
  k_octo_pgm<<<(unsigned)std::min<size_t>(4096, (m + 255) / 256), 256, 0, st>>>(M->d_grid, (uint32_t)G.width, (uint32_t)G.height, M->d_pgm);
  PCM_HIPCK(c, hipGetLastError());
  PCM_HIPCK(c, hipStreamSynchronize(st));
  M->G = G;
  M->projected = true;
  return PCM_OK;
}

}  // namespace

extern "C" {

void pcm_octo_default_params(pcm_octo_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->resolution = 0.05;        // OctomapServer.cpp:44-163
  p->prob_hit = 0.7;
  p->prob_miss = 0.4;
  p->clamp_min = 0.12;
  p->clamp_max = 0.97;
  p->max_range = -1.0;
  p->min_range = -1.0;
  p->pointcloud_min_x = p->pointcloud_min_y = p->pointcloud_min_z = -DBL_MAX;
  p->pointcloud_max_x = p->pointcloud_max_y = p->pointcloud_max_z = DBL_MAX;
  p->occupancy_min_z = -DBL_MAX;
  p->occupancy_max_z = DBL_MAX;
  p->min_x_size = 0.0;
  p->min_y_size = 0.0;
  p->filter_speckles = 0;
  p->initial_cells = 65536;
  p->max_cells = 1ull << 28;
}

int pcm_octo_reset(pcm_ctx* c, const pcm_octo_params* params) {
  OctoMap* M = nullptr;
  int rc = check_ctx_octo(c, &M, false);
  if (rc != PCM_OK) return rc;
  pcm_octo_params p;
  if (params) p = *params; else pcm_octo_default_params(&p);
  if ((rc = check_params(c, p)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipSetDevice(c->device));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  M->have_params = false;   // until every buffer below exists: a reset that fails half-way leaves no map, not one with a missing table
  M->n_slots = 0; M->cells_cap = 0;
  if ((rc = ensure_small(c, M)) != PCM_OK) return rc;
  const uint32_t ns = slots_for(p.initial_cells);
  if (!M->tab || ns > M->tab.cap) {
    if ((rc = M->tab.reserve(c, ns, ns)) != PCM_OK) return rc;
  }
  if ((rc = M->touched.reserve(c, (size_t)p.initial_cells, (size_t)p.initial_cells)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipMemsetAsync(M->tab, 0, sizeof(Slot) * (size_t)ns, c->stream));
  PCM_HIPCK(c, hipMemsetAsync(M->d_back.p, 0, sizeof(Back), c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  std::memset(M->h_back.p, 0, sizeof(Back));
  M->n_slots = ns;
  M->cells_cap = (uint32_t)p.initial_cells;
  M->P = p;
  OctoRules& R = M->R;
  R.res = p.resolution; R.max_range = p.max_range; R.min_range = p.min_range; R.occ_min_z = p.occupancy_min_z; R.occ_max_z = p.occupancy_max_z;
  R.hit = octo_logodds(p.prob_hit); R.miss = octo_logodds(p.prob_miss); R.clamp_min = octo_logodds(p.clamp_min); R.clamp_max = octo_logodds(p.clamp_max);
  R.lo[0] = octo_limit(p.pointcloud_min_x); R.lo[1] = octo_limit(p.pointcloud_min_y); R.lo[2] = octo_limit(p.pointcloud_min_z);
  R.hi[0] = octo_limit(p.pointcloud_max_x); R.hi[1] = octo_limit(p.pointcloud_max_y); R.hi[2] = octo_limit(p.pointcloud_max_z);
  M->epoch = 0;
  M->projected = false;
  M->have_params = true;
  return PCM_OK;
}

int pcm_octo_insert_scan(pcm_ctx* c, const void* ground, size_t n_ground, const void* nonground, size_t n_nonground, size_t stride, int memory,
                         const float origin[3], const float* sensor_to_world, pcm_octo_insert_result* result) {
  if (result) std::memset(result, 0, sizeof(*result));
  OctoMap* M = nullptr;
  int rc = check_ctx_octo(c, &M, true);
  if (rc == PCM_OK && !origin) { c->err = "null origin"; rc = PCM_ERR_INVALID_ARGUMENT; }
  if (rc == PCM_OK) rc = check_point_records(c, ground, n_ground, stride, memory, 0x3fffffffull);
  if (rc == PCM_OK) rc = check_point_records(c, nonground, n_nonground, stride, memory, 0x3fffffffull);
  if (rc != PCM_OK) { if (result) result->status = rc; return rc; }
  auto fail = [&](int e) { if (result) result->status = e; return e; };
  const void* src[2] = {ground, nonground};
  const size_t ns[2] = {n_ground, n_nonground};
  Seg seg[2] = {{nullptr, (uint32_t)n_ground, 1u}, {nullptr, (uint32_t)n_nonground, 0u}};
  hipError_t he = hipSetDevice(c->device);
  if (he != hipSuccess) { c->err = std::string("hipSetDevice: ") + hipGetErrorString(he); return fail(PCM_ERR_HIP); }
  const bool in_place = memory == PCM_MEM_DEVICE && stride == sizeof(float4);
  size_t staged = 0;
  for (int k = 0; k < 2; k++)
    if (ns[k] && !(in_place && (reinterpret_cast<uintptr_t>(src[k]) % sizeof(float4)) == 0)) staged += ns[k];
  if (staged && (rc = reserve_half(c, &M->stage, staged)) != PCM_OK) return fail(rc);
  size_t at = 0;
  for (int k = 0; k < 2; k++) {
    if (!ns[k]) continue;
    if (in_place && (reinterpret_cast<uintptr_t>(src[k]) % sizeof(float4)) == 0) { seg[k].pts = static_cast<const float4*>(src[k]); continue; }
    if ((rc = load_xyzw_rows(c, src[k], ns[k], stride, memory, false, M->stage + at)) != PCM_OK) return fail(rc);   // w is never read
    seg[k].pts = M->stage + at;
    at += ns[k];
  }
  float T12[12];
  if (sensor_to_world) for (int a = 0; a < 12; a++) T12[a] = sensor_to_world[a];
  return insert_device(c, M, seg, origin, sensor_to_world ? T12 : nullptr, result);
}

int pcm_octo_insert_keyframes(pcm_ctx* c, int first, int n) {
  OctoMap* M = nullptr;
  int rc = check_ctx_octo(c, &M, true);
  if (rc != PCM_OK) return rc;
  if (c->cfg.model != PCM_MODEL_LOAM) { c->err = "pcm_octo_insert_keyframes needs a context created with PCM_MODEL_LOAM"; return PCM_ERR_INVALID_ARGUMENT; }
  const loam::KeyPose* kp = nullptr;
  const int K = loam::loam_keyposes(c, &kp);
  if (first < 0 || n < 0 || (long long)first + n > K) { c->err = "pcm_octo_insert_keyframes: first + n exceeds the number of key frames"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int i = 0; i < n; i++) {
    Seg seg[2];
    float pose[6], T[12], trig[6];
    for (int k = 0; k < 2; k++) {
      seg[k].ground = 0u;
      if (!loam::loam_keyframe_cloud(c, first + i, k, &seg[k].pts, &seg[k].n)) { c->err = "pcm_octo_insert_keyframes: no such key frame"; return PCM_ERR_INTERNAL; }
    }
    if (!loam::loam_keyframe_pose(c, first + i, pose)) { c->err = "pcm_octo_insert_keyframes: no such key frame"; return PCM_ERR_INTERNAL; }
    loam::pose_matrix(pose, T, trig);
    const float origin[3] = {pose[3], pose[4], pose[5]};
    if ((rc = insert_device(c, M, seg, origin, T, nullptr)) != PCM_OK) return rc;
  }
  return PCM_OK;
}

int pcm_octo_info(pcm_ctx* c, pcm_octo_map_info* info) {
  OctoMap* M = nullptr;
  int rc = check_ctx_octo(c, &M, true);
  if (rc != PCM_OK) return rc;
  if (!info) { c->err = "null info"; return PCM_ERR_INVALID_ARGUMENT; }
  std::memset(info, 0, sizeof(*info));
  const Back& B = *back_of(M);
  info->cells = B.stats.cells; info->occupied = B.stats.occupied; info->free_cells = B.stats.free_cells;
  info->capacity = M->cells_cap; info->epoch = M->epoch;
  info->resolution = M->R.res;
  info->hit = M->R.hit; info->miss = M->R.miss; info->clamp_min = M->R.clamp_min; info->clamp_max = M->R.clamp_max;
  if (B.stats.cells) {
    for (int a = 0; a < 3; a++) {
      info->key_min[a] = B.stats.kmin[a]; info->key_max[a] = B.stats.kmax[a];
      info->metric_min[a] = octo_coord(B.stats.kmin[a], M->R.res) - M->R.res / 2.0;
      info->metric_max[a] = octo_coord(B.stats.kmax[a], M->R.res) + M->R.res / 2.0;
    }
  }
  return PCM_OK;
}

int pcm_octo_debug(pcm_ctx* c, int mark_variant, int timed) {
  OctoMap* M = nullptr;
  int rc = check_ctx_octo(c, &M, false);
  if (rc != PCM_OK) return rc;
  if (mark_variant < 0 || mark_variant > 3) { c->err = "mark_variant must be 0 .. 3"; return PCM_ERR_INVALID_ARGUMENT; }
  M->variant = mark_variant;
  M->timed = timed != 0;
  if (M->timed && !M->ev[0]) {
    PCM_HIPCK(c, hipSetDevice(c->device));
    for (hipEvent_t& e : M->ev) PCM_HIPCK(c, hipEventCreate(&e));
  }
  return PCM_OK;
}

int pcm_octo_phase_ms(pcm_ctx* c, float ms[4]) {
  OctoMap* M = nullptr;
  int rc = check_ctx_octo(c, &M, false);
  if (rc != PCM_OK) return rc;
  if (!ms) { c->err = "null ms"; return PCM_ERR_INVALID_ARGUMENT; }
  for (int a = 0; a < 4; a++) ms[a] = M->phase_ms[a];
  return PCM_OK;
}

int pcm_octo_get_cells(pcm_ctx* c, void* out, size_t capacity, int memory, size_t* n) { return get_records(c, 0, out, capacity, memory, n); }

int pcm_octo_get_occupied(pcm_ctx* c, void* out, size_t capacity, int memory, size_t* n) { return get_records(c, 1, out, capacity, memory, n); }

int pcm_octo_project(pcm_ctx* c, pcm_octo_grid_info* info, int8_t* grid, size_t capacity, int memory) {
  OctoMap* M = nullptr;
  int rc = check_ctx_octo(c, &M, true);
  if (rc != PCM_OK) return rc;
  if ((rc = check_memory(c, memory, "memory")) != PCM_OK) return rc;
  if ((rc = ensure_project(c, M)) != PCM_OK) return rc;
  if (info) {
    std::memset(info, 0, sizeof(*info));
    info->width = M->G.width; info->height = M->G.height; info->min_key_x = M->G.min_key[0]; info->min_key_y = M->G.min_key[1];
    info->resolution = M->G.resolution; info->origin_x = M->G.origin_x; info->origin_y = M->G.origin_y;
  }
  if (!grid) return PCM_OK;
  const size_t m = (size_t)M->G.width * (size_t)M->G.height;
  if (capacity < m) { c->err = "capacity too small (pcm_octo_project without a grid gives width x height)"; return PCM_ERR_INVALID_ARGUMENT; }
  return copy_out(c, grid, M->d_grid, m, memory);
}

int pcm_octo_get_pgm(pcm_ctx* c, uint8_t* data, size_t capacity, int memory) {
  OctoMap* M = nullptr;
  int rc = check_ctx_octo(c, &M, true);
  if (rc != PCM_OK) return rc;
  if ((rc = check_memory(c, memory, "memory")) != PCM_OK) return rc;
  if ((rc = ensure_project(c, M)) != PCM_OK) return rc;
  const size_t m = (size_t)M->G.width * (size_t)M->G.height;
  if (m == 0) return PCM_OK;
  if (!data) { c->err = "null output buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  if (capacity < m) { c->err = "capacity too small (pcm_octo_project gives width x height)"; return PCM_ERR_INVALID_ARGUMENT; }
  return copy_out(c, data, M->d_pgm, m, memory);
}

}  // extern "C"
