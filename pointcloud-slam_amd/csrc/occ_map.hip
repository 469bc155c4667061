// occ_map.hip -- 2D occupancy grid mapping of jueying_slam (src/tool/occupancy_mapping) on the device (include/pcm_amd.h, pcm_occ_*):
// getScan (mapping_server.cc:99-136), processScan (:346-382) with TraceLine (:42-97), getGridMap (:153-216) and saveMap's bytes
// (:301-313).  Arithmetic: occ_map.h.
//
// State: a dense rectangle of cells, two uint32 counters each (n_occ, n_free, interleaved), grown on the host before any launch
// from the poses of the batch; a kernel never forms an address from data alone: occ_slot() drops a cell outside the rectangle
// and the drop is counted (the count must stay 0 and is reported as an error).
// k_occ_scan: one lane per point of the whole batch (grid-stride), unsigned atomicMin on the bits of the (non-negative) range into
// the S x beam_size table.  k_occ_trace: one lane per (scan, beam), atomicAdd of 1 on the end cell and along the Bresenham walk.
// Integer minima and integer sums do not depend on the schedule or on how scans are batched.
// k_occ_bounds: bounding box and number of the known cells; k_occ_render: the cropped int8 grid, its PGM bytes and the counters.
#include "host_util.h"
#include "loam_device.h"
#include "occ_map.h"
#include "voxel_grid.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace pcm;
using namespace pcm::occ;

namespace {

constexpr uint32_t kChunkBeams = 1u << 24;    // entries of the beam table of one set of launches
constexpr uint64_t kChunkPoints = 1ull << 30; // points of one set of launches
enum { kOverflow = 0, kMinX = 1, kMaxX = 2, kMinY = 3, kMaxY = 4, kKnown = 5, kSmallWords = 8 };

struct OccSeg {   // one cloud of one scan
  const float4* pts;
  uint32_t n;
  uint32_t scan;   // within the chunk
};

struct OccPose { double yaw, x, y; };

__global__ void k_occ_fill(uint32_t* __restrict__ p, uint32_t n, uint32_t v) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// old rectangle -> its place in the new one (the new one covers it)
__global__ void k_occ_move(const uint2* __restrict__ src, OccRect a, uint2* __restrict__ dst, OccRect b) {
  const long long n = a.w * a.h;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long cy = i / a.w, cx = i - cy * a.w;
    const long long tx = cx + a.x0 - b.x0, ty = cy + a.y0 - b.y0;
    if (tx >= 0 && ty >= 0 && tx < b.w && ty < b.h) dst[ty * b.w + tx] = src[i];
  }
}

// off[s] <= g < off[s + 1]: the segment of point g
__global__ void __launch_bounds__(256) k_occ_scan(const OccSeg* __restrict__ segs, const uint32_t* __restrict__ off, uint32_t nseg, uint32_t total, OccParams P,
                                                  uint32_t beams, uint32_t* __restrict__ table) {
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < total; g += gridDim.x * blockDim.x) {
    const uint32_t lo = table_row_of(off, 1u, nseg, g);
    const OccSeg sg = segs[lo];
    const uint32_t k = g - off[lo];
    if (k >= sg.n) continue;
    const float4 p = sg.pts[k];
    uint32_t beam;
    float range;
    if (occ_point_beam(p.x, p.y, p.z, P, beams, &beam, &range)) atomicMin(&table[(size_t)sg.scan * beams + beam], __float_as_uint(range));
  }
}

__device__ inline void occ_add(uint32_t* __restrict__ cells, const OccRect& R, int ix, int iy, int which, uint32_t* __restrict__ small) {
  const long long s = occ_slot(ix, iy, R);
  if (s < 0) { atomicAdd(&small[kOverflow], 1u); return; }
  atomicAdd(&cells[2 * s + which], 1u);
}

__global__ void __launch_bounds__(256) k_occ_trace(const uint32_t* __restrict__ table, const OccPose* __restrict__ poses, uint32_t n_scans, uint32_t beams, OccParams P,
                                                   uint32_t* __restrict__ cells, OccRect R, uint32_t* __restrict__ small) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_scans * beams) return;
  const uint32_t s = idx / beams, b = idx - s * beams;
  const float r = occ_beam_range(__uint_as_float(table[idx]), P);
  double dist;
  bool hit, trace;
  if (!occ_beam_dist(r, P, &dist, &hit, &trace)) return;
  const OccPose q = poses[s];
  const int rx = occ_cell(q.x, P.resolution), ry = occ_cell(q.y, P.resolution);
  int cx, cy;
  occ_end_cell(dist, occ_beam_angle(b, P.angle_increment), q.yaw, q.x, q.y, P.resolution, &cx, &cy);
  if (hit) occ_add(cells, R, cx, cy, 0, small);
  if (trace) occ_trace_line(rx, ry, cx, cy, [&](int x, int y) { occ_add(cells, R, x, y, 1, small); });
}

// bounding box (offsets inside the rectangle) and number of the known cells; init_slot: the cell the map was initialised at, or -1
__global__ void __launch_bounds__(256) k_occ_bounds(const uint2* __restrict__ cells, OccRect R, long long init_slot, uint32_t* __restrict__ small) {
  const long long n = R.w * R.h;
  uint32_t mnx = 0xffffffffu, mxx = 0u, mny = 0xffffffffu, mxy = 0u, cnt = 0u;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const uint2 c = cells[i];
    if (c.x == 0u && c.y == 0u && i != init_slot) continue;
    const long long cy = i / R.w, cx = i - cy * R.w;
    mnx = min(mnx, (uint32_t)cx); mxx = max(mxx, (uint32_t)cx);
    mny = min(mny, (uint32_t)cy); mxy = max(mxy, (uint32_t)cy);
    cnt++;
  }
  cnt = vg::wave_sum_u32(cnt);
  if (cnt == 0u) return;   // the same in every lane of the wave
  mnx = vg::wave_min_u32(mnx); mxx = vg::wave_max_u32(mxx); mny = vg::wave_min_u32(mny); mxy = vg::wave_max_u32(mxy);
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&small[kMinX], mnx); atomicMax(&small[kMaxX], mxx);
    atomicMin(&small[kMinY], mny); atomicMax(&small[kMaxY], mxy);
    atomicAdd(&small[kKnown], cnt);
  }
}

// the crop [cx0, cx0 + w) x [cy0, cy0 + h) of the rectangle: value (row-major, i + j * w), PGM byte (rows top-down) and counters
__global__ void __launch_bounds__(256) k_occ_render(const uint2* __restrict__ cells, OccRect R, long long init_slot, uint32_t cx0, uint32_t cy0, uint32_t w, uint32_t h,
                                                    double log_occ, double log_free, int8_t* __restrict__ grid, unsigned char* __restrict__ pgm,
                                                    uint32_t* __restrict__ n_occ, uint32_t* __restrict__ n_free) {
  const size_t n = (size_t)w * h;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
    const uint32_t j = (uint32_t)(k / w), i = (uint32_t)(k - (size_t)j * w);
    const long long s = (long long)(cy0 + j) * R.w + (cx0 + i);
    const uint2 c = cells[s];
    const int v = occ_cell_value(c.x, c.y, s == init_slot, log_occ, log_free);
    grid[k] = (int8_t)v;
    pgm[(size_t)(h - 1 - j) * w + i] = occ_pgm_byte(v);
    n_occ[k] = c.x;
    n_free[k] = c.y;
  }
}

struct OccMap {
  OccParams P{};
  uint32_t beams = 0;
  OccRect R{0, 0, 0, 0};
  DevBuf<uint2> cells;           // cap: cells of the allocation (a reset keeps it)
  bool have_init = false;
  int init_x = 0, init_y = 0;
  uint64_t n_scans = 0, overflow = 0;
  // the last set of launches
  DevBuf<uint32_t> table;
  uint32_t last_scans = 0;
  DevBuf<OccSeg> d_seg;
  DevBuf<uint32_t> d_off;
  DevBuf<OccPose> d_pose;
  DevBuf<float4> stage;
  DevBuf<uint32_t> d_small;
  PinnedBuf<uint32_t> h_small;
  // the last render
  bool rendered = false;
  uint32_t cw = 0, ch = 0, n_known = 0;
  long long cx0 = 0, cy0 = 0;    // cell index of the crop's first cell
  DevBuf<int8_t> d_grid;
  DevBuf<unsigned char> d_pgm;
  DevBuf<uint32_t> d_cnt;        // [2][cw * ch]
};

int check_ctx_occ(pcm_ctx* c, OccMap** out, bool need_params) {
  *out = nullptr;
  if (!c) return PCM_ERR_INVALID_ARGUMENT;
  if (c->device < 0) return PCM_ERR_HIP;
  *out = c->occ.get_or_create<OccMap>();
  if (!*out) { c->err = "the occupancy map could not be allocated (out of host memory)"; return PCM_ERR_INTERNAL; }
  if (need_params && (*out)->beams == 0) { c->err = "no occupancy map yet: call pcm_occ_reset first"; return PCM_ERR_NO_INPUT; }
  return PCM_OK;
}

int check_oparams(pcm_ctx* c, const pcm_occ_params& p) {
  const double v[9] = {p.min_z, p.max_z, p.angle_increment, p.min_range, p.max_range, p.log_occ, p.log_free, p.resolution, p.max_radius};
  for (double x : v) if (!finite_d(x)) { c->err = "every occupancy parameter must be finite"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.angle_increment > 0.0) || (3.1415927 - (-3.1415927)) / p.angle_increment > (double)kOccMaxBeams) {
    c->err = "angle_increment must be positive and give at most 2^20 beams"; return PCM_ERR_INVALID_ARGUMENT;
  }
  if (!(p.resolution > 0.0)) { c->err = "resolution must be positive"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.max_radius > 0.0)) { c->err = "max_radius must be positive"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.min_range >= 0.0) || !(p.max_range >= p.min_range) || !(p.max_range < 1.0e30)) { c->err = "0 <= min_range <= max_range < 1e30 is required"; return PCM_ERR_INVALID_ARGUMENT; }
  if (((2.0 * (p.max_radius + 0.1)) / p.resolution + 8.0) * ((2.0 * (p.max_radius + 0.1)) / p.resolution + 8.0) > (double)kOccMaxCells) {
    c->err = "max_radius / resolution: one scan alone would exceed the cap of 2^28 cells"; return PCM_ERR_INVALID_ARGUMENT;
  }
  return PCM_OK;
}

// the rectangle covers [lx, hx] x [ly, hy] afterwards: reallocation + copy when it does not yet, grown by half the size on the
// sides that moved so that a trajectory does not reallocate per scan
int ensure_rect(pcm_ctx* c, OccMap* M, long long lx, long long hx, long long ly, long long hy) {
  const OccRect& R = M->R;
  const bool empty = !M->cells || R.w == 0 || R.h == 0;
  if (!empty && lx >= R.x0 && ly >= R.y0 && hx < R.x0 + R.w && hy < R.y0 + R.h) return PCM_OK;
  long long ux0 = lx, ux1 = hx, uy0 = ly, uy1 = hy;   // the union, inclusive
  if (!empty) { ux0 = std::min(ux0, R.x0); ux1 = std::max(ux1, R.x0 + R.w - 1); uy0 = std::min(uy0, R.y0); uy1 = std::max(uy1, R.y0 + R.h - 1); }
  long long gx0 = ux0, gx1 = ux1, gy0 = uy0, gy1 = uy1;
  if (!empty) {
    const long long pw = (ux1 - ux0 + 1) / 2, ph = (uy1 - uy0 + 1) / 2;
    if (ux0 < R.x0) gx0 -= pw;
    if (ux1 > R.x0 + R.w - 1) gx1 += pw;
    if (uy0 < R.y0) gy0 -= ph;
    if (uy1 > R.y0 + R.h - 1) gy1 += ph;
  }
  auto cells_of = [](long long a0, long long a1, long long b0, long long b1) { return (double)(a1 - a0 + 1) * (double)(b1 - b0 + 1); };
  if (cells_of(gx0, gx1, gy0, gy1) > (double)kOccMaxCells) { gx0 = ux0; gx1 = ux1; gy0 = uy0; gy1 = uy1; }   // no room for the margin
  if (cells_of(gx0, gx1, gy0, gy1) > (double)kOccMaxCells) {
    c->err = "the occupancy map would exceed the cap of 2^28 cells (coarser resolution, or one map per area)";
    return PCM_ERR_INVALID_ARGUMENT;
  }
  const OccRect N{gx0, gy0, gx1 - gx0 + 1, gy1 - gy0 + 1};
  const size_t n = (size_t)(N.w * N.h);
  if (empty && M->cells && n <= M->cells.cap) {   // after a reset: the allocation is reused
    PCM_HIPCK(c, hipMemsetAsync(M->cells, 0, sizeof(uint2) * n, c->stream));
    M->R = N;
    return PCM_OK;
  }
  // a growth that is more than a copy (the old rectangle moves into its place in the new one): allocated here, adopted below
  uint2* nc = nullptr;
  PCM_HIPCK(c, hipMalloc(reinterpret_cast<void**>(&nc), sizeof(uint2) * n));
  hipError_t e = hipMemsetAsync(nc, 0, sizeof(uint2) * n, c->stream);
  if (e == hipSuccess && !empty) {
    const unsigned grid = (unsigned)std::min<long long>(4096, (R.w * R.h + 255) / 256);
    k_occ_move<<<grid, 256, 0, c->stream>>>(M->cells, R, nc, N);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { hipFree(nc); c->err = std::string("occupancy map growth: ") + hipGetErrorString(e); return PCM_ERR_HIP; }
  M->cells.adopt(nc, n);   // synchronised above
  M->R = N;
  return PCM_OK;
}

// the scratch of a set of launches and the staging rows grow by half
template <typename T>
int reserve_half(pcm_ctx* c, DevBuf<T>* b, size_t n) { return b->reserve(c, n, n + n / 2 + 64); }

int ensure_small(pcm_ctx* c, OccMap* M) {
  if (!M->d_small) {
    int rc = M->d_small.reserve(c, kSmallWords, kSmallWords);
    if (rc != PCM_OK) return rc;
    PCM_HIPCK(c, hipMemsetAsync(M->d_small, 0, sizeof(uint32_t) * kSmallWords, c->stream));
  }
  return M->h_small.reserve(c, kSmallWords, kSmallWords);
}

struct HostScan {
  const float4* pts[2];
  uint32_t n[2];
  float pose[6];
};

// one set of launches per chunk of scans: the rectangle first, then table, scan kernel, trace kernel, overflow check
int insert_scans(pcm_ctx* c, OccMap* M, const std::vector<HostScan>& scans) {
  if (scans.empty()) return PCM_OK;
  const OccParams& P = M->P;
  long long lx = 0, hx = 0, ly = 0, hy = 0;
  bool first = true;
  for (const HostScan& s : scans) {
    for (int k = 0; k < 6; k++) if (!occ_finite(s.pose[k])) { c->err = "the poses must be finite"; return PCM_ERR_INVALID_ARGUMENT; }
    long long a, b, d, e;
    if (!occ_pose_rect((double)s.pose[3], (double)s.pose[4], P, &a, &b, &d, &e)) { c->err = "a pose lies outside +-2^30 cells"; return PCM_ERR_INVALID_ARGUMENT; }
    if (first) { lx = a; hx = b; ly = d; hy = e; first = false; }
    else { lx = std::min(lx, a); hx = std::max(hx, b); ly = std::min(ly, d); hy = std::max(hy, e); }
  }
  PCM_HIPCK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_rect(c, M, lx, hx, ly, hy)) != PCM_OK) return rc;
  if ((rc = ensure_small(c, M)) != PCM_OK) return rc;
  hipStream_t st = c->stream;
  if (!M->have_init) {   // initializeMap: the first scan's cell is a node of the map from now on
    M->init_x = occ_cell((double)scans[0].pose[3], P.resolution);
    M->init_y = occ_cell((double)scans[0].pose[4], P.resolution);
    M->have_init = true;
  }
  M->rendered = false;
  const uint32_t beams = M->beams;
  const size_t max_scans = std::max<size_t>(1, kChunkBeams / beams);
  std::vector<OccSeg> segs;
  std::vector<uint32_t> off;
  std::vector<OccPose> poses;
  for (size_t s0 = 0; s0 < scans.size();) {
    segs.clear(); off.clear(); poses.clear();
    uint64_t total = 0;
    size_t s1 = s0;
    while (s1 < scans.size() && s1 - s0 < max_scans) {
      const HostScan& h = scans[s1];
      if (s1 > s0 && total + h.n[0] + h.n[1] > kChunkPoints) break;
      for (int k = 0; k < 2; k++) {
        if (h.n[k] == 0) continue;
        off.push_back((uint32_t)total);
        segs.push_back(OccSeg{h.pts[k], h.n[k], (uint32_t)(s1 - s0)});
        total += h.n[k];
      }
      poses.push_back(OccPose{(double)h.pose[2], (double)h.pose[3], (double)h.pose[4]});
      s1++;
    }
    if (total > 0xfffffff0ull) { c->err = "a scan has too many points"; return PCM_ERR_INVALID_ARGUMENT; }
    const uint32_t S = (uint32_t)(s1 - s0), nseg = (uint32_t)segs.size();
    const uint32_t nt = S * beams;
    if ((rc = reserve_half(c, &M->table, (size_t)nt)) != PCM_OK) return rc;
    if ((rc = reserve_half(c, &M->d_pose, (size_t)S)) != PCM_OK) return rc;
    if ((rc = reserve_half(c, &M->d_seg, (size_t)nseg + 1)) != PCM_OK) return rc;
    if ((rc = reserve_half(c, &M->d_off, (size_t)nseg + 1)) != PCM_OK) return rc;
    PCM_HIPCK(c, hipMemcpyAsync(M->d_pose, poses.data(), sizeof(OccPose) * S, hipMemcpyHostToDevice, st));
    if (nseg) {
      PCM_HIPCK(c, hipMemcpyAsync(M->d_seg, segs.data(), sizeof(OccSeg) * nseg, hipMemcpyHostToDevice, st));
      PCM_HIPCK(c, hipMemcpyAsync(M->d_off, off.data(), sizeof(uint32_t) * nseg, hipMemcpyHostToDevice, st));
    }
    k_occ_fill<<<(nt + 255) / 256, 256, 0, st>>>(M->table, nt, __builtin_bit_cast(uint32_t, occ_range_init(P.max_range)));
    if (total > 0) {
      const unsigned grid = (unsigned)std::min<uint64_t>(8192, (total + 255) / 256);
      k_occ_scan<<<grid, 256, 0, st>>>(M->d_seg, M->d_off, nseg, (uint32_t)total, P, beams, M->table);
    }
    k_occ_trace<<<(nt + 255) / 256, 256, 0, st>>>(M->table, M->d_pose, S, beams, P, reinterpret_cast<uint32_t*>(M->cells.p), M->R, M->d_small);
    PCM_HIPCK(c, hipGetLastError());
    PCM_HIPCK(c, hipMemcpyAsync(M->h_small, M->d_small, sizeof(uint32_t) * kSmallWords, hipMemcpyDeviceToHost, st));
    PCM_HIPCK(c, hipStreamSynchronize(st));   // the vectors above and the caller's buffers are free again
    M->last_scans = S;
    M->n_scans += S;
    if (M->h_small[kOverflow] != 0) {
      M->overflow += M->h_small[kOverflow];
      PCM_HIPCK(c, hipMemsetAsync(M->d_small, 0, sizeof(uint32_t), st));
      c->err = "occupancy map: cells outside the allocated rectangle were dropped (internal error: the host bound did not cover a ray)";
      return PCM_ERR_INTERNAL;
    }
    s0 = s1;
  }
  return PCM_OK;
}

int ensure_render(pcm_ctx* c, OccMap* M) {
  if (M->rendered) return PCM_OK;
  M->cw = M->ch = 0; M->n_known = 0; M->cx0 = M->cy0 = 0;
  if (!M->cells || M->R.w == 0) { M->rendered = true; return PCM_OK; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_small(c, M)) != PCM_OK) return rc;
  hipStream_t st = c->stream;
  const uint32_t init_words[kSmallWords] = {0u, 0xffffffffu, 0u, 0xffffffffu, 0u, 0u, 0u, 0u};
  PCM_HIPCK(c, hipMemcpyAsync(M->d_small, init_words, sizeof(init_words), hipMemcpyHostToDevice, st));
  const long long init_slot = M->have_init ? occ_slot(M->init_x, M->init_y, M->R) : -1;
  const long long n = M->R.w * M->R.h;
  const unsigned grid = (unsigned)std::min<long long>(8192, (n + 255) / 256);
  k_occ_bounds<<<grid, 256, 0, st>>>(M->cells, M->R, init_slot, M->d_small);
  PCM_HIPCK(c, hipGetLastError());
  PCM_HIPCK(c, hipMemcpyAsync(M->h_small, M->d_small, sizeof(uint32_t) * kSmallWords, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipStreamSynchronize(st));
  const uint32_t* h = M->h_small;
  if (h[kKnown] == 0) { M->rendered = true; return PCM_OK; }
  if (h[kMaxX] >= (uint64_t)M->R.w || h[kMaxY] >= (uint64_t)M->R.h || h[kMinX] > h[kMaxX] || h[kMinY] > h[kMaxY]) {
    c->err = "occupancy map: inconsistent bounding box"; return PCM_ERR_INTERNAL;
  }
  const uint32_t w = h[kMaxX] - h[kMinX] + 1, hh = h[kMaxY] - h[kMinY] + 1;
  const size_t m = (size_t)w * hh;
  const size_t cap = m + m / 4 + 256;
  if ((rc = M->d_grid.reserve(c, m, cap)) != PCM_OK || (rc = M->d_pgm.reserve(c, m, cap)) != PCM_OK || (rc = M->d_cnt.reserve(c, 2 * m, 2 * cap)) != PCM_OK) return rc;
  const unsigned rgrid = (unsigned)std::min<size_t>(8192, (m + 255) / 256);
  k_occ_render<<<rgrid, 256, 0, st>>>(M->cells, M->R, init_slot, h[kMinX], h[kMinY], w, hh, M->P.log_occ, M->P.log_free, M->d_grid, M->d_pgm, M->d_cnt, M->d_cnt + m);
  PCM_HIPCK(c, hipGetLastError());
  PCM_HIPCK(c, hipStreamSynchronize(st));
  M->cw = w; M->ch = hh; M->n_known = h[kKnown];
  M->cx0 = M->R.x0 + h[kMinX]; M->cy0 = M->R.y0 + h[kMinY];
  M->rendered = true;
  return PCM_OK;
}

int read_back(pcm_ctx* c, OccMap* M, void* dst, const void* src, size_t bytes, size_t capacity, size_t elems) {
  if (elems == 0) return PCM_OK;
  if (!dst) { c->err = "null output buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  if (capacity < elems) { c->err = "capacity too small (pcm_occ_info gives width x height)"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  return PCM_OK;
}

}  // namespace

extern "C" {

void pcm_occ_default_params(pcm_occ_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_z = -0.15;             // config/rslidar.yaml, config/livox.yaml
  p->max_z = 1.5;
  p->angle_increment = 0.006;
  p->min_range = 0.5;
  p->max_range = 200.0;
  p->log_occ = 0.1;
  p->log_free = -0.01;
  p->resolution = 0.1;
  p->max_radius = 20.0;
  p->fill_with_white = 1;
  p->use_nan = 0;
}

int pcm_occ_reset(pcm_ctx* c, const pcm_occ_params* params) {
  OccMap* M = nullptr;
  int rc = check_ctx_occ(c, &M, false);
  if (rc != PCM_OK) return rc;
  pcm_occ_params p;
  if (params) p = *params; else pcm_occ_default_params(&p);
  if ((rc = check_oparams(c, p)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipSetDevice(c->device));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  M->P = OccParams{p.min_z, p.max_z, p.angle_increment, p.min_range, p.max_range, p.log_occ, p.log_free, p.resolution, p.max_radius, p.fill_with_white ? 1 : 0, p.use_nan ? 1 : 0};
  M->beams = occ_beam_size(p.angle_increment);
  M->R = OccRect{0, 0, 0, 0};   // the allocation stays for the next rectangle
  if (M->d_small) PCM_HIPCK(c, hipMemsetAsync(M->d_small, 0, sizeof(uint32_t) * kSmallWords, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  M->have_init = false;
  M->n_scans = 0; M->overflow = 0; M->last_scans = 0;
  M->rendered = false;
  return PCM_OK;
}

int pcm_occ_insert_scans(pcm_ctx* c, const void* points, const size_t* n_points, const float* poses6, int num_scans, size_t stride, int memory) {
  OccMap* M = nullptr;
  int rc = check_ctx_occ(c, &M, true);
  if (rc != PCM_OK) return rc;
  if (num_scans < 0) { c->err = "num_scans must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (num_scans == 0) return PCM_OK;
  if (!n_points || !poses6) { c->err = "null n_points / poses"; return PCM_ERR_INVALID_ARGUMENT; }
  if ((rc = check_point_records(c, points, 0, stride, memory, 0x3fffffffull)) != PCM_OK) return rc;   // stride and memory kind; sizes and the buffer below
  size_t total = 0;
  for (int s = 0; s < num_scans; s++) {
    if (n_points[s] > 0x3fffffffull) { c->err = "cloud too large"; return PCM_ERR_INVALID_ARGUMENT; }
    total += n_points[s];
  }
  if (total > 0xfffffff0ull) { c->err = "batch too large (split it)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (total && !points) { c->err = "null point buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  const float4* base = nullptr;
  if (total) {
    if (memory == PCM_MEM_DEVICE && stride == sizeof(float4) && (reinterpret_cast<uintptr_t>(points) % sizeof(float4)) == 0) {
      base = static_cast<const float4*>(points);   // in place
    } else {
      if ((rc = reserve_half(c, &M->stage, total)) != PCM_OK) return rc;
      if ((rc = load_xyzw_rows(c, points, total, stride, memory, false, M->stage)) != PCM_OK) return rc;   // w is never read
      base = M->stage;
    }
  }
  std::vector<HostScan> scans((size_t)num_scans);
  size_t at = 0;
  for (int s = 0; s < num_scans; s++) {
    HostScan& h = scans[(size_t)s];
    h.pts[0] = base ? base + at : nullptr; h.n[0] = (uint32_t)n_points[s];
    h.pts[1] = nullptr; h.n[1] = 0;
    for (int k = 0; k < 6; k++) h.pose[k] = poses6[6 * s + k];
    at += n_points[s];
  }
  return insert_scans(c, M, scans);
}

int pcm_occ_insert_keyframes(pcm_ctx* c, int first, int n) {
  OccMap* M = nullptr;
  int rc = check_ctx_occ(c, &M, true);
  if (rc != PCM_OK) return rc;
  if (c->cfg.model != PCM_MODEL_LOAM) { c->err = "pcm_occ_insert_keyframes needs a context created with PCM_MODEL_LOAM"; return PCM_ERR_INVALID_ARGUMENT; }
  const loam::KeyPose* kp = nullptr;
  const int K = loam::loam_keyposes(c, &kp);
  if (first < 0 || n < 0 || (long long)first + n > K) { c->err = "pcm_occ_insert_keyframes: first + n exceeds the number of key frames"; return PCM_ERR_INVALID_ARGUMENT; }
  std::vector<HostScan> scans((size_t)n);
  for (int i = 0; i < n; i++) {
    HostScan& h = scans[(size_t)i];
    for (int k = 0; k < 2; k++)
      if (!loam::loam_keyframe_cloud(c, first + i, k, &h.pts[k], &h.n[k])) { c->err = "pcm_occ_insert_keyframes: no such key frame"; return PCM_ERR_INTERNAL; }
    if (!loam::loam_keyframe_pose(c, first + i, h.pose)) { c->err = "pcm_occ_insert_keyframes: no such key frame"; return PCM_ERR_INTERNAL; }
  }
  return insert_scans(c, M, scans);
}

int pcm_occ_get_scan(pcm_ctx* c, int s, float* ranges, double* angles) {
  OccMap* M = nullptr;
  int rc = check_ctx_occ(c, &M, true);
  if (rc != PCM_OK) return rc;
  if (s < 0 || (uint32_t)s >= M->last_scans) { c->err = "pcm_occ_get_scan: scan outside the last set of launches"; return PCM_ERR_INVALID_ARGUMENT; }
  const uint32_t B = M->beams;
  if (ranges) {
    PCM_HIPCK(c, hipSetDevice(c->device));
    PCM_HIPCK(c, hipMemcpyAsync(ranges, M->table + (size_t)s * B, sizeof(float) * B, hipMemcpyDeviceToHost, c->stream));
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < B; i++) ranges[i] = occ_beam_range(ranges[i], M->P);
  }
  if (angles) for (uint32_t i = 0; i < B; i++) angles[i] = occ_beam_angle(i, M->P.angle_increment);
  return PCM_OK;
}

int pcm_occ_status(pcm_ctx* c, int32_t* beam_size, uint64_t* n_scans, uint64_t* overflow, int64_t rect[4]) {
  OccMap* M = nullptr;
  int rc = check_ctx_occ(c, &M, true);
  if (rc != PCM_OK) return rc;
  if (beam_size) *beam_size = (int32_t)M->beams;
  if (n_scans) *n_scans = M->n_scans;
  if (overflow) *overflow = M->overflow;
  if (rect) { rect[0] = M->R.x0; rect[1] = M->R.y0; rect[2] = M->R.w; rect[3] = M->R.h; }
  return PCM_OK;
}

int pcm_occ_info(pcm_ctx* c, int32_t* width, int32_t* height, double* origin_x, double* origin_y, double* resolution, int64_t* n_known) {
  OccMap* M = nullptr;
  int rc = check_ctx_occ(c, &M, true);
  if (rc != PCM_OK) return rc;
  if ((rc = ensure_render(c, M)) != PCM_OK) return rc;
  if (width) *width = (int32_t)M->cw;
  if (height) *height = (int32_t)M->ch;
  if (origin_x) *origin_x = (double)M->cx0 * M->P.resolution;
  if (origin_y) *origin_y = (double)M->cy0 * M->P.resolution;
  if (resolution) *resolution = M->P.resolution;
  if (n_known) *n_known = (int64_t)M->n_known;
  return PCM_OK;
}

int pcm_occ_get_map(pcm_ctx* c, int8_t* data, size_t capacity) {
  OccMap* M = nullptr;
  int rc = check_ctx_occ(c, &M, true);
  if (rc != PCM_OK) return rc;
  if ((rc = ensure_render(c, M)) != PCM_OK) return rc;
  const size_t m = (size_t)M->cw * M->ch;
  return read_back(c, M, data, M->d_grid, m, capacity, m);
}

int pcm_occ_get_pgm(pcm_ctx* c, uint8_t* data, size_t capacity) {
  OccMap* M = nullptr;
  int rc = check_ctx_occ(c, &M, true);
  if (rc != PCM_OK) return rc;
  if ((rc = ensure_render(c, M)) != PCM_OK) return rc;
  const size_t m = (size_t)M->cw * M->ch;
  return read_back(c, M, data, M->d_pgm, m, capacity, m);
}

int pcm_occ_get_counts(pcm_ctx* c, uint32_t* n_occ, uint32_t* n_free, size_t capacity) {
  OccMap* M = nullptr;
  int rc = check_ctx_occ(c, &M, true);
  if (rc != PCM_OK) return rc;
  if ((rc = ensure_render(c, M)) != PCM_OK) return rc;
  const size_t m = (size_t)M->cw * M->ch;
  if (n_occ && (rc = read_back(c, M, n_occ, M->d_cnt, sizeof(uint32_t) * m, capacity, m)) != PCM_OK) return rc;
  if (n_free && (rc = read_back(c, M, n_free, M->d_cnt + m, sizeof(uint32_t) * m, capacity, m)) != PCM_OK) return rc;
  return PCM_OK;
}

}  // extern "C"
