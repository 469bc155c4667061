// voxel_grid_large.hip -- pcl::VoxelGridLarge (jueying_slam/include/voxel_grid_large.cpp:23-255) on the device: a VoxelGrid whose
// index would overflow is cut in two along its longest axis, both halves are filtered on their own and the results concatenated.
// The recursion becomes a loop over levels.  Every point carries the id of its piece; the ids of a level are in depth-first
// order, so the concatenation is the order of the ids.  A level:
//   box      the min / max of every piece that is not yet a leaf piece (the first level: partial boxes, folded; later: per
//            workgroup in LDS, flushed with one atomic per word and piece)
//   decide   vg::split per piece: leaf piece (its box stays), cut (axis, mid), or no progress
//   [one read-back of three words: cuts, first stuck piece, first piece past the depth cap -- the only host wait of a level]
//   scan     cuts before a piece; new id = id + cuts before, the halves of a cut piece new and new + 1
//   renumber the tables of the next level (leaf flag, box)
//   relabel  every point of a cut piece: new + (v > mid)
// After the last level the segmented pipeline of voxel_grid.h runs with segment = piece: 64-bit keys, one stable sort, one wave
// per cell.  The boxes of the leaf pieces are the ones the levels left, so no min / max pass follows.  gfx950.
#include "pcm_device.h"
#include "pcm_host.h"
#include "pre_layouts.h"
#include "voxel_grid.h"

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdio>

namespace pcm {

namespace {

constexpr uint32_t kNoPiece = 0xffffffffu;   // the id of a point with a non-finite coordinate: it counts nowhere
constexpr uint32_t kSlots = 128;             // pieces a workgroup keeps in LDS during a box pass (direct mapped by id)

struct Cloud {
  const char* base; size_t stride;
  __device__ const float* rec(uint32_t g) const { return reinterpret_cast<const float*>(base + (size_t)g * stride); }
};

using Tables = VlTables;
constexpr uint32_t kBoxBlocks = kVlBoxBlocks;

// the tables of up to cap pieces (pre_layouts.h) at `base` (null: the size alone), *bytes = what they occupy
Tables tables_layout(char* base, size_t cap, size_t* bytes) {
  size_t scan_tmp = 0;
  uint32_t* v = nullptr;
  (void)rocprim::exclusive_scan(nullptr, scan_tmp, v, v, 0u, cap, rocprim::plus<uint32_t>(), nullptr);
  ArenaCarver a(base);
  const Tables T = vl_tables_layout(a, cap, scan_tmp);
  *bytes = a.used();
  return T;
}

// the first level: every finite point is of piece 0.  A lane keeps the box of its points, the workgroup stores one partial box.
__global__ void __launch_bounds__(256) k_vl_first_box(Cloud C, uint32_t N, uint32_t* __restrict__ id, unsigned int* __restrict__ part) {
  unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < N; i += gridDim.x * 256u) {
    const float* p = C.rec(i);
    const float c[3] = {p[0], p[1], p[2]};
    const bool ok = isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]);
    id[i] = ok ? 0u : kNoPiece;
    if (ok)
      for (int a = 0; a < 3; a++) { const unsigned int o = f2ord(c[a]); lo[a] = min(lo[a], o); hi[a] = max(hi[a], o); }
  }
  vg::fold_block_box(lo, hi, part + 6 * (size_t)blockIdx.x);
}

// empty boxes for the pieces a level measures, and its status words
__global__ void __launch_bounds__(256) k_vl_clear(uint32_t P, const uint32_t* __restrict__ fin, unsigned int* __restrict__ mm, uint32_t* __restrict__ status) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p == 0) { status[0] = 0u; status[1] = kNoPiece; status[2] = kNoPiece; }
  if (p >= P || fin[p]) return;
  for (int a = 0; a < 3; a++) { mm[6 * (size_t)p + a] = 0xffffffffu; mm[6 * (size_t)p + 3 + a] = 0u; }
}

// a box into the workgroup's table when the piece owns its slot (or takes a free one), else straight into memory
__device__ inline void vl_put(uint32_t p, const unsigned int (&lo)[3], const unsigned int (&hi)[3], uint32_t* tag, unsigned int (*bx)[6], unsigned int* __restrict__ mm) {
  const uint32_t s = p & (kSlots - 1);
  const uint32_t old = atomicCAS(&tag[s], kNoPiece, p);
  unsigned int* dst = (old == kNoPiece || old == p) ? bx[s] : mm + 6 * (size_t)p;
  for (int a = 0; a < 3; a++) { atomicMin(&dst[a], lo[a]); atomicMax(&dst[3 + a], hi[a]); }
}

// a later level: the boxes of the pieces that are still cut.  A wave whose points share a piece folds its box with a butterfly
// and one lane adds it; the workgroup's table goes to memory once, at the end.
__global__ void __launch_bounds__(256) k_vl_box(Cloud C, uint32_t N, const uint32_t* __restrict__ id, const uint32_t* __restrict__ fin, unsigned int* __restrict__ mm) {
  __shared__ uint32_t tag[kSlots];
  __shared__ unsigned int bx[kSlots][6];
  for (uint32_t s = threadIdx.x; s < kSlots; s += 256u) {
    tag[s] = kNoPiece;
    for (int a = 0; a < 3; a++) { bx[s][a] = 0xffffffffu; bx[s][3 + a] = 0u; }
  }
  __syncthreads();
  for (uint32_t base = blockIdx.x * 256u; base < N; base += gridDim.x * 256u) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t p = i < N ? id[i] : kNoPiece;
    const bool act = p != kNoPiece && !fin[p];
    const unsigned long long am = __ballot(act);
    if (am == 0) continue;
    unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (act) {
      const float* q = C.rec(i);
      for (int a = 0; a < 3; a++) lo[a] = hi[a] = f2ord(q[a]);
    }
    const uint32_t p0 = (uint32_t)__shfl((int)p, __ffsll(am) - 1, 64);
    if (__ballot(act && p != p0) == 0) {
      for (int a = 0; a < 3; a++) { lo[a] = vg::wave_min_u32(lo[a]); hi[a] = vg::wave_max_u32(hi[a]); }
      if ((threadIdx.x & 63u) == 0) vl_put(p0, lo, hi, tag, bx, mm);
    } else if (act) {
      vl_put(p, lo, hi, tag, bx, mm);
    }
  }
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < kSlots; s += 256u) {
    const uint32_t p = tag[s];
    if (p == kNoPiece) continue;
    for (int a = 0; a < 3; a++) { atomicMin(&mm[6 * (size_t)p + a], bx[s][a]); atomicMax(&mm[6 * (size_t)p + 3 + a], bx[s][3 + a]); }
  }
}

// leaf piece, cut or stuck, per piece that is not yet a leaf piece.  may_cut: the depth cap is not reached.
__global__ void __launch_bounds__(256) k_vl_decide(uint32_t P, float leaf, int may_cut, const unsigned int* __restrict__ mm, uint32_t* __restrict__ fin, uint32_t* __restrict__ flag,
                                                   int32_t* __restrict__ axis, float* __restrict__ mid, uint32_t* __restrict__ status) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  uint32_t cut = 0u;
  if (p < P && !fin[p]) {
    int ax; float m;
    const int kind = vg::split(mm + 6 * (size_t)p, leaf, &ax, &m);
    axis[p] = ax; mid[p] = m;
    if (kind == vg::kPieceLeaf) fin[p] = 1u;
    else if (kind == vg::kPieceStuck) atomicMin(&status[1], p);
    else if (!may_cut) atomicMin(&status[2], p);
    else cut = 1u;
  }
  if (p < P) flag[p] = cut;
  const uint32_t cuts = vg::wave_sum_u32(cut);
  if ((threadIdx.x & 63u) == 0 && cuts) atomicAdd(&status[0], cuts);
}

// the tables of the next level: a leaf piece keeps its box under its new id, the halves of a cut piece are open
__global__ void __launch_bounds__(256) k_vl_renumber(uint32_t P, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ before, const unsigned int* __restrict__ mm,
                                                     uint32_t* __restrict__ fin_next, unsigned int* __restrict__ mm_next) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= P) return;
  const uint32_t nw = p + before[p];
  if (flag[p]) { fin_next[nw] = 0u; fin_next[nw + 1] = 0u; return; }
  fin_next[nw] = 1u;   // every piece that is not cut is a leaf piece (a stuck one ends the call)
  for (int a = 0; a < 6; a++) mm_next[6 * (size_t)nw + a] = mm[6 * (size_t)p + a];
}

__global__ void __launch_bounds__(256) k_vl_relabel(Cloud C, uint32_t N, uint32_t* __restrict__ id, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ before,
                                                    const int32_t* __restrict__ axis, const float* __restrict__ mid) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const uint32_t p = id[i];
  if (p == kNoPiece) return;
  uint32_t nw = p + before[p];
  if (flag[p] && C.rec(i)[axis[p]] > mid[p]) nw++;   // the first half keeps v <= mid, the negative filter v > mid
  id[i] = nw;
}

// the elements of the segmented pass: one row, element j = point j, segment = its piece
struct LargeElems {
  static constexpr int kFields = 16;
  Cloud C; int nfields; const uint32_t* id; float leaf_size; float* out; uint32_t* small;
  __device__ int fields() const { return nfields; }
  __device__ const float* fetch(uint32_t g, uint32_t) const { return C.rec(g); }
  __device__ bool slot(uint32_t, uint32_t j, uint32_t* g) const { *g = j; return true; }
  __device__ vg::Elem elem(uint32_t, uint32_t j) const {
    const float* p = C.rec(j);
    const uint32_t s = id[j];
    return vg::Elem{s != kNoPiece, s, j, make_float4(p[0], p[1], p[2], 0.f)};
  }
  __device__ float leaf(uint32_t) const { return leaf_size; }
  __device__ void overflow(uint32_t) const { small[2] = 1u; }   // cannot happen: a leaf piece passed the same test in vg::split
  __device__ void put(uint32_t cell, const float (&mean)[kFields]) const {
#pragma unroll
    for (int f = 0; f < kFields; f++)
      if (f < nfields) out[(size_t)cell * nfields + f] = mean[f];
  }
};

#define CHECK_CTX(c)                                                   \
  do {                                                                 \
    if (!(c)) return PCM_ERR_INVALID_ARGUMENT;                         \
    if ((c)->device < 0) return PCM_ERR_HIP;                           \
  } while (0)

// the text of a piece that cannot be cut: its extent and the axis
std::string stuck_text(const unsigned int* mm, float leaf, uint32_t piece, uint32_t depth) {
  int ax; float mid;
  (void)vg::split(mm, leaf, &ax, &mid);
  char buf[512];
  std::snprintf(buf, sizeof buf,
                "pcm_voxel_downsample_large: piece %u at depth %u overflows the leaf index but cannot be cut along %c: its extent is x [%.9g, %.9g] y [%.9g, %.9g] z [%.9g, %.9g], "
                "mid %.9g is not below the maximum (a flat axis chosen by the reference's tie rule, or adjacent floats)",
                piece, depth, ax >= 0 ? "xyz"[ax] : '?', (double)vg::ord2f(mm[0]), (double)vg::ord2f(mm[3]), (double)vg::ord2f(mm[1]), (double)vg::ord2f(mm[4]),
                (double)vg::ord2f(mm[2]), (double)vg::ord2f(mm[5]), (double)mid);
  return buf;
}

int run_large(pcm_ctx* c, const void* points, size_t n, size_t stride, int memory, float leaf, void* out, size_t capacity_points, pcm_voxel_large_result* r) {
  hipStream_t st = c->stream;
  const uint32_t N = (uint32_t)n;
  const int nfields = (int)(stride / 4);
  // per-point memory: the ids, and a copy of a host cloud.  Everything here goes when the call returns (hipFree waits).
  DevBuf<char> pts("VoxelGridLarge points"), tab("VoxelGridLarge piece tables"), work("VoxelGridLarge sort arrays"), cells("VoxelGridLarge cells");
  VlPoints L;
  auto layout = [&](ArenaStage& a) { L = vl_points_layout(a, n, memory, points, stride); };
  ArenaStage size = arena_stage(c, nullptr);
  layout(size);
  const size_t pts_bytes = size.used();
  int rc = pts.reserve(c, pts_bytes, pts_bytes);
  if (rc != PCM_OK) return rc;
  ArenaStage S = arena_stage(c, pts.p);
  layout(S);
  if (S.rc != PCM_OK) return S.rc;
  uint32_t* id = L.id;
  const Cloud C{static_cast<const char*>(L.cloud), stride};
  size_t cap = std::min<size_t>(4096, n), tab_bytes = 0;
  (void)tables_layout(nullptr, cap, &tab_bytes);
  if ((rc = tab.reserve(c, tab_bytes, tab_bytes)) != PCM_OK) return rc;
  Tables T = tables_layout(tab.p, cap, &tab_bytes);
  size_t peak_tab = tab_bytes;

  uint32_t P = 1, depth = 0, levels = 0, waits = 0;
  int b = 0;
  const unsigned nb_pts = (N + 255) / 256, nb_box = std::min<unsigned>(kBoxBlocks, nb_pts);
  for (;;) {
    if (std::min<size_t>(2 * (size_t)P, n) > cap) {   // the next level may have twice the pieces (never more than points)
      const size_t ncap = std::min<size_t>(4 * (size_t)P, n);
      size_t nbytes = 0;
      (void)tables_layout(nullptr, ncap, &nbytes);
      DevBuf<char> grown("VoxelGridLarge piece tables");
      if ((rc = grown.reserve(c, nbytes, nbytes)) != PCM_OK) return rc;
      const Tables G = tables_layout(grown.p, ncap, &nbytes);
      PCM_HIPCK(c, hipMemcpyAsync(G.mm[b], T.mm[b], 24 * (size_t)P, hipMemcpyDeviceToDevice, st));
      PCM_HIPCK(c, hipMemcpyAsync(G.fin[b], T.fin[b], 4 * (size_t)P, hipMemcpyDeviceToDevice, st));
      PCM_HIPCK(c, hipStreamSynchronize(st));
      waits++;
      tab.swap(grown);
      T = G; cap = ncap;
      peak_tab = std::max(peak_tab, nbytes);
    }
    const unsigned nb_p = (P + 255) / 256;
    if (levels == 0) {
      k_vl_first_box<<<nb_box, 256, 0, st>>>(C, N, id, T.part);
      vg::Work F{};
      F.mm = T.mm[b]; F.small = T.status + 4;
      vg::fold_boxes(st, T.part, nb_box, F);
      PCM_HIPCK(c, hipMemsetAsync(T.fin[b], 0, 4, st));
      k_vl_clear<<<1, 256, 0, st>>>(0u, T.fin[b], T.mm[b], T.status);   // the status words only
    } else {
      k_vl_clear<<<nb_p, 256, 0, st>>>(P, T.fin[b], T.mm[b], T.status);
      k_vl_box<<<nb_box, 256, 0, st>>>(C, N, id, T.fin[b], T.mm[b]);
    }
    k_vl_decide<<<nb_p, 256, 0, st>>>(P, leaf, depth < PCM_VOXEL_LARGE_MAX_DEPTH ? 1 : 0, T.mm[b], T.fin[b], T.flag, T.axis, T.mid, T.status);
    PCM_HIPCK(c, hipGetLastError());
    uint32_t status[3] = {0u, kNoPiece, kNoPiece};
    PCM_HIPCK(c, hipMemcpyAsync(status, T.status, sizeof status, hipMemcpyDeviceToHost, st));
    PCM_HIPCK(c, hipStreamSynchronize(st));
    waits++; levels++;
    if (status[1] != kNoPiece || status[2] != kNoPiece) {
      const uint32_t piece = std::min(status[1], status[2]);   // the first in depth-first order
      unsigned int mm[6];
      PCM_HIPCK(c, hipMemcpy(mm, T.mm[b] + 6 * (size_t)piece, sizeof mm, hipMemcpyDeviceToHost));
      if (piece == status[1]) c->err = stuck_text(mm, leaf, piece, depth);
      else {
        char buf[256];
        std::snprintf(buf, sizeof buf, "pcm_voxel_downsample_large: piece %u still overflows the leaf index after %d cuts (PCM_VOXEL_LARGE_MAX_DEPTH); x [%.9g, %.9g] y [%.9g, %.9g] z [%.9g, %.9g]",
                      piece, PCM_VOXEL_LARGE_MAX_DEPTH, (double)vg::ord2f(mm[0]), (double)vg::ord2f(mm[3]), (double)vg::ord2f(mm[1]), (double)vg::ord2f(mm[4]), (double)vg::ord2f(mm[2]),
                      (double)vg::ord2f(mm[5]));
        c->err = buf;
      }
      r->depth = depth; r->levels = levels; r->host_waits = waits;
      return PCM_ERR_OUT_OF_RANGE;
    }
    const uint32_t cuts = status[0];
    if (cuts == 0) break;
    size_t tb = T.tmp_bytes;
    PCM_HIPCK(c, rocprim::exclusive_scan(T.tmp, tb, T.flag, T.before, 0u, (size_t)P, rocprim::plus<uint32_t>(), st));
    k_vl_renumber<<<nb_p, 256, 0, st>>>(P, T.flag, T.before, T.mm[b], T.fin[1 - b], T.mm[1 - b]);
    k_vl_relabel<<<nb_pts, 256, 0, st>>>(C, N, id, T.flag, T.before, T.axis, T.mid);
    PCM_HIPCK(c, hipGetLastError());
    P += cuts; depth++; b ^= 1;
  }

  // the VoxelGrid of every piece: segment = piece, the boxes the levels left
  size_t work_bytes = 0;
  (void)vg::work_layout(nullptr, n, sizeof(uint64_t), P, &work_bytes);
  if ((rc = work.reserve(c, work_bytes, work_bytes)) != PCM_OK) return rc;
  vg::Work W = vg::work_layout(work.p, n, sizeof(uint64_t), P, &work_bytes);
  vg::clear(st, W);
  W.mm = T.mm[b];
  LargeElems E{C, nfields, id, leaf, nullptr, W.small};
  if ((rc = vg::seg_sort(&c->err, st, E, 1u, N, N, W)) != PCM_OK) return rc;
  uint32_t totals[3] = {0u, 0u, 0u};   // cells, finite points, index overflow
  PCM_HIPCK(c, hipMemcpyAsync(totals, W.small, sizeof totals, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipStreamSynchronize(st));
  waits++;
  r->cells = totals[0]; r->finite_points = totals[1]; r->pieces = totals[1] ? P : 0;
  r->depth = depth; r->levels = levels; r->host_waits = waits;
  r->workspace_bytes = pts_bytes + peak_tab + work_bytes;
  if (totals[2]) { c->err = "pcm_voxel_downsample_large: a leaf piece overflows the leaf index"; return PCM_ERR_INTERNAL; }
  const size_t m = totals[0];
  if (capacity_points < m) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "pcm_voxel_downsample_large: the output buffer holds %zu records, the result has %zu", capacity_points, m);
    c->err = buf;
    return PCM_ERR_INVALID_ARGUMENT;
  }
  if (m == 0) return PCM_OK;
  ArenaStage cells_size = arena_stage(c, nullptr);   // the cells of a host call: a staged output in a block of its own
  (void)cells_size.out(memory, out, m * stride);
  if (cells_size.used() && (rc = cells.reserve(c, m * stride, m * stride)) != PCM_OK) return rc;
  r->workspace_bytes += cells_size.used();
  E.out = static_cast<float*>(arena_stage(c, cells.p).out(memory, out, m * stride));
  if ((rc = vg::seg_average(&c->err, st, E, N, W)) != PCM_OK) return rc;
  if ((rc = stage_back(c, memory, out, E.out, m * stride)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(st));   // the workspace is released on return
  r->host_waits = ++waits;
  return PCM_OK;
}

}  // namespace

}  // namespace pcm

using namespace pcm;

extern "C" {

// pcl::VoxelGridLarge::filter (jueying_slam/include/voxel_grid_large.cpp:23-255)
int pcm_voxel_downsample_large(pcm_ctx* c, const void* points, size_t n, size_t stride, int memory, float leaf, void* out, size_t capacity_points,
                               pcm_voxel_large_result* result) {
  CHECK_CTX(c);
  if (!result) { c->err = "pcm_voxel_downsample_large: result is null"; return PCM_ERR_INVALID_ARGUMENT; }
  *result = pcm_voxel_large_result{};
  if ((!points && n) || (!out && capacity_points)) { c->err = "pcm_voxel_downsample_large: null buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  if (stride < 12 || stride > 64 || (stride % 4) != 0) { c->err = "records must be 3..16 floats"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(leaf > 0.f)) { c->err = "leaf size must be > 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (n > 0x7fffffffull) { c->err = "pcm_voxel_downsample_large: more than 2^31 - 1 points"; return PCM_ERR_OUT_OF_RANGE; }
  if (n == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  pcm_voxel_large_result r{};
  const int rc = run_large(c, points, n, stride, memory, leaf, out, capacity_points, &r);
  *result = r;
  return rc;
}

}  // extern "C"
