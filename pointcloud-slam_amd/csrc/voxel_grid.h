// voxel_grid.h -- pcl::VoxelGrid (pcl/filters/impl/voxel_grid.hpp), stated once for every down-sampler of the library:
// cell = floor(p * inverse_leaf_size) - min_b, linear index ijk . (1, dx, dx dy), one centroid per occupied cell in increasing
// index order, every float field averaged.  PCL sorts (index, point) pairs with std::sort and sums in float; here: a stable radix
// sort, one wave per cell, double sums (64 interleaved partial sums + a fixed tree), so a result does not depend on the schedule.
//
// The box, the cell index and the layout of a Work compile for the host as well -- with a host compiler alone (tests/voxel_grid_hooks.cpp), no HIP
// header is read then.  Everything else is device code and the launchers of the two pipelines of voxel_grid.hip:
//   single segment, 32-bit keys:  clear | fold_boxes, [single_minmax], single_cells  -> {cells, valid elements, overflow}, no wait
//   segmented, 64-bit keys:       clear, [seg_minmax], seg_cells                     -> the same, and cells per segment
// vg::split is pcl::VoxelGridLarge's decision for a piece whose index overflows (voxel_grid_large.hip cuts the cloud with it and runs
// the segmented pipeline with segment = piece); it compiles for the host as well (tests/voxel_grid_large_hooks.cpp).
// A caller hands its elements over as a functor (Elems below): where a point lives, whether it counts, which segment and leaf
// it has, where a cell's mean goes.  Both pipelines run on a Work, which work_layout sizes and places in memory the caller owns.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "arena_carver.h"

#if defined(__HIPCC__)
#include <algorithm>

#include "dev_buf.h"
#include "pcm_device.h"
#define PCM_VG_HD __host__ __device__
#else
#define PCM_VG_HD
#endif

namespace pcm {
namespace vg {

// inverse of pcm_device.h's f2ord, branch-free (the select form crashes this compiler's instruction selection when followed by
// float arithmetic)
PCM_VG_HD inline float ord2f(unsigned int o) {
  const unsigned int m = (unsigned int)((int)o >> 31), u = o ^ (~m | 0x80000000u);
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// the box of pcl::VoxelGrid from a segment's min / max (mm: 6 ordered-int words, min then max): b = {min_b x, y, z, divb_mul[1],
// divb_mul[2], state} (state 0: empty or no leaf, 1: index overflow, 2: valid).  The products are formed in double: exact, as a
// valid box has fewer than 2^31 cells, and no extent overflows them.  Returns whether the index overflows.
PCM_VG_HD inline bool box(const unsigned int* __restrict__ mm, float leaf, long long* __restrict__ b) {
  b[5] = 0;
  if (mm[0] == 0xffffffffu) return false;   // empty segment
  if (!(leaf > 0.f)) return false;
  const float inv = 1.0f / leaf;
  float mn[3], mx[3];
  for (int a = 0; a < 3; a++) { mn[a] = ord2f(mm[a]); mx[a] = ord2f(mm[3 + a]); }
  double cells = 1.0;
  for (int a = 0; a < 3; a++) cells *= ::trunc((double)((mx[a] - mn[a]) * inv)) + 1.0;   // int64_t((max - min) * inv) + 1, max >= min
  const bool over = cells > 2147483647.0;
  int mb[3], xb[3];
  for (int a = 0; a < 3; a++) { mb[a] = (int)::floorf(mn[a] * inv); xb[a] = (int)::floorf(mx[a] * inv); }
  const double div0 = (double)xb[0] - (double)mb[0] + 1.0, div1 = (double)xb[1] - (double)mb[1] + 1.0;
  b[0] = mb[0]; b[1] = mb[1]; b[2] = mb[2];
  b[3] = over ? 0 : (long long)div0;
  b[4] = over ? 0 : (long long)(div0 * div1);
  b[5] = over ? 1 : 2;
  return over;
}

// linear leaf index of a point in a valid box
PCM_VG_HD inline uint64_t cell(float x, float y, float z, float leaf, const long long* __restrict__ b) {
  const float inv = 1.0f / leaf;
  const int mb0 = (int)b[0], mb1 = (int)b[1], mb2 = (int)b[2];
  const long long i0 = (long long)(::floorf(x * inv) - (float)mb0), i1 = (long long)(::floorf(y * inv) - (float)mb1),
                  i2 = (long long)(::floorf(z * inv) - (float)mb2);
  return (uint64_t)(i0 + i1 * b[3] + i2 * b[4]);
}

// pcl::VoxelGridLarge::applyFilter's decision for a piece from its min / max (mm as for box()): a piece whose index does not
// overflow -- box()'s own test -- is a leaf piece, as is an empty one; any other is cut at *mid along *axis, x where dx is
// strictly the largest, else y where dy is, else z (ties go to z, the reference's rule).  mid = min + (max - min) / 2 in float:
// the first piece keeps v <= mid, the second v > mid.  A cut with mid >= max would leave the piece whole (a degenerate axis
// chosen by the tie rule, adjacent floats, an extent that overflows float): kPieceStuck, where the reference recurses for ever.
enum { kPieceLeaf = 0, kPieceSplit = 1, kPieceStuck = 2 };
PCM_VG_HD inline int split(const unsigned int* __restrict__ mm, float leaf, int* __restrict__ axis, float* __restrict__ mid) {
  *axis = -1; *mid = 0.f;
  if (mm[0] == 0xffffffffu || !(leaf > 0.f)) return kPieceLeaf;
  const float inv = 1.0f / leaf;
  float mn[3], mx[3];
  double d[3];
  for (int a = 0; a < 3; a++) { mn[a] = ord2f(mm[a]); mx[a] = ord2f(mm[3 + a]); d[a] = ::trunc((double)((mx[a] - mn[a]) * inv)) + 1.0; }
  if (!(d[0] * d[1] * d[2] > 2147483647.0)) return kPieceLeaf;
  const int ax = (d[0] > d[1] && d[0] > d[2]) ? 0 : (d[1] > d[0] && d[1] > d[2]) ? 1 : 2;
  const float m = mn[ax] + (mx[ax] - mn[ax]) / 2;
  *axis = ax; *mid = m;
  return m < mx[ax] ? kPieceSplit : kPieceStuck;
}

// The arrays of one pass over N elements with keys of key_bytes (4: single segment; 8: (segment << 32 | cell), nseg segments).
struct Work {
  void* keys; void* keys_s;          // [N]
  uint32_t* vals; uint32_t* vals_s;  // [N]; after the sort stage vals holds the first sorted element of every cell
  uint32_t* slot;                    // [N]
  uint32_t* head;                    // [N], segmented
  unsigned int* mm;                  // [max(nseg, 1)][6] ordered-int boxes, min then max
  long long* box;                    // [nseg][6], segmented (the single pass derives its box inside the key kernel)
  uint32_t* small;                   // [0] cells, [1] valid elements, [2] index overflow (single pass), [3] free;
  uint32_t nseg;                     //   segmented: then [nseg] cells per segment, [nseg] first cell of the segment
  void* tmp; size_t tmp_bytes; void* tmp2; size_t tmp2_bytes;   // rocPRIM temporaries: sort, scan
  uint32_t* scnt() const { return small + kSmallWords; }
  uint32_t* sfirst() const { return small + kSmallWords + nseg; }
  static constexpr int kSmallWords = 4;
};
// the Work of N elements carved from `a`; nseg == 0: the single pass.  sort_tmp_bytes, scan_tmp_bytes: rocPRIM's sizes (work_layout asks)
inline Work work_carve(ArenaCarver& a, size_t N, size_t key_bytes, size_t nseg, size_t sort_tmp_bytes, size_t scan_tmp_bytes) {
  Work W{};
  W.keys = a.take<char>(key_bytes * N); W.keys_s = a.take<char>(key_bytes * N);
  W.vals = a.take<uint32_t>(N); W.vals_s = a.take<uint32_t>(N);
  W.slot = a.take<uint32_t>(N);
  W.head = a.take<uint32_t>(nseg ? N : 0);
  W.mm = a.take<unsigned int>(6 * (nseg ? nseg : 1));
  W.box = a.take<long long>(6 * nseg);
  W.small = a.take<uint32_t>(Work::kSmallWords + 2 * nseg);
  W.nseg = (uint32_t)nseg;
  W.tmp_bytes = sort_tmp_bytes; W.tmp2_bytes = scan_tmp_bytes;
  W.tmp = a.take<char>(sort_tmp_bytes); W.tmp2 = a.take<char>(scan_tmp_bytes);
  return W;
}

#if defined(__HIPCC__)
constexpr uint32_t kInvalid32 = 0x80000000u;   // 32-bit key of an element without a cell (a valid box has fewer than 2^31 cells)

// The Work of N elements at `base` (256-byte aligned; null: sizes only), *bytes = what it occupies.  nseg == 0: the single pass.
// A pass may run on fewer elements and segments than its Work was laid out for (set nseg to the pass's).
Work work_layout(char* base, size_t N, size_t key_bytes, size_t nseg, size_t* bytes);
// empty boxes and zero counts
void clear(hipStream_t st, const Work& W);
// the single pass's clear when the box comes as n_part partial boxes (6 ordered words each) instead of atomics
void fold_boxes(hipStream_t st, const unsigned int* part, uint32_t n_part, const Work& W);
// the middle of a pass: keys -> sorted keys, the start of every cell in W.vals, the totals in W.small.  32: the heads are scanned
// on the fly and nothing per segment exists; 64: heads stored, cells per segment and first cells counted.
int sort_cells32(std::string* err, hipStream_t st, const Work& W, uint32_t N);
int sort_cells64(std::string* err, hipStream_t st, const Work& W, uint32_t N);

// 64-lane butterfly reductions (every lane ends with the result); the double sum in the same fixed order is wave_sum
// (pcm_device.h).  linearize_common.h's DPP reductions are another order and stay apart.
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

// a lane's point into the bounding box of its segment (mm: 6 ordered-int words per segment, min then max)
__device__ inline void wave_minmax(bool valid, uint32_t seg, const float4& pt, unsigned int* __restrict__ mm) {
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

// the box of a workgroup of 256 lanes from its lanes' boxes (ordered words), into out[0..6): a butterfly per wave, then the four
// waves through LDS; lanes 0..5 store.  No atomics: what fold_boxes reads.
__device__ __forceinline__ void fold_block_box(unsigned int lo[3], unsigned int hi[3], unsigned int* __restrict__ out) {
  __shared__ unsigned int wave_box[4][6];
  for (int a = 0; a < 3; a++) { lo[a] = wave_min_u32(lo[a]); hi[a] = wave_max_u32(hi[a]); }
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; a++) { wave_box[threadIdx.x >> 6][a] = lo[a]; wave_box[threadIdx.x >> 6][3 + a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    const uint32_t a = threadIdx.x;
    unsigned int v = wave_box[0][a];
    for (int w = 1; w < 4; w++) v = a < 3 ? min(v, wave_box[w][a]) : max(v, wave_box[w][a]);
    out[a] = v;
  }
}

// What a pass reads its elements through, and writes its cells through: a functor of the caller's with
//   static constexpr int kFields;  int fields() const      float fields of an element: room for, in use
//   fetch(g, seg)                                          element g (of segment seg): a float4, or a pointer to its fields
//   void put(cell, const float (&mean)[kFields]) const     a cell's mean
// the single pass also asks
//   bool point(g, float4* pt) const                        element g's position; false: the element does not count
// and the segmented pass, whose elements lie in `rows` rows (blockIdx.y) of up to per_row slots,
//   bool slot(row, j, uint32_t* g) const                   false: no element at (row, j); else g = its index in [0, N)
//   Elem elem(row, j) const                                valid, segment, order within the segment (the key without a leaf), position
//   float leaf(seg) const;  void overflow(seg) const       the segment's leaf (<= 0: one cell per element, in order); its index overflows
struct Elem { bool valid; uint32_t seg, ord; float4 pt; };

__device__ inline void add_fields(double* __restrict__ acc, int, const float4& q) {
  acc[0] += (double)q.x; acc[1] += (double)q.y; acc[2] += (double)q.z; acc[3] += (double)q.w;
}
__device__ inline void add_fields(double* __restrict__ acc, int nfields, const float* __restrict__ p) {
  for (int f = 0; f < nfields; f++) acc[f] += (double)p[f];
}

// The mean of the cell whose run is [b, e) of the sorted order, by one wave: lane l sums elements l, l + 64, ... in double, a fixed
// butterfly adds the 64 partial sums (deterministic; a dense leaf near the sensor holds thousands of points, which one lane
// alone would walk serially), then the division by the run length and the cast.  Every lane ends with the mean.
template <class Elems>
__device__ inline void cell_mean(const Elems& E, uint32_t seg, const uint32_t* __restrict__ vals_s, uint32_t b, uint32_t e, uint32_t lane, float (&mean)[Elems::kFields]) {
  double acc[Elems::kFields];
  for (int f = 0; f < Elems::kFields; f++) acc[f] = 0.0;
  const int nfields = E.fields();
  for (uint32_t j = b + lane; j < e; j += 64) add_fields(acc, nfields, E.fetch(vals_s[j], seg));
  const double m = (double)(e - b);
#pragma unroll
  for (int f = 0; f < Elems::kFields; f++)
    if (f < nfields) mean[f] = (float)(wave_sum(acc[f]) / m);
}

// one wave per cell (grid-stride) of either pipeline; the totals are read on the device
template <class Key, class Elems>
__global__ void __launch_bounds__(256) k_average(Elems E, const Key* __restrict__ keys_s, const uint32_t* __restrict__ vals_s, const uint32_t* __restrict__ pos,
                                                 const uint32_t* __restrict__ small) {
  const uint32_t ncells = small[0], nvalid = small[1];
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t cell = blockIdx.x * 4 + (threadIdx.x >> 6); cell < ncells; cell += gridDim.x * 4) {
    const uint32_t b = pos[cell], e = cell + 1 < ncells ? pos[cell + 1] : nvalid;
    const uint32_t seg = sizeof(Key) == 8 ? (uint32_t)((uint64_t)keys_s[b] >> 32) : 0u;
    float mean[Elems::kFields];
    cell_mean(E, seg, vals_s, b, e, lane, mean);
    if (lane == 0) E.put(cell, mean);
  }
}

// ---- single segment, 32-bit keys --------------------------------------------------------------------------------------------
template <class Elems>
__global__ void __launch_bounds__(256) k_single_minmax(Elems E, uint32_t N, unsigned int* __restrict__ mm) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  float4 pt = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool valid = g < N && E.point(g, &pt);
  wave_minmax(valid, 0u, pt, mm);
}

// every workgroup derives the box from the finished min / max (a few dozen operations of one lane)
template <class Elems>
__global__ void __launch_bounds__(256) k_single_keys(Elems E, uint32_t N, float leaf, const unsigned int* __restrict__ mm, uint32_t* __restrict__ keys,
                                                     uint32_t* __restrict__ vals, uint32_t* __restrict__ small) {
  __shared__ long long b[6];
  if (threadIdx.x == 0) {
    const bool over = box(mm, leaf, b);
    if (over && blockIdx.x == 0) small[2] = 1u;
  }
  __syncthreads();
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= N) return;
  float4 pt;
  keys[g] = (b[5] == 2 && E.point(g, &pt)) ? (uint32_t)cell(pt.x, pt.y, pt.z, leaf, b) : kInvalid32;
  vals[g] = g;
}

// the box by atomics, one per wave (a caller whose producer kernel sees every point calls wave_minmax there instead)
template <class Elems> void single_minmax(hipStream_t st, const Elems& E, uint32_t N, const Work& W) {
  k_single_minmax<<<(N + 255) / 256, 256, 0, st>>>(E, N, W.mm);
}

// keys from the finished box, sort, cell starts and totals, means; queues and does not wait
template <class Elems> int single_cells(std::string* err, hipStream_t st, const Elems& E, uint32_t N, float leaf, const Work& W) {
  k_single_keys<<<(N + 255) / 256, 256, 0, st>>>(E, N, leaf, W.mm, static_cast<uint32_t*>(W.keys), W.vals, W.small);
  PCM_HIPCK_ERR(err, hipGetLastError());
  const int rc = sort_cells32(err, st, W, N);
  if (rc != PCM_OK) return rc;
  k_average<uint32_t><<<std::min<unsigned>(1024u, (N + 3) / 4), 256, 0, st>>>(E, static_cast<const uint32_t*>(W.keys_s), W.vals_s, W.vals, W.small);
  PCM_HIPCK_ERR(err, hipGetLastError());
  return PCM_OK;
}

// ---- segmented, 64-bit keys ---------------------------------------------------------------------------------------------------
template <class Elems>
__global__ void k_seg_minmax(Elems E, uint32_t per_row, unsigned int* __restrict__ mm) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const Elem e = j < per_row ? E.elem(blockIdx.y, j) : Elem{false, 0u, 0u, make_float4(0.f, 0.f, 0.f, 0.f)};
  wave_minmax(e.valid, e.seg, e.pt, mm);
}

template <class Elems>
__global__ void k_seg_boxes(Elems E, const unsigned int* __restrict__ mm, uint32_t nseg, long long* __restrict__ boxes) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  if (box(mm + 6 * (size_t)s, E.leaf(s), boxes + 6 * (size_t)s)) E.overflow(s);
}

template <class Elems>
__global__ void k_seg_keys(Elems E, uint32_t per_row, const long long* __restrict__ boxes, uint32_t nseg, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t g;
  if (j >= per_row || !E.slot(blockIdx.y, j, &g)) return;
  const Elem e = E.elem(blockIdx.y, j);
  uint64_t key = (uint64_t)nseg << 32;   // invalid: behind every segment
  if (e.valid) {
    const float leaf = E.leaf(e.seg);
    const long long* b = boxes + 6 * (size_t)e.seg;
    if (!(leaf > 0.f)) key = ((uint64_t)e.seg << 32) | e.ord;   // no down-sampling: one cell per element, in order
    else if (b[5] == 2) key = ((uint64_t)e.seg << 32) | cell(e.pt.x, e.pt.y, e.pt.z, leaf, b);
  }
  keys[g] = key;
  vals[g] = g;
}

template <class Elems> void seg_minmax(hipStream_t st, const Elems& E, uint32_t rows, uint32_t per_row, const Work& W) {
  k_seg_minmax<<<dim3((per_row + 255) / 256, rows), 256, 0, st>>>(E, per_row, W.mm);
}

// the two halves of seg_cells, for a caller that has to see the totals before a mean is written: boxes and keys from the
// finished min / max, one sort for all segments, cell starts and counts ...
template <class Elems> int seg_sort(std::string* err, hipStream_t st, const Elems& E, uint32_t rows, uint32_t per_row, uint32_t N, const Work& W) {
  k_seg_boxes<<<(W.nseg + 255) / 256, 256, 0, st>>>(E, W.mm, W.nseg, W.box);
  k_seg_keys<<<dim3((per_row + 255) / 256, rows), 256, 0, st>>>(E, per_row, W.box, W.nseg, static_cast<uint64_t*>(W.keys), W.vals);
  PCM_HIPCK_ERR(err, hipGetLastError());
  return sort_cells64(err, st, W, N);
}
// ... and the means
template <class Elems> int seg_average(std::string* err, hipStream_t st, const Elems& E, uint32_t N, const Work& W) {
  k_average<uint64_t><<<std::min<unsigned>(1024u, (N + 3) / 4), 256, 0, st>>>(E, static_cast<const uint64_t*>(W.keys_s), W.vals_s, W.vals, W.small);
  PCM_HIPCK_ERR(err, hipGetLastError());
  return PCM_OK;
}

// boxes and keys from the finished min / max, one sort for all segments, cell starts and counts, means; queues and does not wait
template <class Elems> int seg_cells(std::string* err, hipStream_t st, const Elems& E, uint32_t rows, uint32_t per_row, uint32_t N, const Work& W) {
  const int rc = seg_sort(err, st, E, rows, per_row, N, W);
  return rc != PCM_OK ? rc : seg_average(err, st, E, N, W);
}
#endif   // __HIPCC__

}  // namespace vg
}  // namespace pcm
