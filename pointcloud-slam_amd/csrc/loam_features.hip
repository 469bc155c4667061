// loam_features.hip -- the LOAM front end on the device: jueying_slam's imageProjection (projectPointCloud, cloudExtraction),
// featureExtraction (calculateSmoothness, markOccludedPoints, extractFeatures with its per-ring VoxelGrid) and the two mapping
// VoxelGrids of downsampleCurrentScan, from one ring-tagged scan to the LOAM source of a PCM_MODEL_LOAM context
// (include/pcm_amd.h, pcm_loam_extract_features / pcm_loam_frame_begin[_batch]).
//
// Reference: jueying_slam/src/imageProjection.cpp:736-823, featureExtraction.cpp:84-247,
// mapOptmization.cpp:1232-1247.  Deskew (imageProjection.cpp:704-733) is the identity as written (relative point time compared
// against absolute IMU / odometry stamps, :535/:548/:624/:632/:777): no IMU input, the timestamp field is never read.
// The *_deskew entry points run the live form instead (new_localization.cpp:1948-1977, loam_deskew.h):
// the <true> instantiations of k_lf_clear / k_lf_project / k_lf_extract and k_lf_dk_start between the last two.
//
// Launches of one batch (grid.y = frame), all on the stream of the first context, one read-back at the end:
//   k_lf_clear, k_lf_project (atomicMin cell owner = first point wins), k_lf_rowcount, k_lf_rings (ring prefix, start/end),
//   k_lf_extract (pointColInd, pointRange, extracted cloud), k_lf_smooth, k_lf_occlude, k_lf_snapshot (marks for the hook),
//   k_lf_select<first ring> then k_lf_select<other rings> (sort, invariance check / serial std::sort, greedy passes),
//   k_lf_corner_compact, segmented VoxelGrid stage 1 (per ring, odometry leaf), stage 2 (corner / surf, mapping leaves), k_lf_finish.
#include "host_util.h"
#include "intro_sort.h"
#include "loam_deskew.h"
#include "loam_device.h"
#include "pre_layouts.h"
#include "voxel_grid.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace pcm;

namespace {

constexpr int kMaxPicks = 20;   // largestPickedNum <= 20 (featureExtraction.cpp:177)

// per-frame counters, read back once per batch
struct LfInfo {
  uint32_t count;          // extracted points
  int32_t first_ring;      // first ring with points (-1: none)
  uint32_t n_corner_scan;  // cornerCloud
  uint32_t n_surf_scan;    // surfaceCloud (rings concatenated after the odometry VoxelGrid)
  uint32_t n_corner;       // after the mapping VoxelGrids
  uint32_t n_surf;
  uint32_t sectors, sectors_serial;
  uint32_t overflow;       // a VoxelGrid index overflowed
  uint32_t bad_sector;     // a sector was larger than the sort buffer (library bug)
  uint32_t first1;         // first stage-1 cell of the frame
  uint32_t first2;         // first stage-2 cell of the frame
};

// deskew of one frame (pcm_loam_deskew on the device); enabled == 0: the frame's points stay as they are
struct LfDeskew {
  loam::DeskewTable imu, odo;   // odo.n == 0: no odometry table
  double time_scan_cur;
  uint32_t toff;           // offset of the time field in a record
  int32_t tkind;           // PCM_LOAM_TIME_*
  int32_t enabled;
  uint32_t* first;         // smallest record index that passed the ring, column and range tests (0xffffffff: none)
  float* start_inv;        // transStartInverse, 12 floats
};

struct LfFrame {
  const char* pts;         // input records (device)
  uint32_t n, stride, ioff, roff;
  uint32_t cap1;           // min(n, n_scan * horizon_scan): extracted-point bound
  uint32_t base1, base2;   // offsets of the frame's elements in the stage-1 / stage-2 arrays
  // context state (persists between frames)
  int32_t* col_ind; float* range; float4* cloud; float* curv; int32_t* picked; int32_t* label; DistId* smooth;
  // last-frame outputs of the context (parity hook)
  int32_t* start; int32_t* end; int32_t* picked_occ; float4* corner_scan; float4* surf_scan; float4* out;
  float4* src;             // pcm_loam_frame_begin: the context's LOAM source (w = index), else nullptr
  // batch scratch
  uint32_t* owner; uint32_t* rowcnt; uint32_t* roff_arr; int32_t* member; int32_t* cpick; int32_t* ccnt;
  LfInfo* info;
  LfDeskew dk;
};

struct LfParams {
  int n_scan, H, rate, A;
  float min_range, max_range, edge, surf, ang_res_x;
  float leaf_odo, leaf_corner, leaf_surf;
  int force_serial;
  int ppr;                 // corner picks per ring = A * 20
  int P;                   // sort buffer entries (power of two >= the largest sector + 1)
};

__device__ inline uint32_t cap_of(const LfParams& p) { return (uint32_t)p.n_scan * (uint32_t)p.H; }

// ---------------------------------------------------------------------------------------------------------------------------
// projection (imageProjection.cpp:736-797)
// ---------------------------------------------------------------------------------------------------------------------------
template <bool kDeskew>
__global__ void k_lf_clear(const LfFrame* __restrict__ fr, LfParams p) {
  const LfFrame& F = fr[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap_of(p)) F.owner[i] = 0xffffffffu;
  if (i < (uint32_t)p.n_scan) { F.rowcnt[i] = 0u; F.ccnt[i] = 0; }
  if (kDeskew && i == 0 && F.dk.enabled) *F.dk.first = 0xffffffffu;
  if (i == 0) {
    LfInfo z;
    memset(&z, 0, sizeof(z));
    z.first_ring = -1;
    *F.info = z;
  }
}

struct Proj { int row, col; float range; };

// false: the point is skipped.  Keeps the C++ types and evaluation order of :753-776 (atan2f pinned to float(atan2(double, double)))
__device__ inline bool project_point(const LfFrame& F, const LfParams& p, uint32_t i, Proj* o, float4* pt) {
  const char* r = F.pts + (size_t)i * F.stride;
  const float x = *reinterpret_cast<const float*>(r), y = *reinterpret_cast<const float*>(r + 4), z = *reinterpret_cast<const float*>(r + 8);
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  const int row = (int)*reinterpret_cast<const uint16_t*>(r + F.roff);
  if (row < 0 || row >= p.n_scan) return false;
  if (row % p.rate != 0) return false;
  const float a = (float)atan2((double)x, (double)y);
  const float horizonAngle = (float)((double)(a * 180.0f) / M_PI);
  int col = (int)(-round(((double)horizonAngle - 90.0) / (double)p.ang_res_x) + (double)(p.H / 2));
  if (col >= p.H) col -= p.H;
  if (col < 0 || col >= p.H) return false;
  const float range = sqrtf((x * x + y * y) + z * z);
  if (range < p.min_range || range > p.max_range) return false;
  o->row = row; o->col = col; o->range = range;
  if (pt) *pt = make_float4(x, y, z, (float)*reinterpret_cast<const uint8_t*>(r + F.ioff));
  return true;
}

// kDeskew: the smallest passing record index of the frame as well (one atomicMin per wave).  It owns its cell, so it is the first
// point that reaches deskewPoint (firstPointFlag, new_localization.cpp:1961-1965).
template <bool kDeskew>
__global__ void k_lf_project(const LfFrame* __restrict__ fr, LfParams p) {
  const LfFrame& F = fr[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  Proj q;
  const bool ok = i < F.n && project_point(F, p, i, &q, nullptr);
  if (ok) atomicMin(&F.owner[(uint32_t)q.row * (uint32_t)p.H + (uint32_t)q.col], i);   // rangeMat != FLT_MAX -> skip (:774): first point wins
  if constexpr (kDeskew) {
    if (!F.dk.enabled) return;   // the same in every lane of the block
    uint32_t m = ok ? i : 0xffffffffu;
    for (int off = 32; off >= 1; off >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0 && m != 0xffffffffu) atomicMin(F.dk.first, m);
  }
}

// pointTime = timeScanCur + (timestamp[i] - timestamp[0]) (imageProjection.cpp:777, new_localization.cpp:1953): the difference
// in the field's type, the sum in double.  Record 0 is the input's, whether or not it passes the tests.
__device__ inline double point_time(const LfFrame& F, uint32_t i) {
  const char* r0 = F.pts + F.dk.toff;
  const char* ri = r0 + (size_t)i * F.stride;
  const double rel = F.dk.tkind == PCM_LOAM_TIME_FLOAT ? (double)(*reinterpret_cast<const float*>(ri) - *reinterpret_cast<const float*>(r0))
                                                       : *reinterpret_cast<const double*>(ri) - *reinterpret_cast<const double*>(r0);
  return F.dk.time_scan_cur + rel;
}

// one lane per frame: transStartInverse from the first point
__global__ void __launch_bounds__(64) k_lf_dk_start(const LfFrame* __restrict__ fr) {
  const LfFrame& F = fr[blockIdx.x];
  if (threadIdx.x != 0 || !F.dk.enabled) return;
  const uint32_t first = *F.dk.first;
  if (first == 0xffffffffu) return;   // no point passed: nothing reads the transform
  const double t = point_time(F, first);
  float rot[3], pos[3], inv[12];
  loam::deskew_find(F.dk.imu, t, rot);
  loam::deskew_find(F.dk.odo, t, pos);
  loam::deskew_start(rot, pos, inv);
  for (int k = 0; k < 12; k++) F.dk.start_inv[k] = inv[k];
}

// one block of 256 per (row, frame): occupied cells of the row
__global__ void __launch_bounds__(256) k_lf_rowcount(const LfFrame* __restrict__ fr, LfParams p) {
  const LfFrame& F = fr[blockIdx.y];
  const uint32_t row = blockIdx.x;
  __shared__ uint32_t s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  uint32_t c = 0;
  for (int j = threadIdx.x; j < p.H; j += 256) c += F.owner[row * (uint32_t)p.H + j] != 0xffffffffu ? 1u : 0u;
  for (int off = 32; off >= 1; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) F.rowcnt[row] = s_cnt;
}

// one block of 256 per frame: ring prefix, startRingIndex / endRingIndex (cloudExtraction :803-821)
__global__ void __launch_bounds__(256) k_lf_rings(const LfFrame* __restrict__ fr, LfParams p) {
  const LfFrame& F = fr[blockIdx.x];
  __shared__ uint32_t s[256];
  const int r = threadIdx.x;
  const uint32_t v = r < p.n_scan ? F.rowcnt[r] : 0u;
  s[r] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {   // inclusive Hillis-Steele scan
    const uint32_t t = r >= off ? s[r - off] : 0u;
    __syncthreads();
    s[r] += t;
    __syncthreads();
  }
  if (r < p.n_scan) {
    const int before = (int)(s[r] - v), after = (int)s[r];
    F.roff_arr[r] = (uint32_t)before;
    F.start[r] = before - 1 + 5;
    F.end[r] = after - 1 - 5;
    if (r == p.n_scan - 1) {
      F.roff_arr[p.n_scan] = (uint32_t)after;
      F.info->count = (uint32_t)after;
    }
    if (v && (r == 0 || s[r - 1] == 0)) F.info->first_ring = r;
  }
}

// one block of 256 per (row, frame): the row's occupied cells in column order.  kDeskew: the stored point and its range are the
// deskewed point's (imageProjection.cpp:777-782); the column stays the raw point's.
template <bool kDeskew>
__global__ void __launch_bounds__(256) k_lf_extract(const LfFrame* __restrict__ fr, LfParams p) {
  const LfFrame& F = fr[blockIdx.y];
  const uint32_t row = blockIdx.x;
  if (F.rowcnt[row] == 0) return;
  const int per = (p.H + 255) / 256;   // <= 16 columns per thread
  const int j0 = threadIdx.x * per;
  uint32_t own = 0;
  for (int k = 0; k < per; k++) {
    const int j = j0 + k;
    if (j < p.H && F.owner[row * (uint32_t)p.H + j] != 0xffffffffu) own++;
  }
  __shared__ uint32_t s[256];
  s[threadIdx.x] = own;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const uint32_t t = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0u;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  uint32_t pos = F.roff_arr[row] + s[threadIdx.x] - own;
  for (int k = 0; k < per; k++) {
    const int j = j0 + k;
    if (j >= p.H) break;
    const uint32_t i = F.owner[row * (uint32_t)p.H + j];
    if (i == 0xffffffffu) continue;
    Proj q;
    float4 pt;
    project_point(F, p, i, &q, &pt);   // the owner passed every test in k_lf_project
    if constexpr (kDeskew) {
      if (F.dk.enabled) {
        const double t = point_time(F, i);
        float rot[3], tr[3], inv[12], d[3];
        loam::deskew_find(F.dk.imu, t, rot);
        loam::deskew_find(F.dk.odo, t, tr);
        for (int k = 0; k < 12; k++) inv[k] = F.dk.start_inv[k];
        loam::deskew_point(inv, rot, tr, pt.x, pt.y, pt.z, d);
        pt.x = d[0]; pt.y = d[1]; pt.z = d[2];
        q.range = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);   // pointDistance(thisPoint) :779
      }
    }
    F.col_ind[pos] = j;
    F.range[pos] = q.range;
    F.cloud[pos] = pt;
    pos++;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// calculateSmoothness (featureExtraction.cpp:84-105) and markOccludedPoints (:107-145)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void k_lf_smooth(const LfFrame* __restrict__ fr, LfParams p) {
  const LfFrame& F = fr[blockIdx.y];
  const int n = (int)F.info->count;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < 5 || i >= n - 5) return;
  const float* r = F.range;
  // strictly left to right, no contraction (-ffp-contract=off)
  float d = r[i - 5] + r[i - 4];
  d = d + r[i - 3];
  d = d + r[i - 2];
  d = d + r[i - 1];
  d = d - r[i] * 10.0f;
  d = d + r[i + 1];
  d = d + r[i + 2];
  d = d + r[i + 3];
  d = d + r[i + 4];
  d = d + r[i + 5];
  const float c = d * d;
  F.curv[i] = c;
  F.picked[i] = 0;
  F.label[i] = 0;
  F.smooth[i] = DistId{c, (uint32_t)i};
}

// every mark is a store of 1, so concurrent marks commute; they follow every reset (separate launch)
__global__ void k_lf_occlude(const LfFrame* __restrict__ fr, LfParams p) {
  const LfFrame& F = fr[blockIdx.y];
  const int n = (int)F.info->count;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < 5 || i >= n - 6) return;
  const float depth1 = F.range[i], depth2 = F.range[i + 1];
  const int columnDiff = abs(F.col_ind[i + 1] - F.col_ind[i]);
  if (columnDiff < 10) {
    if ((double)(depth1 - depth2) > 0.3) {
      for (int l = -5; l <= 0; l++) F.picked[i + l] = 1;
    } else if ((double)(depth2 - depth1) > 0.3) {
      for (int l = 1; l <= 6; l++) F.picked[i + l] = 1;
    }
  }
  const float ri = F.range[i];
  const float diff1 = fabsf(F.range[i - 1] - ri), diff2 = fabsf(F.range[i + 1] - ri);
  if ((double)diff1 > 0.02 * (double)ri && (double)diff2 > 0.02 * (double)ri) F.picked[i] = 1;
}

__global__ void k_lf_snapshot(const LfFrame* __restrict__ fr, LfParams p) {
  const LfFrame& F = fr[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F.info->count) F.picked_occ[i] = F.picked[i];
}

// ---------------------------------------------------------------------------------------------------------------------------
// extractFeatures (:147-247): one wave per (ring, frame).  The ring's pointColInd, cloudNeighborPicked and cloudLabel with a +-5
// halo live in LDS; any other position (only the stale slot 4 of the first ring can name one) is read and written in global
// memory, which is why the first ring runs in a launch of its own before the others.
// ---------------------------------------------------------------------------------------------------------------------------
struct Ring {
  int wlo, whi, cap;
  int16_t* col; uint8_t* pick; int8_t* lab;
  const LfFrame* F;
  __device__ bool in(int i) const { return i >= wlo && i < whi; }
  // outside [0, cap) the reference reads beyond its vectors (only the initial stale entry {0, 0} can get there): a column jump
  __device__ int col_at(int i) const { return in(i) ? (int)col[i - wlo] : (i < 0 || i >= cap) ? -100000 : F->col_ind[i]; }
  __device__ int pick_at(int i) const { return in(i) ? (int)pick[i - wlo] : F->picked[i]; }
  __device__ int lab_at(int i) const { return in(i) ? (int)lab[i - wlo] : F->label[i]; }
  // every lane of the wave stores the same value (each then reads its own store back: no cross-lane ordering needed)
  __device__ void set_pick(int i) const { if (in(i)) pick[i - wlo] = 1; else F->picked[i] = 1; }
  __device__ void set_lab(int i, int v) const { if (in(i)) lab[i - wlo] = (int8_t)v; else F->label[i] = v; }
  __device__ void suppress(int ind) const {   // :186-201 / :213-230
    for (int l = 1; l <= 5; l++) {
      if (abs(col_at(ind + l) - col_at(ind + l - 1)) > 10) break;
      set_pick(ind + l);
    }
    for (int l = -1; l >= -5; l--) {
      if (abs(col_at(ind + l) - col_at(ind + l + 1)) > 10) break;
      set_pick(ind + l);
    }
  }
};

// one greedy pass over the visit order (corner: ent[S], ent[S-1], ..., ent[0]; surf: ent[0], ..., ent[S]) by ballot: the first
// eligible lane of a 64-entry window is taken, its marks are made, the lanes behind it are evaluated again
template <bool kCorner>
__device__ void greedy_pass(const Ring& R, const DistId* ent, int S, float thr, int32_t* cpick, int* ccount) {
  const int lane = threadIdx.x;
  int picks = 0;
  for (int base = 0; base <= S; base += 64) {
    const int v = base + lane;
    int ind = 0;
    bool cand = false;
    if (v <= S) {
      ind = (int)ent[kCorner ? S - v : v].id;
      const float c = R.F->curv[ind];
      cand = kCorner ? (c > thr) : (c < thr);
    }
    for (;;) {
      const bool elig = cand && R.pick_at(ind) == 0;
      const uint64_t m = __ballot(elig);
      if (m == 0) break;
      const int l = __ffsll((unsigned long long)m) - 1;
      const int pind = __shfl(ind, l, 64);
      if (kCorner) {
        if (++picks > kMaxPicks) return;   // the 21st eligible candidate breaks the loop before it is marked (:178-183)
        R.set_lab(pind, 1);
        if (lane == 0) cpick[*ccount] = pind;
        ++*ccount;
      } else {
        R.set_lab(pind, -1);
      }
      R.set_pick(pind);
      R.suppress(pind);
      cand = cand && lane > l;
    }
  }
}

// the bitonic order of (value, position) equals std::sort's order as far as the passes can tell
__device__ bool order_invariant(const Ring& R, const DistId* ent, int S, int sp, const LfParams& p) {
  bool bad = false;
  for (int t = threadIdx.x; t < S && !bad; t += 64) {
    const float v = ent[t].d;
    const int ia = (int)ent[t].id;
    const float ca = R.F->curv[ia];
    const bool cc = ca > p.edge, cs = ca < p.surf;
    if (!cc && !cs) continue;
    for (int u = t + 1; u < S && ent[u].d == v; u++) {
      if (u - t > 256) { bad = true; break; }   // very large tie group: serial
      const int ib = (int)ent[u].id;
      const float cb = R.F->curv[ib];
      if (cc && cb > p.edge) { bad = true; break; }   // two corner candidates in one tie group
      if (cs && cb < p.surf && abs(ia - ib) <= 5) { bad = true; break; }
    }
  }
  // std::sort leaves one of the minimum's ties in slot sp; slot 4 outlives the frame (the stale entry of the next one)
  if (sp == 4 && S >= 2 && ent[0].d == ent[1].d) bad = true;
  return __ballot(bad) == 0;
}

template <bool kFirst>
__global__ void __launch_bounds__(64) k_lf_select(const LfFrame* __restrict__ fr, LfParams p) {
  const LfFrame& F = fr[blockIdx.y];
  const int first = F.info->first_ring;
  if (first < 0) return;
  const int r = kFirst ? first : (int)blockIdx.x;
  if (!kFirst && r == first) return;
  const int c = (int)F.roff_arr[r], n = (int)F.roff_arr[r + 1] - c;
  if (n == 0) return;
  const int cap = p.n_scan * p.H;
  extern __shared__ char smem[];
  DistId* ent = reinterpret_cast<DistId*>(smem);
  uint64_t* key = reinterpret_cast<uint64_t*>(smem);   // the same bytes: keys first, entries after the sort
  const int W = p.H + 10;
  int16_t* s_col = reinterpret_cast<int16_t*>(smem + (size_t)p.P * 8);
  uint8_t* s_pick = reinterpret_cast<uint8_t*>(s_col + W);
  int8_t* s_lab = reinterpret_cast<int8_t*>(s_pick + W);
  Ring R;
  R.wlo = max(0, c - 5);
  R.whi = min(cap, c + n + 5);
  R.cap = cap;
  R.col = s_col; R.pick = s_pick; R.lab = s_lab; R.F = &F;
  const int lane = threadIdx.x;
  for (int k = lane; k < R.whi - R.wlo; k += 64) {
    s_col[k] = (int16_t)F.col_ind[R.wlo + k];
    s_pick[k] = (uint8_t)F.picked[R.wlo + k];
    s_lab[k] = (int8_t)F.label[R.wlo + k];
  }
  for (int k = c + lane; k < c + n; k += 64) F.member[k] = -1;
  __syncthreads();
  const int start = c - 1 + 5, end = c + n - 1 - 5, A = p.A;
  int32_t* cpick = F.cpick + (size_t)r * p.ppr;
  int ccount = 0, sectors = 0, serial = 0, bad_sector = 0;
  for (int j = 0; j < A; j++) {
    const int sp = (start * (A - j) + end * j) / A;            // C++ int division truncates toward zero
    const int ep = (start * (A - 1 - j) + end * (j + 1)) / A - 1;
    if (sp >= ep) continue;
    const int S = ep - sp;                                      // std::sort covers [sp, ep); the entry at ep stays
    if (S + 1 > p.P) { bad_sector = 1; continue; }
    sectors++;
    bool ok = false;
    if (!p.force_serial) {
      for (int t = lane; t < p.P; t += 64)
        key[t] = t < S ? (((uint64_t)__float_as_uint(F.smooth[sp + t].d) << 32) | (uint32_t)t) : ~0ull;   // curvatures are >= 0
      __syncthreads();
      int P2 = 1;
      while (P2 < S) P2 <<= 1;
      for (int k = 2; k <= P2; k <<= 1)
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
          for (int t = lane; t < P2; t += 64) {
            const int u = t ^ jj;
            if (u > t) {
              const uint64_t a = key[t], b = key[u];
              if ((a > b) == ((t & k) == 0)) { key[t] = b; key[u] = a; }
            }
          }
          __syncthreads();
        }
      // keys -> entries in place: slot t's key and entry share the same 8 bytes and one lane owns the slot
      for (int t = lane; t < S; t += 64) {
        const uint32_t pos = (uint32_t)(key[t] & 0xffffffffu);
        ent[t] = F.smooth[sp + pos];
      }
      if (lane == 0) ent[S] = F.smooth[ep];
      __syncthreads();
      ok = order_invariant(R, ent, S, sp, p);
    }
    if (!ok) {   // std::sort itself on the array order
      for (int t = lane; t <= S; t += 64) ent[t] = F.smooth[sp + t];
      __syncthreads();
      if (lane == 0) intro_sort_libstdcxx(ent, S);
      __syncthreads();
      serial++;
    }
    for (int t = lane; t < S; t += 64) F.smooth[sp + t] = ent[t];   // the sorted sector persists (slot 4 feeds the next frame)
    greedy_pass<true>(R, ent, S, p.edge, cpick, &ccount);
    greedy_pass<false>(R, ent, S, p.surf, nullptr, nullptr);
    for (int k = sp + lane; k <= ep; k += 64)                   // surfaceCloudScan (:234-240): labels -1 and 0
      if (R.lab_at(k) <= 0) F.member[k] = r;
    __syncthreads();
  }
  // write back: labels of the ring's own positions, marks (stores of 1 commute with the neighbouring rings' ones)
  for (int k = lane; k < R.whi - R.wlo; k += 64) {
    const int i = R.wlo + k;
    if (i >= c && i < c + n) F.label[i] = s_lab[k];
    if (s_pick[k]) F.picked[i] = 1;
  }
  if (lane == 0) {
    F.ccnt[r] = ccount;
    atomicAdd(&F.info->sectors, (uint32_t)sectors);
    atomicAdd(&F.info->sectors_serial, (uint32_t)serial);
    if (bad_sector) F.info->bad_sector = 1u;
  }
}

// cornerCloud in pick order: rings concatenated (one block of 256 per frame)
__global__ void __launch_bounds__(256) k_lf_corner_compact(const LfFrame* __restrict__ fr, LfParams p) {
  const LfFrame& F = fr[blockIdx.x];
  __shared__ uint32_t s[256];
  const int r = threadIdx.x;
  const uint32_t v = r < p.n_scan ? (uint32_t)F.ccnt[r] : 0u;
  s[r] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const uint32_t t = r >= off ? s[r - off] : 0u;
    __syncthreads();
    s[r] += t;
    __syncthreads();
  }
  if (r == 255) F.info->n_corner_scan = s[255];
  if (r < p.n_scan) {
    const uint32_t o = s[r] - v;
    for (uint32_t t = 0; t < v; t++) F.corner_scan[o + t] = F.cloud[F.cpick[(size_t)r * p.ppr + t]];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// segmented pcl::VoxelGrid (voxel_grid.h's segmented pipeline, one box per segment):
//   stage 1: segment = frame * n_scan + ring, the ring's surfaceCloudScan, leaf odometrySurfLeafSize (:243-245)
//   stage 2: segment = 2 frame (corner) / 2 frame + 1 (surf), leaf mappingCornerLeafSize / mappingSurfLeafSize
//            (downsampleCurrentScan, mapOptmization.cpp:1238-1246); leaf 0 = no down-sampling (one cell per element, in order)
// keys (segment << 32 | cell index) are radix-sorted once for all segments of all frames; double centroid sums.
// ---------------------------------------------------------------------------------------------------------------------------
template <int kStage>
__device__ inline vg::Elem elem_of(const LfFrame& F, const LfParams& p, uint32_t f, uint32_t j, const float4* cells1) {
  vg::Elem e{false, 0u, 0u, make_float4(0.f, 0.f, 0.f, 0.f)};
  if (kStage == 1) {
    if (j < F.info->count && F.member[j] >= 0) {
      e.valid = true; e.seg = f * (uint32_t)p.n_scan + (uint32_t)F.member[j]; e.ord = j; e.pt = F.cloud[j];
    }
  } else {
    const uint32_t nc = (uint32_t)p.n_scan * (uint32_t)p.ppr;
    if (j < nc) {
      const uint32_t r = j / (uint32_t)p.ppr, t = j % (uint32_t)p.ppr;
      if (t < (uint32_t)F.ccnt[r]) { e.valid = true; e.seg = 2u * f; e.ord = j; e.pt = F.cloud[F.cpick[j]]; }
    } else if (j - nc < F.info->n_surf_scan) {
      e.valid = true; e.seg = 2u * f + 1u; e.ord = j; e.pt = cells1[F.info->first1 + (j - nc)];
    }
  }
  return e;
}

__device__ inline float seg_leaf(int stage, const LfParams& p, uint32_t seg) {
  return stage == 1 ? p.leaf_odo : ((seg & 1u) ? p.leaf_surf : p.leaf_corner);
}

// a stage's elements as the pipeline reads them: row = frame, slot j of the frame's range; the cells of all frames go to `out`
template <int kStage>
struct LfElems {
  static constexpr int kFields = 4;
  const LfFrame* fr; LfParams p; const float4* cells1; float4* out;
  __device__ uint32_t segs_per_frame() const { return kStage == 1 ? (uint32_t)p.n_scan : 2u; }
  __device__ uint32_t base(const LfFrame& F) const { return kStage == 1 ? F.base1 : F.base2; }
  __device__ int fields() const { return 4; }
  __device__ bool slot(uint32_t f, uint32_t j, uint32_t* g) const {
    const LfFrame& F = fr[f];
    *g = base(F) + j;
    return j < (kStage == 1 ? F.cap1 : (uint32_t)p.n_scan * (uint32_t)p.ppr + F.cap1);   // the frame's own range (a row is the largest of the batch)
  }
  __device__ vg::Elem elem(uint32_t f, uint32_t j) const { return elem_of<kStage>(fr[f], p, f, j, cells1); }
  __device__ float4 fetch(uint32_t g, uint32_t seg) const {
    const uint32_t f = seg / segs_per_frame();
    const LfFrame& F = fr[f];
    return elem_of<kStage>(F, p, f, g - base(F), cells1).pt;
  }
  __device__ float leaf(uint32_t seg) const { return seg_leaf(kStage, p, seg); }
  __device__ void overflow(uint32_t seg) const { fr[seg / segs_per_frame()].info->overflow = 1u; }   // every writer stores 1
  __device__ void put(uint32_t cell, const float (&m)[kFields]) const { out[cell] = make_float4(m[0], m[1], m[2], m[3]); }
};

// per-frame totals of a stage from the segment counts (one block of 256 per frame)
template <int kStage>
__global__ void __launch_bounds__(256) k_sv_frames(const LfFrame* __restrict__ fr, LfParams p, const uint32_t* __restrict__ scnt, const uint32_t* __restrict__ sfirst) {
  const uint32_t f = blockIdx.x;
  const LfFrame& F = fr[f];
  const uint32_t spf = kStage == 1 ? (uint32_t)p.n_scan : 2u;
  __shared__ uint32_t s_tot, s_first;
  if (threadIdx.x == 0) { s_tot = 0; s_first = 0xffffffffu; }
  __syncthreads();
  for (uint32_t r = threadIdx.x; r < spf; r += 256) {
    const uint32_t c = scnt[f * spf + r];
    if (c) { atomicAdd(&s_tot, c); atomicMin(&s_first, sfirst[f * spf + r]); }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (kStage == 1) { F.info->n_surf_scan = s_tot; F.info->first1 = s_first == 0xffffffffu ? 0u : s_first; }
    else {
      F.info->n_corner = scnt[2 * f]; F.info->n_surf = scnt[2 * f + 1];
      F.info->first2 = s_first == 0xffffffffu ? 0u : s_first;
    }
  }
}

// the frame's outputs: surfaceCloud (stage 1) and the mapping-down-sampled features (stage 2), corner first, then surf
__global__ void k_lf_finish(const LfFrame* __restrict__ fr, LfParams p, const float4* __restrict__ cells1, const float4* __restrict__ cells2) {
  const LfFrame& F = fr[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const LfInfo& I = *F.info;
  if (i < I.n_surf_scan) F.surf_scan[i] = cells1[I.first1 + i];
  const uint32_t nf = I.n_corner + I.n_surf;
  if (i < nf) {
    const float4 q = cells2[I.first2 + i];
    F.out[i] = q;
    if (F.src) {   // k_load_points' layout: w = the index within its own cloud
      const uint32_t w = i < I.n_corner ? i : i - I.n_corner;
      F.src[i] = make_float4(q.x, q.y, q.z, __uint_as_float(w));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------
// the cross-frame state of one context (the reference node's members) and its last frame's outputs
struct FeatState {
  int n_scan = 0, H = 0, A = 0;
  DevBuf<int32_t> col_ind; DevBuf<float> range; DevBuf<float4> cloud; DevBuf<float> curv;
  DevBuf<int32_t> picked; DevBuf<int32_t> label; DevBuf<DistId> smooth;
  DevBuf<int32_t> picked_occ; DevBuf<int32_t> start;
  int32_t* end = nullptr;   // end = start + n_scan (one allocation)
  DevBuf<float4> corner_scan, surf_scan, out;
  uint64_t out_gen = 0;   // bumps with every frame that rewrites `out` (the key-frame store checks it, loam_source_view)
  LfInfo last{};
  bool have_last = false;
  // batch workspace (used when this context leads a batch)
  DevBuf<LfFrame> d_fr; PinnedBuf<LfFrame> h_fr;
  DevBuf<LfInfo> d_info; PinnedBuf<LfInfo> h_info;
  DevBuf<char> ws;
  std::vector<double> dk_host;   // the deskew tables of a batch as the device reads them (staging of their upload)
};

FeatState* fe_of(pcm_ctx* c) { return c->loam_fe.get_or_create<FeatState>(); }

int check_fparams(pcm_ctx* c, const pcm_loam_feature_params& p) {
  if (p.n_scan < 1 || p.horizon_scan < 2) { c->err = "n_scan must be >= 1 and horizon_scan >= 2"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.n_scan > 256 || p.horizon_scan > 4096) { c->err = "n_scan > 256 or horizon_scan > 4096 is not supported"; return PCM_ERR_UNSUPPORTED; }
  if (p.downsample_rate < 1 || p.area_num < 1 || p.area_num > 4096) { c->err = "downsample_rate must be >= 1 and area_num in [1, 4096]"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.min_range >= 0.f) || !(p.max_range <= 1e30f) || !(p.edge_threshold == p.edge_threshold) || !(p.surf_threshold == p.surf_threshold)) {
    c->err = "ranges must be in [0, 1e30] and the thresholds numbers"; return PCM_ERR_INVALID_ARGUMENT;
  }
  if (!(p.odometry_surf_leaf > 0.f) || !(p.mapping_corner_leaf >= 0.f) || !(p.mapping_surf_leaf >= 0.f)) {
    c->err = "odometry_surf_leaf must be > 0, the mapping leaves >= 0 (0: no down-sampling)"; return PCM_ERR_INVALID_ARGUMENT;
  }
  return PCM_OK;
}

// the context's state arrays for (n_scan, horizon_scan): zero at creation (cloudSmoothness is value-initialised; the three
// new T[] arrays of featureExtraction are taken as zero) and again whenever the shape changes
int ensure_state(pcm_ctx* c, FeatState* S, const pcm_loam_feature_params& p) {
  const size_t cap = (size_t)p.n_scan * (size_t)p.horizon_scan;
  if (S->col_ind && S->n_scan == p.n_scan && S->H == p.horizon_scan) return PCM_OK;
  (void)hipStreamSynchronize(c->stream);
  S->n_scan = S->H = 0;   // until every array below has the new shape
  S->have_last = false;
  S->col_ind.release(); S->range.release(); S->cloud.release(); S->curv.release(); S->picked.release(); S->label.release(); S->smooth.release();
  auto fresh = [&](auto& b) { return b.reserve(c, cap, cap, true); };
  int rc;
  if ((rc = fresh(S->col_ind)) != PCM_OK || (rc = fresh(S->range)) != PCM_OK || (rc = fresh(S->cloud)) != PCM_OK || (rc = fresh(S->curv)) != PCM_OK ||
      (rc = fresh(S->picked)) != PCM_OK || (rc = fresh(S->label)) != PCM_OK || (rc = fresh(S->smooth)) != PCM_OK)
    return rc;
  S->n_scan = p.n_scan; S->H = p.horizon_scan;
  return PCM_OK;
}

int next_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// one stage: N element slots in B rows of up to size_per_frame, nseg segments; the cells of all frames go to cells_out
template <int kStage>
int run_vg(pcm_ctx* c0, hipStream_t st, const LfFrame* d_fr, const LfParams& P, int B, uint32_t size_per_frame, uint32_t N, uint32_t nseg, vg::Work W,
           const float4* cells1, float4* cells_out) {
  if (N == 0 || size_per_frame == 0) return PCM_OK;
  W.nseg = nseg;
  const LfElems<kStage> E{d_fr, P, cells1, cells_out};
  vg::clear(st, W);
  vg::seg_minmax(st, E, (uint32_t)B, size_per_frame, W);
  const int rc = vg::seg_cells(&c0->err, st, E, (uint32_t)B, size_per_frame, N, W);
  if (rc != PCM_OK) return rc;
  k_sv_frames<kStage><<<B, 256, 0, st>>>(d_fr, P, W.scnt(), W.sfirst());
  PCM_HIPCK(c0, hipGetLastError());
  return PCM_OK;
}

}  // namespace

namespace pcm {
namespace loam {
// the context's last front-end features with their averaged intensity (k_lf_finish's F.out), alive until the next frame
bool loam_features_last_out(pcm_ctx* c, const float4** out, uint32_t* n_c, uint32_t* n_s, uint64_t* gen) {
  const FeatState* S = c->loam_fe.get<FeatState>();
  if (!S || !S->have_last || !S->out) return false;
  *gen = S->out_gen;
  *out = S->out; *n_c = S->last.n_corner; *n_s = S->last.n_surf;
  return true;
}
}  // namespace loam
}  // namespace pcm

namespace {

pcm_loam_feature_params params_or_default(const pcm_loam_feature_params* params) {
  pcm_loam_feature_params p;
  if (params) p = *params; else pcm_loam_default_feature_params(&p);
  return p;
}

LfParams dev_params(const pcm_loam_feature_params& q) {
  LfParams p;
  std::memset(&p, 0, sizeof(p));
  p.n_scan = q.n_scan; p.H = q.horizon_scan; p.rate = q.downsample_rate; p.A = q.area_num;
  p.min_range = q.min_range; p.max_range = q.max_range; p.edge = q.edge_threshold; p.surf = q.surf_threshold;
  p.ang_res_x = (float)(360.0 / (double)(float)q.horizon_scan);   // static float ang_res_x = 360.0/float(Horizon_SCAN) (:741)
  p.leaf_odo = q.odometry_surf_leaf; p.leaf_corner = q.mapping_corner_leaf; p.leaf_surf = q.mapping_surf_leaf;
  p.force_serial = (q.flags & PCM_LOAM_FEATURES_FORCE_SERIAL_SORT) ? 1 : 0;
  p.ppr = q.area_num * kMaxPicks;
  const int smax = (q.horizon_scan - 10) / q.area_num;   // ep - sp <= (end - start) / area_num, end - start = points - 10
  p.P = next_pow2(std::max(1, smax + 1));
  return p;
}

int check_ctx_fe(pcm_ctx* c) {
  const int rc = loam::loam_check_ctx(c, PCM_ERR_UNSUPPORTED, "pcm_loam_* needs a context created with PCM_MODEL_LOAM");
  if (rc != PCM_OK) return rc;
  if (!fe_of(c)) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  return PCM_OK;
}

constexpr size_t kDkStateWords = 16;   // per frame: the first-point word, then transStartInverse (12 floats)

// a live descriptor (non-null, imu_available != 0) against the record layout, before any device work
int check_deskew(pcm_ctx* c0, const pcm_loam_deskew& d, const void* pts, size_t stride, int memory) {
  if (d.n_imu > loam::kDeskewMaxEntries || d.n_odom > loam::kDeskewMaxEntries) { c0->err = "a deskew table holds at most 1024 entries"; return PCM_ERR_UNSUPPORTED; }
  if (d.n_imu < 1 || d.n_odom < 0 || !d.imu_time || !d.imu_rot_x || !d.imu_rot_y || !d.imu_rot_z ||
      (d.n_odom > 0 && (!d.odom_time || !d.odom_incre_x || !d.odom_incre_y || !d.odom_incre_z))) {
    c0->err = "deskew: imu_available needs an IMU table of >= 1 entries; a table with entries needs its four arrays";
    return PCM_ERR_INVALID_ARGUMENT;
  }
  if (d.time_kind != PCM_LOAM_TIME_DOUBLE && d.time_kind != PCM_LOAM_TIME_FLOAT) { c0->err = "deskew: time_kind must be PCM_LOAM_TIME_DOUBLE or PCM_LOAM_TIME_FLOAT"; return PCM_ERR_INVALID_ARGUMENT; }
  const size_t w = d.time_kind == PCM_LOAM_TIME_DOUBLE ? 8 : 4;
  if (d.time_offset_bytes + w > stride) { c0->err = "deskew: the time field lies past the record"; return PCM_ERR_INVALID_ARGUMENT; }
  // host records are staged at a 256-byte boundary; device records are read where they lie
  const size_t base = memory == PCM_MEM_DEVICE ? (size_t)reinterpret_cast<uintptr_t>(pts) : 0;
  if ((stride % w) != 0 || ((base + d.time_offset_bytes) % w) != 0) { c0->err = "deskew: the time field is not aligned to its size in every record"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

// rows of one table behind `out`: prefix maximum, time, x, y, z
void pack_table(std::vector<double>& out, const double* t, const double* x, const double* y, const double* z, int n) {
  const size_t at = out.size();
  out.resize(at + 5 * (size_t)n);
  if (n == 0) return;
  loam::deskew_prefix_max(t, n, out.data() + at);
  std::memcpy(out.data() + at + (size_t)n, t, sizeof(double) * (size_t)n);
  std::memcpy(out.data() + at + 2 * (size_t)n, x, sizeof(double) * (size_t)n);
  std::memcpy(out.data() + at + 3 * (size_t)n, y, sizeof(double) * (size_t)n);
  std::memcpy(out.data() + at + 4 * (size_t)n, z, sizeof(double) * (size_t)n);
}

// the whole front end for n frames (one context each) in one set of launches on the first context's stream.  dks: null, or one
// descriptor per frame (any may be null); a frame is deskewed when its descriptor says imu_available (deskewPoint's own test)
int run_frames(pcm_ctx* const* ctxs, int B, const void* const* points, const size_t* n_points, size_t stride, size_t ioff, size_t roff, int memory,
               const pcm_loam_feature_params* params, bool to_source, pcm_loam_features_result* results, const pcm_loam_deskew* const* dks = nullptr) {
  if (!ctxs || B <= 0 || !points || !n_points || !results) return PCM_ERR_INVALID_ARGUMENT;
  pcm_ctx* c0 = ctxs[0];
  int rc = check_ctx_fe(c0);
  if (rc != PCM_OK) return rc;
  const pcm_loam_feature_params q = params_or_default(params);
  if ((rc = check_fparams(c0, q)) != PCM_OK) return rc;
  if (stride < 12 || ioff + 1 > stride || roff + 2 > stride || (stride % 4) != 0 || (roff % 2) != 0) {
    c0->err = "stride must be a multiple of 4 >= 12 holding the 1-byte intensity and the 2-byte aligned ring";
    return PCM_ERR_INVALID_ARGUMENT;
  }
  if (check_memory(c0, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < B; i++) {
    if ((rc = check_ctx_fe(ctxs[i])) != PCM_OK) { if (ctxs[i] && ctxs[i] != c0) c0->err = ctxs[i]->err; return rc; }
    if (ctxs[i]->device != c0->device) { c0->err = "all contexts of a batch must live on one device"; return PCM_ERR_INVALID_ARGUMENT; }
    for (int j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) { c0->err = "a context appears twice in the batch"; return PCM_ERR_INVALID_ARGUMENT; }
    if (!points[i] && n_points[i]) { c0->err = "null point buffer"; return PCM_ERR_INVALID_ARGUMENT; }
    if (n_points[i] > 0x3fffffffull) { c0->err = "cloud too large"; return PCM_ERR_INVALID_ARGUMENT; }
  }
  std::vector<const pcm_loam_deskew*> live((size_t)B, nullptr);
  bool any_dk = false;
  for (int i = 0; i < B && dks; i++) {
    if (!dks[i] || !dks[i]->imu_available) continue;
    if ((rc = check_deskew(c0, *dks[i], points[i], stride, memory)) != PCM_OK) return rc;
    live[(size_t)i] = dks[i];
    any_dk = true;
  }
  PCM_HIPCK(c0, hipSetDevice(c0->device));
  const LfParams P = dev_params(q);
  const size_t cap = (size_t)q.n_scan * q.horizon_scan;
  const size_t ncs = (size_t)q.n_scan * P.ppr;   // corner picks per frame
  // LDS of k_lf_select: the sort buffer (<= 4096 entries of 8 bytes: a sector holds at most (horizon_scan - 10) / area_num + 1
  // entries) and the ring window (horizon_scan + 10 positions of 4 bytes): at most 48.1 KiB within the caps checked above
  const size_t lds = (size_t)P.P * 8 + (size_t)(q.horizon_scan + 10) * 4;
  if (lds > 65536) { c0->err = "k_lf_select's LDS exceeds 64 KiB (library bug: the caps keep it below 48.1 KiB)"; return PCM_ERR_INTERNAL; }
  // per-context state and outputs
  std::vector<size_t> cap1((size_t)B), base1((size_t)B), base2((size_t)B);
  size_t N1 = 0, N2 = 0;
  uint32_t max1 = 1;
  for (int i = 0; i < B; i++) {
    pcm_ctx* c = ctxs[i];
    FeatState* S = fe_of(c);
    if ((rc = ensure_state(c, S, q)) != PCM_OK) { if (c != c0) c0->err = c->err; return rc; }
    cap1[(size_t)i] = std::min(n_points[i], cap);
    base1[(size_t)i] = N1; N1 += cap1[(size_t)i];
    base2[(size_t)i] = N2; N2 += ncs + cap1[(size_t)i];
    max1 = std::max<uint32_t>(max1, (uint32_t)cap1[(size_t)i]);
    const size_t n_ring = 2 * (size_t)q.n_scan, n_surf = cap1[(size_t)i];
    if ((rc = S->picked_occ.reserve(c, cap, cap)) != PCM_OK || (rc = S->start.reserve(c, n_ring, n_ring)) != PCM_OK ||
        (rc = S->corner_scan.reserve(c, ncs, ncs)) != PCM_OK || (rc = S->surf_scan.reserve(c, n_surf, n_surf)) != PCM_OK ||
        (rc = S->out.reserve(c, ncs + n_surf, ncs + n_surf)) != PCM_OK) {
      if (c != c0) c0->err = c->err;
      return rc;
    }
    S->end = S->start + q.n_scan;
    S->A = q.area_num;
    S->out_gen++;
  }
  std::vector<float4*> src((size_t)B, nullptr);
  if (to_source)
    for (int i = 0; i < B; i++)
      if ((rc = loam::loam_source_reserve(ctxs[i], ncs + cap1[(size_t)i], &src[(size_t)i])) != PCM_OK) { if (ctxs[i] != c0) c0->err = ctxs[i]->err; return rc; }
  // batch workspace of the leading context
  FeatState* S0 = fe_of(c0);
  const size_t nseg_max = std::max<size_t>((size_t)B * q.n_scan, 2 * (size_t)B);
  const size_t n_vg = std::max(N1, N2);   // the VoxelGrid's arrays are shared by the two stages
  size_t vg_bytes = 0;
  (void)vg::work_layout(nullptr, n_vg, sizeof(uint64_t), nseg_max, &vg_bytes);
  std::vector<const void*> pts((size_t)B, nullptr);
  LfBatch Lw;
  // the deskew tables of the batch, frame after frame (IMU rows, then odometry rows), and one state block per frame
  std::vector<size_t> dk_at((size_t)B, 0);
  size_t dk_total = 0;
  for (int i = 0; i < B; i++)
    if (const pcm_loam_deskew* d = live[(size_t)i]) { dk_at[(size_t)i] = dk_total; dk_total += 5 * ((size_t)d->n_imu + (size_t)d->n_odom); }
  const double* dk_tab = nullptr;
  uint32_t* dk_state = nullptr;
  auto layout = [&](ArenaStage& a) {
    Lw = loam_batch_layout(a, B, memory, points, n_points, stride, pts.data(), cap, q.n_scan, P.ppr, N1, N2, vg_bytes);
    if (any_dk) {
      dk_tab = a.upload(a.take<double>(dk_total), S0->dk_host.data(), sizeof(double) * dk_total);
      dk_state = a.take<uint32_t>(kDkStateWords * (size_t)B);
    }
  };
  ArenaStage ws_size = arena_stage(c0, nullptr);
  layout(ws_size);
  hipStream_t st = c0->stream;
  PCM_HIPCK(c0, hipStreamSynchronize(st));   // the pinned staging of an earlier batch, and dk_host, are free again
  S0->dk_host.clear();
  for (int i = 0; i < B; i++)
    if (const pcm_loam_deskew* d = live[(size_t)i]) {
      pack_table(S0->dk_host, d->imu_time, d->imu_rot_x, d->imu_rot_y, d->imu_rot_z, d->n_imu);
      pack_table(S0->dk_host, d->odom_time, d->odom_incre_x, d->odom_incre_y, d->odom_incre_z, d->n_odom);
    }
  if ((rc = S0->ws.reserve(c0, ws_size.used(), ws_size.used())) != PCM_OK) return rc;
  if ((rc = S0->d_fr.reserve(c0, (size_t)B, (size_t)B)) != PCM_OK || (rc = S0->h_fr.reserve(c0, (size_t)B, (size_t)B)) != PCM_OK ||
      (rc = S0->d_info.reserve(c0, (size_t)B, (size_t)B)) != PCM_OK || (rc = S0->h_info.reserve(c0, (size_t)B, (size_t)B)) != PCM_OK)
    return rc;
  ArenaStage ws = arena_stage(c0, S0->ws.p);   // the clouds in host memory are staged here
  layout(ws);
  if (ws.rc != PCM_OK) return ws.rc;
  uint32_t maxn = 1;
  for (int i = 0; i < B; i++) {
    FeatState* S = fe_of(ctxs[i]);
    LfFrame& F = S0->h_fr[i];
    std::memset(&F, 0, sizeof(F));
    F.pts = static_cast<const char*>(pts[(size_t)i]);
    F.n = (uint32_t)n_points[i]; F.stride = (uint32_t)stride; F.ioff = (uint32_t)ioff; F.roff = (uint32_t)roff;
    F.cap1 = (uint32_t)cap1[(size_t)i]; F.base1 = (uint32_t)base1[(size_t)i]; F.base2 = (uint32_t)base2[(size_t)i];
    F.col_ind = S->col_ind; F.range = S->range; F.cloud = S->cloud; F.curv = S->curv; F.picked = S->picked; F.label = S->label; F.smooth = S->smooth;
    F.start = S->start; F.end = S->end; F.picked_occ = S->picked_occ; F.corner_scan = S->corner_scan; F.surf_scan = S->surf_scan; F.out = S->out;
    F.src = src[(size_t)i];
    F.owner = Lw.owner + (size_t)i * cap;
    F.rowcnt = Lw.rowcnt + (size_t)i * q.n_scan;
    F.roff_arr = Lw.roff + (size_t)i * (q.n_scan + 1);
    F.member = Lw.member + (size_t)i * cap;
    F.cpick = Lw.cpick + (size_t)i * ncs;
    F.ccnt = Lw.ccnt + (size_t)i * q.n_scan;
    F.info = S0->d_info + i;
    if (const pcm_loam_deskew* d = live[(size_t)i]) {
      const double* tab = dk_tab + dk_at[(size_t)i];
      F.dk.imu = loam::DeskewTable{tab, d->n_imu};
      F.dk.odo = loam::DeskewTable{tab + 5 * (size_t)d->n_imu, d->n_odom};
      F.dk.time_scan_cur = d->time_scan_cur;
      F.dk.toff = (uint32_t)d->time_offset_bytes;
      F.dk.tkind = d->time_kind;
      F.dk.enabled = 1;
      F.dk.first = dk_state + kDkStateWords * (size_t)i;
      F.dk.start_inv = reinterpret_cast<float*>(F.dk.first + 1);
    }
    maxn = std::max<uint32_t>(maxn, F.n);
  }
  PCM_HIPCK(c0, hipMemcpyAsync(S0->d_fr, S0->h_fr, sizeof(LfFrame) * (size_t)B, hipMemcpyHostToDevice, st));
  const LfFrame* d_fr = S0->d_fr;
  const unsigned gcap = (unsigned)((std::max<size_t>(cap, (size_t)q.n_scan) + 255) / 256);
  if (any_dk) {
    k_lf_clear<true><<<dim3(gcap, B), 256, 0, st>>>(d_fr, P);
    k_lf_project<true><<<dim3((maxn + 255) / 256, B), 256, 0, st>>>(d_fr, P);
    k_lf_dk_start<<<B, 64, 0, st>>>(d_fr);
  } else {
    k_lf_clear<false><<<dim3(gcap, B), 256, 0, st>>>(d_fr, P);
    k_lf_project<false><<<dim3((maxn + 255) / 256, B), 256, 0, st>>>(d_fr, P);
  }
  k_lf_rowcount<<<dim3(q.n_scan, B), 256, 0, st>>>(d_fr, P);
  k_lf_rings<<<B, 256, 0, st>>>(d_fr, P);
  if (any_dk) k_lf_extract<true><<<dim3(q.n_scan, B), 256, 0, st>>>(d_fr, P);
  else k_lf_extract<false><<<dim3(q.n_scan, B), 256, 0, st>>>(d_fr, P);
  const unsigned g1 = (max1 + 255) / 256;
  k_lf_smooth<<<dim3(g1, B), 256, 0, st>>>(d_fr, P);
  k_lf_occlude<<<dim3(g1, B), 256, 0, st>>>(d_fr, P);
  k_lf_snapshot<<<dim3(g1, B), 256, 0, st>>>(d_fr, P);
  k_lf_select<true><<<dim3(1, B), 64, lds, st>>>(d_fr, P);
  k_lf_select<false><<<dim3(q.n_scan, B), 64, lds, st>>>(d_fr, P);
  k_lf_corner_compact<<<B, 256, 0, st>>>(d_fr, P);
  PCM_HIPCK(c0, hipGetLastError());
  float4* cells1 = static_cast<float4*>(Lw.cells1);
  float4* cells2 = static_cast<float4*>(Lw.cells2);
  const vg::Work W = vg::work_layout(Lw.vg, n_vg, sizeof(uint64_t), nseg_max, &vg_bytes);
  if ((rc = run_vg<1>(c0, st, d_fr, P, B, max1, (uint32_t)N1, (uint32_t)(B * q.n_scan), W, cells1, cells1)) != PCM_OK) return rc;
  const uint32_t size2 = (uint32_t)(ncs + max1);
  if ((rc = run_vg<2>(c0, st, d_fr, P, B, size2, (uint32_t)N2, (uint32_t)(2 * B), W, cells1, cells2)) != PCM_OK) return rc;
  k_lf_finish<<<dim3((size2 + 255) / 256, B), 256, 0, st>>>(d_fr, P, cells1, cells2);
  PCM_HIPCK(c0, hipGetLastError());
  PCM_HIPCK(c0, hipMemcpyAsync(S0->h_info, S0->d_info, sizeof(LfInfo) * (size_t)B, hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c0, hipStreamSynchronize(st));
  int worst = PCM_OK;
  for (int i = 0; i < B; i++) {
    const LfInfo& I = S0->h_info[i];
    FeatState* S = fe_of(ctxs[i]);
    S->last = I;
    S->have_last = true;
    pcm_loam_features_result& r = results[i];
    std::memset(&r, 0, sizeof(r));
    r.num_extracted = (int32_t)I.count;
    r.num_corner_scan = (int32_t)I.n_corner_scan;
    r.num_surf_scan = (int32_t)I.n_surf_scan;
    r.num_corner = (int32_t)I.n_corner;
    r.num_surf = (int32_t)I.n_surf;
    r.sectors = (int32_t)I.sectors;
    r.sectors_serial = (int32_t)I.sectors_serial;
    r.status = PCM_OK;
    if (I.bad_sector) { r.status = PCM_ERR_INTERNAL; ctxs[i]->err = "a sector exceeded the sort buffer"; }
    else if (I.overflow) { r.status = PCM_ERR_OUT_OF_RANGE; ctxs[i]->err = "leaf size too small for the extent of the cloud (index overflow)"; }
    if (r.status == PCM_OK && to_source) loam::loam_source_commit(ctxs[i], I.n_corner, I.n_surf);
    if (r.status != PCM_OK && worst == PCM_OK) { worst = r.status; if (ctxs[i] != c0) c0->err = ctxs[i]->err; }
  }
  return worst;
}

void copy_xyzi(const float4* d, size_t n, float* host) { for (size_t i = 0; i < n; i++) { host[4 * i] = d[i].x; host[4 * i + 1] = d[i].y; host[4 * i + 2] = d[i].z; host[4 * i + 3] = d[i].w; } }

}  // namespace

extern "C" {

void pcm_loam_default_feature_params(pcm_loam_feature_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->n_scan = 16;                 // utility.h:241
  p->horizon_scan = 1800;         // :242
  p->downsample_rate = 1;         // :244
  p->area_num = 6;                // :252
  p->min_range = 1.0f;            // :223
  p->max_range = 150.0f;          // :224
  p->edge_threshold = 0.1f;       // :265
  p->surf_threshold = 0.1f;       // :266
  p->odometry_surf_leaf = 0.2f;   // :270
  p->mapping_corner_leaf = 0.2f;  // :271
  p->mapping_surf_leaf = 0.2f;    // :272
}

int pcm_loam_extract_features(pcm_ctx* c, const void* points, size_t n, size_t stride_bytes, size_t intensity_offset_bytes, size_t ring_offset_bytes, int memory,
                              const pcm_loam_feature_params* params, float* corner, size_t cap_corner, float* surf, size_t cap_surf, pcm_loam_features_result* res) {
  return pcm_loam_extract_features_deskew(c, points, n, stride_bytes, intensity_offset_bytes, ring_offset_bytes, memory, params, corner, cap_corner, surf, cap_surf, res, nullptr);
}

int pcm_loam_extract_features_deskew(pcm_ctx* c, const void* points, size_t n, size_t stride_bytes, size_t intensity_offset_bytes, size_t ring_offset_bytes, int memory,
                                     const pcm_loam_feature_params* params, float* corner, size_t cap_corner, float* surf, size_t cap_surf, pcm_loam_features_result* res,
                                     const pcm_loam_deskew* deskew) {
  if (!c || !res) return PCM_ERR_INVALID_ARGUMENT;
  pcm_ctx* arr[1] = {c};
  const void* pts[1] = {points};
  size_t ns[1] = {n};
  const pcm_loam_deskew* dks[1] = {deskew};
  int rc = run_frames(arr, 1, pts, ns, stride_bytes, intensity_offset_bytes, ring_offset_bytes, memory, params, false, res, dks);
  if (rc != PCM_OK) return rc;
  const size_t nc = (size_t)res->num_corner, nsf = (size_t)res->num_surf;
  if ((nc && !corner) || (nsf && !surf) || nc > cap_corner || nsf > cap_surf) { c->err = "output capacity too small (counts are in the result)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (nc + nsf == 0) return PCM_OK;
  std::vector<float4> h(nc + nsf);
  FeatState* S = fe_of(c);
  PCM_HIPCK(c, hipMemcpyAsync(h.data(), S->out, sizeof(float4) * h.size(), hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  copy_xyzi(h.data(), nc, corner);
  copy_xyzi(h.data() + nc, nsf, surf);
  return PCM_OK;
}

int pcm_loam_frame_begin(pcm_ctx* c, const void* points, size_t n, size_t stride_bytes, size_t intensity_offset_bytes, size_t ring_offset_bytes, int memory,
                         const pcm_loam_feature_params* params, pcm_loam_features_result* res) {
  pcm_ctx* arr[1] = {c};
  const void* pts[1] = {points};
  size_t ns[1] = {n};
  return run_frames(arr, 1, pts, ns, stride_bytes, intensity_offset_bytes, ring_offset_bytes, memory, params, true, res);
}

int pcm_loam_frame_begin_batch(pcm_ctx* const* ctxs, int n, const void* const* points, const size_t* n_points, size_t stride_bytes, size_t intensity_offset_bytes,
                               size_t ring_offset_bytes, int memory, const pcm_loam_feature_params* params, pcm_loam_features_result* results) {
  return run_frames(ctxs, n, points, n_points, stride_bytes, intensity_offset_bytes, ring_offset_bytes, memory, params, true, results);
}

int pcm_loam_frame_begin_deskew(pcm_ctx* c, const void* points, size_t n, size_t stride_bytes, size_t intensity_offset_bytes, size_t ring_offset_bytes, int memory,
                                const pcm_loam_feature_params* params, pcm_loam_features_result* res, const pcm_loam_deskew* deskew) {
  pcm_ctx* arr[1] = {c};
  const void* pts[1] = {points};
  size_t ns[1] = {n};
  const pcm_loam_deskew* dks[1] = {deskew};
  return run_frames(arr, 1, pts, ns, stride_bytes, intensity_offset_bytes, ring_offset_bytes, memory, params, true, res, dks);
}

int pcm_loam_frame_begin_batch_deskew(pcm_ctx* const* ctxs, int n, const void* const* points, const size_t* n_points, size_t stride_bytes, size_t intensity_offset_bytes,
                                      size_t ring_offset_bytes, int memory, const pcm_loam_feature_params* params, pcm_loam_features_result* results,
                                      const pcm_loam_deskew* const* deskew) {
  return run_frames(ctxs, n, points, n_points, stride_bytes, intensity_offset_bytes, ring_offset_bytes, memory, params, true, results, deskew);
}

int pcm_loam_deskew_tables(const pcm_loam_deskew_input* in, double* imu_table, size_t cap_imu, double* odom_table, size_t cap_odom, pcm_loam_deskew* deskew,
                           pcm_loam_deskew_result* res) {
  if (!in || !res || in->n_imu < 0 || in->n_odom < 0 || (in->n_imu && !in->imu) || (in->n_odom && !in->odom)) return PCM_ERR_INVALID_ARGUMENT;
  static_assert(sizeof(pcm_loam_imu_sample) == sizeof(loam::DeskewImu) && sizeof(pcm_loam_odom_sample) == sizeof(loam::DeskewOdom), "sample layouts");
  std::memset(res, 0, sizeof(*res));
  res->start_odom_index = -1;
  constexpr int K = loam::kDeskewMaxEntries;
  std::vector<double> imu(4 * (size_t)K), odo(4 * (size_t)K);
  loam::DeskewTables t;
  const loam::DeskewBuild b = loam::deskew_tables(in->time_scan_cur, in->time_scan_next, reinterpret_cast<const loam::DeskewImu*>(in->imu), in->n_imu,
                                                  reinterpret_cast<const loam::DeskewOdom*>(in->odom), in->n_odom, imu.data(), odo.data(), K, &t);
  if (b == loam::kDeskewTooMany) return PCM_ERR_UNSUPPORTED;
  if (b == loam::kDeskewWaiting) { res->status = PCM_LOAM_DESKEW_WAITING; return PCM_OK; }
  res->status = PCM_LOAM_DESKEW_READY;
  res->imu_skipped = t.imu_skipped; res->odom_skipped = t.odom_skipped;
  res->n_imu = t.n_imu; res->n_odom = t.n_odom;
  res->imu_available = t.imu_available; res->odom_available = t.odom_available; res->odom_deskew = t.odom_deskew;
  res->start_odom_index = t.start_odom;
  if ((size_t)t.n_imu > cap_imu || (size_t)t.n_odom > cap_odom || (t.n_imu && !imu_table) || (t.n_odom && !odom_table)) return PCM_ERR_INVALID_ARGUMENT;
  for (int r = 0; r < 4; r++) {
    if (t.n_imu) std::memcpy(imu_table + (size_t)r * cap_imu, imu.data() + (size_t)r * K, sizeof(double) * (size_t)t.n_imu);
    if (t.n_odom) std::memcpy(odom_table + (size_t)r * cap_odom, odo.data() + (size_t)r * K, sizeof(double) * (size_t)t.n_odom);
  }
  if (deskew) {
    std::memset(deskew, 0, sizeof(*deskew));
    deskew->time_scan_cur = in->time_scan_cur;
    if (t.n_imu) { deskew->imu_time = imu_table; deskew->imu_rot_x = imu_table + cap_imu; deskew->imu_rot_y = imu_table + 2 * cap_imu; deskew->imu_rot_z = imu_table + 3 * cap_imu; }
    if (t.n_odom) { deskew->odom_time = odom_table; deskew->odom_incre_x = odom_table + cap_odom; deskew->odom_incre_y = odom_table + 2 * cap_odom; deskew->odom_incre_z = odom_table + 3 * cap_odom; }
    deskew->n_imu = t.n_imu; deskew->n_odom = t.n_odom;
    deskew->imu_available = t.imu_available;
    deskew->time_offset_bytes = 24;   // PointXYZIRT's double timestamp
    deskew->time_kind = PCM_LOAM_TIME_DOUBLE;
  }
  return PCM_OK;
}

int pcm_loam_feature_info(pcm_ctx* c, int32_t counts[4], int32_t* start_ring, int32_t* end_ring, int32_t* col_ind, float* range, float* cloud, float* curvature,
                          int32_t* neighbor_picked, int32_t* label, float* corner_scan, float* surf_scan) {
  int rc = check_ctx_fe(c);
  if (rc != PCM_OK) return rc;
  FeatState* S = fe_of(c);
  if (!S->have_last) { c->err = "no frame has run through the front end of this context"; return PCM_ERR_NO_INPUT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  const size_t n = S->last.count, ns = (size_t)S->n_scan, nc = S->last.n_corner_scan, nss = S->last.n_surf_scan;
  if (counts) { counts[0] = (int32_t)n; counts[1] = (int32_t)nc; counts[2] = (int32_t)nss; counts[3] = (int32_t)ns; }
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  if (start_ring) PCM_HIPCK(c, hipMemcpy(start_ring, S->start, 4 * ns, hipMemcpyDeviceToHost));
  if (end_ring) PCM_HIPCK(c, hipMemcpy(end_ring, S->end, 4 * ns, hipMemcpyDeviceToHost));
  if (col_ind && n) PCM_HIPCK(c, hipMemcpy(col_ind, S->col_ind, 4 * n, hipMemcpyDeviceToHost));
  if (range && n) PCM_HIPCK(c, hipMemcpy(range, S->range, 4 * n, hipMemcpyDeviceToHost));
  if (cloud && n) PCM_HIPCK(c, hipMemcpy(cloud, S->cloud, 16 * n, hipMemcpyDeviceToHost));
  if (curvature && n) PCM_HIPCK(c, hipMemcpy(curvature, S->curv, 4 * n, hipMemcpyDeviceToHost));
  if (neighbor_picked && n) PCM_HIPCK(c, hipMemcpy(neighbor_picked, S->picked_occ, 4 * n, hipMemcpyDeviceToHost));
  if (label && n) PCM_HIPCK(c, hipMemcpy(label, S->label, 4 * n, hipMemcpyDeviceToHost));
  if (corner_scan && nc) PCM_HIPCK(c, hipMemcpy(corner_scan, S->corner_scan, 16 * nc, hipMemcpyDeviceToHost));
  if (surf_scan && nss) PCM_HIPCK(c, hipMemcpy(surf_scan, S->surf_scan, 16 * nss, hipMemcpyDeviceToHost));
  return PCM_OK;
}

}  // extern "C"
