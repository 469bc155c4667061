// linearize_common.h -- device helpers shared by the point-to-plane search kernels (kernels.hip: the per-tile LDS search and
// the LIO variant; neighbour_lists.hip: the walk of per-voxel candidate lists; linearize_counted.hip, linearize_reforder.hip):
// neighbour-cell tables in the reference's order
// (jueying_lio/include/ivox3d/ivox3d.h:211-235), the float pose transform of laser_mapping.cc:602-612, the running 5-best list
// of IVoxNode::KNNPointByCondition / IVox::GetClosestPoint (ivox3d_node.hpp:140-205, ivox3d.h:132-204) and the per-lane search
// against the global brick hash.
#pragma once

#include "pcm_device.h"
#include "brick_table.h"
#include "plane_fit.h"

namespace pcm {

// neighbour cells in the reference's order (ivox3d.h:211-235): CENTER, NEARBY6, NEARBY18, NEARBY26 are prefixes
// (compile-time copy for the unrolled LDS search: the offsets become immediates)
constexpr int kNearby[27][3] = {
  {0, 0, 0},   {-1, 0, 0},  {1, 0, 0},   {0, 1, 0},   {0, -1, 0},  {0, 0, -1},  {0, 0, 1},
  {1, 1, 0},   {-1, 1, 0},  {1, -1, 0},  {-1, -1, 0}, {1, 0, 1},   {-1, 0, 1},  {1, 0, -1},
  {-1, 0, -1}, {0, 1, 1},   {0, -1, 1},  {0, 1, -1},  {0, -1, -1}, {1, 1, 1},   {-1, 1, 1},
  {1, -1, 1},  {1, 1, -1},  {-1, -1, 1}, {-1, 1, -1}, {1, -1, -1}, {-1, -1, -1}};
// IEKF reduction terms (LIO rows = 12 Jacobian columns, h, selected): 78 x HTH upper triangle, 12 x H^T h, sum h^2, count
static __constant__ int8_t c_lio_a[96] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 5, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 8, 8, 8, 8, 9, 9, 9, 10, 10, 11, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 0, 0, 0, 0};
static __constant__ int8_t c_lio_b[96] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 3, 4, 5, 6, 7, 8, 9, 10, 11, 4, 5, 6, 7, 8, 9, 10, 11, 5, 6, 7, 8, 9, 10, 11, 6, 7, 8, 9, 10, 11, 7, 8, 9, 10, 11, 8, 9, 10, 11, 9, 10, 11, 10, 11, 11, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 13, 0, 0, 0, 0};
// term j of the normal equations = row[c_term_a[j]] * row[c_term_b[j]] with row = (J0..J5, e, selected)
static __constant__ int8_t c_term_a[32] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5, 0, 1, 2, 3, 4, 5, 6, 7, 0, 0, 0};
static __constant__ int8_t c_term_b[32] = {0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 2, 3, 4, 5, 3, 4, 5, 4, 5, 5, 6, 6, 6, 6, 6, 6, 6, 7, 0, 0, 0};
static __constant__ int8_t c_nearby[27][4] = {
  {0, 0, 0, 0},   {-1, 0, 0, 0},  {1, 0, 0, 0},   {0, 1, 0, 0},   {0, -1, 0, 0},  {0, 0, -1, 0},  {0, 0, 1, 0},
  {1, 1, 0, 0},   {-1, 1, 0, 0},  {1, -1, 0, 0},  {-1, -1, 0, 0}, {1, 0, 1, 0},   {-1, 0, 1, 0},  {1, 0, -1, 0},
  {-1, 0, -1, 0}, {0, 1, 1, 0},   {0, -1, 1, 0},  {0, 1, -1, 0},  {0, -1, -1, 0}, {1, 1, 1, 0},   {-1, 1, 1, 0},
  {1, -1, 1, 0},  {1, 1, -1, 0},  {-1, -1, 1, 0}, {-1, 1, -1, 0}, {1, -1, -1, 0}, {-1, -1, -1, 0}};

struct PoseF {
  float r[9];
  float t[3];
};

__device__ inline PoseF load_pose(const double* T) {
  PoseF p;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) p.r[i * 3 + j] = (float)T[i * 4 + j];  // trans.cast<float>()  laser_mapping.cc:602-603
    p.t[i] = (float)T[i * 4 + 3];
  }
  return p;
}

__device__ inline void transform(const PoseF& P, const float4& p, float (&q)[3]) {
#pragma unroll
  for (int a = 0; a < 3; a++) q[a] = (P.r[a * 3 + 0] * p.x + P.r[a * 3 + 1] * p.y) + P.r[a * 3 + 2] * p.z + P.t[a];
}

// ---- the LIO ObsModel's view of one scan point, shared by the search kernel (kernels.hip) and the effect cloud (lio_outputs.hip)
// p_body.norm() of the 81 pd2^2 test  laser_mapping.cc:631
__device__ inline float lio_body_norm(const float4& p) { return pcm_sqrtf_rn(p.x * p.x + p.y * p.y + p.z * p.z); }
// p_w = R_wl * p_body + t_wl with R_wl a float quaternion (Eigen _transformVector)  laser_mapping.cc:602-612
__device__ inline void lio_world_point(const float* q_wl, const float* t_wl, const float4& p, float (&q)[3]) {
  const float qx = q_wl[0], qy = q_wl[1], qz = q_wl[2], qw = q_wl[3];
  float uv[3] = {qy * p.z - qz * p.y, qz * p.x - qx * p.z, qx * p.y - qy * p.x};
  uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
  const float c3[3] = {qy * uv[2] - qz * uv[1], qz * uv[0] - qx * uv[2], qx * uv[1] - qy * uv[0]};
  q[0] = (p.x + qw * uv[0] + c3[0]) + t_wl[0];
  q[1] = (p.y + qw * uv[1] + c3[1]) + t_wl[1];
  q[2] = (p.z + qw * uv[2] + c3[2]) + t_wl[2];
}
// the default semantics' row test: a plane was found (x not NaN) and |p_body| > 81 pd2^2 at the world point q (:627-631); res = pd2
__device__ inline bool lio_row_selected(const float4& pl, const float (&q)[3], float pn_body, float& res) {
  bool sel = !(pl.x != pl.x);
  if (sel) {
    res = pl.x * q[0] + pl.y * q[1] + pl.z * q[2] + pl.w;
    sel = pn_body > 81.f * res * res;
  }
  return sel;
}

// running 5-best list: ascending distance, equal distances keep visit order
struct Best {
  float d[K];
  uint32_t i[K];
  float thr;   // min(d[K - 1], max_range^2): a candidate changes the list iff its distance is below this
  int m;       // candidates within max_range, at most K (= finite entries of d; set by best_finish)
};

__device__ inline void best_init(Best& b, float max_r2f) {
#pragma unroll
  for (int j = 0; j < K; j++) { b.d[j] = __builtin_inff(); b.i[j] = 0xffffffffu; }
  b.thr = max_r2f;
  b.m = 0;
}

// every in-range candidate enters the list while it has a free (infinite) slot, so the reference's
// count min(K, #in range) is the number of finite entries
__device__ inline void best_finish(Best& b) {
  int m = 0;
#pragma unroll
  for (int j = 0; j < K; j++) m += b.d[j] < __builtin_inff() ? 1 : 0;
  b.m = m;
}

// Offer one map point.  `max_r2f` is the smallest float >= max_range^2, so
// `d2 < max_r2f` is exactly the reference's `double(d2) < max_range * max_range`
// (ivox3d_node.hpp:162) without a double-precision compare per candidate.
// Sorted insert with strict '<' (an equal distance goes behind the entries
// already there = visit order); new d[j] = median(d2, d[j-1], d[j]).
// best_offer_d2 takes the squared distance ready-made (a caller that forms the distances of several candidates before the first
// insert: k_linearize_lists); +inf is never inserted (thr <= max_r2f <= +inf and the compare is strict).
__device__ inline void best_offer_d2(Best& b, float d2, uint32_t id, float max_r2f) {
  if (d2 < b.thr) {   // in range (d2 < max_r2f) and ahead of the current K-th (strict: an equal distance stays behind)
    {
      const bool c0 = d2 < b.d[0], c1 = d2 < b.d[1], c2 = d2 < b.d[2], c3 = d2 < b.d[3];
      b.i[4] = c3 ? b.i[3] : id;
      // distances are non-negative and never NaN here: unsigned integer min / max of the bit patterns order them
      // exactly and skip the NaN canonicalisation fminf / fmaxf carry
      b.d[4] = __uint_as_float(max(__float_as_uint(d2), __float_as_uint(b.d[3])));
      b.i[3] = c2 ? b.i[2] : (c3 ? id : b.i[3]);
      b.d[3] = __builtin_amdgcn_fmed3f(d2, b.d[2], b.d[3]);
      b.i[2] = c1 ? b.i[1] : (c2 ? id : b.i[2]);
      b.d[2] = __builtin_amdgcn_fmed3f(d2, b.d[1], b.d[2]);
      b.i[1] = c0 ? b.i[0] : (c1 ? id : b.i[1]);
      b.d[1] = __builtin_amdgcn_fmed3f(d2, b.d[0], b.d[1]);
      b.i[0] = c0 ? id : b.i[0];
      b.d[0] = __uint_as_float(min(__float_as_uint(d2), __float_as_uint(b.d[0])));
      b.thr = __uint_as_float(min(__float_as_uint(b.d[4]), __float_as_uint(max_r2f)));
    }
  }
}

__device__ inline void best_offer(Best& b, const float4& mp, const float (&q)[3], uint32_t id, float max_r2f) {
  const float dx = mp.x - q[0], dy = mp.y - q[1], dz = mp.z - q[2];
  const float d2 = dx * dx + dy * dy + dz * dz;  // distance2()  ivox3d_node.hpp:13-16
  best_offer_d2(b, d2, id, max_r2f);
}

// Per-lane search straight against the global structures (tiles whose voxel box
// does not fit the LDS grid): brick probe (re-used while consecutive cells stay in
// one brick) -> occupancy bit -> rank -> vox_start -> the voxel's points.
template <bool STATS>
__device__ inline void knn_global(const TargetView& tg, const float (&q)[3], int cx, int cy, int cz, int num_neighbors, float max_range_sq, Best& best,
                                  uint32_t& n_cand, uint32_t& n_probe) {
  BrickCursor cur;
  for (int g = 0; g < num_neighbors; g++) {
    const int v = voxel_rank<STATS>(tg, cur, cx + c_nearby[g][0], cy + c_nearby[g][1], cz + c_nearby[g][2], n_probe);
    if (v < 0) continue;
    uint32_t start, end;
    voxel_run(tg, (uint32_t)v, start, end);
    for (uint32_t k = start; k < end; k++) {
      const float4 mp = gload4(tg.pts + k);
      if (STATS) n_cand++;
      best_offer(best, mp, q, k, max_range_sq);
    }
  }
}

// ---- wave64 data-parallel primitives on the DPP path (no LDS round trip: __shfl_* compiles to ds_bpermute_b32, one LDS-latency
// hop per step).  gfx9 DPP controls: row_shr:n = 0x110 + n (shift inside a row of 16 lanes), row_bcast:15 = 0x142 (lane 15 of a
// row to the next row), row_bcast:31 = 0x143 (lane 31 to rows 2 and 3).  A lane without a source keeps `old`.
template <int CTRL, int ROW_MASK = 0xf>
__device__ inline int dpp_mov(int old, int src) { return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, 0xf, false); }

// inclusive prefix sum inside each half (lanes 0..31, 32..63) of the wave
__device__ inline uint32_t scan_add_half(uint32_t v) {
  int x = (int)v;
  x += dpp_mov<0x111>(0, x);
  x += dpp_mov<0x112>(0, x);
  x += dpp_mov<0x114>(0, x);
  x += dpp_mov<0x118>(0, x);
  x += dpp_mov<0x142, 0xa>(0, x);   // rows 1 and 3 add the total of rows 0 and 2
  return (uint32_t)x;
}
// inclusive prefix sum over the wave
__device__ inline uint32_t scan_add_wave(uint32_t v) {
  int x = (int)scan_add_half(v);
  x += dpp_mov<0x143, 0xc>(0, x);   // rows 2 and 3 add the total of the lower half
  return (uint32_t)x;
}
// minimum / maximum over the wave, returned to every lane
__device__ inline int wave_min_i32(int x) {
  x = min(x, dpp_mov<0x111>(x, x));
  x = min(x, dpp_mov<0x112>(x, x));
  x = min(x, dpp_mov<0x114>(x, x));
  x = min(x, dpp_mov<0x118>(x, x));
  x = min(x, dpp_mov<0x142, 0xa>(x, x));
  x = min(x, dpp_mov<0x143, 0xc>(x, x));
  return __builtin_amdgcn_readlane(x, 63);
}
__device__ inline int wave_max_i32(int x) {
  x = max(x, dpp_mov<0x111>(x, x));
  x = max(x, dpp_mov<0x112>(x, x));
  x = max(x, dpp_mov<0x114>(x, x));
  x = max(x, dpp_mov<0x118>(x, x));
  x = max(x, dpp_mov<0x142, 0xa>(x, x));
  x = max(x, dpp_mov<0x143, 0xc>(x, x));
  return __builtin_amdgcn_readlane(x, 63);
}

// ---- tail of a linearize tile: residual / Jacobian row of every lane -> 29 sums of the tile -> one partial row.
// e = n.(T p) + d (laser_mapping.cc:627-629), valid iff |p_body| > 81 e^2 (:631), left-perturbation Jacobian [ (q x n)^T , n^T ];
// products formed in double from the float values like h_x (esekfom.hpp:1687), 8 groups of 32 rows each summed in row order, then
// the groups in order: the fixed order k_finish_round continues.  All 256 threads call it; `smem` is 16-byte aligned LDS of at
// least kReduceLdsBytes that nobody else touches any more (the caller's last barrier lies behind every other use); two barriers inside.
constexpr int kReduceLdsBytes = 256 * 8 * 8 + 8 * kPartialStride * 8;
template <bool WRITE_PLANES>
__device__ inline void residual_and_reduce(const PairDesc& d, uint32_t i, uint32_t tile_x, bool live, const float4& pl, const float (&q)[3], float pn_body, void* smem) {
  double* const s_row = reinterpret_cast<double*>(smem);   // [256][8]: J0..J5, e, selected
  double* const s_grp = s_row + 256 * 8;                   // [8][32] group partials
  {
    float row[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
      bool sel = !(pl.x != pl.x);
      if (sel) {
        const float pd2 = pl.x * q[0] + pl.y * q[1] + pl.z * q[2] + pl.w;
        sel = pn_body > 81.f * pd2 * pd2;
        if (sel) {
          row[0] = q[1] * pl.z - q[2] * pl.y;
          row[1] = q[2] * pl.x - q[0] * pl.z;
          row[2] = q[0] * pl.y - q[1] * pl.x;
          row[3] = pl.x; row[4] = pl.y; row[5] = pl.z;
          row[6] = pd2;
          row[7] = 1.f;
        }
      }
      if (WRITE_PLANES) gstore4(d.planes + i, sel ? pl : make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f));   // the selected set, for trial passes / parity hooks
    }
    double2* dst = reinterpret_cast<double2*>(s_row + threadIdx.x * 8);
#pragma unroll
    for (int a = 0; a < 4; a++) dst[a] = make_double2((double)row[2 * a], (double)row[2 * a + 1]);
  }
  __syncthreads();
  {
    const int j = threadIdx.x & 31, g = threadIdx.x >> 5;
    double v = 0.0;
    if (j < kNumSums) {
      const int ia = c_term_a[j], ib = c_term_b[j];
      const double* r0 = s_row + (g * 32) * 8;
#pragma unroll 8
      for (int k = 0; k < 32; k++) v = fma(r0[k * 8 + ia], r0[k * 8 + ib], v);
    }
    s_grp[g * kPartialStride + j] = v;
  }
  __syncthreads();
  if (threadIdx.x < kNumSums) {
    double v = 0.0;
#pragma unroll
    for (int g = 0; g < 8; g++) v += s_grp[g * kPartialStride + threadIdx.x];
    gstore_d(d.partials + (size_t)tile_x * kPartialStride + threadIdx.x, v);
  }
}

// ---- tail of a jueying_lio measurement tile (laser_mapping.cc:674-698): the 16-float row of every lane (12 Jacobian columns, h,
// selected) -> the IEKF's HTH = h_x^T h_x and h_x^T h (esekfom.hpp:1687,1706): 92 sums per tile, formed in double, 8 groups of 32
// rows each summed in row order, then the groups in order, one partial row per tile for k_lio_finish.  The tail of k_lio_lists
// (neighbour_lists.hip).  Its TWIN is the `if constexpr (LIO)` block at the end of k_linearize (kernels.hip), statement for
// statement: called from there this function left that kernel its 96 VGPRs, 31 664 B of LDS and 5 waves but changed its scratch
// (56 -> 44 bytes per lane, another spill schedule), and the tile kernel is the yardstick of the LIO path, so it keeps its own
// text.  A change of the row or of the order of the sums goes to both.  `do_search`: this call matched (pl is the plane just
// fitted, ref_fit / ref_ok what esti_plane did under the reference semantics), else pl is the stored plane.  All 256 threads
// call it; `smem` is 16-byte aligned LDS of at least kLioReduceLdsBytes that nobody else touches any more; two barriers inside.
constexpr int kLioReduceLdsBytes = 256 * 16 * 4 + 8 * kLioStride * 8;
__device__ inline void lio_row_and_reduce(const PairDesc& d, const KernelParams& kp, uint32_t i, uint32_t tile_x, bool live, bool do_search, const float4& p, const float (&q)[3],
                                          float pn_body, const float4& pl, bool ref_fit, bool ref_ok, void* smem) {
  float* s_row = reinterpret_cast<float*>(smem);                      // [256][16]: 12 columns, h, selected
  double* s_grp = reinterpret_cast<double*>(s_row + 256 * 16);        // [8][96] group partials
  {
    float row[16];
#pragma unroll
    for (int a = 0; a < 16; a++) row[a] = 0.f;
    if (live) {
      bool sel;
      float res = 0.f;
      if (kp.lio_ref) {
        // the members of LaserMapping as they are: the flag and the plane of a point change only when a matching call
        // reaches them, and a selected point that fails the 81 pd2^2 test keeps its flag and the residual stored for its
        // index by an earlier call -- of this frame or of an older one (laser_mapping.cc:335-339, 616-636, 646-650)
        const uint32_t oi = kp.lio_ref == 2 ? __float_as_uint(p.w) : i;
        PCM_GLOBAL float* aux = (PCM_GLOBAL float*)d.lio_aux + 2 * (size_t)oi;
        res = aux[0];
        sel = aux[1] != 0.f;
        if (do_search) {
          sel = ref_fit && ref_ok;
          if (ref_fit) gstore4(d.planes + oi, pl);
        }
        if (sel) {
          const float pd2 = pl.x * q[0] + pl.y * q[1] + pl.z * q[2] + pl.w;
          const float pn = pn_body;
          if (pn > 81.f * pd2 * pd2) res = pd2;
        }
        aux[0] = res;
        aux[1] = sel ? 1.f : 0.f;
      } else {
        if (do_search) gstore4(d.planes + i, pl);                        // plane_coef_[i]; the residual test is re-evaluated every call
        sel = lio_row_selected(pl, q, pn_body, res);
      }
      {
        const float pd2 = res;
        if (sel) {
          const float* oR = d.lio.off_R;
          const float* Rt = d.lio.Rt;
          float pt[3], C[3];
#pragma unroll
          for (int a = 0; a < 3; a++) pt[a] = (oR[a * 3 + 0] * p.x + oR[a * 3 + 1] * p.y) + oR[a * 3 + 2] * p.z + d.lio.off_t[a];   // point_this
#pragma unroll
          for (int a = 0; a < 3; a++) C[a] = (Rt[a * 3 + 0] * pl.x + Rt[a * 3 + 1] * pl.y) + Rt[a * 3 + 2] * pl.z;               // C = R^T n
          row[0] = pl.x; row[1] = pl.y; row[2] = pl.z;
          row[3] = (0.f * C[0] + -pt[2] * C[1]) + pt[1] * C[2];                                                                 // A = skew(point_this) C
          row[4] = (pt[2] * C[0] + 0.f * C[1]) + -pt[0] * C[2];
          row[5] = (-pt[1] * C[0] + pt[0] * C[1]) + 0.f * C[2];
          if (kp.lio_extrinsic) {   // B = (skew(p_body) off_R^T) C ; then C
            const float S[9] = {0.f, -p.z, p.y, p.z, 0.f, -p.x, -p.y, p.x, 0.f};
#pragma unroll
            for (int a = 0; a < 3; a++) {
              float sm[3];
#pragma unroll
              for (int b = 0; b < 3; b++) sm[b] = (S[a * 3 + 0] * oR[b * 3 + 0] + S[a * 3 + 1] * oR[b * 3 + 1]) + S[a * 3 + 2] * oR[b * 3 + 2];
              row[6 + a] = (sm[0] * C[0] + sm[1] * C[1]) + sm[2] * C[2];
              row[9 + a] = C[a];
            }
          }
          row[12] = -pd2;    // ekfom_data.h(i) = -residual
          row[13] = 1.f;
        }
      }
    }
    float4* dst = reinterpret_cast<float4*>(s_row + threadIdx.x * 16);
#pragma unroll
    for (int a = 0; a < 4; a++) dst[a] = make_float4(row[4 * a], row[4 * a + 1], row[4 * a + 2], row[4 * a + 3]);
  }
  __syncthreads();
  {
    const int j = threadIdx.x & 31, g = threadIdx.x >> 5;
    const float* r0 = s_row + (g * 32) * 16;
#pragma unroll
    for (int tt = 0; tt < 3; tt++) {
      const int term = j + 32 * tt;
      if (term < kLioSums) {
        const int ia = c_lio_a[term], ib = c_lio_b[term];
        double v = 0.0;
#pragma unroll 8
        for (int k = 0; k < 32; k++) v = fma((double)r0[k * 16 + ia], (double)r0[k * 16 + ib], v);
        s_grp[g * kLioStride + term] = v;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kLioSums) {
    double v = 0.0;
#pragma unroll
    for (int g = 0; g < 8; g++) v += s_grp[g * kLioStride + threadIdx.x];
    gstore_d(d.partials + (size_t)tile_x * kLioStride + threadIdx.x, v);
  }
}

}  // namespace pcm
