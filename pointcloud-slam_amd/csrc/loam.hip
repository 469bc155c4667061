// loam.hip -- jueying_slam's LOAM scan-to-map optimisation on the device (mapOptmization.cpp:1255-1586; loam_step.h cites each piece).
//
// One iteration = two launches, queued for all iterations up front (no host round trip; a context that has converged returns at
// the top of every later launch):
//   k_loam_pass  one lane per scan feature (corner features first, then surf features: the row order of
//                combineOptimizationCoeffs :1421-1440), 64-lane workgroups.  Each lane maps its feature with the current pose, walks
//                the map cells that can hold a point within distance 1, keeps the 5 nearest (ties: smaller caller index) in
//                registers, fits the edge line or the plane, and forms its Jacobian row.  The products of A^T A, A^T b and the
//                selection / fitness counters are summed in double over the wave (xor butterfly) into one partial row per workgroup.
//   k_loam_step  one workgroup per context: the partial rows summed in block order, then loam_step() on one lane (6x6 solve,
//                iteration-0 eigen-decomposition and projector, pose update, convergence) -- the k_finish_round pattern.
// The neighbour search only has to be exact within distance 1: every test of the reference reads sqDis[4] < 1 or sqDis[0] <= 1,
// and a fifth neighbour beyond 1 rejects the point whatever it is.  The walk covers [q - 1.01, q + 1.01] on each axis (cells of
// >= 1 m: at most 4 per axis), so the result does not depend on the cell size.
#include "linearize_common.h"
#include "loam_device.h"

namespace pcm {
namespace loam {

namespace {

struct Knn5 {
  float d[5];
  uint32_t id[5];   // caller index (tie order)
  uint32_t k[5];    // position in the map's point array
};

// sorted insert by (d2, id); the caller offers only d2 <= 1
__device__ inline void knn_offer(Knn5& b, float d2, uint32_t id, uint32_t k) {
  bool lt[5];
#pragma unroll
  for (int j = 0; j < 5; j++) lt[j] = d2 < b.d[j] || (d2 == b.d[j] && id < b.id[j]);
  if (!lt[4]) return;
#pragma unroll
  for (int j = 4; j > 0; j--) {
    if (lt[j - 1]) { b.d[j] = b.d[j - 1]; b.id[j] = b.id[j - 1]; b.k[j] = b.k[j - 1]; }
    else if (lt[j]) { b.d[j] = d2; b.id[j] = id; b.k[j] = k; }
  }
  if (lt[0]) { b.d[0] = d2; b.id[0] = id; b.k[0] = k; }
}

__device__ inline int cell_lo(float v, float inv) {
  const float c = floorf(v * inv);
  return (int)fminf(fmaxf(c, -(float)(kCoordBias - 1)), (float)(kCoordBias - 1));
}

// every map point with d2 <= 1 of q is offered (COORD_FLOOR_MUL cells: floor(p * inv_res), monotone in p)
__device__ inline void knn_walk(const TargetView& tg, const float (&q)[3], Knn5& b) {
#pragma unroll
  for (int j = 0; j < 5; j++) { b.d[j] = __builtin_inff(); b.id[j] = 0xffffffffu; b.k[j] = 0u; }
  if (!(fabsf(q[0]) < 1e30f && fabsf(q[1]) < 1e30f && fabsf(q[2]) < 1e30f) || tg.num_points == 0) return;
  const float r = 1.01f, inv = tg.inv_res;
  int lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = cell_lo(q[a] - r, inv);
    hi[a] = min(cell_lo(q[a] + r, inv), lo[a] + 3);
  }
  BrickCursor cur;
  for (int x = lo[0]; x <= hi[0]; x++) {
    for (int y = lo[1]; y <= hi[1]; y++) {
      for (int z = lo[2]; z <= hi[2]; z++) {
        const int v = voxel_rank(tg, cur, x, y, z);
        if (v < 0) continue;
        uint32_t start, end;
        voxel_run(tg, (uint32_t)v, start, end);
        for (uint32_t k = start; k < end; k++) {
          const float4 mp = gload4(tg.pts + k);
          const float d2 = dist2(mp.x, mp.y, mp.z, q);
          if (d2 <= 1.f) knn_offer(b, d2, __float_as_uint(mp.w), k);
        }
      }
    }
  }
}

__global__ void k_tag_input_index(float4* __restrict__ pts, const uint32_t* __restrict__ order, uint32_t n) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) pts[k].w = __uint_as_float(order[k]);
}

__global__ void k_loam_init(const LoamDesc* __restrict__ descs) {
  const LoamDesc& d = descs[blockIdx.x];
  LoamState s;
  init_state(s, d.x0);
  *d.st = s;
}

__global__ void __launch_bounds__(kLanes) k_loam_pass(const LoamDesc* __restrict__ descs) {
  const LoamDesc& d = descs[blockIdx.y];
  const LoamState* st = d.st;
  if (st->done) return;
  const uint32_t n = d.n_c + d.n_s;
  if (blockIdx.x >= num_blocks(n)) return;
  const uint32_t i = blockIdx.x * kLanes + threadIdx.x;
  float row[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  double sel_c = 0.0, sel_s = 0.0, fit_c = 0.0, fit_cn = 0.0, fit_s = 0.0, fit_sn = 0.0;
  if (i < n) {
    const bool corner = i < d.n_c;
    float T[12], trig[6];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = st->T[k];
#pragma unroll
    for (int k = 0; k < 6; k++) trig[k] = st->trig[k];
    const TargetView& tg = d.map[corner ? 0 : 1];
    const float4 p = gload4(d.feats + i);
    float q[3];
    to_map(T, p.x, p.y, p.z, q);
    Knn5 b;
    knn_walk(tg, q, b);
    if (b.d[0] <= 1.f) {   // localization.cpp:689-693 / :790-794
      if (corner) { fit_c = (double)b.d[0]; fit_cn = 1.0; } else { fit_s = (double)b.d[0]; fit_sn = 1.0; }
    }
    Coeff c{0.f, 0.f, 0.f, 0.f, false};
    if (b.d[4] < 1.f) {    // pointSearchSqDis[4] < 1.0  :1273, :1370
      float nx[5], ny[5], nz[5];
#pragma unroll
      for (int j = 0; j < 5; j++) {
        const float4 mp = gload4(tg.pts + b.k[j]);
        nx[j] = mp.x; ny[j] = mp.y; nz[j] = mp.z;
      }
      c = corner ? edge_coeff(nx, ny, nz, q) : plane_coeff(nx, ny, nz, q);
    }
    if (d.coeff_out) {
      const float qnan = __builtin_nanf("");
      gstore4(d.coeff_out + i, c.selected ? make_float4(c.x, c.y, c.z, c.w) : make_float4(qnan, qnan, qnan, qnan));
    }
    if (d.nn_out) {
#pragma unroll
      for (int j = 0; j < 5; j++) d.nn_out[(size_t)i * 5 + j] = b.d[j] <= 1.f ? (int32_t)b.id[j] : -1;
    }
    if (c.selected) {
      jacobian_row(trig, p.x, p.y, p.z, c, row);
      if (corner) sel_c = 1.0; else sel_s = 1.0;
    }
  }
  double* out = d.partials + (size_t)blockIdx.x * kSums;
  const bool lane0 = threadIdx.x == 0;
  int t = kSumAtA;
#pragma unroll
  for (int a = 0; a < 6; a++) {
#pragma unroll
    for (int c = a; c < 6; c++) {
      const double v = wave_sum((double)row[a] * (double)row[c]);
      if (lane0) gstore_d(out + t, v);
      t++;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; a++) {
    const double v = wave_sum((double)row[a] * (double)row[6]);
    if (lane0) gstore_d(out + kSumAtB + a, v);
  }
  const double extra[6] = {sel_c, sel_s, fit_c, fit_cn, fit_s, fit_sn};
#pragma unroll
  for (int a = 0; a < 6; a++) {
    const double v = wave_sum(extra[a]);
    if (lane0) gstore_d(out + kSumCorner + a, v);
  }
}

__global__ void __launch_bounds__(kLanes) k_loam_step(const LoamDesc* __restrict__ descs, StepParams p) {
  const LoamDesc& d = descs[blockIdx.x];
  if (d.st->done) return;
  __shared__ double sums[kSums];
  const uint32_t nb = num_blocks(d.n_c + d.n_s);
  if (threadIdx.x < kSums) {
    double s = 0.0;
    for (uint32_t b = 0; b < nb; b++) s += gload_d(d.partials + (size_t)b * kSums + threadIdx.x);
    sums[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (d.sums_out) {
    for (int k = 0; k < kSums; k++) gstore_d(d.sums_out + k, sums[k]);
    return;
  }
  LoamState s = *d.st;
  loam_step(s, sums, p);
  *d.st = s;
}

}  // namespace

void launch_tag_input_index(hipStream_t stream, float4* pts, const uint32_t* order, uint32_t n) {
  if (n) k_tag_input_index<<<(n + 255) / 256, 256, 0, stream>>>(pts, order, n);
}

void launch_init(hipStream_t stream, const LoamDesc* d_descs, int n) { k_loam_init<<<n, 1, 0, stream>>>(d_descs); }

void launch_round(hipStream_t stream, const LoamDesc* d_descs, int n, uint32_t max_blocks, const StepParams& p) {
  k_loam_pass<<<dim3(max_blocks, (unsigned)n), kLanes, 0, stream>>>(d_descs);
  k_loam_step<<<n, kLanes, 0, stream>>>(d_descs, p);
}

}  // namespace loam
}  // namespace pcm
