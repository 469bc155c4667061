// nn_walk.h -- the exact nearest-neighbour walk over a built map (brick table + voxel columns), shared by the kernels that ask for
// one nearest map point per query: the GICP correspondence search, pcm_fitness_score and the GICP-BFGS correspondence step
// (gicp.hip), and point-to-point ICP (icp.hip).  Device code; every translation unit that includes it gets its own copy.
#pragma once

#include "pcm_device.h"
#include "brick_table.h"

namespace pcm {

namespace {

// Visit every map point whose voxel lies under the box q +- rb.  A point p with |p - q|_inf <= rb is
// visited: the voxel coordinate is monotone in the position.  Inside a brick the voxels of one (x, y)
// column are adjacent bits of one mask word and their points one contiguous run.
template <class F>
__device__ inline void scan_box(const TargetView& tg, int mode, const float (&q)[3], float rb, F&& visit) {
  const float lim = (float)(kCoordBias - 64) * tg.res;
  int lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = voxel_coord(fminf(fmaxf(q[a] - rb, -lim), lim), tg.res, tg.inv_res, mode);
    hi[a] = voxel_coord(fminf(fmaxf(q[a] + rb, -lim), lim), tg.res, tg.inv_res, mode);
  }
  for (int bx = lo[0] >> kBrickShift; bx <= (hi[0] >> kBrickShift); bx++) {
    const int x0 = (lo[0] > bx * 8 ? lo[0] : bx * 8) & 7, x1 = (hi[0] < bx * 8 + 7 ? hi[0] : bx * 8 + 7) & 7;
    for (int by = lo[1] >> kBrickShift; by <= (hi[1] >> kBrickShift); by++) {
      const int y0 = (lo[1] > by * 8 ? lo[1] : by * 8) & 7, y1 = (hi[1] < by * 8 + 7 ? hi[1] : by * 8 + 7) & 7;
      for (int bz = lo[2] >> kBrickShift; bz <= (hi[2] >> kBrickShift); bz++) {
        const int z0 = (lo[2] > bz * 8 ? lo[2] : bz * 8) & 7, z1 = (hi[2] < bz * 8 + 7 ? hi[2] : bz * 8 + 7) & 7;
        const uint64_t key = pack_brick(bx, by, bz);
        uint32_t h = hash_coord(bx, by, bz) & tg.mask;
        uint4 s;
        bool found = false;
        for (;;) {
          s = gload4u(&tg.bricks[h]);
          const uint64_t sk = slot_key(s);
          if (sk == key) { found = true; break; }
          if (sk == kEmptyKey) break;
          h = (h + 1) & tg.mask;
        }
        if (!found) continue;
        const uint32_t zbits = (1u << (z1 - z0 + 1)) - 1u;
        for (int x = x0; x <= x1; x++) {
          for (int y = y0; y <= y1; y++) {
            const uint32_t w = (uint32_t)(x * 2 + (y >> 2)), sh = (uint32_t)((y & 3) * 8 + z0);
            const uint32_t m = gload_u(&tg.bmask[(size_t)h * 16 + w]);
            const uint32_t sel = m & (zbits << sh);
            if (!sel) continue;
            const uint32_t vs = s.z + gload_u16(&tg.bpref[(size_t)h * 16 + w]) + (uint32_t)__popc(m & ((1u << sh) - 1u));
            const uint32_t ps = gload_u(&tg.vox_start[vs]), pe = gload_u(&tg.vox_start[vs + (uint32_t)__popc(sel)]);
            for (uint32_t p = ps; p < pe; p++) {
              const float4 c = gload4(tg.pts + p);
              const float ex = c.x - q[0], ey = c.y - q[1], ez = c.z - q[2];
              visit(p, ex * ex + ey * ey + ez * ez);
            }
          }
        }
      }
    }
  }
}

// Sweep of the whole brick table, skipping bricks whose box is provably farther than bound().
template <class B, class F>
__device__ inline void scan_all(const TargetView& tg, int mode, const float (&q)[3], B&& bound, F&& visit) {
  const float shift = mode == COORD_ROUND ? -0.5f : 0.5f;   // voxel c covers [(c + shift) res, (c + shift + 1) res]
  for (uint32_t h = 0; h <= tg.mask; h++) {
    const uint4 s = gload4u(&tg.bricks[h]);
    const uint64_t sk = slot_key(s);
    if (sk == kEmptyKey) continue;
    const int b[3] = {(int)(sk >> 36) - kBrickBias, (int)((sk >> 18) & 0x3ffff) - kBrickBias, (int)(sk & 0x3ffff) - kBrickBias};
    float lb = 0.f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float slack = 1e-3f * tg.res + 4e-6f * fabsf(q[a]);
      const float blo = ((float)(b[a] * 8) + shift) * tg.res - slack, bhi = ((float)(b[a] * 8 + 8) + shift) * tg.res + slack;
      const float d = fmaxf(fmaxf(blo - q[a], q[a] - bhi), 0.f);
      lb += d * d;
    }
    if (lb * 0.999f > bound()) continue;
    const uint4 s2 = gload4u(reinterpret_cast<const uint4*>(&tg.bricks[h]) + 1);   // pt_start, npts
    for (uint32_t p = s2.x; p < s2.x + s2.y; p++) {
      const float4 c = gload4(tg.pts + p);
      const float ex = c.x - q[0], ey = c.y - q[1], ez = c.z - q[2];
      visit(p, ex * ex + ey * ey + ez * ez);
    }
  }
}

__device__ inline bool finite3(const float (&q)[3]) { return isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]); }

// exact nearest map point of q: index or -1 when (double)d2 >= max_sq   (nearestKSearch(pt, 1) + the threshold of fast_gicp_impl.hpp:136)
__device__ inline int nearest1(const TargetView& tg, int mode, const float (&q)[3], double max_sq) {
  if (!finite3(q)) return -1;
  uint64_t best = ~0ull;
  auto visit = [&](uint32_t p, float d2) {
    const uint64_t key = ((uint64_t)__float_as_uint(d2) << 32) | p;
    if (d2 == d2 && key < best) best = key;
  };
  float r = tg.res;
  bool exact = false;
  for (;;) {
    best = ~0ull;
    scan_box(tg, mode, q, r * 1.0001f, visit);
    const float d2 = __uint_as_float((uint32_t)(best >> 32));
    if (best != ~0ull && d2 < r * r) { exact = true; break; }
    if ((double)r * (double)r >= max_sq) { exact = true; break; }   // nothing closer than the threshold exists
    const float rn = best != ~0ull ? sqrtf(d2) * 1.001f : 2.f * r;
    if (rn > 32.f * tg.res) break;
    r = rn;
  }
  if (!exact) {
    best = ~0ull;
    scan_all(tg, mode, q, [&]() { return best == ~0ull ? 3.0e38f : __uint_as_float((uint32_t)(best >> 32)); }, visit);
  }
  if (best == ~0ull) return -1;
  const float d2 = __uint_as_float((uint32_t)(best >> 32));
  return (double)d2 < max_sq ? (int)(uint32_t)best : -1;
}

}  // namespace

}  // namespace pcm
