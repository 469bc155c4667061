// brick_table.h -- the shared reader of the brick table (layout: pcm_device.h; built by voxel_hash.hip) for the point-to-plane
// kernels, LOAM, pclomp NDT and the list builds.  NOT the only one: the fast_gicp-family kernels (ndt.hip, gicp.hip) keep their own.
//
// A voxel lookup is: probe the linear-probed brick hash -> one occupancy bit of the brick's 512-bit mask -> rank prefix of the
// mask word + a popcount = the voxel's rank -> vox_start[rank], vox_start[rank + 1] = its run of points.  The kernels named
// above do it through the functions below.  The helpers keep the loads (gload_* accessors) and the integer arithmetic of the
// hand-written chains they replaced, in their order.
//
// Ranks are returned as int, -1 = no such voxel: a table has at most kMaxBrickSlots / 4 bricks of 512 voxels, so a rank stays
// below 2^29.
//
// These sites still read the table themselves and MUST BE EDITED TOGETHER WITH THIS FILE when the slot, key, mask or prefix
// format changes (why each was left: DESIGN.md section 27):
//   - ndt.hip: voxel_lookup (probe, bit, rank; its cursor is five reference arguments), ndt_offset + c_direct7;
//   - gicp.hip: scan_box, scan_all, the voxel-column segment loop of k_covariances, vg_lookup, c_vg_direct7;
//   - pclndt.hip, neighbour_leaves, the branch-free lambda `one`: its own bmask / bpref loads (the probe is brick_find).
#pragma once

#include "pcm_device.h"

namespace pcm {

__device__ inline uint64_t slot_key(const uint4& s) { return ((uint64_t)s.y << 32) | s.x; }

// find a brick in the linear-probed brick table: slot index (or ~0u) and its first voxel
template <bool STATS = false>
__device__ inline uint32_t brick_find(const TargetView& tg, int bx, int by, int bz, uint32_t& vox_base, uint32_t& n_probe) {
  const uint64_t key = pack_brick(bx, by, bz);
  uint32_t h = hash_coord(bx, by, bz) & tg.mask;
  for (;;) {
    const uint4 s = gload4u(&tg.bricks[h]);
    if (STATS) n_probe++;
    const uint64_t sk = slot_key(s);
    if (sk == key) { vox_base = s.z; return h; }
    if (sk == kEmptyKey) { vox_base = 0; return ~0u; }
    h = (h + 1) & tg.mask;
  }
}
__device__ inline uint32_t brick_find(const TargetView& tg, int bx, int by, int bz, uint32_t& vox_base) {
  uint32_t n_probe = 0;
  return brick_find<false>(tg, bx, by, bz, vox_base, n_probe);
}

// the same probe with both 16-byte halves of the slot in flight together: the brick's run of points (0, 0 when it is absent)
template <bool STATS = false>
__device__ inline uint32_t brick_find_points(const TargetView& tg, int bx, int by, int bz, uint32_t& pt_start, uint32_t& npts, uint32_t& n_probe) {
  const uint64_t key = pack_brick(bx, by, bz);
  uint32_t h = hash_coord(bx, by, bz) & tg.mask;
  pt_start = 0; npts = 0;
  for (;;) {
    const uint4 s0 = gload4u(&tg.bricks[h]);
    const uint4 s1 = gload4u(reinterpret_cast<const char*>(&tg.bricks[h]) + 16);
    if (STATS) n_probe++;
    const uint64_t sk = slot_key(s0);
    if (sk == key) { pt_start = s1.x; npts = s1.y; return h; }
    if (sk == kEmptyKey) return ~0u;
    h = (h + 1) & tg.mask;
  }
}

// occupied voxels of a mask word below bit `bit`
__device__ inline uint32_t bit_rank(uint32_t m, uint32_t bit) { return (uint32_t)__popc(m & ((1u << bit) - 1u)); }

// rank of voxel (vx, vy, vz) in the brick found in `slot`, or -1: one occupancy bit, the word's prefix, one popcount
__device__ inline int rank_in_brick(const TargetView& tg, uint32_t slot, uint32_t vox_base, int vx, int vy, int vz) {
  const uint32_t li = local_index(vx, vy, vz), w = li >> 5, bit = li & 31;
  const uint32_t m = gload_u(&tg.bmask[(size_t)slot * 16 + w]);
  if (!((m >> bit) & 1u)) return -1;
  return (int)(vox_base + gload_u16(&tg.bpref[(size_t)slot * 16 + w]) + bit_rank(m, bit));
}

// the points of voxel `rank`: two adjacent vox_start words
__device__ inline void voxel_run(const TargetView& tg, uint32_t rank, uint32_t& s, uint32_t& e) {
  s = gload_u(&tg.vox_start[rank]);
  e = gload_u(&tg.vox_start[rank + 1]);
}

// the last brick probed: re-used while consecutive cells stay in one brick
struct BrickCursor { int bx = 0x7fffffff, by = 0, bz = 0; uint32_t slot = ~0u, base = 0; };

// the slot of the brick of voxel (vx, vy, vz), or ~0u: a probe only when the voxel left the cursor's brick
template <bool STATS = false>
__device__ inline uint32_t brick_seek(const TargetView& tg, BrickCursor& c, int vx, int vy, int vz, uint32_t& n_probe) {
  const int bx = vx >> kBrickShift, by = vy >> kBrickShift, bz = vz >> kBrickShift;
  if (bx != c.bx || by != c.by || bz != c.bz) {
    c.slot = brick_find<STATS>(tg, bx, by, bz, c.base, n_probe);
    c.bx = bx; c.by = by; c.bz = bz;
  }
  return c.slot;
}
__device__ inline uint32_t brick_seek(const TargetView& tg, BrickCursor& c, int vx, int vy, int vz) {
  uint32_t n_probe = 0;
  return brick_seek<false>(tg, c, vx, vy, vz, n_probe);
}
// rank of voxel (vx, vy, vz) or -1
template <bool STATS = false>
__device__ inline int voxel_rank(const TargetView& tg, BrickCursor& c, int vx, int vy, int vz, uint32_t& n_probe) {
  if (brick_seek<STATS>(tg, c, vx, vy, vz, n_probe) == ~0u) return -1;
  return rank_in_brick(tg, c.slot, c.base, vx, vy, vz);
}
__device__ inline int voxel_rank(const TargetView& tg, BrickCursor& c, int vx, int vy, int vz) {
  uint32_t n_probe = 0;
  return voxel_rank<false>(tg, c, vx, vy, vz, n_probe);
}
// one-shot: a probe of its own
__device__ inline int voxel_rank(const TargetView& tg, int vx, int vy, int vz) {
  uint32_t base;
  const uint32_t slot = brick_find(tg, vx >> kBrickShift, vy >> kBrickShift, vz >> kBrickShift, base);
  if (slot == ~0u) return -1;
  return rank_in_brick(tg, slot, base, vx, vy, vz);
}

// Offset k of the DIRECT1 / 7 / 27 neighbourhoods (nO = 1, 7, 27) of pclomp NDT and of the list builds.  7: {0, +x, -x, +y, -y,
// +z, -z}, the order of getNeighborhoodAtPoint7 (voxel_grid_covariance_omp_impl.hpp:414-428) and of fast_gicp (ndt_cuda.cu:35-88).
// 27: the whole 3 x 3 x 3 block, x slowest, z fastest -- fast_gicp's DIRECT27 loops.  For pclomp's DIRECT26 the same 27 cells in
// that order are this project's reading of pcl::getAllNeighborCellIndices, whose header is not part of the reference tree (it may
// hold 26 cells, centre excluded, in another order): the oracle reads it the same way, parity with PCL itself is unpinned.
// The DIRECT7 / 27 order exists twice more, c_direct7 + ndt_offset (ndt.hip) and c_vg_direct7 (gicp.hip): a change goes to all three.
__device__ inline void direct_offset(int nO, int k, int& ox, int& oy, int& oz) {
  if (nO == 27) { ox = k / 9 - 1; oy = (k / 3) % 3 - 1; oz = k % 3 - 1; return; }
  ox = oy = oz = 0;
  if (k == 1) ox = 1; else if (k == 2) ox = -1; else if (k == 3) oy = 1; else if (k == 4) oy = -1; else if (k == 5) oz = 1; else if (k == 6) oz = -1;
}

}  // namespace pcm
