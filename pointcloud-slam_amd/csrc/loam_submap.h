// loam_submap.h -- which key frames make the surrounding submap: jueying_slam's extractNearby / extractCloud selection
// (mapOptmization.cpp:1153-1222), publishGlobalMap's (:555-583) and the key window of loopFindNearKeyframes (:972-1018), as plain C++ over the host mirror of
// the key poses.  K is at most some ten thousand and the work is microseconds, so it runs on the host in the API layer
// (loam_submap.hip); tests/test_loam_submap.py compiles this header with g++ and checks it against the numpy restatement
// (tests/loam_submap_ref.py).  Every float operation below is one IEEE operation in the order written (-ffp-contract=off).
//
// Pinned where the reference tree cannot pin it:
//   * FLANN's radius test is d2 < r2 with d2 = (dx^2 + dy^2) + dz^2 in float and r2 the float square of the radius;
//   * the radius search returns ascending (d2, index) (it only fixes the summation order inside a pose leaf);
//   * the VoxelGrid over the poses follows pcm_voxel_downsample: double sums in input order, leaves in index order.  The leaf's
//     intensity is the mean of integer key indices: sums below 2^24 are exact and the division is correctly rounded, so the
//     truncated key index is exact.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace pcm {
namespace loam {

struct KeyPose {
  float x, y, z;   // cloudKeyPoses3D
  double time;     // cloudKeyPoses6D.time
};

struct SubmapSelection {
  std::vector<int32_t> keys;   // key frame of every used entry, in list order (a key may appear more than once)
  int32_t num_near = 0;        // (a) key poses inside the radius
  int32_t num_pose_leaves = 0; // (b) leaves of the pose VoxelGrid
  int32_t num_skipped = 0;     // entries farther than the radius from the last key pose
  int32_t status = 0;          // 0, or -1: the pose VoxelGrid's index overflows (leaf too small)
};

// Parts (a) and (b), part (c) when recent (the key frames of the last `window` seconds before time_cur) and the skip test: the
// body the two selections below share.  K >= 1.
inline SubmapSelection select_entries(const KeyPose* kp, int K, float radius, float density, bool recent, double time_cur, double window) {
  SubmapSelection S;
  if (K <= 0) return S;
  const KeyPose& last = kp[K - 1];
  // (a) radiusSearch around the last key pose
  struct Near { float d2; int32_t id; };
  std::vector<Near> near;
  const float r2 = radius * radius;
  for (int i = 0; i < K; i++) {
    const float dx = kp[i].x - last.x, dy = kp[i].y - last.y, dz = kp[i].z - last.z;
    const float d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < r2) near.push_back({d2, (int32_t)i});
  }
  std::sort(near.begin(), near.end(), [](const Near& a, const Near& b) { return a.d2 != b.d2 ? a.d2 < b.d2 : a.id < b.id; });
  S.num_near = (int32_t)near.size();
  // (b) VoxelGrid(density) over (x, y, z, intensity = index): one entry per leaf, all four fields averaged
  struct Entry { float x, y, z, intensity; };
  std::vector<Entry> list;
  if (!near.empty()) {
    const float inv = 1.0f / density;
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (const Near& n : near) {
      const float p[3] = {kp[n.id].x, kp[n.id].y, kp[n.id].z};
      for (int a = 0; a < 3; a++) { if (p[a] < mn[a]) mn[a] = p[a]; if (p[a] > mx[a]) mx[a] = p[a]; }
    }
    // the cell count in double against 2^31, as vg::box (voxel_grid.h) does on the device (a NaN or infinite product fails the test too), and
    // the leaf coordinates inside the int range before they are converted
    double cells = 1.0;
    for (int a = 0; a < 3; a++) cells *= trunc((double)((mx[a] - mn[a]) * inv)) + 1.0;
    bool fits = cells <= 2147483647.0;
    for (int a = 0; a < 3; a++) fits = fits && fabsf(mn[a] * inv) < 2147483520.0f && fabsf(mx[a] * inv) < 2147483520.0f;
    if (!fits) { S.status = -1; return S; }
    int mb[3], xb[3];
    for (int a = 0; a < 3; a++) { mb[a] = (int)floorf(mn[a] * inv); xb[a] = (int)floorf(mx[a] * inv); }
    const int64_t div0 = (int64_t)xb[0] - mb[0] + 1, div1 = (int64_t)xb[1] - mb[1] + 1;
    struct Item { int64_t leaf; int32_t ord; };
    std::vector<Item> items(near.size());
    for (size_t j = 0; j < near.size(); j++) {
      const KeyPose& q = kp[near[j].id];
      const int64_t i0 = (int64_t)(floorf(q.x * inv) - (float)mb[0]), i1 = (int64_t)(floorf(q.y * inv) - (float)mb[1]),
                    i2 = (int64_t)(floorf(q.z * inv) - (float)mb[2]);
      items[j] = {i0 + i1 * div0 + i2 * div0 * div1, (int32_t)j};
    }
    std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.leaf != b.leaf ? a.leaf < b.leaf : a.ord < b.ord; });
    for (size_t s = 0; s < items.size();) {
      size_t e = s;
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      while (e < items.size() && items[e].leaf == items[s].leaf) {
        const int32_t id = near[(size_t)items[e].ord].id;
        acc[0] += (double)kp[id].x; acc[1] += (double)kp[id].y; acc[2] += (double)kp[id].z; acc[3] += (double)(float)id;
        e++;
      }
      const double m = (double)(e - s);
      list.push_back({(float)(acc[0] / m), (float)(acc[1] / m), (float)(acc[2] / m), (float)(acc[3] / m)});
      s = e;
    }
  }
  S.num_pose_leaves = (int32_t)list.size();
  // (c) every key frame of the last `window` seconds, newest first, with its exact index
  for (int i = K - 1; recent && i >= 0; --i) {
    if (time_cur - kp[i].time < window) list.push_back({kp[i].x, kp[i].y, kp[i].z, (float)i});
    else break;
  }
  // extractCloud / publishGlobalMap :578: pointDistance(entry, last) > radius skips the entry
  for (const Entry& e : list) {
    const float dx = e.x - last.x, dy = e.y - last.y, dz = e.z - last.z;
    const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    if (dist > radius) { S.num_skipped++; continue; }
    S.keys.push_back((int32_t)e.intensity);
  }
  return S;
}

// extractNearby + the skip test of extractCloud
inline SubmapSelection select_surrounding(const KeyPose* kp, int K, float radius, float density, double time_cur, double window) {
  return select_entries(kp, K, radius, density, true, time_cur, window);
}

// publishGlobalMap's selection (mapOptmization.cpp:555-583): extractNearby without the window of recent key frames
inline SubmapSelection select_global(const KeyPose* kp, int K, float radius, float density) {
  return select_entries(kp, K, radius, density, false, 0.0, 0.0);
}

// loopFindNearKeyframes: key - search_num .. key + search_num inside [0, K)
inline std::vector<int32_t> select_near(int K, int key, int search_num) {
  std::vector<int32_t> keys;
  for (int64_t i = -(int64_t)search_num; i <= (int64_t)search_num; ++i) {
    const int64_t k = (int64_t)key + i;
    if (k < 0 || k >= K) continue;
    keys.push_back((int32_t)k);
  }
  return keys;
}

}  // namespace loam
}  // namespace pcm
