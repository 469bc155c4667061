"""The LOAM adapters (include/pcm_amd/registration.hpp) hand the library packed (x, y, z, intensity) records, not PCL points as they
lie in memory: pcl::PointXYZI keeps the padding of its xyz block as the fourth float and the intensity at byte 16 (the layout of
tests/stubs/pcl/point_types.h), and the library reads a record's fourth float as its intensity.  The adapter is compiled against
stand-ins of the few pcm_* calls it makes, which record what they were given, and run on the CPU: LoamScanToMap::setInputFeatures,
LoamKeyFrameMap::saveKeyFrame with clouds, and the unpacking of loopFindNearKeyframes.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <pcm_amd/registration.hpp>
#include <cstdio>
#include <cstring>
#include <memory>

// ---- stand-ins for the library: they check the records they receive -------------------------------------------------------
static int g_bad = 0, g_calls = 0;
static void check_records(const void* p, size_t n, size_t stride, float first_intensity) {
  g_calls++;
  if (stride != 16) { std::printf("stride %zu\n", stride); g_bad++; return; }
  const float* f = static_cast<const float*>(p);
  for (size_t i = 0; i < n; i++) {
    const float want[4] = {1.0f + i, 2.0f + i, 3.0f + i, first_intensity + i};
    if (std::memcmp(f + 4 * i, want, sizeof(want)) != 0) { std::printf("record %zu: %g %g %g %g\n", i, f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]); g_bad++; }
  }
}
extern "C" {
void pcm_default_config(pcm_config* c) { std::memset(c, 0, sizeof(*c)); }
pcm_ctx* pcm_create(int, const pcm_config*) { return reinterpret_cast<pcm_ctx*>(&g_calls); }
void pcm_destroy(pcm_ctx*) {}
const char* pcm_last_error(const pcm_ctx*) { return "stub"; }
void pcm_loam_default_params(pcm_loam_params* p) { std::memset(p, 0, sizeof(*p)); }
void pcm_loam_default_submap_params(pcm_loam_submap_params* p) { std::memset(p, 0, sizeof(*p)); }
int pcm_loam_set_source(pcm_ctx*, const void* corner, size_t nc, const void* surf, size_t ns, size_t stride, int, uint64_t) {
  check_records(corner, nc, stride, 100.0f); check_records(surf, ns, stride, 200.0f); return PCM_OK;
}
int pcm_loam_keyframe_add(pcm_ctx*, const float*, double, const void* corner, size_t nc, const void* surf, size_t ns, size_t stride, int) {
  check_records(corner, nc, stride, 100.0f); check_records(surf, ns, stride, 200.0f); return PCM_OK;
}
int pcm_loam_keyframe_count(pcm_ctx*) { return 3; }
static int g_gets = 0, g_nears = 0;
int pcm_loam_keyframe_get(pcm_ctx*, int, float*, size_t, float*, size_t, size_t* nc, size_t* ns) { g_gets++; *nc = 2; *ns = 3; return PCM_OK; }
int pcm_loam_submap_near(pcm_ctx*, int, int, int, float, float* out, size_t cap, size_t* n) {
  g_nears++;
  *n = 4;
  if (cap < 10) return PCM_ERR_INVALID_ARGUMENT;   // two key frames of 2 + 3 points inside [0, 3) around key 0 with searchNum 1
  for (int i = 0; i < 4; i++) { out[4 * i] = 1.0f + i; out[4 * i + 1] = 2.0f + i; out[4 * i + 2] = 3.0f + i; out[4 * i + 3] = 50.0f + i; }
  return PCM_OK;
}
}

using PointType = pcl::PointXYZI;
using Cloud = pcl::PointCloud<PointType>;
static std::shared_ptr<const Cloud> cloud(size_t n, float first_intensity) {
  auto c = std::make_shared<Cloud>();
  c->points.resize(n);
  for (size_t i = 0; i < n; i++) {
    PointType& q = c->points[i];
    q.x = 1.0f + i; q.y = 2.0f + i; q.z = 3.0f + i; q.pad = 1.0f; q.intensity = first_intensity + i; q.p1 = q.p2 = q.p3 = -7.0f;
  }
  return c;
}
int main() {
  pcm_amd::LoamScanToMap<PointType> loam(0);
  pcm_amd::LoamKeyFrameMap<PointType> keyframes(loam);
  auto corner = cloud(5, 100.0f), surf = cloud(9, 200.0f);
  loam.setInputFeatures(corner, surf);
  const float pose[6] = {0, 0, 0, 0, 0, 0};
  keyframes.saveKeyFrame(pose, 1.0, corner, surf);
  Cloud near;
  keyframes.loopFindNearKeyframes(near, 0, 1);
  int bad = g_bad;
  if (g_calls != 4) { std::printf("calls %d\n", g_calls); bad++; }
  if (g_nears != 1 || g_gets != 2) { std::printf("near calls %d, count queries %d\n", g_nears, g_gets); bad++; }   // one pass, sized from the counts
  if (near.points.size() != 4) bad++;
  for (size_t i = 0; i < near.points.size(); i++)
    if (near.points[i].x != 1.0f + i || near.points[i].intensity != 50.0f + i) bad++;
  std::printf("bad %d\n", bad);
  return bad ? 1 : 0;
}
'''


def test_adapter_passes_intensity_not_padding(tmp_path):
    src = tmp_path / "loam_adapter_intensity.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_adapter_intensity"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
