"""The C++ adapter (include/pcm_amd/registration.hpp) EXECUTED on the GPU box: a program written like the reference's call sites
(jueying_slam/src/localization.cpp:162-189,317-340; fast_gicp/src/align.cpp:61-99) drives pcm_amd::P2PlaneRegistration and
pclomp::NormalDistributionsTransform on a seeded pair and prints what it reads back; every number must equal the ctypes path's
bit for bit -- which checks the adapter's Eigen (column-major) <-> C ABI (row-major) conversions, its config hand-over and the
pointer-identity caching.  PCL / Eigen are the minimal stand-ins of tests/stubs (neither exists in the image).  ``-m gpu``."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#define PCM_AMD_PCLOMP_ALIASES
#include <pcm_amd/registration.hpp>
#include <cstdio>
#include <memory>
#include <vector>
using P = pcl::PointXYZ;
using Cloud = pcl::PointCloud<P>;
static std::shared_ptr<Cloud> load(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END); long bytes = ftell(f); fseek(f, 0, SEEK_SET);
  auto c = std::make_shared<Cloud>();
  c->points.resize(bytes / sizeof(P));
  if (fread(c->points.data(), sizeof(P), c->points.size(), f) != c->points.size()) exit(3);
  fclose(f);
  return c;
}
template <typename M> static void print(const char* tag, const M& m, int R, int C) {   // row by row: the order of the C ABI's arrays
  printf("%s", tag);
  for (int i = 0; i < R; i++) for (int j = 0; j < C; j++) printf(" %.17g", (double)m(i, j));
  printf("\n");
}
int main(int argc, char** argv) {
  auto tgt = load(argv[1]); auto src = load(argv[2]);
  float g[16];
  { FILE* f = fopen(argv[3], "rb"); if (!f || fread(g, 4, 16, f) != 16) return 4; fclose(f); }
  Eigen::Matrix4f guess;
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) guess(i, j) = g[i * 4 + j];
  {
    pcm_amd::P2PlaneRegistration<P, P> reg;
    reg.setNumNeighborCells(27);
    reg.setResolution(0.5);
    reg.setOptimizer(pcm_amd::LSQ_OPTIMIZER_TYPE::GaussNewton);
    reg.setMaximumIterations(64);
    reg.setInputTarget(tgt);
    reg.setInputSource(src);
    reg.setInputSource(src);   // pointer-identity cache (fast_gicp_impl.hpp:72-74): no second upload
    Cloud aligned;
    reg.align(aligned, guess);
    print("p2p_T", reg.getFinalTransformation(), 4, 4);
    print("p2p_H", reg.getFinalHessian(), 6, 6);
    printf("p2p_meta %d %d\n", reg.hasConverged() ? 1 : 0, reg.getFinalNumIteration());
    Eigen::Matrix<double, 6, 6> H; Eigen::Matrix<double, 6, 1> b;
    const double c = reg.evaluateCost(reg.getFinalTransformation(), &H, &b);
    printf("p2p_cost %.17g\n", c);
    print("p2p_evalH", H, 6, 6);
    print("p2p_evalb", b, 6, 1);
    printf("p2p_fitness %.17g\n", reg.getFitnessScore());
  }
  {
    pclomp::NormalDistributionsTransform<P, P> ndt;     // localization.cpp:162-189
    ndt.setTransformationEpsilon(0.01);
    ndt.setResolution(1.0);
    ndt.setNeighborhoodSearchMethod(pclomp::DIRECT7);
    ndt.setInputTarget(tgt);
    ndt.setInputSource(src);
    Cloud aligned;
    ndt.align(aligned, guess);                          // :317-340
    print("ndt_T", ndt.getFinalTransformation(), 4, 4);
    printf("ndt_meta %d %d\n", ndt.hasConverged() ? 1 : 0, ndt.getFinalNumIteration());
    printf("ndt_prob %.17g\n", ndt.getTransformationProbability());
    printf("ndt_fitness %.17g\n", ndt.getFitnessScore());
  }
  return 0;
}
'''


def test_adapter_program_runs_and_matches_ctypes(pcm, synth, tmp_path):
    p = synth.make_pair(5, 8000, 80000)
    d = str(tmp_path)
    p.submap.astype(np.float32).tofile(os.path.join(d, "map.bin"))
    p.scan.astype(np.float32).tofile(os.path.join(d, "scan.bin"))
    p.guess.astype(np.float32).tofile(os.path.join(d, "guess.bin"))
    lib = os.path.join(ROOT, "pointcloud-slam_amd", "libpcm_amd.so")
    exe = os.path.join(d, "adapter_run")
    inc = ["-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include")]
    subprocess.run(["g++", "-O1", "-std=c++17", "-x", "c++", "-", "-o", exe] + inc +
                   ["-L", os.path.dirname(lib), "-lpcm_amd", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--unresolved-symbols=ignore-in-shared-libs"],
                   input=SRC.encode(), check=True)
    out = subprocess.check_output([exe, os.path.join(d, "map.bin"), os.path.join(d, "scan.bin"), os.path.join(d, "guess.bin")], timeout=300).decode()
    got = {}
    for line in out.strip().splitlines():
        k, *v = line.split()
        got[k] = np.array([float(x) for x in v])

    g = pcm.P2PlaneRegistration(0, optimizer="GN", voxel_resolution=0.5, num_neighbors=27, max_iterations=64)
    g.set_input_target(p.submap); g.set_input_source(p.scan)
    r = g.align(p.guess)
    assert np.array_equal(got["p2p_T"].reshape(4, 4), r.T.astype(np.float64))
    assert np.array_equal(got["p2p_H"].reshape(6, 6), r.H)
    assert got["p2p_meta"].tolist() == [float(r.converged), float(r.iterations)]
    c, H, b, _ = g.evaluate_cost(r.T.astype(np.float64))
    assert got["p2p_cost"][0] == c and np.array_equal(got["p2p_evalH"].reshape(6, 6), H) and np.array_equal(got["p2p_evalb"], b)
    assert got["p2p_fitness"][0] == g.get_fitness_score(T=r.T)

    n = pcm.PclNdtRegistration(0, voxel_resolution=1.0, num_neighbors=7, translation_eps=0.01)
    n.set_input_target(p.submap); n.set_input_source(p.scan)
    rn = n.align(p.guess)
    assert np.array_equal(got["ndt_T"].reshape(4, 4), rn.T.astype(np.float64))
    assert got["ndt_meta"].tolist() == [float(rn.converged), float(rn.iterations)]
    assert got["ndt_fitness"][0] == n.get_fitness_score(T=rn.T)
