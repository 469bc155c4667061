"""The timing protocol of the reference's gicp_align (fast_gicp/src/align.cpp:51-104) on a synthetic pair: both clouds are
filtered by ApproximateVoxelGrid at 0.1 m on the device, as align.cpp:136-147 prepares them, and every method runs
  single          clear target, clear source, set target, set source, align -- once, then the fitness score
  100times        the same, 100 times
  100times_reuse  100 times: swap source and target, clear source, set target, set source, align, the two clouds trading places
                  (set_input_* carries a tag per cloud, which stands for the reference's pointer comparison)
for GICP, VGICP, VGICP_CUDA and NDT_CUDA with the settings their classes start with.  The source is the scan under the pair's
guess, so the alignment starts from identity as the reference's does.  Host clocks, as the reference's; the protocol is run
--runs times per method and the medians are reported.
Usage: python tools/bench_align_protocol.py [--runs 3] [--scan 20000] [--map 200000] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def protocol(reg, target, source):
    def once(t, s, tt, st):
        reg.set_input_target(t, tag=tt)
        reg.set_input_source(s, tag=st)
        return reg.align()

    t0 = time.perf_counter()
    reg.clear_target(); reg.clear_source()
    r = once(target, source, 1, 2)
    single = (time.perf_counter() - t0) * 1e3
    fitness = reg.get_fitness_score()
    t0 = time.perf_counter()
    for _ in range(100):
        reg.clear_target(); reg.clear_source()
        once(target, source, 1, 2)
    multi = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    t, s, tt, st = target, source, 1, 2
    for _ in range(100):
        reg.swap_source_and_target()
        reg.clear_source()
        once(t, s, tt, st)
        t, s, tt, st = s, t, st, tt
    reuse = (time.perf_counter() - t0) * 1e3
    return single, multi, reuse, fitness, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scan", type=int, default=20000)
    ap.add_argument("--map", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_protocol_bench.json"))
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    synth = importlib.import_module("pointcloud-slam_amd.synth")
    pygicp = importlib.import_module("pointcloud-slam_amd.pygicp")
    p = synth.make_pair(0, a.scan, a.map, density=60.0)
    G = p.guess.astype(np.float64)
    source = (p.scan[:, :3].astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
    target = np.ascontiguousarray(p.submap[:, :3], np.float32)
    want = p.T_gt @ np.linalg.inv(G)          # what the alignment from identity should find
    ctx = pcm.P2PlaneRegistration(0)
    t_dev, s_dev = torch.from_numpy(target).cuda(), torch.from_numpy(source).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t_f, _ = pygicp.approx_voxel_downsample(ctx, t_dev, 0.1)
    s_f, _ = pygicp.approx_voxel_downsample(ctx, s_dev, 0.1)
    filter_ms = (time.perf_counter() - t0) * 1e3
    rows = []
    for method, make in (("GICP", pcm.GicpRegistration), ("VGICP", pcm.VgicpRegistration), ("VGICP_CUDA", pcm.VgicpCudaRegistration), ("NDT_CUDA", pcm.NdtRegistration)):
        reg = make(0)
        protocol(reg, t_f, s_f)              # warm-up: allocations, first launches
        runs = [protocol(reg, t_f, s_f) for _ in range(a.runs)]
        r = runs[-1][4]
        D = np.linalg.inv(want) @ r.T64
        rows.append({"method": method, "single_ms": float(np.median([x[0] for x in runs])), "100times_ms": float(np.median([x[1] for x in runs])),
                     "100times_reuse_ms": float(np.median([x[2] for x in runs])), "fitness_score": float(runs[-1][3]), "iterations": int(r.iterations),
                     "converged": bool(r.converged), "translation_error_m": float(np.linalg.norm(D[:3, 3])),
                     "rotation_error_deg": float(np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))))})
        del reg
    out = {"bench": "align_protocol", "runs": a.runs, "device": torch.cuda.get_device_name(0), "leaf": 0.1,
           "target_points": [len(target), len(t_f)], "source_points": [len(source), len(s_f)], "filter_both_ms": filter_ms, "rows": rows}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
