"""ApproximateVoxelGrid benchmark (pcm_approx_voxel_downsample).  Three inputs of 16-byte records: a 16 x 1800 spinning scan of a
box room (column after column, as the sensor delivers it), a 100 k Livox-shaped scan (synth.livox_scan) and a 1 M-point map
(synth.sample_submap), each at leaf 0.1 m and 0.5 m, from host buffers and from device buffers.  In the same process, alternating
with it, pcm_voxel_downsample on the same input; and for the smallest input, once, the serial Python restatement
(tests/approx_voxel_ref.py).  Medians of --runs after a warm-up; host clocks around calls that end in a wait.
Usage: python tools/bench_approx_voxel.py [--runs 9] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEAVES = (0.1, 0.5)


def spinning_scan(rings=16, cols=1800):
    """ranges to the walls, floor and ceiling of a 40 x 30 x 6 m room from a sensor 1.8 m above the floor"""
    az = np.repeat(np.linspace(0.0, 2.0 * np.pi, cols, endpoint=False), rings)
    el = np.tile(np.radians(np.linspace(-15.0, 15.0, rings)), cols)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    lo, hi = np.array([-22.0, -13.0, -1.8]), np.array([18.0, 17.0, 4.2])
    with np.errstate(divide="ignore"):
        t = np.where(d > 0, hi / d, np.where(d < 0, lo / d, np.inf)).min(axis=1)
    p = np.zeros((rings * cols, 4), np.float32)
    p[:, :3] = d * t[:, None]
    p[:, 3] = np.tile(np.arange(rings), cols)
    return p


def inputs():
    import importlib
    synth = importlib.import_module("pointcloud-slam_amd.synth")
    scene = synth.scene_for_points(0, 1_000_000)
    return [("scan_16x1800", spinning_scan()),
            ("livox_100k", np.ascontiguousarray(synth.make_pair(0, 100_000, 20_000).scan[:, :4], np.float32)),
            ("map_1M", np.ascontiguousarray(synth.sample_submap(scene, 1_000_000, 0)[:, :4], np.float32))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "approx_voxel_bench.json"))
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    import approx_voxel_ref as AV
    capi = pcm.capi
    reg = pcm.P2PlaneRegistration(0)
    L, h = reg._L, reg.handle
    rows = []
    for i, (name, pts) in enumerate(inputs()):
        n = len(pts)
        host_out = np.zeros_like(pts)
        d_in, d_out = torch.from_numpy(pts).cuda(), torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for leaf in LEAVES:
            m, d, mv = C.c_size_t(), C.c_size_t(), C.c_size_t()
            calls = {
                "approx_host": lambda: reg._check(L.pcm_approx_voxel_downsample(h, pts.ctypes.data, n, 16, capi.MEM_HOST, leaf, host_out.ctypes.data, n, C.byref(m), C.byref(d))),
                "approx_device": lambda: reg._check(L.pcm_approx_voxel_downsample(h, d_in.data_ptr(), n, 16, capi.MEM_DEVICE, leaf, d_out.data_ptr(), n, C.byref(m), C.byref(d))),
                "voxel_grid_host": lambda: reg._check(L.pcm_voxel_downsample(h, pts.ctypes.data, n, 16, capi.MEM_HOST, leaf, host_out.ctypes.data, n, C.byref(mv))),
                "voxel_grid_device": lambda: reg._check(L.pcm_voxel_downsample(h, d_in.data_ptr(), n, 16, capi.MEM_DEVICE, leaf, d_out.data_ptr(), n, C.byref(mv))),
            }
            ts = {k: [] for k in calls}
            for f in calls.values():
                f()
            for _ in range(a.runs):      # alternating
                for k, f in calls.items():
                    t = time.perf_counter(); f(); ts[k].append((time.perf_counter() - t) * 1e3)
            row = {"input": name, "points": n, "leaf": leaf, "approx_records": m.value, "approx_dropped": d.value, "voxel_grid_cells": mv.value}
            for k, v in ts.items():
                row[k + "_ms"] = float(np.median(v))
                row[k + "_min_max_ms"] = [min(v), max(v)]
            if i == 0:
                t = time.perf_counter()
                runs, _ = AV.apply_filter(pts[:, :3], leaf)
                AV.means(pts, runs)
                row["python_restatement_once_ms"] = (time.perf_counter() - t) * 1e3
                assert len(runs) == m.value
            rows.append(row)
        del d_in, d_out
        torch.cuda.empty_cache()
    out = {"bench": "approx_voxel", "runs": a.runs, "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
