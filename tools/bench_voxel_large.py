"""VoxelGridLarge benchmark (pcm_voxel_downsample_large).  The input is shaped like an exported map: K key frames of 10 000 points
(16 x 16 x 4 m each) on a lawn-mower with 12 m between key frames and lanes, key frame after key frame, in a device buffer.
Per size, in one process:
  (a) a leaf that does not overflow: the new call against pcm_voxel_downsample on the same buffers, alternating, and the spread of
      pcm_voxel_downsample's own times;
  (b) leaves that overflow: time per call, pieces, depth, levels, host waits, workspace bytes; for the smallest size also the
      route it replaces, once: the read-back and the numpy restatement (tests/voxel_grid_large_ref.py) on the host.
Medians of --runs after a warm-up; host clocks around calls that end in a wait.  The split of a call into kernels, and with it
the box pass at one piece and at many (c), comes from a kernel trace of --trace-only (one call per leaf, no timing).
Usage: python tools/bench_voxel_large.py [--runs 7] [--keyframes 200 2000] [--out FILE] [--trace-only]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIT_LEAF = 1.0
OVERFLOW_LEAVES = (0.02, 0.005, 0.002, 0.001)


def make_map(torch, K, per_frame=10000, seed=0):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    cols = int(math.ceil(math.sqrt(K)))
    k = torch.arange(K, device="cuda:0")
    lane, j = k // cols, k % cols
    cx = 12.0 * torch.where(lane % 2 == 0, j, cols - 1 - j).float() + 1.0
    cy = 12.0 * lane.float() + 1.0
    pts = torch.rand((K, per_frame, 4), generator=g, device="cuda:0", dtype=torch.float32)
    pts[:, :, 0] = pts[:, :, 0] * 16.0 - 8.0 + cx[:, None]
    pts[:, :, 1] = pts[:, :, 1] * 16.0 - 8.0 + cy[:, None]
    pts[:, :, 2] = pts[:, :, 2] * 4.0 + 3.0
    pts[:, :, 3] = torch.floor(pts[:, :, 3] * 256.0)
    return pts.reshape(K * per_frame, 4).contiguous()


def times_ms(f, runs):
    f()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--keyframes", type=int, nargs="+", default=[200, 2000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_large_bench.json"))
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import ctypes as C
    import torch
    import pointcloud_slam_amd as pcm
    import voxel_grid_large_ref as VL
    capi = pcm.capi
    reg = pcm.P2PlaneRegistration(0)
    rows = []
    for K in a.keyframes:
        src = make_map(torch, K)
        n = src.shape[0]
        dst = torch.zeros_like(src)
        torch.cuda.synchronize()
        if a.trace_only:
            for leaf in (FIT_LEAF,) + OVERFLOW_LEAVES:
                reg.voxel_downsample_large(src, leaf, out=dst)
            continue
        row = {"keyframes": K, "points": n}
        m = C.c_size_t()

        def plain():
            reg._check(reg._L.pcm_voxel_downsample(reg.handle, src.data_ptr(), n, 16, capi.MEM_DEVICE, FIT_LEAF, dst.data_ptr(), n, C.byref(m)))

        def large(leaf=FIT_LEAF):
            return reg.voxel_downsample_large(src, leaf, out=dst)

        plain(); large()
        tp, tl = [], []
        for _ in range(a.runs):      # alternating
            t = time.perf_counter(); plain(); tp.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter(); large(); tl.append((time.perf_counter() - t) * 1e3)
        cells, r = large()
        assert cells == m.value and (r.pieces, r.depth, r.levels) == (1, 0, 1)
        row["fit"] = {"leaf": FIT_LEAF, "cells": cells, "voxel_downsample_ms": float(np.median(tp)), "voxel_downsample_min_max_ms": [min(tp), max(tp)],
                      "voxel_downsample_large_ms": float(np.median(tl)), "voxel_downsample_large_min_max_ms": [min(tl), max(tl)],
                      "ratio": float(np.median(tl) / np.median(tp)), "host_waits": r.host_waits, "workspace_bytes": r.workspace_bytes}
        row["overflow"] = []
        for leaf in OVERFLOW_LEAVES:
            ts = times_ms(lambda: large(leaf), a.runs)
            cells, r = large(leaf)
            e = {"leaf": leaf, "ms": float(np.median(ts)), "min_max_ms": [min(ts), max(ts)], "cells": cells, "pieces": r.pieces, "depth": r.depth, "levels": r.levels,
                 "host_waits": r.host_waits, "workspace_bytes": r.workspace_bytes, "workspace_bytes_per_point": r.workspace_bytes / n}
            if K == min(a.keyframes) and leaf == OVERFLOW_LEAVES[1]:
                t = time.perf_counter()
                host = src.cpu().numpy()
                t1 = time.perf_counter()
                want = VL.apply_filter(host, leaf)
                e["host_route_once_ms"] = {"read_back": (t1 - t) * 1e3, "numpy_restatement": (time.perf_counter() - t1) * 1e3}
                e["host_route_cells"] = len(want)
            row["overflow"].append(e)
        rows.append(row)
        del src, dst
        torch.cuda.empty_cache()
    if a.trace_only:
        return
    out = {"bench": "voxel_large", "runs": a.runs, "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
