"""LOAM global-map benchmark (pcm_loam_global_map / pcm_loam_map_export): K key frames of n_corner / n_surf points on a lawn-mower
with 12 m between key frames and between lanes, so that at the reference's defaults (radius 1000 m, pose density 10 m, leaf 1 m)
every key frame is its own pose leaf and all K are selected.  Per K, on one store in one process:
  (i)   keyframe_global_map at the defaults into a device buffer (in place) and to the host;
  (ii)  the route it replaces: keyframe_get per selected key frame, the float32 transform and the concatenation on the host,
        voxel_downsample of the upload;
  (iii) export_map of the whole store (device buffer, host) against the keyframe_get loop with the host transform;
  (iv)  the two gathers on the same entry table, alternating (pcm_loam_global_gather_ms: device events around the gather and its
        companion kernel), and that both leave the same box;
  (v)   the host time of allocating and releasing the pass's workspace, and its size.
Medians of --runs after a warm-up; host clocks around calls that end in a synchronise.  Prints one JSON line.
Usage: python tools/bench_loam_global.py [--runs 7] [--keyframes 200 2000] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32


def median_ms(f, runs):
    f()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def make_store(K, n_corner, n_surf, seed=0):
    """poses (K,6), and 8 distinct (corner, surf) body-frame cloud pairs used in turn"""
    rng = np.random.default_rng(seed)
    cols = int(math.ceil(math.sqrt(K)))
    poses = np.zeros((K, 6), F)
    for k in range(K):
        lane, j = divmod(k, cols)
        poses[k] = [rng.normal(0, 0.01), rng.normal(0, 0.01), (0.0 if lane % 2 == 0 else math.pi) + rng.normal(0, 0.02),
                    12.0 * (j if lane % 2 == 0 else cols - 1 - j) + 1.0, 12.0 * lane + 1.0, 5.0 + rng.normal(0, 0.03)]
    clouds = []
    for _ in range(8):
        pair = []
        for n in (n_corner, n_surf):
            c = rng.uniform(-8.0, 8.0, (n, 4)).astype(F)
            c[:, 2] *= 0.25
            c[:, 3] = rng.integers(0, 256, n).astype(F)
            pair.append(c)
        clouds.append(pair)
    return poses, clouds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--keyframes", type=int, nargs="+", default=[200, 2000])
    ap.add_argument("--n-corner", type=int, default=2000)
    ap.add_argument("--n-surf", type=int, default=8000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    import loam_ref
    capi = pcm.capi
    out = {"runs": a.runs, "n_corner": a.n_corner, "n_surf": a.n_surf}
    for K in a.keyframes:
        poses, clouds = make_store(K, a.n_corner, a.n_surf)
        g = pcm.LoamRegistration(0)
        for k in range(K):
            g.add_keyframe(poses[k], 100.0 + 0.7 * k, *clouds[k % 8])
        keys = g.keyframe_global_keys()
        assert len(keys) == K, (len(keys), K)
        mats = [loam_ref.pose_matrix(poses[k])[0].astype(F) for k in range(K)]
        N = K * (a.n_corner + a.n_surf)
        dev = torch.zeros((N, 4), dtype=torch.float32, device="cuda:0")
        row = {"points_in": N}

        def to_device():
            g.keyframe_global_map(out=dev)

        row["global_map_device_ms"] = median_ms(to_device, a.runs)
        row["points_out"] = g.keyframe_global_result.points_out
        host = np.zeros((row["points_out"], 4), F)
        row["global_map_host_ms"] = median_ms(lambda: g.keyframe_global_map(out=host), a.runs)
        vg = pcm.P2PlaneRegistration(0)

        def gathered(ks, which=(0, 1)):
            parts = []
            for k in ks:
                pair = g.get_keyframe(int(k))
                T = mats[int(k)]
                for w in which:
                    c = pair[w].copy()
                    c[:, :3] = c[:, :3] @ T[:3, :3].T + T[:3, 3]
                    parts.append(c)
            return np.concatenate(parts)

        replaced = [None]

        def old_route():
            replaced[0] = vg.voxel_downsample(gathered(keys), 1.0)

        row["replaced_route_ms"] = median_ms(old_route, a.runs)
        assert len(replaced[0]) == row["points_out"], (len(replaced[0]), row["points_out"])
        row["export_device_ms"] = median_ms(lambda: (g.export_map("both", out=dev), torch.cuda.synchronize()), a.runs)
        whole = np.zeros((N, 4), F)
        row["export_host_ms"] = median_ms(lambda: g.export_map("both", out=whole), a.runs)
        row["export_replaced_route_ms"] = median_ms(lambda: (gathered(range(K), (0,)), gathered(range(K), (1,))), a.runs)
        # the two gathers, alternating
        p = capi.PcmLoamGlobalParams()
        g._L.pcm_loam_default_global_params(C.byref(p))
        ms, wms, nbytes = C.c_float(0), C.c_float(0), C.c_size_t(0)
        boxes = [np.zeros(6, np.uint32), np.zeros(6, np.uint32)]
        t = {0: [], 1: []}
        w = []
        for i in range(2 * (a.runs + 1)):
            v = i % 2
            g._check(g._L.pcm_loam_global_gather_ms(g.handle, C.byref(p), v, C.byref(ms), boxes[v].ctypes.data, C.byref(nbytes), C.byref(wms)))
            if i >= 2:
                t[v].append(ms.value)
                w.append(wms.value)
        assert np.array_equal(boxes[0], boxes[1])
        row["gather_atomics_ms"] = float(np.median(t[0]))
        row["gather_partial_boxes_ms"] = float(np.median(t[1]))
        row["gather_atomics_all_ms"] = [round(x, 4) for x in t[0]]
        row["gather_partial_boxes_all_ms"] = [round(x, 4) for x in t[1]]
        row["workspace_bytes"] = nbytes.value
        row["workspace_alloc_release_ms"] = float(np.median(w))
        out["K_%d" % K] = row
        del g, dev
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
