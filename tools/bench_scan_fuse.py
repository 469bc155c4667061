"""Scan-fusion benchmark (pcm_scan_fuse, LoamRegistration.frame_begin_fused): a 16 x 1800 and a 128 x 1800 LiDAR cloud (vendor
XYZIRT records, uint8 intensity) with 0, 1 and 3 depth clouds of 640 x 480, inputs in host memory and in device memory; median of
--runs after a warm-up.  Per configuration: fuse_ms (output in the context's buffer), fuse + frame_begin ms, the algorithmic bytes
(every input record read once + every output record written once) over fuse_ms as a fraction of the 6.29 TB/s an MI355X streams,
and the caller's path of today on the same inputs: the numpy restatement (tests/scan_fuse_ref.py) on the host, then frame_begin
with the fused host cloud.  The reference's node needs ROS and PCL and cannot be built here, so no reference time is reported.
Prints one JSON line.  Usage: python tools/bench_scan_fuse.py [--runs 7] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_S = 6.29e12


def median_ms(f, runs):
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    import scan_fuse_cases as K
    import scan_fuse_ref as R
    S = importlib.import_module("pointcloud-slam_amd.synth_fusion")
    out = {"runs": a.runs, "hbm_bytes_per_s": HBM_BYTES_PER_S}
    cams = [R.Depth(S.depth_cloud(20 + k, S.camera_T(k), 640 * 480, width=640, branches=False), S.camera_T(k), 0, 1000000 * (k + 1)) for k in range(3)]
    for rows in (16, 128):
        pts, row, _, _ = S.lidar_cloud(1, rows, 1800, nan_frac=0.05)
        pts[np.isinf(pts).any(axis=1)] = np.nan
        rec, lay = S.pack_rs_u8(pts, row, 3)
        P = K.default_params()
        P.pitch_table = np.arange(52, dtype=np.int32) % rows
        P.ring_below, P.ring_otherwise = 0, rows - 1
        pd = K.params_dict(P)
        fp = dict(n_scan=rows, horizon_scan=1800)
        for ncam in (0, 1, 3):
            segs = [R.LidarXYZIRT(rec, **lay)] + cams[:ncam]
            key = f"{rows}x1800_{ncam}cam"
            g = pcm.LoamRegistration(0)
            res = {}
            for place in ("host", "device"):
                api = [K.to_api(s, None if place == "host" else (lambda x: torch.from_numpy(x).cuda())) for s in segs]
                torch.cuda.synchronize()
                _, counts = g.fuse_scans(api, pd)          # warm-up (module load, allocations)
                g.frame_begin_fused(api, pd, **fp)
                res[f"fuse_ms_{place}"] = median_ms(lambda: g.fuse_scans(api, pd), a.runs)
                res[f"fuse_plus_frame_begin_ms_{place}"] = median_ms(lambda: g.frame_begin_fused(api, pd, **fp), a.runs)
            nbytes = sum(s.rec.nbytes for s in segs) + 32 * counts["n_out"]
            res.update(points_in=int(sum(counts["n_in"])), points_out=int(counts["n_out"]), algorithmic_bytes=int(nbytes))
            for place in ("host", "device"):
                res[f"hbm_fraction_{place}"] = nbytes / (res[f"fuse_ms_{place}"] * 1e-3) / HBM_BYTES_PER_S
            if not a.no_cpu:
                t = time.perf_counter()
                fused = R.fuse(segs, P)
                res["numpy_restatement_ms"] = (time.perf_counter() - t) * 1e3
                g.set_input_scan(fused.out, stride=32, intensity_offset=16, ring_offset=20, **fp)
                res["frame_begin_host_cloud_ms"] = median_ms(lambda: g.set_input_scan(fused.out, stride=32, intensity_offset=16, ring_offset=20, **fp), a.runs)
                res["todays_path_ms"] = res["numpy_restatement_ms"] + res["frame_begin_host_cloud_ms"]
            out[key] = res
    out["reference_node"] = "not built (needs ROS and PCL); no reference time"
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
