"""cachePointCloud benchmark (pcm_loam_cloud_prepare / pcm_loam_frame_begin_cloud): organised 16 x 1800
(rslidar_16) and 128 x 1800 (rslidar_ruby) clouds of 32-byte message records without a time field, 5 % NaN records, is_dense = 0.
  prepare_device / prepare_host   pcm_loam_cloud_prepare alone into the context's buffer, from device and from host bytes;
  frame_cloud_host                pcm_loam_frame_begin_cloud from host bytes, with deskew tables of 50 entries;
  host_route                      what a caller had before: a VECTORISED numpy cachePointCloud (ring, time, NaN removal, packing of the
                                  48-byte records; not the reference's per-point loop, which would flatter the result) followed by
                                  pcm_loam_frame_begin_deskew from the host records; numpy_part is its numpy share alone.
Every variant is warmed up; a run is `--calls` back-to-back frames (each ends in a stream synchronise) and the variants alternate
inside a round, so drift of the shared machine hits them alike; the figure is the median over `--runs` rounds of the per-frame
time.  Prints one JSON line.  Usage: python tools/bench_loam_cloud.py [--runs 7] [--calls 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def numpy_cache_point_cloud(raw, height, width, ruby):
    """The RoboSense branch of cachePointCloud for the benchmark's message layout (x y z @0, uint8 intensity @12, ring @28, no time
    field), vectorised: 48-byte PointXYZIRT records of the finite points."""
    n = height * width
    xyz = raw[:, 0:12].copy().view(np.float32).reshape(n, 3)
    h, w = np.divmod(np.arange(n), width)
    inside = (h < height - 1) & (w < width - 1)
    ring = raw[:, 28:30].copy().view(np.uint16).reshape(n)
    if ruby:
        k = (h + 1) % 64
        k = np.where(k == 0, 64, k)
        t = 3.236 * ((k - 1).astype(np.float32) / np.float32(4.0)).astype(np.float64) * 1e-6 + w * 55.552 * 1e-6
        r = h
    else:
        t = h * 2.8 * 1e-6 + w * 55.5 * 1e-6
        r = np.where(h < 8, h, 15 - (h - 8))
    ring = np.where(inside, r.astype(np.uint16), ring)
    t = np.where(inside, t, 0.0)
    keep = np.isfinite(xyz).all(axis=1)
    m = int(keep.sum())
    rec = np.zeros((m, 48), np.uint8)
    rec[:, 0:12] = raw[keep, 0:12]
    rec[:, 12:16] = np.frombuffer(np.float32(1.0).tobytes(), np.uint8)
    rec[:, 16] = raw[keep, 12]
    rec[:, 24:32] = np.ascontiguousarray(t[keep]).view(np.uint8).reshape(m, 8)
    rec[:, 32:34] = np.ascontiguousarray(ring[keep]).view(np.uint8).reshape(m, 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    from pointcloud_slam_amd import capi, loam
    import loam_cloud_ref as R
    import loam_deskew_ref as D
    tsc = 1000.0
    imu, odom = D.sampled_tables(tsc, 49 / 0.15, 0.15, (0.2, 0.2, 1.0), (2.0, 0.5, 0.1))
    dk = loam.loam_deskew_tables(tsc, imu, odom)
    out = {"runs": a.runs, "calls_per_run": a.calls, "message": "32-byte records, x y z @0, uint8 intensity @12, ring @28, no time field, 5 % NaN, is_dense 0"}
    for n_scan, lidar in ((16, R.RSLIDAR_16), (128, R.RSLIDAR_RUBY)):
        width = 1800
        n = n_scan * width
        rng = np.random.default_rng(n_scan)
        nan_at = tuple(int(i) for i in rng.choice(n, n // 20, replace=False))
        raw, d = R.make_case(n_scan, width, 32, R.MAPPING, lidar, seed=n_scan, has_time=False, synth_time=True, nan_at=nan_at, scene="room")
        raw = np.ascontiguousarray(raw)
        cd = R.capi_desc(capi, d)
        rec = numpy_cache_point_cloud(raw, n_scan, width, lidar == R.RSLIDAR_RUBY)
        if n_scan == 16:   # the vectorised route makes the records the device makes
            g = pcm.LoamRegistration(0)
            got, _ = loam.loam_cloud_prepare(g, raw, cd, out="host")
            assert got.tobytes() == rec.tobytes()
        d_raw = torch.from_numpy(raw).to("cuda:0")
        fp = dict(n_scan=n_scan, horizon_scan=width)
        regs = {k: pcm.LoamRegistration(0) for k in ("prepare_device", "prepare_host", "frame_cloud_host", "host_route", "numpy_part")}

        def frame(k):
            if k == "prepare_device":
                loam.loam_cloud_prepare(regs[k], d_raw, cd)
            elif k == "prepare_host":
                loam.loam_cloud_prepare(regs[k], raw, cd)
            elif k == "frame_cloud_host":
                loam.loam_frame_begin_cloud(regs[k], raw, cd, dk, **fp)
            elif k == "host_route":
                loam.loam_frame_begin_deskew(regs[k], numpy_cache_point_cloud(raw, n_scan, width, lidar == R.RSLIDAR_RUBY), dk, **fp)
            else:
                numpy_cache_point_cloud(raw, n_scan, width, lidar == R.RSLIDAR_RUBY)
        times = {k: [] for k in regs}
        for k in regs:
            for _ in range(3):
                frame(k)
        for _ in range(a.runs):
            for k in regs:
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.calls):
                    frame(k)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t) * 1e3 / a.calls)
        tag = f"{n_scan}x1800"
        out[f"points_{tag}"] = n
        for k, v in times.items():
            out[f"{k}_ms_{tag}"] = float(np.median(v))
        out[f"spread_ms_{tag}"] = {k: [float(min(v)), float(max(v))] for k, v in times.items()}
        out[f"host_route_over_frame_cloud_{tag}"] = out[f"host_route_ms_{tag}"] / out[f"frame_cloud_host_ms_{tag}"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
