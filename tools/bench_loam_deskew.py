"""LOAM deskew benchmark (pcm_loam_frame_begin_deskew against pcm_loam_frame_begin): one ring-tagged scan to the LOAM source at
16 x 1800 and 128 x 1800, without deskew and with IMU / odometry tables of 50 and 500 entries, from host and from device input.
`zero500` is a 500-entry table of a body at rest: the deskewed points equal the raw ones, so the features and the share of sectors
that take the serial sort are those of `plain` and the difference is the cost of the deskew itself; with motion the ranges lose the
synthetic scan's 2 mm quantisation, fewer curvatures tie and fewer sectors take the serial sort, which moves the frame time by more
than the deskew costs (`serial_sector_fraction`).
Every variant is warmed up; a run is `--calls` back-to-back frames (each call ends in a stream synchronise) and the variants
alternate inside a round, so drift of the shared machine hits them alike; the figure is the median over `--runs` rounds of the
per-frame time.  `plain` is the undeskewed entry point of the same build in the same session (what tools/bench_loam_features.py
times).  Prints one JSON line.  Usage: python tools/bench_loam_deskew.py [--runs 7] [--calls 20] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    from pointcloud_slam_amd import loam
    import loam_deskew_ref as D
    synth_spin = importlib.import_module("pointcloud-slam_amd.synth_spin")
    tsc, gyro, vel = 1000.0, (0.2, 0.2, 1.0), (2.0, 0.5, 0.1)
    tables = {}
    for n in (50, 500):
        imu, odom = D.sampled_tables(tsc, (n - 1) / 0.15, 0.15, gyro, vel)
        tables[n] = loam.loam_deskew_tables(tsc, imu, odom)
        assert tables[n]["imu"].shape[0] == n and tables[n]["imu_available"]
    rest = np.zeros((500, 4))
    rest[:, 0] = tsc - 0.005 + 0.15 * np.arange(500) / 499
    tables["zero500"] = dict(time_scan_cur=tsc, imu=rest, odom=rest.copy(), imu_available=1)
    out = {"runs": a.runs, "calls_per_run": a.calls, "tables_in": "global memory (five rows per table, binary search over the prefix maximum)"}
    for n_scan in (16, 128):
        rec = np.ascontiguousarray(synth_spin.make_spin(0, n_scan=n_scan).records)
        out[f"points_{n_scan}x1800"] = int(rec.shape[0])
        for where in ("host", "device"):
            cloud = rec if where == "host" else torch.from_numpy(rec).to("cuda:0")
            regs = {k: pcm.LoamRegistration(0) for k in ("plain", "zero500", 50, 500)}
            serial = {k: [] for k in regs}

            def frame(k):
                if k == "plain":
                    r = regs[k].set_input_scan(cloud, n_scan=n_scan)
                else:
                    r = loam.loam_frame_begin_deskew(regs[k], cloud, tables[k], n_scan=n_scan)
                serial[k].append(r["sectors_serial"] / max(1, r["sectors"]))
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
                    times[k].append((time.perf_counter() - t) * 1e3 / a.calls)
            med = {k: float(np.median(v)) for k, v in times.items()}
            tag = f"{n_scan}x1800_{where}"
            out[f"plain_ms_{tag}"] = med["plain"]
            out[f"zero500_ms_{tag}"] = med["zero500"]
            out[f"deskew50_ms_{tag}"] = med[50]
            out[f"deskew500_ms_{tag}"] = med[500]
            out[f"serial_sector_fraction_{tag}"] = {str(k): float(np.mean(v)) for k, v in serial.items()}
            out[f"spread_ms_{tag}"] = {str(k): [float(min(v)), float(max(v))] for k, v in times.items()}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
