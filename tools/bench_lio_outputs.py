"""Timing of the jueying_lio frame outputs and the saved map (pcm_lio_frame_world, pcm_lio_map_append, pcm_lio_map_export) against the
host route they replace (pcm_get_source + a numpy double transform + np.concatenate), on a 100 k-point dense frame and a 20 k-point
down-sampled frame, and the export of a 20 M-point log with and without a 0.1 m leaf.  Medians of RUNS timed calls after WARMUP
untimed ones; every timed call ends with the device idle.  Writes profiles/lio_outputs_bench.json (or --out PATH)."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RUNS, WARMUP = 9, 3
HBM_PEAK = 8.0e12          # bytes/s, MI355X specification
STATE = dict(rot=[0.0, 0.0, 0.38268343, 0.92387953], pos=[-40.0, -30.0, -2.0], off_R=[0.0, 0.0, 0.0, 1.0], off_T=[0.1713, 0.0, 0.05925])


def med(f, sync, runs=RUNS, warmup=WARMUP):
    ts = []
    for k in range(warmup + runs):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=float(np.median(ts)), min_max_ms=[min(ts), max(ts)])


def main():
    import torch
    import pointcloud_slam_amd as pcm
    import lio_outputs_ref as ref
    synth = importlib.import_module("pointcloud-slam_amd.synth")
    args = (STATE["rot"], STATE["pos"], STATE["off_R"], STATE["off_T"])
    g = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27)
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(5)
    out = dict(bench="lio_outputs", runs=RUNS, warmup=WARMUP, device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, rows=[])
    for label, n_raw, leaf, dense in (("dense_100k", 100000, 0.0, True), ("down_20k", 20000, 0.0, False)):
        msg = np.zeros(n_raw + 1, synth.LIVOX_POINT)
        xyz = rng.uniform(-50, 50, (n_raw + 1, 3)).astype(np.float32)
        msg["x"], msg["y"], msg["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        msg["offset_time"] = np.arange(n_raw + 1) * 900
        msg["reflectivity"] = np.arange(n_raw + 1) % 251
        msg["tag"] = 0x10
        msg["line"] = np.arange(n_raw + 1) % 6
        n = g.lio_frame_begin(msg, None, *args, num_scans=6, point_filter_num=1, blind=0.1, leaf_size=leaf)
        d = torch.zeros((n, 4), device="cuda")
        row = dict(frame=label, points=n)
        row["world_to_device"] = med(lambda: g.lio_frame_world(*args, dense=dense, out=d), sync)
        # the kernel alone: the appends are queued back to back and the stream drained once
        reps = 50
        g.lio_map_clear()
        for _ in range(3):
            g.lio_map_append(*args, dense=dense)
        g.lio_map_get(0, 1)

        def burst():
            g.lio_map_clear()
            for _ in range(reps):
                g.lio_map_append(*args, dense=dense)
            g.lio_map_get(0, 1)                                   # waits for the stream
        b = med(burst, sync)
        per = b["ms"] / reps
        row["append"] = dict(ms=per, burst_of=reps, burst_ms=b["ms"], burst_min_max_ms=b["min_max_ms"])
        useful = n * (16 + 16)                                     # 12 + 4 useful bytes in, 16 out
        moved = n * (48 + 16)                                      # whole 48-byte records cross the memory interface
        row["append_bytes_per_s"] = dict(useful=useful / (per * 1e-3), moved=moved / (per * 1e-3), of_hbm_peak_moved=moved / (per * 1e-3) / HBM_PEAK)
        # the host route: x, y, z down, the transform in double on the host, the concatenation (intensity cannot be reached this way)
        saved = [np.zeros((0, 4), np.float32)]

        def host_route():
            p = g.get_source()
            w = ref.body_to_world_d(STATE, p).astype(np.float32)
            saved[0] = np.concatenate([saved[0][:10 * n], np.concatenate([w, np.zeros((len(w), 1), np.float32)], axis=1)])
        row["host_route"] = med(host_route, sync)
        row["append_vs_host_route"] = row["host_route"]["ms"] / per
        out["rows"].append(row)
        g.lio_map_clear()
    # a 20 M-point log: 200 appends of the dense frame
    msg = np.zeros(100001, synth.LIVOX_POINT)
    xyz = rng.uniform(-60, 60, (100001, 3)).astype(np.float32)
    msg["x"], msg["y"], msg["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2] * 0.05
    msg["offset_time"] = np.arange(100001) * 900; msg["tag"] = 0x10; msg["line"] = np.arange(100001) % 6
    g.lio_map_clear()
    for k in range(200):
        pos = [STATE["pos"][0] + 3.0 * (k % 20), STATE["pos"][1] + 3.0 * (k // 20), STATE["pos"][2]]
        g.lio_frame_begin(msg, None, STATE["rot"], pos, STATE["off_R"], STATE["off_T"], num_scans=6, point_filter_num=1, blind=0.1, leaf_size=0.0)
        info = g.lio_map_append(STATE["rot"], pos, STATE["off_R"], STATE["off_T"], dense=True)
    d = torch.zeros((info["points"], 4), device="cuda")
    ex = dict(points=info["points"], growths=info["growths"], capacity=info["capacity"])
    ex["as_it_is_to_device"] = med(lambda: g.lio_map_export(out=d), sync, 7, 1)
    cells = [0]

    def leafy():
        cells[0] = g.lio_map_export(0.1, out=d)
    ex["leaf_0p1_to_device"] = med(leafy, sync, 7, 1)
    ex["leaf_0p1_cells"] = cells[0]
    ex["leaf_0p1_z_window_to_device"] = med(lambda: g.lio_map_export(0.1, -3.0, 0.0, out=d), sync, 7, 1)
    out["export_20M"] = ex
    print(json.dumps(out))
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "lio_outputs_bench.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
