"""LOAM front-end benchmark (pcm_loam_frame_begin[_batch]): single-frame latency of one ring-tagged scan to the LOAM source
(projection, smoothness, occlusion, selection, the per-ring and the mapping VoxelGrids) at 16 x 1800 and 128 x 1800, frame_begin +
scan2map per frame, frames/s of pcm_loam_frame_begin_batch at B = 8 and 32 (16 x 1800), the serial-sector fraction, and the
numpy restatement (tests/loam_features_ref.py) on the same 16 x 1800 frame.  The reference's PCL nodes cannot be built here
(no PCL), so no reference time is reported.  Prints one JSON line.  Usage: python tools/bench_loam_features.py [--runs 7] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    import pointcloud_slam_amd as pcm
    synth_spin = importlib.import_module("pointcloud-slam_amd.synth_spin")
    out = {"runs": a.runs}
    scans = {n: [synth_spin.make_spin(s, n_scan=n) for s in range(2)] for n in (16, 128)}
    for n in (16, 128):
        g = pcm.LoamRegistration(0)
        recs = [f.records for f in scans[n]]
        g.set_input_scan(recs[0], n_scan=n)   # warm-up (module load, allocations)
        k = [0]
        serial = []

        def one():
            r = g.set_input_scan(recs[k[0] % 2], n_scan=n)
            serial.append(r["sectors_serial"] / max(1, r["sectors"]))
            k[0] += 1
        out[f"frontend_ms_{n}x1800"] = median_ms(one, a.runs)
        out[f"points_{n}x1800"] = int(recs[0].shape[0])
        out[f"serial_sector_fraction_{n}x1800"] = float(np.mean(serial))
    # frame_begin + scan2map of a 16 x 1800 frame against its scene's maps
    f = scans[16][0]
    g = pcm.LoamRegistration(0)
    g.set_input_target(f.corner_map, f.surf_map, tag=7)
    x0 = f.x_gt.copy()
    x0[3] += 0.3

    def both():
        g.set_input_scan(f.records)
        g.scan2map(x0)
    both()
    out["frame_begin_plus_scan2map_ms_16x1800"] = median_ms(both, a.runs)
    for B in (8, 32):
        regs = [pcm.LoamRegistration(0) for _ in range(B)]
        recs = [scans[16][i % 2].records for i in range(B)]
        pcm.loam_frame_begin_batch(regs, recs)
        ms = median_ms(lambda: pcm.loam_frame_begin_batch(regs, recs), a.runs)
        out[f"batch_frames_per_s_B{B}"] = B / (ms / 1e3)
    if not a.no_cpu:
        import loam_features_ref as R
        with tempfile.TemporaryDirectory() as d:
            srt = R.build_std_sort(d)
            t = time.perf_counter()
            R.extract(R.State(16), f.records, srt)
            out["numpy_restatement_ms_16x1800"] = (time.perf_counter() - t) * 1e3
    out["reference_pcl"] = "not built (no PCL on this platform); no reference time"
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
