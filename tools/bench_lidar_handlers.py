"""PointCloud2 handler benchmark (pcm_lidar_filter, pcm_lio_frame_begin_cloud): 16 x 1800, 64 x 1024 (point_filter_num 3) and
128 x 1800 spinning clouds; each handler with point times, the Velodyne and RoboSense handlers without (the yaw path), from host
and from device buffers, host output; lio_frame_begin_cloud whole (RoboSense, host cloud, 11 IMU poses, leaf 0.5).  Each figure is
the median of --runs samples after a warm-up, a sample being the mean of --inner calls that each end in a synchronisation.
In the same process, the only way there was before: the handler on the host -- the serial C++ loop of csrc/lidar_handlers.h built
with g++ -O2, which is the reference's own loop -- and set_input_source of its 48-byte records; --python-ref also times the
per-point Python restatement once.  The reference's node needs ROS and PCL and cannot be built here, so no reference time.
--trace runs nothing but the no-time handler on a device buffer (for one kernel trace of its own).
Prints one JSON line.  Usage: python tools/bench_lidar_handlers.py [--runs 7] [--inner 10] [--out FILE] [--trace]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [("16x1800", 16, 1800, None), ("64x1024_pfn3", 64, 1024, 3), ("128x1800", 128, 1800, None)]


def sample_ms(f, runs, inner):
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        for _ in range(inner):
            f()
        ts.append((time.perf_counter() - t) * 1e3 / inner)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def host_hook():
    """The header's serial loop as a shared object (what tests/test_lidar_handlers.py builds)."""
    so = os.path.join(tempfile.mkdtemp(prefix="lidar_bench_"), "hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "pointcloud-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lidar_handlers_hooks.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.lh_hook_filter.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_uint), C.c_char_p, C.c_size_t]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--python-ref", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    import lidar_handlers_cases as K
    import lidar_handlers_ref as R
    reg = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27)
    if a.trace:
        xyz, ring, col = K.spin_points(1, 128, 1800)
        rec, d = K.pack_case(R.RSLIDAR, xyz, ring, col, False, 1)
        d_rec, desc = torch.from_numpy(rec).cuda(), K.to_api(d)
        torch.cuda.synchronize()
        for _ in range(5):
            out, given = reg.lidar_filter(d_rec, desc)
        print(json.dumps({"trace": "rslidar no-time 128x1800 device", "points_in": len(rec), "points_out": len(out), "given": given}))
        return
    H = host_hook()
    out = {"runs": a.runs, "inner": a.inner}
    poses = K.poses(11, 0.1)
    for key, rings, cols, pfn in SHAPES:
        xyz, ring, col = K.spin_points(1, rings, cols)
        res = {"points_in": len(xyz)}
        for t, name in ((R.VELODYNE, "velodyne"), (R.RSLIDAR, "rslidar"), (R.OUSTER, "ouster"), (R.LIVOX_STD, "livox")):
            for given in ((True, False) if t in (R.VELODYNE, R.RSLIDAR) else (True,)):
                over = {} if pfn is None else {"point_filter_num": pfn}
                rec, d = K.pack_case(t, xyz, ring, col, given, 1, **over)
                desc = K.to_api(d)
                d_rec = torch.from_numpy(rec).cuda()
                torch.cuda.synchronize()
                tag = name + ("_given" if given else "_notime")
                r = {}
                for place, cloud in (("host", rec), ("device", d_rec)):
                    got, g = reg.lidar_filter(cloud, desc)          # warm-up (module load, arena growth)
                    assert g == given
                    r[place + "_ms"], r[place + "_min_ms"], r[place + "_max_ms"] = sample_ms(lambda: reg.lidar_filter(cloud, desc), a.runs, a.inner)
                r["points_out"] = len(got)
                # the way there was before: the handler on the host, then the 48-byte records go up
                flt = np.zeros((len(rec), 12), np.float32)
                m, gv, bad = C.c_size_t(), C.c_int(), C.c_uint()

                def host_handler():
                    H.lh_hook_filter(rec.ctypes.data, len(rec), C.addressof(desc), flt.ctypes.data, len(rec), C.byref(m), C.byref(gv), C.byref(bad), None, 0)
                host_handler()
                assert m.value == len(got)
                r["host_cpp_handler_ms"] = sample_ms(host_handler, a.runs, a.inner)[0]
                kept = flt[:m.value]
                reg.set_input_source(kept)
                r["set_source_48B_ms"] = sample_ms(lambda: reg.set_input_source(kept), a.runs, a.inner)[0]
                r["parent_path_ms"] = r["host_cpp_handler_ms"] + r["set_source_48B_ms"]
                if t == R.RSLIDAR:
                    end = dict(rot_xyzw=(0, 0, 0, 1.0), pos=(0, 0, 0), off_R_xyzw=(0, 0, 0, 1.0), off_T=(0, 0, 0))
                    n_scan = reg.lio_frame_begin_cloud(rec, desc, poses, leaf_size=0.5, **end)
                    r["frame_begin_cloud_host_ms"] = sample_ms(lambda: reg.lio_frame_begin_cloud(rec, desc, poses, leaf_size=0.5, **end), a.runs, a.inner)[0]
                    r["frame_begin_cloud_points"] = n_scan
                if a.python_ref:
                    tt = time.perf_counter()
                    R.handler(rec, d)
                    r["python_restatement_ms"] = (time.perf_counter() - tt) * 1e3
                res[tag] = r
        out[key] = res
    out["reference_node"] = "not built (needs ROS and PCL); no reference time"
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
