#!/usr/bin/env python3
"""Records tests/golden/lio_api_parent.json on the GPU, and names the cases it holds for tests/test_gpu_lio_api_pins.py.

The file pins what the jueying_lio entry points (pcm_obs_model, pcm_lio_update, pcm_map_incremental, pcm_lio_frame_begin,
pcm_lio_frame_begin_cloud, pcm_undistort) computed on the commit before they moved to csrc/lio_api.hip and came to share one
setup, one epilogue and one frame tail: per case the SHA-256 of the raw bytes of every output, through the C ABI.  The pins are
equalities, so the anchor lies outside the code under test.  It also holds a SHA-256 of the generated inputs: when a generator
changes, the tests say so instead of reporting a mismatch of the entry points.  PCM_AMD_LIBRARY names the build to record.
Re-recording with a later commit pins that commit, not the original.

  python tests/make_golden_lio_api.py [out.json]     # rewrites tests/golden/lio_api_parent.json (needs the GPU)
"""
import ctypes as C
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(ROOT, "tests", "golden", "lio_api_parent.json")
KW = dict(voxel_resolution=0.5, num_neighbors=27)
FOLLOW, LIO_REF = 128, 4          # PCM_FLAG_FOLLOWING_LISTS, PCM_FLAG_LIO_REFERENCE_SEMANTICS
PATHS = (("tiles", 0), ("lists", FOLLOW))
LEAVES = (0.0, 0.5)
_CACHE = {}


def _state(T_wl, off_rpy=(0.01, -0.02, 0.03), off_t=(0.1713, 0.0, 0.05925)):
    """the LIO state of a LiDAR at T_wl behind a non-trivial extrinsic: (rot xyzw, pos, off_R xyzw, off_T)"""
    from scipy.spatial.transform import Rotation as R
    offR = R.from_euler("xyz", off_rpy)
    Til = np.eye(4); Til[:3, :3] = offR.as_matrix(); Til[:3, 3] = off_t
    Twi = T_wl @ np.linalg.inv(Til)
    return R.from_matrix(Twi[:3, :3]).as_quat(), Twi[:3, 3].copy(), offR.as_quat(), np.asarray(off_t, np.float64)


def _nudged(T):
    from scipy.spatial.transform import Rotation as R
    Tk = T.copy()
    Tk[:3, 3] += (0.03, -0.02, 0.01)
    Tk[:3, :3] = Tk[:3, :3] @ R.from_rotvec([0.002, -0.001, 0.003]).as_matrix()
    return Tk


def inputs():
    """name -> tuple of arrays.  The map has 3000 points, the scans 257 and 16, the frames 600 records, the undistortion 300."""
    if _CACHE:
        return _CACHE
    S = importlib.import_module("pointcloud-slam_amd.synth")
    import lidar_handlers_cases as K
    import lidar_handlers_ref as LR
    import lio_iekf_ref as iref
    import lio_update_case as ucase
    rng = np.random.default_rng(41)
    scan, submap, T = S.corner_scene(257, 3000, seed=3, noise=0.01)
    _CACHE["scene"] = (submap[:, :3].copy(), scan[:, :3].copy(), T)
    _CACHE["states"] = tuple(np.concatenate(_state(M)) for M in (T, _nudged(T)))
    x0 = ucase.filter_state(ucase.perturb(T, dt=0.05, drot_deg=0.5))
    _CACHE["filter"] = (iref.state_to_vec(x0), np.diag(iref.INIT_P_DIAG))
    add = rng.uniform(0.5, 9.5, (40, 3)); add[:, 2] = rng.normal(0, 0.01, 40)
    _CACHE["insert"] = ((add + np.array([3.0, 4.0, -2.0])).astype(np.float32),)
    # a Livox-shaped driver message: 600 time-ordered records on 6 lines, a few with a noise tag; the points of a corner-scene scan
    fscan = S.corner_scene(600, 3000, seed=4, noise=0.01)[0]
    extras = {"offset_time": np.sort(rng.uniform(0.0, 0.099, 600)), "line": rng.integers(0, 6, 600), "reflectivity": rng.integers(1, 200, 600).astype(np.uint8),
              "tag": np.where(rng.random(600) < 0.03, 0x20, 0x10).astype(np.uint8)}
    _CACHE["livox"] = (S.custom_msg(fscan, extras),)
    # a PointCloud2 cloud of one handler type: 600 RoboSense records of a 16-ring spin with the driver's times
    rec, d = K.sized_case(LR.RSLIDAR, 600, 16, True)
    _CACHE["cloud"] = (np.ascontiguousarray(rec),)
    _CACHE["cloud_desc"] = d
    _CACHE["poses"] = (K.poses(3, 0.1),)
    # 300 PointXYZINormal records, time-ordered stamps [ms] in the curvature column
    r = np.zeros((300, 12), np.float32)
    r[:, :3] = rng.uniform(-8.0, 8.0, (300, 3)); r[:, 7] = rng.uniform(0, 150, 300); r[:, 9] = np.sort(rng.uniform(0.0, 99.0, 300))
    _CACHE["records"] = (r,)
    return _CACHE


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def input_digest():
    h = hashlib.sha256()
    for k in sorted(inputs()):
        if k == "cloud_desc":
            h.update(repr(inputs()[k]).encode())
            continue
        for a in inputs()[k]:
            a = np.ascontiguousarray(a)
            h.update(("%s%s%s" % (k, a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
    return h.hexdigest()


def _st(k):
    v = inputs()["states"][k]
    return v[0:4], v[4:7], v[7:11], v[11:14]


def _reg(pcm, scan, flags=0, **kw):
    submap = inputs()["scene"][0]
    g = pcm.P2PlaneRegistration(0, flags=flags, **KW, **kw)
    g.set_input_target(submap)
    g.set_input_source(scan)
    return g


def _obs_digest(g, n, ref, st, rematch):
    HTH, HTh, n_eff, sum_h2, valid = g.obs_model(*st, False, rematch)
    out = {"HTH": sha(HTH), "HTh": sha(HTh), "sum_h2": sha(np.float64([sum_h2])), "n_eff": int(n_eff), "valid": bool(valid), "search_path": list(g.lio_search_path())}
    planes = g.get_planes(n)
    if ref:
        # reference semantics: plane_coef_[i] is written only where esti_plane ran, the other rows are whatever the buffer held
        res, sel = g.get_lio_members(n)
        rows = np.abs(np.linalg.norm(np.nan_to_num(planes[:, :3].astype(np.float64), posinf=0, neginf=0), axis=1) - 1.0) < 1e-3
        rows &= sel
        out["members"] = sha(res, sel)
        out["planes"] = sha(np.nonzero(rows)[0], planes[rows])
    else:
        out["planes"] = sha(planes)
    return out


def compute_obs_model(pcm):
    """pcm_obs_model(rematch = 1) at the true state, then (rematch = 0) at a nudged one"""
    scan = inputs()["scene"][1]
    out = {}
    for n in (257, 16):
        for sort_source in (0, 1):
            for ref in (0, LIO_REF):
                for path, flag in PATHS:
                    g = _reg(pcm, scan[:n], flags=ref | flag, sort_source=sort_source)
                    name = "n%d/sort%d/ref%d/%s" % (n, sort_source, 1 if ref else 0, path)
                    out[name] = {"match": _obs_digest(g, n, ref, _st(0), True), "update": _obs_digest(g, n, ref, _st(1), False)}
    return out


def _update_digest(g, max_iter):
    x0, P0 = inputs()["filter"]
    r = g.lio_update(x0, P0, max_iter=max_iter)
    xv = np.concatenate([np.asarray(r.x[k], np.float64) for k, _ in g.LIO_STATE_FIELDS])
    out = {"x": sha(xv), "P": sha(r.P), "result": [int(r.iterations), int(r.rematches), int(r.valid_calls), int(r.t), int(r.n_eff_last), int(r.status)],
           "sum_h2_last": sha(np.float64([r.sum_h2_last])), "search_path": list(g.lio_search_path())}
    tr = []
    for k in range(r.iterations):
        t = g.lio_update_trace(k)
        tr.append(sha(np.concatenate([np.asarray(t["x"][f], np.float64) for f, _ in g.LIO_STATE_FIELDS]), np.int32([t["converge"], t["n_eff"]]), t["HTH"], t["HTh"], t["dx_"]))
    out["trace"] = tr
    return out, r


def compute_lio_update(pcm):
    scan = inputs()["scene"][1]
    out = {}
    for max_iter in (1, 4):
        for path, flag in PATHS:
            g = _reg(pcm, scan, flags=flag)
            out["iter%d/%s" % (max_iter, path)] = _update_digest(g, max_iter)[0]
    return out


def _grow_digest(g, st):
    added = g.map_incremental(*st, 0.5, True)
    t = g.get_target()
    return {"num_added": int(added), "target": sha(t), "points": len(t)}


def compute_map_incremental(pcm):
    """pcm_map_incremental after pcm_obs_model and after pcm_lio_update, and -- on lists -- with a pcm_target_insert that the lists
    followed in between: the neighbours of the matching call index entries that have moved since"""
    scan = inputs()["scene"][1]
    out = {}
    for path, flag in PATHS:
        g = _reg(pcm, scan, flags=flag)
        g.obs_model(*_st(0), False, True)
        out["after_obs/" + path] = _grow_digest(g, _st(0))
        g = _reg(pcm, scan, flags=flag)
        r = _update_digest(g, 4)[1]
        out["after_update/" + path] = _grow_digest(g, (r.x["rot"], r.x["pos"], r.x["off_R"], r.x["off_T"]))
    g = _reg(pcm, scan, flags=FOLLOW)
    g.obs_model(*_st(0), False, True)
    g.target_insert(inputs()["insert"][0])
    g.get_target()      # brings the map and the lists up to date
    out["after_obs_and_insert/lists"] = _grow_digest(g, _st(0))
    return out


def _frame_digest(g, n, st):
    return {"n_scan": int(n), "source": sha(g.get_source()), "world_dense": sha(g.lio_frame_world(*st, dense=True)), "world": sha(g.lio_frame_world(*st, dense=False)),
            "body": sha(g.lio_frame_body(*st))}


def _frames(pcm, begin, raw):
    import torch
    poses = inputs()["poses"][0]
    st = _st(0)
    out = {}
    for leaf in LEAVES:
        for np_name, pp in (("poses0", None), ("poses3", poses)):
            for mem in ("host", "device"):
                g = pcm.P2PlaneRegistration(0, **KW)
                msg = raw if mem == "host" else torch.from_numpy(raw.view(np.uint8).reshape(-1).copy()).cuda()
                out["leaf%g/%s/%s" % (leaf, np_name, mem)] = _frame_digest(g, begin(g, msg, pp, st, leaf), st)
    return out


def compute_frame_begin(pcm):
    msg = inputs()["livox"][0]
    return _frames(pcm, lambda g, m, pp, st, leaf: g.lio_frame_begin(m, pp, *st, num_scans=6, point_filter_num=1, blind=0.1, leaf_size=leaf), msg)


def compute_frame_begin_cloud(pcm):
    import lidar_handlers_cases as K
    rec = inputs()["cloud"][0]
    desc = K.to_api(inputs()["cloud_desc"])
    return _frames(pcm, lambda g, m, pp, st, leaf: g.lio_frame_begin_cloud(m, desc, pp, *st, leaf_size=leaf), rec)


def compute_undistort(pcm):
    import torch
    capi = pcm.capi
    rec, poses = inputs()["records"][0], inputs()["poses"][0]
    st = _st(0)
    g = pcm.P2PlaneRegistration(0, **KW)
    out = {"host": sha(g.undistort(rec.copy(), 9, poses, *st))}
    cs = capi.PcmLioState()
    cs.rot[:] = list(map(float, st[0])); cs.pos[:] = list(map(float, st[1])); cs.off_R[:] = list(map(float, st[2])); cs.off_T[:] = list(map(float, st[3]))
    d = torch.from_numpy(rec.copy()).cuda()
    rc = g._L.pcm_undistort(g._h, C.c_void_p(d.data_ptr()), C.c_size_t(len(rec)), C.c_size_t(48), C.c_size_t(36), capi.MEM_DEVICE, C.c_void_p(poses.ctypes.data), int(len(poses)), C.byref(cs))
    assert rc == capi.PCM_OK
    out["device"] = sha(d.cpu().numpy())
    return out


GROUPS = {"obs_model": compute_obs_model, "lio_update": compute_lio_update, "map_incremental": compute_map_incremental, "frame_begin": compute_frame_begin,
          "frame_begin_cloud": compute_frame_begin_cloud, "undistort": compute_undistort}


def load():
    with open(PATH) as f:
        return json.load(f)


def check_inputs(golden):
    assert input_digest() == golden["inputs"], (
        "the generators no longer produce the inputs that tests/golden/lio_api_parent.json was recorded with: "
        "the recorded digests do not apply to these inputs")


def main():
    import pointcloud_slam_amd as pcm
    out = {"inputs": input_digest()}
    for name, fn in GROUPS.items():
        out[name] = fn(pcm)
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded " + ", ".join("%d %s" % (len(out[k]), k) for k in GROUPS))


if __name__ == "__main__":
    main()
