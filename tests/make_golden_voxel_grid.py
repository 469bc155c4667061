#!/usr/bin/env python3
"""Records tests/golden/voxel_grid_parent.json on the GPU, and names the cases it holds for the tests that read it.

The file pins what the VoxelGrid down-samplers computed on the commit before csrc/voxel_grid.h and csrc/voxel_grid.hip replaced
the separate copies in preprocess.hip, loam_features.hip and loam_submap.hip: per case the row count and the SHA-256 of the output
bytes.  tests/test_gpu_voxel_grid_pins.py compares today's results with it as equalities, so the anchor lies outside the code
under test (the oracle and numpy comparisons of the other suites allow 1 ulp and would not notice a changed bit).  It also holds
one SHA-256 of the generated inputs per group: when a generator changes, the tests say so instead of reporting a mismatch of the
clouds.  tests/test_voxel_grid_host.py runs the header's box and cell index on the same down-sampling inputs, without a GPU.
Re-recording with a later commit pins that commit, not the original.

  python tests/make_golden_voxel_grid.py        # rewrites tests/golden/voxel_grid_parent.json (needs the GPU)
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(ROOT, "tests", "golden", "voxel_grid_parent.json")
LEAF = 0.5
INT_FIELDS = ("start", "end", "col_ind", "neighbor_picked", "label")
_CACHE = {}


def _in_one_cell(rng, n, width=4):
    a = rng.uniform(0.0, 255.0, (n, width)).astype(np.float32)
    a[:, :3] = rng.uniform(1.05, 1.45, (n, 3)).astype(np.float32)   # cell (2, 2, 2) at leaf 0.5, away from its faces
    return a


def _cloud2000(width):
    """2000 points in [-4, 4)^3, one NaN, one +inf and one -inf among them; the other fields are noise"""
    rng = np.random.default_rng(11)
    a = rng.uniform(0.0, 255.0, (2000, 16)).astype(np.float32)
    a[:, :3] = rng.uniform(-4.0, 4.0, (2000, 3)).astype(np.float32)
    a[17, 1] = np.nan
    a[600, 0] = np.inf
    a[1999, 2] = -np.inf
    return np.ascontiguousarray(a[:, :width])


def downsample_cases():
    """name -> (points (N, F) float32, leaf): the inputs of reg.voxel_downsample"""
    if "vd" in _CACHE:
        return _CACHE["vd"]
    from test_preprocess import _scan_for_downsample
    rng = np.random.default_rng(7)
    cases = {"one_point": (np.array([[0.3, -1.2, 2.5, 9.0]], np.float32), LEAF)}
    for n in (64, 65):   # the boundary of the strided lane loop and the butterfly
        cases["one_cell_%d" % n] = (_in_one_cell(rng, n), LEAF)
    singles = np.zeros((5, 4), np.float32)
    singles[:, :3] = [[-3.2, 0.1, 0.1], [5.7, 5.7, -2.3], [0.2, -7.9, 1.1], [9.1, 0.3, 0.3], [1.2, 1.2, 6.6]]
    singles[:, 3] = [1, 2, 3, 4, 5]
    mixed = np.concatenate([_in_one_cell(rng, 300), singles])
    cases["one_cell_300_and_5_singletons"] = (mixed[rng.permutation(len(mixed))], LEAF)
    for w in (3, 4, 12, 16):
        cases["uniform_2000_width%d" % w] = (_cloud2000(w), LEAF)
    lattice = np.zeros((2000, 4), np.float32)
    lattice[:, :3] = (rng.integers(-6, 6, (2000, 3)) * LEAF).astype(np.float32)   # multiples of the leaf: points on cell faces
    lattice[:, 3] = rng.uniform(0.0, 255.0, 2000).astype(np.float32)
    cases["lattice_2000"] = (lattice, LEAF)
    bad = np.zeros((9, 4), np.float32)
    bad[:, 0] = np.nan
    bad[3:6, 0] = 1.0
    bad[3:6, 1] = np.inf
    bad[6:, 0] = 2.0
    bad[6:, 2] = -np.inf
    cases["all_non_finite"] = (bad, LEAF)
    cases["scan_seed3_leaf0.2"] = (_scan_for_downsample(3), 0.2)
    _CACHE["vd"] = cases
    return cases


def feature_scans():
    from test_gpu_loam_features import scan
    return [scan(0, 16).records, scan(1, 16, "shuffled").records]


def global_keyframes():
    import make_golden_loam_near as G
    return G.near_keyframes(7)


def digest(a):
    a = np.ascontiguousarray(a)
    return {"rows": int(a.shape[0]), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def arrays_digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def input_digests(groups=("downsample", "features", "global")):
    out = {}
    if "downsample" in groups:
        vd = downsample_cases()
        out["downsample"] = arrays_digest([vd[k][0] for k in sorted(vd)] + [np.float64([vd[k][1] for k in sorted(vd)])])
    if "features" in groups:
        out["features"] = arrays_digest(feature_scans())
    if "global" in groups:
        import make_golden_loam_near as G
        out["global"] = G.input_digest(global_keyframes())
    return out


def frame_digests(reg):
    """the frame a context holds after set_input_scan / loam_frame_begin_batch: the down-sampled corner and surf clouds (read back
    through a key frame made from the source), the ring-wise surf cloud and the integer arrays of feature_info"""
    info = reg.feature_info()
    reg.clear_keyframes()
    reg.add_keyframe(np.zeros(6, np.float32), 0.0)
    corner, surf = reg.get_keyframe(0)
    out = {"corner": digest(corner), "surf": digest(surf), "surf_scan": digest(info["surf_scan"])}
    for k in INT_FIELDS:
        out[k] = digest(info[k])
    return out


def compute_downsample(pcm):
    reg = pcm.P2PlaneRegistration(0)
    return {name: digest(reg.voxel_downsample(pts, leaf)) for name, (pts, leaf) in downsample_cases().items()}


def compute_features(pcm):
    scans = feature_scans()
    out = {}
    for i, rec in enumerate(scans):
        g = pcm.LoamRegistration(0)
        g.set_input_scan(rec)
        out["single/%d" % i] = frame_digests(g)
    regs = [pcm.LoamRegistration(0) for _ in scans]
    pcm.loam_frame_begin_batch(regs, scans)
    for i, g in enumerate(regs):
        out["batch_of_2/%d" % i] = frame_digests(g)
    g = pcm.LoamRegistration(0)
    g.set_input_scan(scans[0], mapping_corner_leaf=0.0, mapping_surf_leaf=0.0)
    out["single/0/mapping_leaves_0"] = frame_digests(g)
    return out


def compute_global(pcm):
    kf = global_keyframes()
    g = pcm.LoamRegistration(0)
    for k in range(len(kf.poses)):
        g.add_keyframe(kf.poses[k], kf.times[k], kf.corner[k], kf.surf[k])
    return {"global_map/default_leaf": digest(g.keyframe_global_map()), "global_map/leaf0": digest(g.keyframe_global_map(leaf=0.0)),
            "export_map/both": digest(g.export_map("both"))}


def load():
    with open(PATH) as f:
        return json.load(f)


def check_inputs(golden, group):
    assert input_digests((group,))[group] == golden["inputs"][group], (
        "the generators no longer produce the inputs that tests/golden/voxel_grid_parent.json was recorded with (%s): "
        "the recorded digests do not apply to these inputs" % group)


def main():
    import pointcloud_slam_amd as pcm
    out = {"inputs": input_digests(), "downsample": compute_downsample(pcm), "features": compute_features(pcm), "global": compute_global(pcm)}
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d down-sampled clouds, %d frames and %d global clouds" % (len(out["downsample"]), len(out["features"]), len(out["global"])))


if __name__ == "__main__":
    main()
