"""CPU checks of pcl::ApproximateVoxelGrid's host side: pointcloud-slam_amd/csrc/approx_voxel.h, compiled with g++ through
tests/approx_voxel_hooks.cpp, gives the voxel, the history entry and the validity of the per-point restatement
(tests/approx_voxel_ref.py), and its emit-position rule (stable partition by entry, run heads, marks in input order, scan, slots --
what the kernels do lane-parallel) reproduces the loop's output order and run membership as equalities.  The pygicp module imports
without the library, names it when it is missing, and refuses an unknown method.  No GPU."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_voxel_ref as AV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloud-slam_amd", "csrc")
HOOKS = os.path.join(ROOT, "tests", "approx_voxel_hooks.cpp")
F = np.float32


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("approx_voxel") / "approx_voxel_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, HOOKS, "-o", so], check=True)
    L = C.CDLL(so)
    L.av_keys.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.av_keys.restype = None
    L.av_emit.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.POINTER(C.c_uint32)]
    L.av_emit.restype = C.c_uint32
    L.av_layout.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p]
    L.av_layout.restype = None
    return L


def header_keys(H, xyz, leaf):
    xyz = np.ascontiguousarray(xyz, F)
    n = len(xyz)
    ijk, h, valid = np.zeros((n, 3), np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    H.av_keys(xyz.ctypes.data, n, 3, leaf, ijk.ctypes.data, h.ctypes.data, valid.ctypes.data)
    return ijk, h, valid.astype(bool)


def key_inputs():
    rng = np.random.default_rng(1)
    wrap = (np.array([[400000, 0, 0], [0, 700000, 0], [0, 0, 600000], [400000, -700000, 600000], [-2000000, 2000000, -2000000], [299593, 697932, 507906]], np.float64)
            + 0.5).astype(F)
    return {
        "random": (AV.random_cloud(2, 5000, 0.0, 40.0), 0.1),
        "negative": (AV.random_cloud(3, 5000, -40.0, 0.0), 0.1),
        "mixed_signs_odd_leaf": (AV.random_cloud(4, 5000, -7.0, 7.0), 0.37),
        "wrap": (wrap, 1.0),                                                        # ix * 7171 leaves 32 bits
        "wrap_random": ((rng.integers(-2 ** 22, 2 ** 22, (5000, 3)).astype(np.float64) + 0.5).astype(F), 1.0),
        "invalid": (np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [0, -1e30, 0], [-2147483648.0, 0, 0], [2147483648.0, 0, 0],
                              [2147483520.0, -2147483520.0, 0.5], [3e9, 0, 0]], F), 1.0),
        "scaled_over_the_limit": (np.array([[3e8, 0, 0], [2e8, 0, 0], [-3e8, 0, 0]], F), 0.1),   # finite, but floorf(v * inv) passes 2^31
    }


@pytest.mark.parametrize("name", sorted(key_inputs()))
def test_key_of_the_header_is_the_restatements(H, name):
    xyz, leaf = key_inputs()[name]
    ijk, h, valid = header_keys(H, xyz, leaf)
    rijk, rh, rvalid = AV.keys(xyz, leaf)
    assert np.array_equal(valid, rvalid)
    assert np.array_equal(ijk[valid].astype(np.int64), rijk[valid]) and np.array_equal(h[valid].astype(np.int64), rh[valid])
    assert (h[~valid] == AV.ENTRIES).all()                     # the sort key of a dropped point
    if name == "invalid":
        assert list(valid) == [False] * 7 + [True, False]
    if name == "scaled_over_the_limit":
        assert list(valid) == [False, True, False]
    if name.startswith("wrap"):
        # the products do leave 32 bits, and the 32-bit reading agrees with exact arithmetic in the low nine bits
        assert (np.abs(rijk[valid].astype(object) * 7171).max() > 2 ** 31)
        wrapped = (rijk[valid, 0] * 7171 & 0xffffffff) + (rijk[valid, 1] * 3079 & 0xffffffff) + (rijk[valid, 2] * 4231 & 0xffffffff)
        assert np.array_equal((wrapped & 0xffffffff) & 511, h[valid])
    if name == "negative":
        assert (ijk[valid] < 0).all()


def header_slots(H, xyz, leaf):
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    slot, dropped = np.zeros(max(len(xyz), 1), np.uint32), C.c_uint32(77)
    runs = H.av_emit(xyz.ctypes.data, len(xyz), 3, leaf, slot.ctypes.data, C.byref(dropped))
    return runs, slot[:len(xyz)], dropped.value


@pytest.mark.parametrize("name", sorted(AV.small_cases()))
def test_emit_rule_reproduces_the_loop_on_the_small_cases(H, name):
    xyz, leaf, expected = AV.small_cases()[name]
    runs, dropped = AV.apply_filter(xyz, leaf)
    if expected is not None:
        assert runs == expected
    got_runs, slot, got_dropped = header_slots(H, xyz, leaf)
    assert (got_runs, got_dropped) == (len(runs), dropped)
    assert np.array_equal(slot, AV.slots(runs, len(xyz)))
    if name == "collision_aba":
        assert len(runs) == 3 and AV.distinct_voxels(xyz, leaf) == 2
    if name == "invalid_points":
        assert dropped == 3
    if name == "negative_and_wrap":
        assert len(runs) > AV.distinct_voxels(xyz, leaf) - 1 and dropped == 0


@pytest.mark.parametrize("name", ["long_runs", "short_runs"])
def test_emit_rule_reproduces_the_loop_on_the_clouds(H, name):
    xyz, leaf = getattr(AV, name)()
    runs, dropped = AV.apply_filter(xyz, leaf)
    got_runs, slot, got_dropped = header_slots(H, xyz, leaf)
    assert (got_runs, got_dropped) == (len(runs), dropped) and np.array_equal(slot, AV.slots(runs, len(xyz)))
    if name == "long_runs":
        assert sorted(len(r) for r in runs) == [65, 257, 5000]   # all three leave in the final flush, by entry
    else:
        assert len(runs) > AV.distinct_voxels(xyz, leaf)       # the approximate behaviour: a voxel leaves more than once


def test_scratch_layout(H):
    off = np.zeros(15, np.uint64)
    n, sort_tmp, scan_tmp = 1000, 5000, 300
    H.av_layout(n, sort_tmp, scan_tmp, off.ctypes.data)
    up = lambda x: (x + 255) & ~255
    want, at = [], 0
    for b in [4 * n] * 9 + [4 * 512] * 2 + [4 * 8, sort_tmp, scan_tmp]:
        want.append(at)
        at += up(b)
    assert list(off[:14]) == want and off[14] == at


def test_hooks_program_builds_and_agrees_with_its_loop(tmp_path):
    """the stand-alone form of the hooks (what a host sanitizer build runs), without a sanitizer here"""
    exe = str(tmp_path / "approx_voxel_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-DAV_MAIN", "-I", CSRC, HOOKS, "-o", exe], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert out.endswith(" 0 mismatches\n") and int(out.split()[0]) > 1000


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
def test_binding_declares_the_symbol():
    capi = importlib.import_module("pointcloud-slam_amd.capi")
    assert "pcm_approx_voxel_downsample" in capi.SYMBOLS
    text = open(os.path.join(CSRC, "exports.map")).read()
    assert "pcm_approx_voxel_downsample;" in text


def test_pygicp_imports_and_names_a_missing_library(tmp_path):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import importlib, numpy as np\n"
            "g = importlib.import_module('pointcloud-slam_amd.pygicp')\n"
            "capi = importlib.import_module('pointcloud-slam_amd.capi')\n"
            "assert capi._LIB is None\n"
            "try:\n"
            "    g.downsample(np.zeros((4, 3)), 0.1)\n"
            "except capi.PcmError as e:\n"
            "    print('PcmError', e.code, e)\n" % ROOT)
    env = dict(os.environ, PCM_AMD_LIBRARY=str(tmp_path / "no_such_libpcm_amd.so"))
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, check=True).stdout.decode()
    assert out.startswith("PcmError -3") and "libpcm_amd.so is not built" in out


def test_align_points_signature_and_unknown_method(capsys):
    import inspect
    g = importlib.import_module("pointcloud-slam_amd.pygicp")
    p = inspect.signature(g.align_points).parameters
    assert list(p)[:11] == ["target", "source", "method", "downsample_resolution", "k_correspondences", "max_correspondence_distance", "voxel_resolution",
                            "num_threads", "neighbor_search_method", "neighbor_search_radius", "initial_guess"]
    defaults = {k: v.default for k, v in p.items()}
    assert (defaults["method"], defaults["downsample_resolution"], defaults["k_correspondences"], defaults["max_correspondence_distance"]) == \
        ("GICP", -1.0, 15, sys.float_info.max)
    assert (defaults["voxel_resolution"], defaults["num_threads"], defaults["neighbor_search_method"], defaults["neighbor_search_radius"]) == (1.0, 0, "DIRECT1", 1.5)
    cloud = np.zeros((10, 3))
    with pytest.raises(ValueError, match="unknown registration method 'ICP'"):
        g.align_points(cloud, cloud, method="ICP")
    captured = capsys.readouterr()
    assert captured.out == "" and captured.err == ""
    with pytest.raises(ValueError):
        g.align_points(np.zeros((10, 4)), cloud)
