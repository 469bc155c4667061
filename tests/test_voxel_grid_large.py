"""CPU checks of pcl::VoxelGridLarge's host side: vg::split of pointcloud-slam_amd/csrc/voxel_grid.h (compiled with g++ through
tests/voxel_grid_large_hooks.cpp) decides as the numpy restatement does -- axis, mid and leaf / cut / stuck as equalities --, and the
recursive restatement (tests/voxel_grid_large_ref.py) gives what an independent statement without recursion gives.  No GPU.

2^31 - 1 is prime and an extent is a float32 truncated plus one, so no box has exactly 2^31 - 1 cells (it would need the extent
2^31 - 2 on one axis, which float32 does not hold).  The bound is tested on its two sides: 1386 x 4681 x 331 = 2^31 - 2 cells, the
largest product a box can have without overflowing, is a leaf piece; 2048 x 1024 x 1024 = 2^31 cells is cut."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import voxel_grid_large_cases as K
import voxel_grid_large_ref as VL
from test_voxel_grid_host import f2ord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloud-slam_amd", "csrc")
F = np.float32


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("voxel_grid_large") / "voxel_grid_large_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, os.path.join(ROOT, "tests", "voxel_grid_large_hooks.cpp"), "-o", so],
                   check=True)
    L = C.CDLL(so)
    L.vgl_split.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    return L


def decision_cases():
    """name -> (min, max, leaf, expected kind, expected axis)"""
    c = {
        "x_longest": ((0, 0, 0), (3000, 2000, 100), 0.05, VL.SPLIT, 0),
        "y_longest": ((-10, -20, 5), (1990, 2980, 105), 0.05, VL.SPLIT, 1),
        "z_longest": ((0, 0, 0), (100, 200, 3000), 0.05, VL.SPLIT, 2),
        "tie_dx_dy": ((0, 0, 0), (3000, 3000, 100), 0.05, VL.SPLIT, 2),
        "tie_dx_dz": ((0, 0, 0), (3000, 100, 3000), 0.05, VL.SPLIT, 2),
        "tie_dy_dz": ((0, 0, 0), (100, 3000, 3000), 0.05, VL.SPLIT, 2),
        "tie_all": ((0, 0, 0), (3000, 3000, 3000), 0.05, VL.SPLIT, 2),
        "tie_flat_z": ((0, 0, 7), (3000, 3000, 7), 0.05, VL.STUCK, 2),
        "adjacent_floats": ((16777218.0, 0, 0), (16777220.0, 1, 1), 1e-6, VL.STUCK, 0),     # mid rounds to even: the maximum
        "adjacent_floats_cut": ((16777216.0, 0, 0), (16777218.0, 1, 1), 1e-6, VL.SPLIT, 0),  # mid rounds to even: the minimum
        "extent_overflows_float": ((-3e38, 0, 0), (3e38, 1, 1), 1.0, VL.STUCK, 0),
        "cells_2p31_minus_2": ((0, 0, 0), (1385.5, 4680.5, 330.5), 1.0, VL.LEAF, -1),
        "cells_2p31": ((0, 0, 0), (2047.5, 1023.5, 1023.5), 1.0, VL.SPLIT, 0),
        "no_overflow": ((0, 0, 0), (10, 10, 10), 0.05, VL.LEAF, -1),
        "one_point": ((5, 5, 5), (5, 5, 5), 0.05, VL.LEAF, -1),
    }
    rng = np.random.default_rng(3)
    for i in range(200):
        mn = rng.uniform(-5000, 5000, 3)
        ext = 10.0 ** rng.uniform(-2, 4.5, 3)
        if i % 5 == 0:
            ext[rng.integers(3)] = ext[rng.integers(3)]   # ties
        c["random_%d" % i] = (mn, mn + ext, float(10.0 ** rng.uniform(-2.5, 0)), None, None)
    return c


def words(mn, mx):
    return np.concatenate([f2ord(np.asarray(mn, F)), f2ord(np.asarray(mx, F))])


def test_split_of_the_header_is_the_restatements(H):
    assert 1386 * 4681 * 331 == 2 ** 31 - 2 and 2048 * 1024 * 1024 == 2 ** 31
    kinds = set()
    for name, (mn, mx, leaf, kind, axis) in decision_cases().items():
        want = VL.decide(np.asarray(mn, F), np.asarray(mx, F), leaf)
        ax, mid = C.c_int(-7), C.c_float(-7.0)
        mm = words(mn, mx)
        got = H.vgl_split(mm.ctypes.data, leaf, C.byref(ax), C.byref(mid))
        assert (got, ax.value) == (want[0], want[1]), name
        assert np.array_equal(np.array([mid.value], F).view(np.uint32), np.array([want[2]], F).view(np.uint32)), name
        if kind is not None:
            assert (got, ax.value) == (kind, axis), name
        kinds.add(got)
    assert kinds == {VL.LEAF, VL.SPLIT, VL.STUCK}
    # an empty piece is a leaf piece
    empty = np.array([0xffffffff] * 3 + [0] * 3, np.uint32)
    ax, mid = C.c_int(0), C.c_float(1.0)
    assert H.vgl_split(empty.ctypes.data, 0.05, C.byref(ax), C.byref(mid)) == VL.LEAF and ax.value == -1


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("name", sorted(K.dyadic_cases()))
def test_restatement_is_the_independent_statement(name):
    pts, leaf = K.dyadic_cases()[name]
    cells, pieces, depth = K.reference(name)
    other, other_pieces, other_depth = VL.independent(pts, leaf)
    assert cells.shape == other.shape and np.array_equal(bits(cells), bits(other))
    assert (pieces, depth) == (other_pieces, other_depth)
    if name == "only_non_finite":
        assert len(cells) == 0 and pieces == 0
    elif name != "n_1":
        assert pieces > 1 and depth >= 1
    if name == "site_4096":
        assert depth >= 10 and pieces >= 256       # about a dozen levels, hundreds of pieces
    from oracle.loader import voxel_downsample
    if name != "only_non_finite" and name != "n_1":
        with pytest.raises(OverflowError):
            voxel_downsample(pts, leaf)


def test_straddled_cell_gives_a_centroid_per_piece():
    pts, leaf, first, second = K.straddle()
    inv = F(1.0) / F(leaf)
    assert np.array_equal(np.floor(first[:3] * inv), np.floor(second[:3] * inv))      # one lattice cell
    kind, axis, mid = VL.decide(pts[:, :3].min(axis=0), pts[:, :3].max(axis=0), leaf)
    assert (kind, axis) == (VL.SPLIT, 0) and first[0] <= mid < second[0]
    cells = VL.apply_filter(pts, leaf)
    assert np.array_equal(bits(cells), bits(np.stack([pts[0], first, second, pts[2]])))
    assert np.array_equal(bits(VL.independent(pts, leaf)[0]), bits(cells))


def test_tie_goes_to_z_and_a_flat_z_is_stuck():
    pts, leaf = K.tie_cloud(flat_z=False)
    p = pts[:, :3]
    assert VL.decide(p.min(axis=0), p.max(axis=0), leaf)[:2] == (VL.SPLIT, 2)
    stats = {}
    cells = VL.apply_filter(pts, leaf, stats=stats)
    other, pieces, depth = VL.independent(pts, leaf)
    assert np.array_equal(bits(cells), bits(other)) and (stats["pieces"], stats["depth"]) == (pieces, depth)
    flat, leaf = K.tie_cloud(flat_z=True)
    with pytest.raises(VL.Stuck):
        VL.apply_filter(flat, leaf)
    with pytest.raises(VL.Stuck):
        VL.independent(flat, leaf)


def test_general_float_input_within_the_voxelgrid_rule():
    """the restatement (sums through the oracle) and the independent statement (numpy sums) on the GPU test's float input"""
    pts, leaf = K.general_float()
    stats = {}
    cells = VL.apply_filter(pts, leaf, stats=stats)
    other, pieces, depth = VL.independent(pts, leaf)
    assert (stats["pieces"], stats["depth"]) == (pieces, depth) and pieces > 1
    assert len(cells) < len(pts)                  # cells of several points exist
    K.close_ulp_share(cells, other)


def test_binding_declares_the_symbol():
    import importlib
    capi = importlib.import_module("pointcloud-slam_amd.capi")
    assert "pcm_voxel_downsample_large" in capi.SYMBOLS
    assert C.sizeof(capi.PcmVoxelLargeResult) == 48
