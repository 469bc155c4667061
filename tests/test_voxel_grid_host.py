"""CPU checks of the VoxelGrid arithmetic every down-sampler shares (pointcloud-slam_amd/csrc/voxel_grid.h, compiled with g++
through tests/voxel_grid_hooks.cpp): the box and the cell index of the header, run on the inputs of
tests/make_golden_voxel_grid.py, give the oracle's cells in the oracle's order, and the box reports an index overflow -- also
one whose cell product exceeds 2^63.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import make_golden_voxel_grid as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloud-slam_amd", "csrc")


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("voxel_grid") / "voxel_grid_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, os.path.join(ROOT, "tests", "voxel_grid_hooks.cpp"), "-o", so],
                   check=True)
    L = C.CDLL(so)
    L.vg_box.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    L.vg_cells.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_float, C.c_void_p, C.c_void_p]
    L.vg_cells.restype = None
    L.vg_ord2f.argtypes = [C.c_uint]
    L.vg_ord2f.restype = C.c_float
    return L


def f2ord(x):
    """pcm_device.h's f2ord: floats to unsigned words of the same order"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def box_of(H, finite_xyz, leaf):
    """(overflow, box words) of the header for the bounding box of the finite points"""
    mm = np.array([0xffffffff] * 3 + [0] * 3, np.uint32)
    if len(finite_xyz):
        mm = np.concatenate([f2ord(finite_xyz.min(axis=0)), f2ord(finite_xyz.max(axis=0))])
    b = np.zeros(6, np.int64)
    over = H.vg_box(mm.ctypes.data, leaf, b.ctypes.data)
    return bool(over), b


def test_header_compiles_alone_and_reads_no_hip_header():
    deps = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-M", "-I", CSRC, "-x", "c++", "-"],
                          input=b'#include "voxel_grid.h"\n', check=True, capture_output=True).stdout.decode()
    assert "voxel_grid.h" in deps and "hip" not in deps and "pcm_device.h" not in deps and "dev_buf.h" not in deps
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", CSRC, "-x", "c++", "-"], input=b'#include "voxel_grid.h"\n', check=True)


def test_ord2f_inverts_f2ord(H):
    x = np.array([0.0, -0.0, 1.5, -1.5, 1e-45, -1e-45, 3.4e38, -3.4e38, np.inf, -np.inf], np.float32)
    back = np.array([H.vg_ord2f(int(o)) for o in f2ord(x)], np.float32)
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))
    assert (np.diff(f2ord(np.sort(x)).astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("name", sorted(G.downsample_cases()))
def test_cells_of_the_header_are_the_oracles(H, name):
    from oracle.loader import voxel_downsample
    pts, leaf = G.downsample_cases()[name]
    want = voxel_downsample(pts, leaf)
    p = np.ascontiguousarray(pts[np.isfinite(pts[:, :3]).all(axis=1)])
    over, b = box_of(H, p[:, :3], leaf)
    assert not over
    if len(p) == 0:
        assert b[5] == 0 and len(want) == 0
        return
    assert b[5] == 2
    idx = np.zeros(len(p), np.uint64)
    H.vg_cells(p.ctypes.data, len(p), p.shape[1], leaf, b.ctypes.data, idx.ctypes.data)
    order = np.argsort(idx, kind="stable")
    uniq, first, count = np.unique(idx[order], return_index=True, return_counts=True)
    assert len(uniq) == len(want)                                   # as many distinct cell indices as the oracle has rows
    assert int(uniq.max()) < 2 ** 31
    # row j of the oracle is the centroid of the points with the j-th index (test_voxel_downsample_oracle's rule, every row)
    mean = np.add.reduceat(p[order].astype(np.float64), first, axis=0) / count[:, None]
    assert np.allclose(want, mean, rtol=1e-6, atol=1e-6)


def test_box_reports_index_overflow(H):
    from test_preprocess import _scan_for_downsample
    far = _scan_for_downsample(6)
    far[0, :3] = 1e7
    p = far[np.isfinite(far[:, :3]).all(axis=1)]
    over, b = box_of(H, p[:, :3], 0.001)
    assert over and b[5] == 1 and b[3] == 0 and b[4] == 0
    # an extent of 1e7 on all three axes at leaf 0.001: 1e30 cells, beyond what a 64-bit integer product can hold
    cube = np.array([[0.0, 0.0, 0.0], [1e7, 1e7, 1e7]], np.float32)
    assert (1e7 / 0.001) ** 3 > 2.0 ** 63
    over, b = box_of(H, cube, 0.001)
    assert over and b[5] == 1
    # and the largest box that still fits
    over, b = box_of(H, np.array([[0.0, 0.0, 0.0], [1023.5, 1023.5, 2046.5]], np.float32), 1.0)
    assert not over and b[5] == 2 and b[3] == 1024 and b[4] == 1024 * 1024
