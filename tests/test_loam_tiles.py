"""CPU checks of the localisation-tile cut: the numpy restatement (tests/loam_tiles_ref.py) against independent statements of its
rules, csrc/loam_tiles.h (compiled with g++ through tests/loam_tiles_hooks.cpp) against the restatement on the index, key and box
arithmetic, the struct layouts of include/pcm_amd.h against ctypes, and the area list of LoamRegistration.tiles_arealist through
write_arealist / read_arealist."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loam_tiles_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloud-slam_amd", "csrc")
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def hooks(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("loam_tiles") / "loam_tiles_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "loam_tiles_hooks.cpp"), "-o", so],
                   check=True)
    L = C.CDLL(so)
    L.lt_tile_index.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_int32)]
    L.lt_tile_key.argtypes = [C.c_int32, C.c_int32]
    L.lt_tile_key.restype = C.c_uint32
    L.lt_key_indices.argtypes = [C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.lt_tile_box_xy.argtypes = [C.c_int32, C.c_int32, C.c_float, C.POINTER(C.c_double)]
    return L


def cloud(seed, n, lo=-30.0, hi=30.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(lo, hi, (n, 4)).astype(F)
    c[:, 2] = rng.uniform(-2.0, 6.0, n).astype(F)
    c[:, 3] = rng.integers(0, 256, n).astype(F)
    return c


def test_leaf_zero_is_a_stable_partition():
    c = cloud(1, 5000)
    c[17, 0] = np.nan
    c[99, 2] = np.inf
    tiles, bad = TR.cut(c, 4.0, 0.0)
    assert bad == 2
    keys = [int(TR.tile_key(t.ix, t.iy)) for t in tiles]
    assert keys == sorted(set(keys))                      # ascending, distinct
    got = np.concatenate([t.points for t in tiles])
    keep = np.isfinite(c[:, :3]).all(axis=1)
    assert got.shape[0] == int(keep.sum()) == 4998
    # a permutation of the finite input that keeps the input order inside a tile: tag every point with its input position
    tagged = c.copy()
    tagged[:, 3] = np.arange(len(c), dtype=F)
    ttiles, _ = TR.cut(tagged, 4.0, 0.0)
    order = np.concatenate([t.points[:, 3] for t in ttiles]).astype(np.int64)
    assert np.array_equal(np.sort(order), np.nonzero(keep)[0])
    for t in ttiles:
        assert (np.diff(t.points[:, 3]) > 0).all()
    assert np.array_equal(bits(got[:, :3]), bits(c[order][:, :3] + F(0.0)))
    # every point lies in its box, in float-consistent terms: the float quotient's floor is the index, and the float bounds hold
    for t in tiles:
        x, y = t.points[:, 0], t.points[:, 1]
        assert np.array_equal(np.floor(x / F(4.0)), np.full(len(x), t.ix, F)) and np.array_equal(np.floor(y / F(4.0)), np.full(len(y), t.iy, F))
        assert (t.box[0] <= x.astype(np.float64)).all() and (x.astype(np.float64) < t.box[3]).all()
        assert (t.box[1] <= y.astype(np.float64)).all() and (y.astype(np.float64) < t.box[4]).all()
        assert t.box[2] == t.points[:, 2].min() and t.box[5] == t.points[:, 2].max()
        assert t.box[3] - t.box[0] == 4.0 and t.box[4] - t.box[1] == 4.0


def test_boundaries_and_zeros():
    c = np.array([[-0.0, 0.5, 1, 0], [-1e-7, 0.5, 1, 0], [4.0, 0.5, 1, 0], [8.0, -4.0, 1, 0], [np.nextafter(F(4.0), F(0.0)), 0.5, 1, 0], [-4.0, -0.0, 1, 0],
                  [np.nextafter(F(-4.0), F(-9.0)), 3.9999998, 2, 0]], F)
    tiles, bad = TR.cut(c, 4.0, 0.0)
    assert bad == 0
    where = {(t.ix, t.iy): t for t in tiles}
    assert sorted(where) == sorted({(0, 0), (-1, 0), (1, 0), (2, -1), (-2, 0)})
    assert len(where[(0, 0)].points) == 2 and len(where[(-1, 0)].points) == 2      # -0.0f and 3.9999998 | -1e-7f and (-4, -0.0)
    assert not np.signbit(where[(0, 0)].points[0, 0])                              # stored as a one-point mean: +0.0
    assert [(t.ix, t.iy) for t in tiles] == [(2, -1), (-2, 0), (-1, 0), (0, 0), (1, 0)]   # ascending (iy, ix)
    with pytest.raises(TR.OutOfRange):
        TR.cut(np.array([[4.0 * 32768, 0, 0, 0]], F), 4.0, 0.0)
    with pytest.raises(TR.OutOfRange):
        TR.cut(np.array([[0, -4.0 * 32768, 0, 0]], F), 4.0, 0.0)    # iy = -32768
    t, _ = TR.cut(np.array([[np.nextafter(F(4.0 * 32768), F(0)), np.nextafter(F(-4.0 * 32767), F(0)), 0, 0]], F), 4.0, 0.0)
    assert (t[0].ix, t[0].iy) == (32767, -32767)


def test_leaf_is_the_voxel_grid_of_the_tile_alone():
    import loam_global_ref as GR
    c = cloud(2, 4000, -9.0, 9.0)
    t0, _ = TR.cut(c, 4.0, 0.0)
    t4, _ = TR.cut(c, 4.0, 0.4)
    assert [(t.ix, t.iy) for t in t0] == [(t.ix, t.iy) for t in t4]
    for a, b in zip(t0, t4):
        assert np.array_equal(bits(b.points), bits(GR.voxel_grid_pinned(a.points, 0.4) + F(0.0)))
        assert len(b.points) <= len(a.points) and a.box[2] <= b.box[2] <= b.box[5] <= a.box[5]
        assert np.array_equal(a.box[[0, 1, 3, 4]], b.box[[0, 1, 3, 4]])
    assert sum(len(t.points) for t in t4) < sum(len(t.points) for t in t0)


def test_header_matches_restatement(hooks):
    rng = np.random.default_rng(3)
    sizes = [F(4.0), F(50.0), F(0.3), F(1e-3), F(7.77)]
    vals = np.concatenate([rng.uniform(-500, 500, 2000).astype(F), np.array([-0.0, 0.0, -1e-7, 1e-7, 4.0, -4.0, 8.0, 50.0, -50.0, 1e30, -1e30, np.inf, -np.inf, np.nan,
                                                                              131072.0, -131072.0, 131071.99, -131071.99], F)])
    vals = np.concatenate([vals, (np.arange(-40, 40) * 0.3).astype(F), np.arange(-40, 40).astype(F) * F(7.77)])
    for ts in sizes:
        want = TR.tile_index(vals, ts)
        for v, w in zip(vals, want):
            i = C.c_int32(77)
            ok = hooks.lt_tile_index(C.c_float(v), C.c_float(ts), C.byref(i))
            in_range = bool(np.isfinite(w)) and abs(w) < TR.LIMIT
            assert bool(ok) == in_range, (v, ts, w)
            if ok:
                assert i.value == int(w), (v, ts, w, i.value)
    for ix, iy in ((0, 0), (-1, 0), (0, -1), (32767, 32767), (-32767, -32767), (5, -9), (-32767, 32767)):
        k = hooks.lt_tile_key(ix, iy)
        assert k == int(TR.tile_key(ix, iy)) and k != 0
        a, b = C.c_int32(0), C.c_int32(0)
        hooks.lt_key_indices(k, C.byref(a), C.byref(b))
        assert (a.value, b.value) == (ix, iy)
        for ts in sizes:
            box = (C.c_double * 4)()
            hooks.lt_tile_box_xy(ix, iy, C.c_float(ts), box)
            assert tuple(box) == tuple(float(v) for v in TR.tile_box_xy(ix, iy, ts))
    ks = [hooks.lt_tile_key(ix, iy) for iy in (-3, 0, 2) for ix in (-5, -1, 0, 7)]
    assert ks == sorted(ks)      # ascending keys are ascending (iy, ix)


def test_struct_layouts(pcm):
    capi = pcm.capi
    P, R = capi.PcmLoamTilesParams, capi.PcmLoamTilesResult
    assert C.sizeof(P) == 48 and (P.tile_size.offset, P.leaf_corner.offset, P.leaf_surf.offset, P.reserved.offset) == (0, 4, 8, 12)
    assert C.sizeof(R) == 72
    assert (R.num_corner_tiles.offset, R.num_surf_tiles.offset, R.corner_points_in.offset, R.surf_points_in.offset, R.corner_points_out.offset,
            R.surf_points_out.offset, R.num_nonfinite.offset, R.reserved.offset) == (0, 4, 8, 16, 24, 32, 40, 48)
    src = r'''
#include <pcm_amd.h>
#include <stddef.h>
#include <stdio.h>
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(pcm_loam_tiles_params), offsetof(pcm_loam_tiles_params, reserved), sizeof(pcm_loam_tiles_result),
         offsetof(pcm_loam_tiles_result, corner_points_in), offsetof(pcm_loam_tiles_result, num_nonfinite), offsetof(pcm_loam_tiles_result, reserved));
  return PCM_ABI_VERSION;
}
'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        r = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True)
    assert r.returncode == capi.PCM_ABI_VERSION == 3
    assert [int(v) for v in r.stdout.split()] == [48, 12, 72, 8, 40, 48]
    for name in ("pcm_loam_default_tiles_params", "pcm_loam_tiles_build", "pcm_loam_tile_info", "pcm_loam_tile_get"):
        assert name in capi.SYMBOLS


class _FakeTiles:
    """LoamRegistration.tiles_arealist on tile_info rows that need no device."""

    def __init__(self, pcm, tiles, tile_size):
        self._tiles, self._tile_size = tiles, tile_size
        self.tiles_arealist = pcm.LoamRegistration.tiles_arealist.__get__(self)

    def num_tiles(self, which):
        return len(self._tiles)

    def tile_info(self, which, i):
        t = self._tiles[i]
        return {"box": t.box, "ixy": (t.ix, t.iy), "n": len(t.points)}


def test_arealist_round_trip(pcm, tmp_path):
    tiles, _ = TR.cut(cloud(5, 3000), 12.5, 0.0)
    rows = _FakeTiles(pcm, tiles, 12.5).tiles_arealist(1, prefix="surf/")
    assert [r[0] for r in rows] == ["surf/12.5_%d_%d.pcd" % (t.ix, t.iy) for t in tiles]
    path = str(tmp_path / "arealist.csv")
    pcm.write_arealist(path, rows)
    back = pcm.read_arealist(path)
    assert [b[0] for b in back] == [r[0] for r in rows]
    for (name, box), t in zip(back, tiles):
        # std::to_string keeps six decimals: the x / y bounds (multiples of 12.5) survive exactly, z to 5e-7
        assert np.array_equal(box[[0, 1, 3, 4]], t.box[[0, 1, 3, 4]]) and np.abs(box - t.box).max() <= 5e-7
    assert _FakeTiles(pcm, tiles, 50.0).tiles_arealist(0)[0][0].startswith("50_")
