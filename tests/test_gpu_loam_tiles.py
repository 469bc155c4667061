"""GPU checks of the key-frame map cut into localisation area tiles (pcm_loam_tiles_build, pcm_loam_tile_info, pcm_loam_tile_get)
against the numpy restatement of tests/loam_tiles_ref.py.  Everything is an equality: the export is transformPointCloud's float32
values, the tile index a float division and a floor, a leaf-0 tile a partition, and a tile's VoxelGrid sums a few dozen float32
values of one tile (at most 4 m apart) in double -- exact in any order, so one rounding gives the same bits on both sides.

K = 6 key frames of 40-300 corner and 60-500 surf points of the synthetic LOAM world, posed over both signs of x and y; tile_size
4 m.  Key frame 2 (identity rotation, x = -0.0f) carries the seams in its surf cloud: a lattice over 9 x 8 tiles far from the other
frames (more than 64 tiles in the list; every lattice tile but one holds exactly 1 point, that one 257), points exactly on
k * tile_size, a point that exports as x = -0.0f, one NaN point.  Key frame 4 has no corner points."""
import ctypes as C
import dataclasses
import importlib

import numpy as np
import pytest

import loam_global_ref as GR
import loam_tiles_ref as TR

pytestmark = pytest.mark.gpu

synth_keyframes = importlib.import_module("pointcloud-slam_amd.synth_keyframes")
F = np.float32
TS = 4.0
K = 6
_CACHE = {}
INVALID, OUT_OF_RANGE = -1, -5


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def seam_surf():
    rng = np.random.default_rng(7)
    pts = []
    for iy in range(-24, -16):          # 8 rows
        for ix in range(20, 29):        # 9 columns
            if (ix, iy) != (22, -20):
                pts.append([TS * ix + 2.0, TS * iy + 2.0, 1.0 + 0.1 * ix, 10.0])
    big = np.zeros((257, 4), F)         # more than a 256-thread workgroup in one tile
    big[:, 0] = rng.uniform(TS * 22 + 0.01, TS * 23 - 0.01, 257)
    big[:, 1] = rng.uniform(TS * -20 + 0.01, TS * -19 - 0.01, 257)
    big[:, 2] = rng.uniform(-1.0, 3.0, 257)
    big[:, 3] = rng.integers(0, 256, 257)
    edge = [[TS * 30, TS * -10, 0.5, 1.0], [TS * 31, TS * -10 + 1.0, 0.5, 2.0], [-TS, -TS, 0.5, 3.0], [-2 * TS, 1.0, 0.5, 4.0], [0.0, TS, 0.5, 5.0],
            [-0.0, -1.0, -1.0, 6.0],    # exports as x = -0.0f under the pose (0, 0, 0, -0.0, 0, 0)
            [-1e-7, -1.5, -1.0, 7.0],
            [np.nan, 1.0, 1.0, 8.0]]
    return np.concatenate([np.array(pts, F), big, np.array(edge, F)]).astype(F)


def frames():
    if "kf" not in _CACHE:
        kf = synth_keyframes.make_keyframes(0, K, n_corner=300, n_surf=500, scan_radius=8.0)
        n_c, n_s = [40, 300, 123, 77, 0, 211], [60, 500, 0, 333, 129, 250]
        corner = [np.ascontiguousarray(kf.corner[k][:n_c[k]], F) for k in range(K)]
        surf = [np.ascontiguousarray(kf.surf[k][:n_s[k]], F) for k in range(K)]
        surf[2] = seam_surf()
        for k in range(K):
            assert len(corner[k]) == n_c[k] and (k == 2 or len(surf[k]) == n_s[k])
        poses = np.array([[0.01, -0.02, 0.3, -9.0, -7.0, 1.5], [0.0, 0.01, -1.2, 6.5, -8.0, 1.4], [0.0, 0.0, 0.0, -0.0, 0.0, 0.0], [-0.01, 0.0, 2.5, -7.5, 9.0, 1.6],
                          [0.02, 0.01, 0.7, 8.0, 7.0, 1.5], [0.0, 0.0, -0.4, 1.0, -2.0, 1.5]], F)
        _CACHE["kf"] = synth_keyframes.KeyFrames(poses, 100.0 + 0.7 * np.arange(K), corner, surf, 105.0)
    return _CACHE["kf"]


def reference(leaf_c, leaf_s, first=0, n=None, poses=None):
    kf = frames()
    key = ("ref", leaf_c, leaf_s, first, n, None if poses is None else poses.tobytes())
    if key not in _CACHE:
        _CACHE[key] = TR.build(kf.poses if poses is None else poses, kf.corner, kf.surf, TS, leaf_c, leaf_s, first, n)
    return _CACHE[key]


def filled(pcm, poses=None):
    kf = frames()
    g = pcm.LoamRegistration(0)
    for k in range(K):
        assert g.add_keyframe((kf.poses if poses is None else poses)[k], kf.times[k], kf.corner[k], kf.surf[k]) == k
    return g


def device_tiles(g, which):
    out = []
    for i in range(g.num_tiles(which)):
        t = g.tile_info(which, i)
        p = g.get_tile(which, i)
        assert p.shape == (t["n"], 4)
        out.append((t["ixy"], t["box"], p))
    return out


def check_list(got, want):
    assert [t[0] for t in got] == [(w.ix, w.iy) for w in want]
    for (ixy, box, pts), w in zip(got, want):
        assert np.array_equal(box, w.box), (ixy, box, w.box)
        assert pts.shape == w.points.shape and np.array_equal(bits(pts), bits(w.points)), ixy


def check_build(g, r, leaf_c, leaf_s, first=0, n=None, poses=None):
    (wc, ws), bad = reference(leaf_c, leaf_s, first, n, poses)
    assert (r.num_corner_tiles, r.num_surf_tiles, r.num_nonfinite) == (len(wc), len(ws), bad)
    assert (r.corner_points_out, r.surf_points_out) == (sum(len(t.points) for t in wc), sum(len(t.points) for t in ws))
    assert (g.num_tiles(0), g.num_tiles(1)) == (len(wc), len(ws))
    check_list(device_tiles(g, 0), wc)
    check_list(device_tiles(g, 1), ws)
    return wc, ws


def test_the_fixture_crosses_the_seams():
    kf = frames()
    (wc, ws), bad = reference(0.0, 0.0)
    assert bad == 1 and len(ws) > 64 and 20 <= len(wc) <= 99
    counts = {(t.ix, t.iy): len(t.points) for t in ws}
    assert counts[(22, -20)] == 257 and counts[(20, -24)] == 1 and counts[(30, -10)] == 1 and counts[(31, -10)] == 1
    n_s, n_c = sum(len(s) for s in kf.surf), sum(len(c) for c in kf.corner)
    assert n_s % 64 != 0 and n_c % 64 != 0 and len(kf.corner[4]) == 0
    ex = GR.export(kf.poses, kf.corner, kf.surf, 1)
    assert (np.signbit(ex[:, 0]) & (ex[:, 0] == 0)).sum() == 1            # the -0.0f survives the transform ...
    t = {(t.ix, t.iy): t for t in ws}[(0, -1)]
    assert (t.points[:, 0] == 0).sum() == 1                               # ... and lies in tile 0, while -1e-7f lies in tile -1
    assert any(p[3] == 7.0 for p in {(t.ix, t.iy): t for t in ws}[(-1, -1)].points)
    assert sum(len(t.points) for t in ws) == n_s - 1                      # the NaN point appears nowhere


def test_leaf_zero_matches_restatement(pcm):
    import torch
    g = filled(pcm)
    r = g.build_tiles(tile_size=TS, leaf_corner=0.0, leaf_surf=0.0)
    kf = frames()
    assert (r.corner_points_in, r.surf_points_in) == (sum(len(c) for c in kf.corner), sum(len(s) for s in kf.surf))
    wc, ws = check_build(g, r, 0.0, 0.0)
    # into a device buffer: exact capacity, and a too small one
    for which, want in ((0, wc), (1, ws)):
        for i in (0, len(want) // 2, len(want) - 1):
            buf = torch.zeros((len(want[i].points), 4), dtype=torch.float32, device="cuda")
            assert g.get_tile(which, i, out=buf) == len(want[i].points)
            assert np.array_equal(bits(buf.cpu().numpy()), bits(want[i].points))
    i257 = [(t.ix, t.iy) for t in ws].index((22, -20))
    small = torch.zeros((256, 4), dtype=torch.float32, device="cuda")
    n = C.c_size_t(0)
    assert g._L.pcm_loam_tile_get(g._h, 1, i257, small.data_ptr(), 256, 1, C.byref(n)) == INVALID and n.value == 257
    assert float(small.abs().sum()) == 0.0
    with pytest.raises(pcm.capi.PcmError):
        g.tile_info(1, len(ws))
    rows = g.tiles_arealist("surf", prefix="s/")
    assert rows[i257][0] == "s/4_22_-20.pcd" and np.array_equal(rows[i257][1], ws[i257].box)
    # the leaf-0 points are the segmented pass's one-point means: the exported -0.0f (intensity 6) is stored as +0.0f, in tile 0
    ex = g.export_map("surf")
    row = ex[ex[:, 3] == 6.0]
    row = row[row[:, 0] == 0]
    assert row.shape[0] == 1 and bits(row[:, 0])[0] == 0x80000000
    i0 = [(t.ix, t.iy) for t in ws].index((0, -1))
    stored = g.get_tile("surf", i0)
    hit = stored[(stored[:, 3] == 6.0) & (stored[:, 0] == 0)]
    assert hit.shape[0] == 1 and bits(hit[:, 0])[0] == 0 and np.array_equal(bits(hit[0, 1:]), bits(row[0, 1:]))
    # the area list names the tiles of a build only
    g.add_tile("surf", [0, 0, 0, 1, 1, 1], np.ones((2, 4), F))
    with pytest.raises(pcm.capi.PcmError):
        g.tiles_arealist("surf")
    g.build_tiles(tile_size=TS, leaf_corner=0.0, leaf_surf=0.0)
    assert len(g.tiles_arealist("surf")) == len(ws)
    g.clear_tiles()
    with pytest.raises(pcm.capi.PcmError):
        g.tiles_arealist("surf")


@pytest.mark.parametrize("leaves", [(0.2, 0.4), (0.4, 0.2)])
def test_leaves_match_restatement_and_voxel_downsample(pcm, leaves):
    g = filled(pcm)
    r = g.build_tiles(tile_size=TS, leaf_corner=leaves[0], leaf_surf=leaves[1])
    check_build(g, r, leaves[0], leaves[1])
    got = (device_tiles(g, 0), device_tiles(g, 1))
    g.build_tiles(tile_size=TS, leaf_corner=0.0, leaf_surf=0.0)
    v = pcm.P2PlaneRegistration(0)
    for which in (0, 1):
        raw = device_tiles(g, which)
        assert [t[0] for t in raw] == [t[0] for t in got[which]]
        for (ixy, _, p0), (_, box, p) in zip(raw, got[which]):
            ds = v.voxel_downsample(p0, leaves[which])
            assert ds.shape == p.shape and np.array_equal(bits(ds), bits(p)), ixy
            assert box[2] == p[:, 2].min() and box[5] == p[:, 2].max()


def crop_state(g, pose, **kw):
    ld = g.load_map(pose, **kw)
    cr = g.crop_map(pose, **kw)
    info = g.dynmap_info()
    return ld, cr, info


def test_hand_over_equals_the_host_route(pcm):
    kf = frames()
    g = filled(pcm)
    g.build_tiles(tile_size=TS, leaf_corner=0.2, leaf_surf=0.2)
    # the route a caller had before: export to the host, cut there, upload tile by tile
    src = filled(pcm)
    h = pcm.LoamRegistration(0)
    for which in (0, 1):
        tiles, _ = TR.cut(src.export_map(which), TS, 0.2)
        for t in tiles:
            h.add_tile(which, t.box, t.points)
    assert (h.num_tiles(0), h.num_tiles(1)) == (g.num_tiles(0), g.num_tiles(1))
    inside, edge, outside = [0, 0, 0, -7.0, -6.0, 1.5], [0, 0, 0, 8.0, -6.0, 1.5], [0, 0, 0, 300.0, 300.0, 1.5]
    for pose, margin in ((inside, 0), (edge, 0), (outside, 0), (inside, 6), (edge, 6)):
        kw = dict(margin=margin, max_range=5.0, crop_x=1)
        a, b = crop_state(g, pose, **kw), crop_state(h, pose, **kw)
        for k in ("num_corner_tiles", "num_surf_tiles", "num_corner_selected", "num_surf_selected", "num_corner_points", "num_surf_points"):
            assert getattr(a[0], k) == getattr(b[0], k), k
        ra, rb = dataclasses.asdict(a[1]), dataclasses.asdict(b[1])
        assert ra == rb
        for k in ("corner_tiles", "surf_tiles"):
            assert np.array_equal(a[2][k], b[2][k])
        for k in ("corner", "surf"):
            assert np.array_equal(bits(a[2][k]), bits(b[2][k]))
        if pose is outside:
            assert a[0].num_corner_selected == 0 and a[0].num_surf_selected == 0
        elif margin == 0:
            assert a[0].num_surf_selected == (2 if pose is edge else 1)    # is_in_area is inclusive: an edge pose lies in both boxes
    x0 = np.array([0.0, 0.0, -0.4, 1.05, -1.95, 1.5], F)
    res = []
    for reg in (g, h):
        reg.load_map(x0, margin=12)
        reg.crop_map(x0, margin=12, max_range=20.0)
        reg.set_input_source(kf.corner[5], kf.surf[5])
        res.append(reg.scan2map(x0))
    a, b = dataclasses.asdict(res[0]), dataclasses.asdict(res[1])
    print("scan2map on the built tiles: status %d, %d iterations, %d corner / %d surf correspondences" % (a["status"], a["iterations"], a["num_corner"], a["num_surf"]))
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_state_is_left_alone_and_builds_replace(pcm):
    kf = frames()
    g, control = filled(pcm), filled(pcm)
    for reg in (g, control):
        reg.sc_add(points=kf.surf[0], leaf=0.0)
        reg.set_input_source(kf.corner[1], kf.surf[1])
    g.add_tile("corner", [0, 0, 0, 1, 1, 1], np.ones((3, 4), F))      # tiles added by hand are replaced
    g.add_tile("surf", [0, 0, 0, 1, 1, 1], np.ones((5, 4), F))
    assert g.tile_info("surf", 0)["ixy"] == (0, 0)
    r1 = g.build_tiles(tile_size=TS, leaf_corner=0.0, leaf_surf=0.2)
    check_build(g, r1, 0.0, 0.2)
    r2 = g.build_tiles(tile_size=TS, leaf_corner=0.0, leaf_surf=0.2)      # twice equals once
    assert r1 == r2
    check_build(g, r2, 0.0, 0.2)
    assert g.sc_count == control.sc_count == 1 and g.num_keyframes == K
    for k in range(K):
        for a, b in zip(g.get_keyframe(k), control.get_keyframe(k)):
            assert np.array_equal(bits(a), bits(b))
    # the context's source: what a key frame without clouds copies from it
    for reg in (g, control):
        reg.add_keyframe(kf.poses[0], 200.0)
    for a, b in zip(g.get_keyframe(K), control.get_keyframe(K)):
        assert len(a) and np.array_equal(bits(a), bits(b))
    # new poses, new tiles
    moved = kf.poses.copy()
    moved[:, 3] += F(1.7)
    moved[:, 5] -= F(0.3)
    g2 = filled(pcm)
    g2.build_tiles(tile_size=TS, leaf_corner=0.0, leaf_surf=0.2)
    g2.set_keyframe_poses(moved)
    r = g2.build_tiles(tile_size=TS, leaf_corner=0.0, leaf_surf=0.2)
    check_build(g2, r, 0.0, 0.2, poses=moved)


def test_sub_ranges(pcm):
    g = filled(pcm)
    for first, n in ((0, 3), (3, 3), (4, 1), (2, 0)):
        r = g.build_tiles(first, n, tile_size=TS, leaf_corner=0.2, leaf_surf=0.0)
        check_build(g, r, 0.2, 0.0, first, n)
    assert (g.num_tiles(0), g.num_tiles(1)) == (0, 0)                    # the empty range leaves zero tiles
    e = pcm.LoamRegistration(0)
    r = e.build_tiles(tile_size=TS)                                      # an empty store
    assert (r.num_corner_tiles, r.num_surf_tiles, r.corner_points_in) == (0, 0, 0)


def test_errors_leave_the_tiles_as_they_were(pcm):
    kf = frames()
    g = filled(pcm)
    r = g.build_tiles(tile_size=TS, leaf_corner=0.0, leaf_surf=0.0)

    def refused(code, reg=g, **kw):
        with pytest.raises(pcm.capi.PcmError) as e:
            reg.build_tiles(**kw)
        assert e.value.code == code and len(str(e.value)) > 20, (kw, e.value)
        check_build(g, r, 0.0, 0.0)

    for ts in (0.0, -4.0, float("nan"), float("inf")):
        refused(INVALID, tile_size=ts)
    refused(INVALID, tile_size=TS, leaf_corner=-0.1)
    refused(INVALID, tile_size=TS, leaf_surf=-1.0)
    refused(INVALID, first=4, n=3, tile_size=TS)
    refused(INVALID, first=-1, n=2, tile_size=TS)
    refused(INVALID, first=K + 1, n=0, tile_size=TS)
    # a pose so far out that |ix| >= 32768: rejected from a count, on the host
    far = kf.poses.copy()
    far[1, 3] = F(TS * 32768 + 100.0)
    g.set_keyframe_poses(far)
    with pytest.raises(TR.OutOfRange):
        TR.build(far, kf.corner, kf.surf, TS, 0.0, 0.0)
    refused(OUT_OF_RANGE, tile_size=TS)
    g.set_keyframe_poses(kf.poses)
    # two points 1 km apart in z in one tile: its VoxelGrid index overflows at leaf 1e-7
    tall = pcm.LoamRegistration(0)
    tall.add_keyframe([0, 0, 0, 0, 0, 0], 1.0, np.array([[1, 1, 0, 0], [1.5, 1, 1000.0, 0]], F), np.array([[9, 9, 0, 0]], F))
    tall.add_tile("surf", [0, 0, 0, 1, 1, 1], np.ones((5, 4), F))
    with pytest.raises(pcm.capi.PcmError) as e:
        tall.build_tiles(tile_size=TS, leaf_corner=1e-7, leaf_surf=0.0)
    assert e.value.code == OUT_OF_RANGE and "overflow" in str(e.value)
    assert (tall.num_tiles(0), tall.num_tiles(1)) == (0, 1) and np.array_equal(tall.get_tile("surf", 0), np.ones((5, 4), F))
    ok = tall.build_tiles(tile_size=TS, leaf_corner=0.5, leaf_surf=0.0)
    assert (ok.num_corner_tiles, ok.num_surf_tiles, ok.corner_points_out) == (1, 1, 2)
    p2 = pcm.P2PlaneRegistration(0)
    assert g._L.pcm_loam_tiles_build(p2._h, None, 0, 0, None) == INVALID and b"PCM_MODEL_LOAM" in g._L.pcm_last_error(p2._h)


def test_build_ms_builds_the_same_tiles(pcm):
    g = filled(pcm)
    ms = g.build_tiles_ms(tile_size=TS, leaf_corner=0.2, leaf_surf=0.0)
    (wc, ws), _ = reference(0.2, 0.0)
    check_list(device_tiles(g, 0), wc)
    check_list(device_tiles(g, 1), ws)
    assert set(ms["surf"]) == set(pcm.capi.TILES_STAGE_NAMES) and all(v >= 0 for v in ms["surf"].values()) and ms["gather"] > 0


def test_scan_context_of_the_near_cloud(pcm):
    """MULTI_SCAN_FEAT (pcm_loam_sc_add_near): descriptor, ring key and sector key equal near_keyframes + sc_add(points, leaf 0)."""
    kf = frames()
    g = pcm.LoamRegistration(0)
    for k in range(K):      # the near pass takes every point as it is: the NaN point stays out of this store
        g.add_keyframe(kf.poses[k], kf.times[k], kf.corner[k], kf.surf[k][np.isfinite(kf.surf[k]).all(axis=1)])
    for n, (key, search_num, wrt, leaf) in enumerate(((1, 1, -1, 0.2), (4, 2, -1, 0.0), (3, 25, 3, 0.4))):
        cloud = g.near_keyframes(key, search_num, wrt, leaf)
        assert len(cloud) > 100
        a = g.sc_add_near(key, search_num, wrt, leaf)
        b = g.sc_add(points=cloud, leaf=0.0)
        assert (a, b) == (2 * n, 2 * n + 1)
        assert g._sc_last_add.num_points == len(cloud)
        for x, y in zip(g.sc_get(a), g.sc_get(b)):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert np.count_nonzero(g.sc_get(a)[0]) > 0
    for bad in ((K, 1, -1, 0.2), (-1, 1, -1, 0.2), (0, -1, -1, 0.2), (0, 1, K, 0.2), (0, 1, -1, -0.5)):
        with pytest.raises(pcm.capi.PcmError) as e:
            g.sc_add_near(*bad)
        assert e.value.code == INVALID
    with pytest.raises(pcm.capi.PcmError) as e:
        g.sc_add_near(2, 1, -1, 1e-7)      # the seam frame spans 150 m: the VoxelGrid index overflows
    assert e.value.code == OUT_OF_RANGE
    assert g.sc_count == 6
    empty = pcm.LoamRegistration(0)
    with pytest.raises(pcm.capi.PcmError) as e:
        empty.sc_add_near(0, 1)
    assert e.value.code == INVALID and empty.sc_count == 0
