"""GPU checks of the 2D occupancy map (pcm_occ_*) against the literal restatement of tests/occ_map_ref.py: equal, no tolerance.
Virtual scans (bits of the ranges), both counters of every cell, the cropped grid, origin, width, height and the PGM bytes.

Device and host share every operation to the last bit except the float atan2 (beam of a point) and the double sin / cos (end
point of a beam).  Each case therefore first asserts, on the restatement's own numbers, that no contributing point lies within
BEAM_MARGIN beams of a beam boundary and no end point within END_MARGIN cells of a cell boundary (margins derived in
tests/test_occ_map.py from the ulp bounds of those functions); a range tie cannot matter, because the range itself,
(float)sqrt((double)x * x + (double)y * y), is the same bits on both sides and a minimum of equal values is that value.
The overflow counter (updates dropped outside the allocation) is asserted 0 everywhere."""
import importlib

import numpy as np
import pytest

import occ_map_ref as R
from test_occ_map import run_ref, same_floats, world_ok

pytestmark = pytest.mark.gpu

synth_occ = importlib.import_module("pointcloud-slam_amd.synth_occ")
F = np.float32
_CACHE = {}


def scans():
    if "s" not in _CACHE:
        _CACHE["s"] = synth_occ.make_scans(0, nx=3, ny=2, step=3.0)
    return _CACHE["s"]


def subset(s, idx):
    return synth_occ.OccScans(s.poses[idx], [s.clouds[i] for i in idx], s.world)


def ref_of(key, s, P):
    if key not in _CACHE:
        m = run_ref(s, P)
        world_ok(s, m)
        _CACHE[key] = m
    return _CACHE[key]


def kwargs_of(P):
    return dict(min_z=P.min_z, max_z=P.max_z, angle_increment=P.angle_increment, min_range=P.min_range, max_range=P.max_range, log_occ=P.log_occ,
                log_free=P.log_free, resolution=P.resolution, max_radius=P.max_radius, fill_with_white=P.fill_with_white, use_nan=P.use_nan)


def check_map(g, m):
    """Everything the device reports about the map against the restatement `m`."""
    assert g.occ_status()["overflow"] == 0
    w, h, ox, oy = m.info()
    grid = g.occ_map()
    assert (grid.width, grid.height) == (w, h)
    assert (grid.origin_x, grid.origin_y, grid.resolution) == (ox, oy, m.P.resolution)
    assert grid.n_known == len(m.logit)
    a, b = g.occ_counts()
    ra, rb = m.counts()
    assert np.array_equal(a, ra), np.argwhere(a != ra)[:5]
    assert np.array_equal(b, rb), np.argwhere(b != rb)[:5]
    rg = m.grid("counts")
    assert np.array_equal(grid.data, rg)
    assert g.occ_pgm().tobytes() == R.pgm_bytes(rg)


def check_scans(g, s, P):
    for i, c in enumerate(s.clouds):
        r, a = g.occ_scan(i)
        rr, ra = R.get_scan(c, P)
        assert same_floats(r, rr), i
        assert np.array_equal(a.view(np.uint64), ra.view(np.uint64))


def test_one_scan(pcm):
    P = R.Params()
    s = subset(scans(), [2])
    m = ref_of("one", s, P)
    g = pcm.OccupancyMap2D(0)
    g.insert_scans(s.clouds, s.poses)
    st = g.status()
    assert st["beam_size"] == 1048 and st["n_scans"] == 1
    check_scans(g, s, P)
    check_map(g, m)


def test_batch_equals_one_by_one_and_the_restatement(pcm):
    P = R.Params()
    s = scans()
    m = ref_of("all", s, P)
    x0, x1, y0, y1 = m.bounds()
    assert x0 < 0 < x1 and y0 < 0 < y1                     # the trajectory and the rays cross cell index 0 on both axes
    cells = [R.world2grid(float(p[k]), P) for p in s.poses for k in (3, 4)]
    assert min(cells[0::2]) < 0 < max(cells[0::2]) and min(cells[1::2]) < 0 < max(cells[1::2])
    g = pcm.OccupancyMap2D(0)
    g.insert_scans(s.clouds, s.poses)
    check_scans(g, s, P)
    check_map(g, m)
    one = pcm.OccupancyMap2D(0)
    for c, p in zip(s.clouds, s.poses):
        one.insert_scans([c], [p])
    assert one.status()["n_scans"] == len(s.clouds)
    check_map(one, m)
    a, b = g.counts()
    a1, b1 = one.counts()
    assert np.array_equal(a, a1) and np.array_equal(b, b1)
    # a reset empties the map, and the same scans give the same map again
    g.reset()
    assert g.map().data.size == 0 and g.status()["n_scans"] == 0
    g.insert_scans(s.clouds, s.poses)
    check_map(g, m)


def test_growth_of_the_rectangle_keeps_the_counters(pcm):
    P = R.Params()
    s = scans()
    m = ref_of("all", s, P)
    g = pcm.OccupancyMap2D(0)
    g.insert_scans(s.clouds[:1], s.poses[:1])
    r0 = g.status()["rect"]
    rects = {r0}
    for i in range(1, len(s.clouds), 3):
        g.insert_scans(s.clouds[i:i + 3], s.poses[i:i + 3])
        rects.add(g.status()["rect"])
    r1 = g.status()["rect"]
    assert len(rects) >= 2 and r1[2] * r1[3] > r0[2] * r0[3]        # it grew
    assert len(rects) < len(range(1, len(s.clouds), 3)) + 1         # geometrically: not at every call
    assert r1[0] <= r0[0] and r1[1] <= r0[1] and r1[0] + r1[2] >= r0[0] + r0[2] and r1[1] + r1[3] >= r0[1] + r0[3]
    check_map(g, m)


@pytest.mark.parametrize("case", ["no_fill", "use_nan", "coarse"])
def test_parameter_variants(pcm, case):
    P = {"no_fill": R.Params(fill_with_white=False, max_radius=5.0), "use_nan": R.Params(use_nan=True, max_radius=6.0),
         "coarse": R.Params(resolution=0.25, log_occ=3.0 / 32.0, log_free=-1.0 / 128.0)}[case]
    s = subset(scans(), list(range(0, len(scans().clouds), 3)))
    m = ref_of(case, s, P)
    g = pcm.OccupancyMap2D(0, **kwargs_of(P))
    g.insert_scans(s.clouds, s.poses)
    check_scans(g, s, P)
    check_map(g, m)
    if case == "coarse":   # dyadic updates: the visit-order sum of the reference is the count rule for every cell
        assert np.array_equal(g.map().data, m.grid("literal"))


def test_keyframes_in_place_equal_scans_and_rebuild_after_set_poses(pcm):
    P = R.Params()
    s = scans()
    corner, surf = s.keyframe_split(0)
    m = ref_of("all", s, P)
    reg = pcm.LoamRegistration(0)
    for k in range(len(s.clouds)):
        reg.add_keyframe(s.poses[k], 10.0 + k, corner[k], surf[k])
    reg.occ_reset()
    reg.occ_insert_keyframes()
    assert reg.occ_status()["n_scans"] == len(s.clouds)
    both = synth_occ.OccScans(s.poses, [np.concatenate([c, f]) for c, f in zip(corner, surf)], s.world)
    check_scans(reg, both, P)
    check_map(reg, m)
    g = pcm.OccupancyMap2D(0)
    g.insert_scans(both.clouds, both.poses)
    a, b = g.counts()
    a1, b1 = reg.occ_counts()
    assert np.array_equal(a, a1) and np.array_equal(b, b1)
    # key frames in two calls are the same map
    reg.occ_reset()
    reg.occ_insert_keyframes(0, 5)
    reg.occ_insert_keyframes(5)
    check_map(reg, m)
    # a loop closure moved the poses: reset + rebuild from the store
    rng = np.random.default_rng(9)
    moved = s.poses.copy()
    moved[:, 2] += rng.normal(0, 0.05, moved.shape[0]).astype(F)
    moved[:, 3:5] += rng.normal(0, 0.3, (moved.shape[0], 2)).astype(F)
    s2 = synth_occ.OccScans(moved, s.clouds, s.world)
    m2 = ref_of("moved", s2, P)
    reg.set_keyframe_poses(moved)
    reg.occ_reset()
    reg.occ_insert_keyframes()
    check_map(reg, m2)
    assert m2.bounds() != m.bounds() or not np.array_equal(m2.counts()[1], m.counts()[1])


def test_errors(pcm):
    g = pcm.OccupancyMap2D(0)
    with pytest.raises(pcm.PcmError):
        g.reset(resolution=0.0)
    with pytest.raises(pcm.PcmError):
        g.reset(resolution=0.001, max_radius=200.0)          # one scan alone exceeds the cap of 2^28 cells
    g.reset()
    with pytest.raises(pcm.PcmError):
        g.insert_scans([np.zeros((4, 3), F)], [[0, 0, 0, np.nan, 0, 0]])
    far = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, 3000.0, 3000.0, 0]], F)   # 30 000 x 30 000 cells: above the cap
    with pytest.raises(pcm.PcmError):
        g.insert_scans([np.zeros((4, 3), F)] * 2, far)
    assert g.status()["overflow"] == 0
    with pytest.raises(pcm.PcmError):
        g._check(g._L.pcm_occ_insert_keyframes(g.handle, 0, 1))   # not a LOAM context
