"""GPU tests of the 3D occupancy map (pcm_octo_*, pointcloud-slam_amd/octo.py) against the Python restatement of octomap_server's
rules (tests/octo_map_ref.py).  Every comparison is an equality: keys are integers and a log-odds is a float sum of a fixed
sequence of hits and misses, because a scan updates a cell once whatever number of rays cross it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import octo_map_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
COUNTS = ("points_in", "dropped_nonfinite", "skipped_window", "skipped_min_range", "truncated", "rejected_rays", "cells_touched", "new_cells")


@pytest.fixture(scope="module")
def octo(pcm):
    from pointcloud_slam_amd import octo as module
    return module


def room(seed, n, half=(5.0, 4.0), height=2.5, centre=(0.0, 0.0)):
    """n points on the walls, floor and ceiling of a box room."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1, 1, (n, 3))
    face = rng.integers(0, 6, n)
    p = np.stack([u[:, 0] * half[0], u[:, 1] * half[1], (u[:, 2] + 1) * 0.5 * height], axis=1)
    p[face == 0, 0], p[face == 1, 0] = half[0], -half[0]
    p[face == 2, 1], p[face == 3, 1] = half[1], -half[1]
    p[face == 4, 2], p[face == 5, 2] = 0.0, height
    p[:, 0] += centre[0]
    p[:, 1] += centre[1]
    return p.astype(F)


def pillar(seed, n, at, radius=0.3, height=2.0):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi, n)
    return np.stack([at[0] + radius * np.cos(a), at[1] + radius * np.sin(a), rng.uniform(0.1, height, n)], axis=1).astype(F)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def params_of(P: R.Params, **extra):
    import dataclasses
    return dict(dataclasses.asdict(P), **extra)


def same_map(m, ref: R.Map):
    cells = m.cells()
    keys, values = ref.sorted_cells()
    assert np.array_equal(cells["key"], keys)
    assert np.array_equal(bits(cells["log_odds"]), bits(values))
    info = m.info()
    assert (info["cells"], info["occupied"], info["free_cells"]) == ref.counts()
    if ref.cells:
        assert (info["key_min"], info["key_max"]) == ref.key_box()


def same_result(got: dict, want: dict):
    assert {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}
    assert got["status"] == 0


def same_products(octo, m, ref: R.Map, tmp_path, name):
    """Grid, geometry, occupied centres, pgm bytes and both files."""
    g = m.project()
    want = ref.project()
    pts = m.occupied_points()
    assert np.array_equal(bits(pts), bits(ref.occupied_points()))
    if want is None:
        assert (g.width, g.height) == (0, 0) and m.pgm().size == 0 and m.save_map(str(tmp_path / name)) is None
        return None
    G, grid = want
    assert (g.width, g.height, g.min_key) == (G.width, G.height, G.min_key)
    assert (g.origin_x, g.origin_y, g.resolution) == (G.origin_x, G.origin_y, ref.P.resolution)
    assert np.array_equal(g.data, grid)
    assert m.pgm().tobytes() == R.pgm_body(grid)
    prefix = str(tmp_path / name)
    pgm, yaml = m.save_map(prefix)
    wp, wy = R.map_files(prefix, G, grid, ref.P.resolution)
    assert open(pgm, "rb").read() == wp and open(yaml, "rb").read() == wy
    info = m.info()
    assert (info["metric_min"], info["metric_max"]) == (G.metric_min, G.metric_max)
    return grid


# ---- 1: one scan -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_scan():
    P = R.Params(resolution=0.1)
    cloud, origin = room(0, 2500), (1.3, -0.7, 0.9)
    ref = R.Map(P)
    res = ref.insert_scan(cloud, origin)
    return P, cloud, origin, ref, res


def test_one_scan_of_a_room(octo, one_scan):
    P, cloud, origin, ref, want = one_scan
    m = octo.OccupancyMap3D(0, **params_of(P, initial_cells=1 << 17))
    info = m.info()
    assert [bits(F(info[k]))[0] for k in ("hit", "miss", "clamp_min", "clamp_max")] == \
        [bits(R.logodds(p))[0] for p in (P.prob_hit, P.prob_miss, P.clamp_min, P.clamp_max)]
    got = m.insert_scan(cloud, origin)
    same_result(got, want)
    assert got["table_growths"] == 0 and got["cells_touched"] == got["new_cells"] > 1000
    same_map(m, ref)
    assert m.info()["epoch"] == 1


# ---- 2: twelve scans -------------------------------------------------------------------------------------------------------------
def test_twelve_scans_reach_both_clamps_and_flip_cells(octo):
    P = R.Params(resolution=0.25)
    ref, m = R.Map(P), octo.OccupancyMap3D(0, **params_of(P, initial_cells=4096))
    first_pillar, second_pillar = (2.0, 1.0), (-2.0, -1.5)
    mid = None
    for s in range(12):
        origin = (-1.0 + 0.15 * s, 0.5 - 0.1 * s, 1.0 + 0.02 * s)
        cloud = np.concatenate([room(100 + s, 350, half=(4.0, 4.0)), pillar(200 + s, 60, first_pillar if s < 6 else second_pillar)])
        same_result(m.insert_scan(cloud, origin), ref.insert_scan(cloud, origin))
        same_map(m, ref)
        if s == 5:
            mid = dict(ref.cells)
    lo, hi = R.logodds(P.clamp_min), R.logodds(P.clamp_max)
    values = list(ref.cells.values())
    assert hi in values and lo in values                                                           # both clamps are reached
    assert any(v >= 0 and ref.cells[k] < 0 for k, v in mid.items())                                # occupied, later freed
    assert any(v < 0 and ref.cells[k] >= 0 for k, v in mid.items())                                # free, later occupied
    assert m.info()["epoch"] >= 12


# ---- 3, 4: one update per cell; ground clears only -------------------------------------------------------------------------------
def test_end_cell_crossed_by_another_ray_gets_one_hit(octo):
    P = R.Params(resolution=0.1)
    cloud, origin = np.array([[1.0, 0.02, 0.02], [2.0, 0.04, 0.04], [1.0, 0.02, 0.02]], F), (0.02, 0.02, 0.02)
    ref, m = R.Map(P), octo.OccupancyMap3D(0, **params_of(P))
    same_result(m.insert_scan(cloud, origin), ref.insert_scan(cloud, origin))
    end = R.key3(cloud[0], 0.1)
    assert end in ref.last_free and end in ref.last_occ
    cells = m.cells()
    at = np.nonzero((cells["key"] == np.array(end, np.int32)).all(axis=1))[0]
    assert len(at) == 1 and bits(cells["log_odds"][at])[0] == bits(R.logodds(P.prob_hit))[0]
    same_map(m, ref)


def test_ground_cloud_clears_only(octo):
    P = R.Params(resolution=0.1, max_range=6.0)
    rng = np.random.default_rng(4)
    ground = np.stack([rng.uniform(-8, 8, 600), rng.uniform(-8, 8, 600), np.zeros(600)], axis=1).astype(F)
    origin = (0.3, 0.2, 1.2)
    ref, m = R.Map(P), octo.OccupancyMap3D(0, **params_of(P))
    want = ref.insert_scan(None, origin, ground=ground)
    same_result(m.insert_scan(None, origin, ground=ground), want)
    same_map(m, ref)
    assert want["truncated"] > 50 and not ref.last_occ and m.info()["occupied"] == 0
    lone = np.array([[3.0, 3.0, 0.0]], F)      # a single ground ray: its end cell stays unknown
    ref2, m2 = R.Map(P), octo.OccupancyMap3D(0, **params_of(P))
    same_result(m2.insert_scan(None, origin, ground=lone), ref2.insert_scan(None, origin, ground=lone))
    same_map(m2, ref2)
    assert R.key3(lone[0], 0.1) not in ref2.cells and len(ref2.cells) > 10
    # the same point as non-ground: the end cell is known and occupied
    ref2.insert_scan(lone, origin)
    m2.insert_scan(lone, origin)
    same_map(m2, ref2)
    assert ref2.cells[R.key3(lone[0], 0.1)] == R.logodds(P.prob_hit)


# ---- 5: max_range ----------------------------------------------------------------------------------------------------------------
def test_rays_beyond_max_range_clear_their_truncated_end(octo):
    P = R.Params(resolution=0.1, max_range=3.0, min_range=0.8)
    cloud, origin = room(5, 1500), (0.5, 0.4, 1.1)
    near = (np.array(origin, F) + np.array([[0.3, 0.2, 0.1], [-0.5, 0.1, 0.2]], F)).astype(F)      # inside min_range
    cloud = np.concatenate([cloud, near])
    ref, m = R.Map(P), octo.OccupancyMap3D(0, **params_of(P))
    want = ref.insert_scan(cloud, origin)
    same_result(m.insert_scan(cloud, origin), want)
    same_map(m, ref)
    assert want["truncated"] > 500 and want["skipped_min_range"] == 2
    far = next(p for p in cloud if float(R.norm(*(p - np.array(origin, F)))) > 3.0)
    _, e, truncated = R.point_rule(np.array(origin, F), far, False, 3.0, 0.8)
    assert truncated and ref.cells[R.key3(e, 0.1)] == R.logodds(P.prob_miss)                       # the truncated end key is free


# ---- 6: what is counted and never inserted ---------------------------------------------------------------------------------------
def test_nonfinite_window_and_key_range_points_are_counted(octo):
    P = R.Params(resolution=0.1, pointcloud_min_z=0.05, pointcloud_max_z=2.2, pointcloud_max_x=4.5)
    good, origin = room(6, 1200), (0.2, -0.3, 1.0)
    bad = np.array([[np.nan, 0, 1], [1, np.inf, 1], [1, 1, -np.inf], [4000.0, 0.5, 1.0], [0.5, -5000.0, 1.0]], F)
    cloud = np.concatenate([good[:600], bad, good[600:]])
    ref, m = R.Map(P), octo.OccupancyMap3D(0, **params_of(P))
    want = ref.insert_scan(cloud, origin)
    same_result(m.insert_scan(cloud, origin), want)
    same_map(m, ref)
    assert want["dropped_nonfinite"] == 3 and want["rejected_rays"] == 1 and want["skipped_window"] > 300    # x = 4000 is outside the x window
    only_good = octo.OccupancyMap3D(0, **params_of(P))
    only_good.insert_scan(good, origin)
    assert only_good.cells().tobytes() == m.cells().tobytes()
    # an origin outside the key range: every ray is rejected, the end points are still occupied
    P2 = R.Params(resolution=0.1)
    ref2, m2 = R.Map(P2), octo.OccupancyMap3D(0, **params_of(P2))
    want2 = ref2.insert_scan(good[:50], (4000.0, 0.0, 0.0))
    same_result(m2.insert_scan(good[:50], (4000.0, 0.0, 0.0)), want2)
    same_map(m2, ref2)
    assert want2["rejected_rays"] == 50 and m2.info()["free_cells"] == 0


# ---- 7, 8: growth ----------------------------------------------------------------------------------------------------------------
def test_table_growth_changes_nothing(octo, one_scan):
    P, cloud, origin, ref, want = one_scan
    small = octo.OccupancyMap3D(0, **params_of(P, initial_cells=1024))
    got = small.insert_scan(cloud, origin)
    same_result(got, want)
    assert got["table_growths"] >= 3 and small.info()["capacity"] >= want["cells_touched"]
    same_map(small, ref)
    large = octo.OccupancyMap3D(0, **params_of(P, initial_cells=1 << 20))
    assert large.insert_scan(cloud, origin)["table_growths"] == 0
    assert large.cells().tobytes() == small.cells().tobytes()


def test_max_cells_too_small_leaves_the_map_unchanged(octo, pcm, one_scan):
    P, cloud, origin, _, _ = one_scan
    ref, m = R.Map(P), octo.OccupancyMap3D(0, **params_of(P, initial_cells=1024, max_cells=4096))
    few = cloud[:12]
    same_result(m.insert_scan(few, origin), ref.insert_scan(few, origin))
    before, info_before = m.cells().tobytes(), m.info()
    r = m.insert_scan(cloud, origin, allow=(pcm.capi.PCM_ERR_OUT_OF_RANGE,))
    assert r["status"] == pcm.capi.PCM_ERR_OUT_OF_RANGE
    with pytest.raises(pcm.PcmError) as e:
        m.insert_scan(cloud, origin)
    assert e.value.code == pcm.capi.PCM_ERR_OUT_OF_RANGE
    after = m.info()
    assert m.cells().tobytes() == before and {k: after[k] for k in ("cells", "occupied", "free_cells", "key_min", "key_max")} == \
        {k: info_before[k] for k in ("cells", "occupied", "free_cells", "key_min", "key_max")}
    same_map(m, ref)
    more = cloud[12:20]                      # the map still works afterwards
    same_result(m.insert_scan(more, origin), ref.insert_scan(more, origin))
    same_map(m, ref)


def test_one_ray_per_wave_marks_the_same_map(octo, one_scan):
    """The mark kernel's second form (one ray per wave, 64 keys marked at once) against the restatement and against the default
    form, through table growth, truncation, min_range, windows, a ground cloud, non-finite and far-away (truncated) points; and the phase
    clock of the measurement hook."""
    P, cloud, origin, ref, want = one_scan
    m = octo.OccupancyMap3D(0, **params_of(P, initial_cells=1024))
    m.debug("wave", timed=True)
    got = m.insert_scan(cloud, origin)
    same_result(got, want)
    same_map(m, ref)
    ph = m.phase_ms()
    assert ph["mark_passes"] == got["table_growths"] + 1 >= 4 and ph["mark_ms"] > 0 and ph["apply_ms"] > 0 and ph["growth_ms"] > 0
    P2 = R.Params(resolution=0.1, max_range=3.5, min_range=0.7, pointcloud_max_x=4.5)
    bad = np.array([[np.nan, 0, 1], [0.5, -5000.0, 1.0], [1, np.inf, 1]], F)
    cloud2 = np.concatenate([cloud[:900], bad, cloud[900:1800]])
    ground = np.stack([cloud[:300, 0] * F(0.6), cloud[:300, 1] * F(0.6), np.zeros(300, F)], axis=1).astype(F)
    runs = []
    for variant in ("lane", "wave"):
        v = octo.OccupancyMap3D(0, **params_of(P2, initial_cells=1 << 16))
        v.debug(variant)
        results = [v.insert_scan(cloud2, origin, ground=ground), v.insert_scan(cloud2[::3], (0.1, 0.2, 1.4))]
        runs.append((results, v.cells().tobytes(), v.project().data.tobytes()))
    assert runs[0] == runs[1] and runs[0][0][0]["dropped_nonfinite"] == 2 and runs[0][0][0]["truncated"] > 100


# ---- 9: memory kinds, strides, repeatability -------------------------------------------------------------------------------------
def test_host_device_strides_and_runs_give_the_same_bytes(octo, one_scan):
    import torch
    P, cloud, origin, ref, _ = one_scan
    ground = np.stack([cloud[:300, 0] * F(0.5), cloud[:300, 1] * F(0.5), np.zeros(300, F)], axis=1).astype(F)

    def padded(a, cols):
        out = np.full((a.shape[0], cols), 7.5, F)
        out[:, :3] = a
        return out

    def run(make):
        m = octo.OccupancyMap3D(0, **params_of(P, initial_cells=1 << 16))
        m.insert_scan(make(cloud), origin, ground=make(ground))
        return m.cells().tobytes(), m.occupied_points().tobytes(), m.project().data.tobytes()

    base = run(lambda a: a)
    assert run(lambda a: a) == base                                         # two runs
    assert run(lambda a: padded(a, 4)) == base and run(lambda a: padded(a, 8)) == base       # stride 16 and 32 on the host
    dev = torch.device("cuda:0")
    assert run(lambda a: torch.from_numpy(padded(a, 4)).to(dev)) == base    # read in place
    assert run(lambda a: torch.from_numpy(padded(a, 8)).to(dev)) == base    # staged on the device
    assert run(lambda a: torch.from_numpy(a.copy()).to(dev)) == base        # stride 12
    # output into a device buffer
    m = octo.OccupancyMap3D(0, **params_of(P))
    m.insert_scan(cloud, origin, ground=ground)
    n = m.info()["cells"]
    out = torch.zeros((n + 5, 4), dtype=torch.float32, device=dev)
    assert m.cells(out=out) == n
    assert out[:n].cpu().numpy().tobytes() == base[0]


# ---- 10: projection --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["z window", "speckles kept", "speckles filtered", "padding", "negative coordinates"])
def test_projection_and_map_files(octo, tmp_path, case):
    extra = {"z window": dict(occupancy_min_z=0.3, occupancy_max_z=1.8), "speckles kept": dict(occupancy_min_z=0.3, occupancy_max_z=1.8),
             "speckles filtered": dict(occupancy_min_z=0.3, occupancy_max_z=1.8, filter_speckles=1), "padding": dict(min_x_size=14.0, min_y_size=3.0),
             "negative coordinates": dict(occupancy_min_z=-19.5)}[case]
    P = R.Params(resolution=0.2, **extra)
    shift = (-30.0, -20.0, -20.0) if case == "negative coordinates" else (0.0, 0.0, 0.0)
    cloud = room(10, 1500, half=(4.0, 3.0), centre=shift[:2])
    cloud[:, 2] += F(shift[2])
    origin = (0.4 + shift[0], 0.3 + shift[1], 1.0 + shift[2])
    speckle = np.array([[1.5 + shift[0], -1.1 + shift[1], 1.1 + shift[2]]], F)       # one point in mid-air: an isolated occupied cell
    cloud = np.concatenate([cloud, speckle])
    ref, m = R.Map(P), octo.OccupancyMap3D(0, **params_of(P))
    same_result(m.insert_scan(cloud, origin), ref.insert_scan(cloud, origin))
    same_map(m, ref)
    ks = R.key3(speckle[0], 0.2)
    assert ref.cells[ks] >= 0 and ref.is_speckle(ks)
    grid = same_products(octo, m, ref, tmp_path, "map")
    G = ref.project()[0]
    at = grid[ks[1] - G.min_key[1], ks[0] - G.min_key[0]]
    assert 100 in grid and 0 in grid
    if case == "speckles filtered":
        assert at != 100
    elif case == "speckles kept":
        assert at == 100
    if case == "padding":
        assert G.width == R.key_d(7.0, 0.2) - R.key_d(-7.0, 0.2) + 1 and G.origin_x == R.coord(R.key_d(-7.0, 0.2), 0.2) - 0.1
    if case == "negative coordinates":
        assert all(v < KEY0 for v in ref.key_box()[1]) and G.origin_x < -30.0
    if case == "z window":
        everything = R.Map(R.Params(resolution=0.2))
        everything.cells = ref.cells
        assert not np.array_equal(everything.project()[1], grid)            # the window changes the map (floor and ceiling leave it)


KEY0 = R.KEY0


# ---- 11: fewer than two cells ----------------------------------------------------------------------------------------------------
def test_fewer_than_two_cells_give_empty_products(octo, tmp_path):
    P = R.Params(resolution=0.1)
    ref, m = R.Map(P), octo.OccupancyMap3D(0, **params_of(P))
    assert m.cells().shape == (0,) and m.occupied_points().shape == (0, 4) and m.info()["cells"] == 0
    same_products(octo, m, ref, tmp_path, "empty")
    assert m.insert_scan(np.zeros((0, 3), F), (0, 0, 0))["points_in"] == 0
    one = np.array([[0.03, 0.04, 0.05]], F)          # in the origin's cell: the ray is empty, the end cell is occupied
    same_result(m.insert_scan(one, (0.01, 0.01, 0.01)), ref.insert_scan(one, (0.01, 0.01, 0.01)))
    same_map(m, ref)
    assert len(ref.cells) == 1
    same_products(octo, m, ref, tmp_path, "one")


# ---- 12: key frames --------------------------------------------------------------------------------------------------------------
def test_keyframes_in_place_equal_transformed_scans(octo, pcm):
    import loam_global_ref as G
    rng = np.random.default_rng(12)
    K = 6
    poses = np.concatenate([rng.uniform(-0.2, 0.2, (K, 2)), rng.uniform(-3, 3, (K, 1)), rng.uniform(-4, 4, (K, 2)), rng.uniform(0.5, 1.5, (K, 1))], axis=1).astype(F)
    corner = [np.concatenate([rng.uniform(-6, 6, (150, 3)), rng.uniform(0, 1, (150, 1))], axis=1).astype(F) for _ in range(K)]
    surf = [np.concatenate([rng.uniform(-6, 6, (250, 3)), rng.uniform(0, 1, (250, 1))], axis=1).astype(F) for _ in range(K)]
    P = R.Params(resolution=0.2, max_range=5.0)
    reg = pcm.LoamRegistration(0)
    for k in range(K):
        reg.add_keyframe(poses[k], 10.0 + k, corner[k], surf[k])
    octo.octo_reset(reg, **params_of(P))
    octo.octo_insert_keyframes(reg, 0, 4)
    octo.octo_insert_keyframes(reg, 4, 2)
    m = octo.OccupancyMap3D(0, **params_of(P))
    ref = R.Map(P)
    for k in range(K):
        world = G.export(poses, corner, surf, 2, k, 1)
        m.insert_scan(world, poses[k, 3:6])
        if k < 2:
            ref.insert_scan(world, poses[k, 3:6])
            if k == 1:
                two = octo.OccupancyMap3D(0, **params_of(P))
                for j in range(2):
                    two.insert_scan(G.export(poses, corner, surf, 2, j, 1), poses[j, 3:6])
                same_map(two, ref)
    assert octo.octo_cells(reg).tobytes() == m.cells().tobytes() and octo.octo_info(reg)["cells"] > 500
    assert octo.octo_project(reg).data.tobytes() == m.project().data.tobytes()
    with pytest.raises(pcm.PcmError):
        octo.octo_insert_keyframes(reg, 4, 3)
    with pytest.raises(pcm.PcmError):
        octo.octo_insert_keyframes(m, 0, 1)        # not a LOAM context


# ---- 13: sensor_to_world ---------------------------------------------------------------------------------------------------------
def test_sensor_to_world_equals_clouds_transformed_beforehand(octo):
    P = R.Params(resolution=0.15, pointcloud_min_z=0.3)      # world frame: the floor is cut away
    a, b = 0.7, -0.1
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry, (1.5, -2.0, 0.8)
    T = T.astype(F)
    body = room(13, 1200, half=(4.0, 3.0))
    body[:, 2] -= F(0.8)
    origin = T[:3, 3]
    world = np.stack([R.transform(T, p) for p in body]).astype(F)
    ref, m, pre = R.Map(P), octo.OccupancyMap3D(0, **params_of(P)), octo.OccupancyMap3D(0, **params_of(P))
    want = ref.insert_scan(body, origin, sensor_to_world=T)
    same_result(m.insert_scan(body, origin, sensor_to_world=T), want)
    same_map(m, ref)
    same_result(pre.insert_scan(world, origin), want)
    assert pre.cells().tobytes() == m.cells().tobytes() and want["skipped_window"] > 0
