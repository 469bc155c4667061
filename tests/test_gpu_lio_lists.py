"""The jueying_lio measurement model on candidate lists (k_lio_lists) and the wave-per-run rewrite of following lists.

Comparison rule: context A carries PCM_FLAG_FOLLOWING_LISTS (or PCM_FLAG_NEIGHBOUR_LISTS) and runs the lists kernel, context B carries
no list flag and runs the tile kernel, which the LIO tests pin to the oracle.  After every matching call A's lists counter of
lio_search_path() has advanced and B's is still 0; every comparison is bit for bit.  Run on the MI355X box with ``-m gpu``.
"""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation as R

pytestmark = pytest.mark.gpu

FOLLOW, LISTS, LIO_REF = 128, 16, 4
RES = 0.5
KW = dict(voxel_resolution=RES, num_neighbors=27)
OFF_R0, OFF_T0 = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]


def _state(T_wl, off_rpy=(0.01, -0.02, 0.03), off_t=(0.1713, 0.0, 0.05925)):   # as tests/test_gpu_lio.py
    offR = R.from_euler("xyz", off_rpy)
    Til = np.eye(4); Til[:3, :3] = offR.as_matrix(); Til[:3, 3] = off_t
    Twi = T_wl @ np.linalg.inv(Til)
    return R.from_matrix(Twi[:3, :3]).as_quat(), Twi[:3, 3], offR.as_quat(), np.asarray(off_t)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


class Pair:
    """A (lists kernel) and B (tile kernel) driven through the same calls; every call compares its results bit for bit."""

    def __init__(self, pcm, target, flags_a=FOLLOW, flags=0, **kw):
        cfg = dict(KW); cfg.update(kw)
        self.ref = bool(flags & LIO_REF)
        self.a = pcm.P2PlaneRegistration(0, flags=flags | flags_a, **cfg)
        self.b = pcm.P2PlaneRegistration(0, flags=flags, **cfg)
        self.a.set_input_target(target); self.b.set_input_target(target)
        self.n = 0

    def both(self):
        return (self.a, self.b)

    def source(self, scan):
        self.n = len(scan)
        for g in self.both():
            g.set_input_source(scan)

    def obs(self, st, ext, rematch, min_eff=1):
        before = self.a.lio_search_path()
        ra, rb = self.a.obs_model(*st, ext, rematch), self.b.obs_model(*st, ext, rematch)
        assert _same_bits(ra[0], rb[0]) and _same_bits(ra[1], rb[1])             # HTH, HTh
        assert ra[2] == rb[2] and _same_bits(np.float64(ra[3]), np.float64(rb[3])) and ra[4] == rb[4]   # n_eff, sum_h2, valid
        assert ra[2] >= min_eff
        pa, pb = self.a.get_planes(self.n), self.b.get_planes(self.n)
        if self.ref:
            # reference semantics: plane_coef_[i] is written only where esti_plane ran, the other rows are whatever the buffer held;
            # a row that is a plane (unit normal) in either context must be the same plane in both
            unit = lambda p: np.abs(np.linalg.norm(np.nan_to_num(p[:, :3].astype(np.float64), posinf=0, neginf=0), axis=1) - 1.0) < 1e-3
            rows = unit(pa) | unit(pb)
            assert rows.sum() >= min_eff
            pa, pb = pa[rows], pb[rows]
        assert _same_bits(pa, pb)
        if self.ref:
            (res_a, sel_a), (res_b, sel_b) = self.a.get_lio_members(self.n), self.b.get_lio_members(self.n)
            assert _same_bits(res_a, res_b) and np.array_equal(sel_a, sel_b)
        after = self.a.lio_search_path()
        if rematch:
            assert after[0] == before[0] + 1 and after[1] == before[1]           # served by the lists kernel
        else:
            assert after == before
        assert self.b.lio_search_path()[0] == 0
        return ra

    def map_incremental(self, st, fs=0.5, inited=True):
        na, nb = self.a.map_incremental(*st, fs, inited), self.b.map_incremental(*st, fs, inited)
        assert na == nb
        ta, tb = self.a.get_target(), self.b.get_target()
        assert _same_bits(ta, tb)                                                   # point for point
        return na, len(ta)


@pytest.fixture(scope="module")
def world(synth):
    """A 60 000-point submap and four 6 000-point Livox frames along a 0.6 m / frame track (computed once, never changed)."""
    scene = synth.scene_for_points(1234, 60000, 8.0)
    submap = synth.sample_submap(scene, 60000, 4321)
    T = synth.sensor_pose(scene, 77)
    frames = []
    for f in range(4):
        Tf = T.copy(); Tf[:3, 3] += Tf[:3, 0] * 0.6 * f
        scan, _ = synth.livox_scan(scene, Tf, 6000, 555 + f)
        frames.append((Tf, scan, synth.custom_msg(*synth.livox_scan(scene, Tf, 6000, 555 + f, point_filter_num=1))))
    return submap, frames


def _frame_calls(pr, Tf, ext):
    """obs_model(rematch) and two non-matching calls at perturbed states, then MapIncremental."""
    pr.obs(_state(Tf), ext, True, min_eff=500)
    for k, d in enumerate(((0.03, -0.02, 0.01), (-0.02, 0.04, 0.015))):
        Tk = Tf.copy(); Tk[:3, 3] += d
        Tk[:3, :3] = Tk[:3, :3] @ R.from_rotvec([0.002 * (k + 1), -0.001, 0.003]).as_matrix()
        pr.obs(_state(Tk), ext, False, min_eff=500)
    return pr.map_incremental(_state(Tf))


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("sort_source", [0, 1])
@pytest.mark.parametrize("ref", [0, LIO_REF])
def test_obs_model_three_frames(pcm, world, ref, sort_source, ext):
    """Test 1: three frames of match, two updates, MapIncremental, new scan."""
    submap, frames = world
    pr = Pair(pcm, submap, flags=ref, sort_source=sort_source)
    for Tf, scan, _ in frames[:3]:
        pr.source(scan)
        added, _ = _frame_calls(pr, Tf, bool(ext))
        assert 0 < added < len(scan)
    info = pr.a.neighbour_list_info()
    assert info["lists"] > 0 and info["updates"] + info["rebuilds"] == 3          # every MapIncremental was followed (get_target brings map and lists up to date)
    assert pr.a.lio_search_path() == (3, 0) and pr.b.lio_search_path() == (0, 3)


def _voxels(pts):
    return len(np.unique(np.round(pts[:, :3] / np.float32(RES)).astype(np.int64), axis=0))


def test_eviction(pcm, world):
    """Test 2: the capacity is one voxel above the submap's, so every frame's new voxels evict as many old ones: after each
    MapIncremental the log is shorter than log + added (whole voxels went) and holds at most capacity - 1 voxels."""
    submap, frames = world
    cap = _voxels(submap) + 2
    pr = Pair(pcm, submap, map_capacity=cap, sort_source=0)
    n_log = len(submap)
    evicting = 0
    for Tf, scan, _ in frames[:3]:
        pr.source(scan)
        added, n_now = _frame_calls(pr, Tf, False)
        pr.source(scan)                      # the next prepare() merges, evicts and updates the lists; the map shows it afterwards
        pr.obs(_state(Tf), False, True, min_eff=500)
        got = pr.a.get_target()
        assert _same_bits(got, pr.b.get_target())
        fell = len(got) < n_log + added
        evicting += int(fell)
        if fell:
            assert _voxels(got) <= cap - 1
        n_log = len(got)
    assert evicting >= 2
    assert pr.a.stats()["lru_batch_hazards"] == pr.b.stats()["lru_batch_hazards"]
    assert pr.a.neighbour_list_info()["updates"] >= 2


def _edge_map_and_scan(submap):
    """Features far outside the submap, each with scan points (body = world: identity state) that walk into them."""
    rng = np.random.default_rng(17)
    lo = submap[:, :3].min(0)
    def at(*c): return (np.round((lo - np.float32(c)) / RES) * RES).astype(np.float32)   # a voxel centre
    maps, scans = [], []
    c = at(30, 0, 0)                                            # a voxel with 300 points: runs longer than kKeyedMaxRun = 128
    dense = c + rng.uniform(-0.24, 0.24, (300, 3)).astype(np.float32); dense[:, 2] = c[2] + 0.01 * (dense[:, 0] - c[0])
    maps.append(dense); scans.append(c + rng.uniform(-0.6, 0.6, (60, 3)).astype(np.float32) * np.float32([1, 1, 0.05]))
    c = at(0, 30, 0)                                            # a lattice patch: exact ties, points on cell boundaries (+-0.25 m)
    gx, gy = np.meshgrid(np.arange(-8, 9), np.arange(-8, 9))
    lat = np.stack([gx.ravel() * 0.25, gy.ravel() * 0.25, np.zeros(gx.size)], 1).astype(np.float32) + c
    maps.append(lat)
    cx, cy = np.meshgrid(np.arange(-6, 6), np.arange(-6, 6))
    mids = np.stack([cx.ravel() * 0.25 + 0.125, cy.ravel() * 0.25 + 0.125, np.full(cx.size, 0.0625)], 1).astype(np.float32) + c   # four nodes at the same distance
    edges = np.stack([cx.ravel() * 0.25 + 0.25, cy.ravel() * 0.25, np.full(cx.size, 0.03125)], 1).astype(np.float32) + c            # on the rounding boundary
    scans += [mids, edges]
    for k, m in enumerate((4, 3, 2, 1)):                        # isolated clumps: 4- and 3-neighbour fits, then fewer than 3
        c = at(0, 0, 30 + 10 * k)
        clump = c + np.float32([[0.1, 0.0, 0.0], [-0.1, 0.05, 0.0], [0.0, -0.1, 0.01], [0.05, 0.1, 0.0]])[:m]
        maps.append(clump); scans.append(c + rng.uniform(-0.3, 0.3, (12, 3)).astype(np.float32) * np.float32([1, 1, 0.1]))
    scans.append(at(60, 60, 60) + rng.uniform(-1, 1, (10, 3)).astype(np.float32))      # a region with no neighbour at all
    extra = np.concatenate(maps)
    target = np.concatenate([submap[:, :3], extra]).astype(np.float32)
    scan = np.concatenate(scans).astype(np.float32)
    scan = np.concatenate([scan, np.float32([[1e7, -1e7, 1e7], [np.nan, np.nan, np.nan], [np.inf, 0, 0]])])   # beyond the key range, not finite
    return target, scan


@pytest.mark.parametrize("ref", [0, LIO_REF])
def test_walk_edge_cases(pcm, world, ref):
    """Test 3: long runs, ties, 3- and 4-neighbour fits, fewer than three neighbours, none, non-finite and out-of-range scan points."""
    submap, frames = world
    target, scan = _edge_map_and_scan(submap)
    pr = Pair(pcm, target, flags=ref, sort_source=0)
    pr.source(scan)
    I = np.eye(4)
    st = (R.from_matrix(I[:3, :3]).as_quat(), I[:3, 3], OFF_R0, OFF_T0)
    r = pr.obs(st, True, True, min_eff=50)
    planes = pr.a.get_planes(len(scan))
    assert np.isnan(planes[-3:, 0]).all() if not ref else True
    T2 = I.copy(); T2[:3, 3] = [0.004, -0.003, 0.002]
    st2 = (st[0], T2[:3, 3], OFF_R0, OFF_T0)
    pr.obs(st2, True, False, min_eff=50)
    # MapIncremental refuses a scan that would put such points into the map (tile kernel or lists alike), so they leave first
    pr.source(scan[:-3])
    pr.obs(st, True, True, min_eff=50)
    added, _ = pr.map_incremental(st)                    # reads nn[0] and nn[4]: ~0u for the points with no / fewer than five neighbours
    assert 0 < added < len(scan)
    pr.obs(st2, False, True, min_eff=50)                 # the grown map, through the updated lists
    assert r[2] < len(scan) - 3


def test_lio_update_and_trace(pcm, world):
    """Test 4: pcm_lio_update on two frames (the LIO_DEV instantiation), flag against none: x, P, counters and every trace record."""
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import lio_iekf_ref as ref
    import lio_update_case as case
    submap, frames = world
    pr = Pair(pcm, submap, sort_source=1)
    P0 = np.diag(ref.INIT_P_DIAG)
    for f, (Tf, scan, _) in enumerate(frames[:2]):
        pr.source(scan)
        x0 = case.filter_state(case.perturb(Tf, 0.05, 0.5))
        before = pr.a.lio_search_path()
        ra, rb = pr.a.lio_update(x0, P0, extrinsic_est_en=bool(f)), pr.b.lio_update(x0, P0, extrinsic_est_en=bool(f))
        assert (ra.iterations, ra.rematches, ra.valid_calls, ra.t, ra.n_eff_last) == (rb.iterations, rb.rematches, rb.valid_calls, rb.t, rb.n_eff_last)
        assert ra.status == 0 and ra.valid_calls >= 2 and ra.n_eff_last > 500
        assert _same_bits(ref.state_to_vec(ra.x), ref.state_to_vec(rb.x)) and _same_bits(ra.P, rb.P)
        for k in range(ra.iterations):
            ta, tb = pr.a.lio_update_trace(k), pr.b.lio_update_trace(k)
            assert ta["converge"] == tb["converge"] and ta["n_eff"] == tb["n_eff"]
            assert _same_bits(ta["HTH"], tb["HTH"]) and _same_bits(ta["HTh"], tb["HTh"]) and _same_bits(ta["dx_"], tb["dx_"])
            assert _same_bits(ref.state_to_vec(ta["x"]), ref.state_to_vec(tb["x"]))
        after = pr.a.lio_search_path()
        assert after == (before[0] + ra.rematches, 0) and ra.rematches >= 1
        assert pr.b.lio_search_path() == (0, after[0])
        assert _same_bits(pr.a.get_planes(len(scan)), pr.b.get_planes(len(scan)))
        xs = ra.x
        pr.map_incremental((xs["rot"], xs["pos"], xs["off_R"], xs["off_T"]))


def test_frame_calls(pcm, world):
    """Test 5: lio_frame_begin -> lio_update -> lio_frame_end over three frames: the scan, the update and the map, as
    tests/test_gpu_lio_frame.py compares them."""
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import lio_iekf_ref as ref
    import lio_update_case as case
    submap, frames = world
    pr = Pair(pcm, submap, map_capacity=1000000)
    P0 = np.diag(ref.INIT_P_DIAG)
    kw = dict(num_scans=6, point_filter_num=1, blind=0.1, leaf_size=0.5)
    for Tf, _, msg in frames[:3]:
        x0 = case.filter_state(case.perturb(Tf, 0.05, 0.5))
        st0 = (x0["rot"], x0["pos"], x0["off_R"], x0["off_T"])
        na, nb = pr.a.lio_frame_begin(msg, None, *st0, **kw), pr.b.lio_frame_begin(msg, None, *st0, **kw)
        assert na == nb > 500 and _same_bits(pr.a.get_source(), pr.b.get_source())
        ra, rb = pr.a.lio_update(x0, P0), pr.b.lio_update(x0, P0)
        assert ra.iterations == rb.iterations and ra.rematches == rb.rematches and ra.valid_calls == rb.valid_calls >= 2
        assert _same_bits(ref.state_to_vec(ra.x), ref.state_to_vec(rb.x)) and _same_bits(ra.P, rb.P)
        xs = ra.x
        ea = pr.a.lio_frame_end(xs["rot"], xs["pos"], xs["off_R"], xs["off_T"], 0.5, True)
        eb = pr.b.lio_frame_end(xs["rot"], xs["pos"], xs["off_R"], xs["off_T"], 0.5, True)
        assert ea == eb > 0
        ta, tb = pr.a.get_target(), pr.b.get_target()
        assert ta.shape == tb.shape and _same_bits(ta, tb)
    pa = pr.a.lio_search_path()
    assert pa[0] >= 3 and pa[1] == 0 and pr.b.lio_search_path() == (0, pa[0])


def test_static_target_and_shared(pcm, world):
    """Test 6: the contiguous instantiation under PCM_FLAG_NEIGHBOUR_LISTS, on its own target and on one shared by share_target."""
    submap, frames = world
    Tf, scan, _ = frames[0]
    pr = Pair(pcm, submap, flags_a=LISTS)
    pr.source(scan)
    pr.obs(_state(Tf), True, True, min_eff=500)
    T1 = Tf.copy(); T1[:3, 3] += [0.03, -0.02, 0.01]
    pr.obs(_state(T1), True, False, min_eff=500)
    pr.obs(_state(T1), False, True, min_eff=500)
    info = pr.a.neighbour_list_info()
    assert info["lists"] > 0 and info["updates"] == 0 and pr.a.lio_search_path() == (2, 0)
    s = pcm.P2PlaneRegistration(0, flags=LISTS, **KW)
    s.share_target(pr.a)
    s.set_input_source(frames[1][1])
    pr.b.set_input_source(frames[1][1])
    n = len(frames[1][1])
    for st, ext, rematch in ((_state(frames[1][0]), False, True), (_state(T1), False, False)):
        rs, rb = s.obs_model(*st, ext, rematch), pr.b.obs_model(*st, ext, rematch)
        assert _same_bits(rs[0], rb[0]) and _same_bits(rs[1], rb[1]) and rs[2] == rb[2] > 500 and rs[3] == rb[3]
        assert _same_bits(s.get_planes(n), pr.b.get_planes(n))
    assert s.lio_search_path() == (1, 0) and pr.b.lio_search_path()[0] == 0


def _runs(g):
    """list voxel (integer coordinates) -> xyz of its real entries, in run order (the logic of tests/test_gpu_following_lists.py)"""
    centres, starts, xyz, _ = g.get_neighbour_lists()
    assert np.all(starts % 4 == 0)
    pad = np.isinf(xyz[:, 0])
    keys = np.round(centres / RES).astype(np.int64)
    out = {}
    for r in range(len(centres)):
        s, e = int(starts[r]), int(starts[r + 1])
        real = ~pad[s:e]
        assert not real[int(real.sum()):].any()    # pad entries only at the run's end
        assert int((~real).sum()) < 4
        out[tuple(keys[r])] = xyz[s:e][real]
    return out


def _same_as_fresh_build(pcm, a, scan, nn):
    f = pcm.P2PlaneRegistration(0, optimizer="GN", voxel_resolution=RES, flags=LISTS, num_neighbors=nn, sort_source=0)
    f.set_input_target(a.get_target()); f.set_input_source(scan)
    f.evaluate_cost(np.eye(4))
    ra, rf = _runs(a), _runs(f)
    for key, run in rf.items():
        assert key in ra, "a list voxel of the fresh build is missing"
        assert _same_bits(ra[key], run), key
    empty = 0
    for key in set(ra) - set(rf):
        assert len(ra[key]) == 0, "a list voxel only the following lists hold must be empty"
        empty += 1
    return empty, max(len(v) for v in ra.values())


@pytest.mark.parametrize("nn", [7, 19, 27])
def test_rewrite_equals_fresh_build(pcm, world, nn):
    """Test 7: the wave-per-run rewrite.  A lonely voxel comes first in the log (the oldest for the LRU), the capacity is one voxel
    above the map's; the batches grow one cell's run past 64 and past 256 entries, make list voxels at negative coordinates and
    evict the lonely voxel, whose lists become empty.  The export does not maintain w after an update (the merges renumber the
    map's array), so w is not compared."""
    submap, _ = world
    body = submap[:12000, :3]
    lo = body.min(0)
    lonely = (np.round((np.minimum(lo, np.float32(0)) - np.float32(40)) / RES) * RES + np.float32([[0.01, 0.0, 0.0], [0.0, 0.02, 0.0], [0.0, 0.0, 0.03]])).astype(np.float32)
    base = np.concatenate([lonely, body]).astype(np.float32)
    cap = _voxels(base) + 3
    scan = body[::5]
    a = pcm.P2PlaneRegistration(0, optimizer="GN", voxel_resolution=RES, flags=FOLLOW, num_neighbors=nn, sort_source=0, map_capacity=cap)
    a.set_input_target(base); a.set_input_source(scan)
    I = np.eye(4)
    a.evaluate_cost(I)
    rng = np.random.default_rng(3)
    lo = np.minimum(lo, np.float32(0))                                                # everything below lies at negative coordinates
    spot = (np.round((lo - np.float32(20)) / RES) * RES).astype(np.float32)          # an empty neighbourhood
    grow70 = spot + rng.uniform(-0.2, 0.2, (70, 3)).astype(np.float32)
    grow200 = spot + rng.uniform(-0.2, 0.2, (200, 3)).astype(np.float32)
    far = (lo - np.float32(25) + rng.uniform(-1.5, 1.5, (40, 3))).astype(np.float32)   # new bricks and list voxels, more voxels than the capacity has room for
    near = body[:3000] + np.float32(0.01)
    for batch in (grow70, near, grow200, far):
        a.target_insert(batch)
        a.evaluate_cost(I)
    info = a.neighbour_list_info()
    print(info)
    assert info["updates"] >= 1 and info["in_place"] + info["relocated"] > 0
    got = a.get_target()
    assert not (np.abs(got - lonely[0]).max(1) < 1.0).any()                            # the lonely voxel was evicted
    empty, longest = _same_as_fresh_build(pcm, a, scan, nn)
    assert empty >= 1 and longest > 256
    assert (got < -19).all(1).any()


def test_default_untouched(pcm, world):
    """Test 8: without a list flag the LIO calls stay on the tile kernel, also once the second-use policy has built lists."""
    submap, frames = world
    Tf, scan, _ = frames[0]
    g = pcm.P2PlaneRegistration(0, **KW)
    g.set_input_target(submap); g.set_input_source(scan)
    g.obs_model(*_state(Tf), False, True)
    g.obs_model(*_state(Tf), False, True)
    assert g.lio_search_path() == (0, 2)
    g.reset_stats()
    assert g.lio_search_path() == (0, 0)
