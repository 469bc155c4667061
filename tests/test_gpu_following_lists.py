"""PCM_FLAG_FOLLOWING_LISTS: the candidate lists of a P2PLANE target stay valid while the target grows (pcm_target_insert /
pcm_map_incremental) -- the lists around the voxels a batch touched are rewritten in a pool, k_linearize_lists keeps running.
Checked bit for bit against the tile kernel (a context without any list flag, whose growing target keeps it on k_linearize), list
for list against a fresh PCM_FLAG_NEIGHBOUR_LISTS build of the final point log, and against the oracle where the map evicts.
Run on the MI355X box with ``-m gpu``.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FOLLOW, LISTS, REF_ORDER = 128, 16, 32
RES = 0.5
PCM_ERR_UNSUPPORTED = -4


def _reg(pcm, p_map, p_scan, flags=0, **kw):
    kw.setdefault("sort_source", 0)
    g = pcm.P2PlaneRegistration(0, optimizer="GN", voxel_resolution=RES, flags=flags, **kw)
    g.set_input_target(p_map); g.set_input_source(p_scan)
    return g


def _same_linearize(a, b, T, n):
    ra, rb = a.evaluate_cost(T), b.evaluate_cost(T)
    pa, pb = a.get_planes(n), b.get_planes(n)
    assert np.array_equal(np.isnan(pa[:, 0]), np.isnan(pb[:, 0]))
    ok = ~np.isnan(pa[:, 0])
    assert ok.sum() > n // 4                       # the comparison is about something
    assert np.array_equal(pa[ok], pb[ok])
    assert ra[3] == rb[3] and ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])


def _same_at_both_poses(a, b, p):
    for T in (p.T_gt, p.guess.astype(np.float64)):
        _same_linearize(a, b, T, len(p.scan))


def _runs(g):
    """list voxel (integer coordinates) -> xyz of its real entries, in run order"""
    centres, starts, xyz, _ = g.get_neighbour_lists()
    assert np.all(starts % 4 == 0)
    pad = np.isinf(xyz[:, 0])
    keys = np.round(centres / RES).astype(np.int64)
    out = {}
    for r in range(len(centres)):
        s, e = int(starts[r]), int(starts[r + 1])
        real = ~pad[s:e]
        assert not real[int(real.sum()):].any()    # pad entries only at the run's end
        out[tuple(keys[r])] = xyz[s:e][real]
    return out


def _same_as_fresh_build(pcm, a, scan, nn):
    """a's lists against the lists a PCM_FLAG_NEIGHBOUR_LISTS context builds from a's point log"""
    f = _reg(pcm, a.get_target(), scan, flags=LISTS, num_neighbors=nn)
    f.evaluate_cost(np.eye(4))
    ra, rf = _runs(a), _runs(f)
    for key, run in rf.items():
        assert key in ra, "a list voxel of the fresh build is missing"
        assert np.array_equal(ra[key], run), key
    for key in set(ra) - set(rf):
        assert len(ra[key]) == 0, "a list voxel only the following lists hold must be empty"


def _batches(p, rng):
    near = p.submap[:5000].copy(); near[:, :3] += np.float32(0.01)               # runs grow
    far = np.ones((2000, 4), np.float32)                                           # new bricks and new list voxels, negative coordinates
    far[:, :3] = rng.uniform(-1.5, 1.5, (2000, 3)) + p.submap[:, :3].min(0) - 20.0
    edge = p.submap[5000:5300].copy()                                              # brick boundaries (voxel 7|8, -1|0 ...) and the rounding boundary at +-0.25 m
    edge[:, 0] = np.repeat(np.float32([-0.25, 0.25, 3.75, -4.25, 7.75, -0.75]), 50) + rng.uniform(-1e-3, 1e-3, 300).astype(np.float32)
    return [near, far, edge]


@pytest.mark.parametrize("nn", [7, 27])
def test_follow_equals_tile_kernel_and_fresh_build(pcm, synth, nn):
    """Tests 1 and 2 of the issue: after every batch planes and sums equal the tile kernel's bit for bit; after the last the lists
    equal a fresh build's; three updates, no full rebuild."""
    p = synth.make_pair(11, 6000, 60000)
    a = _reg(pcm, p.submap, p.scan, flags=FOLLOW, num_neighbors=nn)
    b = _reg(pcm, p.submap, p.scan, num_neighbors=nn)
    _same_at_both_poses(a, b, p)
    assert a.neighbour_list_info()["lists"] > 0
    batches = _batches(p, np.random.default_rng(5))
    for batch in batches:
        a.target_insert(batch); b.target_insert(batch)
        _same_at_both_poses(a, b, p)
        assert a.neighbour_list_info()["lists"] > 0 and b.neighbour_list_info()["lists"] == 0   # b's grown target keeps it on the tile kernel
    info = a.neighbour_list_info()
    print(info)
    assert info["updates"] == len(batches) and info["rebuilds"] == 0
    assert info["relocated"] > 0 and info["live_entries"] <= info["capacity"]
    _same_as_fresh_build(pcm, a, p.scan, nn)


def test_relocation_and_rebuild(pcm, synth):
    """Test 3: with 64 entries of reserved room (plus what the grow-only allocation leaves) 40 batches into the same few voxels
    rewrite runs in place, move them and have everything built again."""
    p = synth.make_pair(11, 6000, 60000)
    a = pcm.P2PlaneRegistration(0, optimizer="GN", voxel_resolution=RES, flags=FOLLOW, sort_source=0)
    a.set_neighbour_list_headroom(0.0, 64)
    a.set_input_target(p.submap); a.set_input_source(p.scan)
    b = _reg(pcm, p.submap, p.scan)
    _same_at_both_poses(a, b, p)
    rng = np.random.default_rng(9)
    i0 = int(np.argmin(np.linalg.norm(p.submap[:, :3] - (p.T_gt[:3, 3] + [2.0, 0.0, 0.0]), axis=1)))   # a map point the scan sees
    centre = p.submap[i0, :3]
    checked_rebuild = False
    for k in range(40):
        batch = np.ones((250, 4), np.float32)
        batch[:, :3] = centre + rng.uniform(-0.4, 0.4, (250, 3))
        a.target_insert(batch); b.target_insert(batch)
        a.evaluate_cost(p.T_gt)
        if not checked_rebuild and a.neighbour_list_info()["rebuilds"] >= 1:
            checked_rebuild = True
            _same_at_both_poses(a, b, p)
            _same_as_fresh_build(pcm, a, p.scan, 27)
    info = a.neighbour_list_info()
    print(info)
    assert info["in_place"] >= 1 and info["relocated"] >= 1 and info["rebuilds"] >= 1
    _same_at_both_poses(a, b, p)
    _same_as_fresh_build(pcm, a, p.scan, 27)


def test_eviction(pcm, synth):
    """Test 4: a sliding map of 2 000 voxels; every batch evicts.  Tile kernel, oracle log, fresh build, hazards."""
    from oracle import Oracle
    cap = 2000
    p = synth.make_pair(11, 6000, 60000)
    pts = p.submap[np.argsort(p.submap[:, 0], kind="stable")]
    vox = np.round(pts[:, :3] / RES).astype(np.int64)
    n0 = 2000
    while len(np.unique(vox[:n0 + 500], axis=0)) < cap - 60:
        n0 += 500
    base, x = pts[:n0], float(pts[n0, 0])
    a = _reg(pcm, base, base[::2], flags=FOLLOW, map_capacity=cap)
    b = _reg(pcm, base, base[::2], map_capacity=cap)
    o = Oracle("P2PLANE", "GN", voxel_resolution=RES, num_neighbors=27, map_capacity=cap)
    o.set_input_target(base); o.set_input_source(base[::2])
    I = np.eye(4)
    _same_linearize(a, b, I, len(base[::2]))
    evicted = 0
    for k in range(12):
        batch = pts[(pts[:, 0] >= x + k) & (pts[:, 0] < x + k + 1.0)]
        assert len(batch) > 100
        scan = batch[::3].copy(); scan[:, :3] += np.float32(0.02)
        before = a.neighbour_list_info()
        for g in (a, b, o):
            g.target_insert(batch); g.set_input_source(scan)
        _same_linearize(a, b, I, len(scan))
        after = a.neighbour_list_info()   # every batch goes through the update (k_evicted_voxels) or the full build its policy asks for, none through invalidate-and-build
        assert (after["updates"], after["rebuilds"]) in ((before["updates"] + 1, before["rebuilds"]), (0, before["rebuilds"] + 1)), (k, before, after)
        got = a.get_target()
        assert np.array_equal(got, b.get_target()) and np.array_equal(got, o.get_target())
        evicted += int(len(got) < n0 + len(batch)); n0 = len(got)
    assert evicted == 12
    assert a.stats()["lru_batch_hazards"] == b.stats()["lru_batch_hazards"]
    info = a.neighbour_list_info()
    print(info)
    assert info["in_place"] + info["relocated"] > 0
    _same_as_fresh_build(pcm, a, scan, 27)     # against the surviving log: a run that held a point of an evicted voxel would differ


def _state(T_wl, off_rpy=(0.01, -0.02, 0.03), off_t=(0.1713, 0.0, 0.05925)):   # as tests/test_gpu_lio.py
    from scipy.spatial.transform import Rotation as R
    offR = R.from_euler("xyz", off_rpy)
    Til = np.eye(4); Til[:3, :3] = offR.as_matrix(); Til[:3, 3] = off_t
    Twi = T_wl @ np.linalg.inv(Til)
    return R.from_matrix(Twi[:3, :3]).as_quat(), Twi[:3, 3], offR.as_quat(), np.asarray(off_t)


def test_map_incremental(pcm, synth):
    """Test 5: obs_model + map_incremental as tests/test_gpu_lio.py runs them, then a P2PLANE linearize."""
    scene = synth.scene_for_points(1234, 60000, 8.0)
    submap = synth.sample_submap(scene, 60000, 4321)
    T = synth.sensor_pose(scene, 77)
    scan, _ = synth.livox_scan(scene, T, 4000, 555)
    a = _reg(pcm, submap, scan, flags=FOLLOW)
    b = _reg(pcm, submap, scan)
    _same_linearize(a, b, T, len(scan))
    for f in range(3):
        Tf = T.copy(); Tf[:3, 3] += Tf[:3, 0] * 0.6 * f
        scan, _ = synth.livox_scan(scene, Tf, 4000, 555 + f)
        added = []
        for g in (a, b):
            g.set_input_source(scan)
            g.obs_model(*_state(Tf), False, True)
            added.append(g.map_incremental(*_state(Tf), 0.5, True))
        assert added[0] == added[1] and 0 < added[0] < len(scan)
        _same_linearize(a, b, Tf, len(scan))
    assert a.neighbour_list_info()["updates"] + a.neighbour_list_info()["rebuilds"] == 3


def _same_result(x, y):
    assert np.array_equal(x.T64, y.T64) and x.iterations == y.iterations and x.num_inliers == y.num_inliers and x.cost == y.cost


def test_whole_registrations(pcm, synth):
    """Test 6: five steps of align + insert, single and through align_batch with two pairs that follow their own targets."""
    pairs = [synth.make_pair(11 + i, 6000, 60000 + 10000 * i) for i in range(2)]
    guesses = np.stack([p.guess for p in pairs])
    A = [_reg(pcm, p.submap, p.scan, flags=FOLLOW, sort_source=1) for p in pairs]
    B = [_reg(pcm, p.submap, p.scan, sort_source=1) for p in pairs]
    for step in range(5):
        _same_result(A[0].align(pairs[0].guess), B[0].align(pairs[0].guess))
        for x, y in zip(pcm.align_batch(A, guesses), pcm.align_batch(B, guesses)):
            _same_result(x, y)
        for g, h, p in zip(A, B, pairs):
            extra = p.submap[3000 * step:3000 * (step + 1)].copy(); extra[:, :3] += np.float32(0.01)
            g.target_insert(extra); h.target_insert(extra)
    for g in A:
        assert g.neighbour_list_info()["updates"] >= 4


def test_flags_and_sharing(pcm, synth):
    """Test 7: next to another kernel flag there are no lists; a shared target carries following lists, inserts are refused."""
    p = synth.make_pair(11, 6000, 60000)
    n = len(p.scan)
    extra = p.submap[:5000].copy(); extra[:, :3] += np.float32(0.01)
    r = _reg(pcm, p.submap, p.scan, flags=FOLLOW | REF_ORDER)
    q = _reg(pcm, p.submap, p.scan, flags=REF_ORDER)
    for step in range(2):
        _same_linearize(r, q, p.T_gt, n)
        assert r.neighbour_list_info()["lists"] == 0
        with pytest.raises(pcm.PcmError):
            r.get_neighbour_lists()
        r.target_insert(extra); q.target_insert(extra)
    a = _reg(pcm, p.submap, p.scan, flags=FOLLOW)
    for k in range(2):
        a.evaluate_cost(p.T_gt)
        a.target_insert(p.submap[5000 * k:5000 * (k + 1)] + np.float32([0.01, 0.01, 0.01, 0]))
    s = pcm.P2PlaneRegistration(0, optimizer="GN", voxel_resolution=RES, flags=FOLLOW, sort_source=0)
    s.set_input_source(p.scan)
    s.share_target(a)
    _same_at_both_poses(a, s, p)
    assert s.neighbour_list_info()["lists"] == a.neighbour_list_info()["lists"] > 0
    for g in (a, s):
        with pytest.raises(pcm.PcmError) as e:
            g.target_insert(extra)
        assert e.value.code == PCM_ERR_UNSUPPORTED


def test_points_outside_the_key_range_and_not_finite(pcm, synth):
    """Test 8: the scan points of tests/test_gpu_neighbour_lists.py:101-102 against a followed target; a batch that holds them is
    refused by both contexts in the same way and leaves both usable."""
    p = synth.make_pair(7, 3001, 9000, density=1.5)
    sc = p.scan.copy()
    sc[5, :3] = [1e7, -1e7, 1e7]
    sc[6, :3] = np.nan
    n = len(sc)
    a = _reg(pcm, p.submap, sc, flags=FOLLOW)
    b = _reg(pcm, p.submap, sc)
    good = p.submap[:2000].copy(); good[:, :3] += np.float32(0.01)
    bad = good[:300].copy(); bad[5, :3] = [1e7, -1e7, 1e7]; bad[6, :3] = np.nan

    def same(T):   # _same_linearize without its floor on the number of planes: this map is sparse
        ra, rb = a.evaluate_cost(T), b.evaluate_cost(T)
        pa, pb = a.get_planes(n), b.get_planes(n)
        assert np.array_equal(np.isnan(pa[:, 0]), np.isnan(pb[:, 0]))
        ok = ~np.isnan(pa[:, 0])
        assert ok.any() and np.array_equal(pa[ok], pb[ok])
        assert ra[3] == rb[3] and ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])

    same(p.T_gt)
    for g in (a, b):
        g.target_insert(good)
    same(p.T_gt); same(p.guess.astype(np.float64))
    codes = []
    for g in (a, b):
        g.target_insert(bad)
        with pytest.raises(pcm.PcmError) as e:
            g.evaluate_cost(p.T_gt)
        codes.append(e.value.code)
    assert codes[0] == codes[1]
    for g in (a, b):                      # a new target: both work again
        g.set_input_target(p.submap)
    same(p.T_gt)
    for g in (a, b):
        g.target_insert(good)
    same(p.T_gt)
    assert a.neighbour_list_info()["lists"] > 0
