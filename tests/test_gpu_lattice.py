"""P2PLANE, the LIO measurement model and the NDT operators on lattice clouds (tests/lattice.py): candidates tie in distance and points
lie exactly on voxel boundaries, so the kNN visit order (cells in nearby_grids_ order, a cell's points in the map's input order, strict
`<`; ivox3d.h:132-235), the stability of the map build and the cell rules decide the result.  Every device path that restates that order
-- the tile kernel with the LDS grid (64) and with per-lane global probing (64|1), k_linearize_counted (8), k_linearize_lists (16),
linearize_reforder.hip (32) -- against the oracle, per point and bit for bit.  tests/test_lattice_fixture.py shows with the oracle alone
that a wrong order cannot pass here.  Run on the MI355X box with ``-m gpu``.
"""
import numpy as np
import pytest

from helpers import HB_RTOL, POSE_TOL_M, POSE_TOL_RAD, pose_error, rel_err
from lattice import lattice_pair

pytestmark = pytest.mark.gpu

TILE, NO_LDS, COUNTED, LISTS, REF_ORDER = 64, 1, 8, 16, 32
KERNELS = [TILE, TILE | NO_LDS, COUNTED, LISTS, REF_ORDER]
PAIR = (0, 4000, 40000)

_oracle_cache = {}


def _maps(info, submap):
    return {"forward": submap, "reversed": info["submap_reversed"]}


def _oracle_linearize(direction, res, nn, order, n):
    """One oracle pass at the lattice pose per configuration, shared by the tests: (planes, selected, cost, H, b, inliers)."""
    key = (direction, res, nn, order, n)
    if key not in _oracle_cache:
        from oracle import Oracle
        scan, submap, T, info = lattice_pair(*PAIR)
        o = Oracle("P2PLANE", "GN", voxel_resolution=res, num_neighbors=nn)
        o.set_knn_order(order)
        o.set_input_target(_maps(info, submap)[direction]); o.set_input_source(scan[:n])
        c, H, b = o.linearize(T)
        pl, sel = o.get_planes(n)
        for a in (pl, sel, H, b):
            a.setflags(write=False)
        _oracle_cache[key] = (pl, sel, c, H, b, o.num_inliers)
    return _oracle_cache[key]


def _reg(pcm, submap, scan, optimizer="GN", **kw):
    g = pcm.P2PlaneRegistration(0, optimizer=optimizer, **kw)
    g.set_input_target(submap); g.set_input_source(scan)
    return g


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_sums(got, ref, rtol):
    c1, H1, b1, inl = got
    _, _, c0, H0, b0, inl0 = ref
    print("inliers %d / %d  rel_err H %.2e b %.2e cost %.2e" % (inl, inl0, rel_err(H1, H0), rel_err(b1, b0), abs(c1 - c0) / abs(c0)))
    assert inl == inl0 and inl0 > 0
    assert rel_err(H1, H0) < rtol and rel_err(b1, b0) < rtol and abs(c1 - c0) <= rtol * abs(c0)


def _check_per_point(g, T, n, ref, rtol):
    """Selection mask equal, selected planes bit-identical (sign bits included), inlier count exact, sums within rtol."""
    got = g.evaluate_cost(T)
    po, so = ref[0], ref[1]
    pg = g.get_planes(n)
    sg = ~np.isnan(pg[:, 0])
    wrong = int((so != sg).sum())
    both = so & sg
    differ = int(np.any(_bits(po[both]) != _bits(pg[both]), axis=1).sum())
    print("selected %d (oracle %d): %d flags and %d planes differ" % (sg.sum(), so.sum(), wrong, differ))
    assert wrong == 0 and differ == 0
    _check_sums(got, ref, rtol)


def _same_linearize(a, b, T, n):
    """Two kernels, same device order of the scan: planes and sums bit for bit (as test_gpu_neighbour_lists._same_linearize)."""
    ra, rb = a.evaluate_cost(T), b.evaluate_cost(T)
    pa, pb = a.get_planes(n), b.get_planes(n)
    assert np.array_equal(np.isnan(pa[:, 0]), np.isnan(pb[:, 0]))
    ok = ~np.isnan(pa[:, 0])
    assert np.array_equal(_bits(pa[ok]), _bits(pb[ok]))
    assert ra[3] == rb[3] and ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    return ra


@pytest.mark.parametrize("res", [0.5, 0.25])
@pytest.mark.parametrize("nn", [1, 7, 19, 27])
@pytest.mark.parametrize("flags", KERNELS)
def test_linearize_at_the_lattice_pose_matches_the_oracle_per_point(pcm, flags, nn, res):
    """sort_source=0: every point's selection flag and plane against the oracle, for the map in forward and in reversed input order
    (each against its own oracle run: the two differ in hundreds of planes).  sort_source=1: the device re-orders the scan, so the
    kernel is compared with the tile kernel bit for bit and with the oracle through the inlier count and the sums.  The row order of
    flag 32 is the oracle's libstdc++ mode; its sums are held to 1e-9 as in test_gpu_reforder.py."""
    scan, submap, T, info = lattice_pair(*PAIR)
    n = len(scan)
    order, rtol = ("libstdcxx", 1e-9) if flags == REF_ORDER else ("ascending", HB_RTOL)
    kw = dict(voxel_resolution=res, num_neighbors=nn)
    for direction, m in _maps(info, submap).items():
        ref = _oracle_linearize(direction, res, nn, order, n)
        _check_per_point(_reg(pcm, m, scan, sort_source=0, flags=flags, **kw), T, n, ref, rtol)
        a = _reg(pcm, m, scan, sort_source=1, flags=flags, **kw)
        a.align(T.astype(np.float32))      # the device order of the scan is fixed by the first align's guess
        if flags in (TILE, REF_ORDER):
            got = a.evaluate_cost(T)
        else:
            b = _reg(pcm, m, scan, sort_source=1, flags=TILE, **kw)
            b.align(T.astype(np.float32))
            got = _same_linearize(a, b, T, n)
        _check_sums(got, ref, rtol)


@pytest.mark.parametrize("n", [257, 449, 1000])
@pytest.mark.parametrize("flags", KERNELS)
def test_ragged_tail_meets_ties(pcm, flags, n):
    """The first n scan points: a partial last tile on tied candidates."""
    scan, submap, T, info = lattice_pair(*PAIR)
    order, rtol = ("libstdcxx", 1e-9) if flags == REF_ORDER else ("ascending", HB_RTOL)
    for direction, m in _maps(info, submap).items():
        ref = _oracle_linearize(direction, 0.5, 27, order, n)
        _check_per_point(_reg(pcm, m, scan[:n], sort_source=0, flags=flags, voxel_resolution=0.5, num_neighbors=27), T, n, ref, rtol)


ALIGN_PAIRS = [(0, 4000, 40000), (1, 3000, 30000), (6, 2777, 26000)]     # the oracle converges on these from the lattice guess (3 - 4 rounds)


@pytest.mark.parametrize("sort_source", [0, 1])
@pytest.mark.parametrize("optimizer", ["GN", "LM"])
def test_align_from_the_lattice_guess(pcm, optimizer, sort_source):
    """The first linearisation is full of ties, the later rounds are generic.  Oracle: counters equal, pose within the parity
    tolerance.  Flags 16 and 8 equal flag 64 bit for bit, singly and through align_batch with three such pairs."""
    from oracle import Oracle
    from oracle.loader import result_T
    pairs = [lattice_pair(*p) for p in ALIGN_PAIRS]
    guesses = np.stack([T.astype(np.float32) for _, _, T, _ in pairs])
    res = {}
    for flags in (TILE, LISTS, COUNTED):
        regs = [_reg(pcm, sm, sc, optimizer, sort_source=sort_source, flags=flags) for sc, sm, _, _ in pairs]
        res[flags] = (pcm.align_batch(regs, guesses), [g.align(G) for g, G in zip(regs, guesses)])
    for k, (sc, sm, T, _) in enumerate(pairs):
        o = Oracle("P2PLANE", optimizer, voxel_resolution=0.5, num_neighbors=27)
        o.set_input_target(sm); o.set_input_source(sc)
        ro = o.align(guesses[k])
        base = res[TILE][1][k]
        dt, dr = pose_error(result_T(ro), base.T64)
        print("pair %d: %d iterations, %d inliers, |dt| %.2e |dR| %.2e" % (k, base.iterations, base.num_inliers, dt, dr))
        assert dt < POSE_TOL_M and dr < POSE_TOL_RAD
        assert base.iterations == ro.iterations and base.num_linearize == ro.num_linearize and base.num_compute_error == ro.num_compute_error
        assert base.num_inliers == ro.num_inliers and base.converged == bool(ro.converged) and base.converged
        for flags in (TILE, LISTS, COUNTED):
            for r in (res[flags][0][k], res[flags][1][k]):
                assert np.array_equal(r.T64, base.T64) and np.array_equal(r.H, base.H) and r.cost == base.cost
                assert r.iterations == base.iterations and r.num_inliers == base.num_inliers and r.num_linearize == base.num_linearize
                assert r.num_compute_error == base.num_compute_error and r.converged == base.converged


LIO_OFF_T = np.array([0.25, -0.125, 0.0625])       # a lattice extrinsic offset
LIO_BATCHES = (17000, 9000, 14000)                 # the map arrives in three batches of unequal size


@pytest.mark.parametrize("reference_semantics", [False, True])
@pytest.mark.parametrize("sort_source", [0, 1])
def test_lio_obs_model_on_a_map_merged_from_batches(pcm, sort_source, reference_semantics):
    """The sliding iVox map built by three adds, each merged into an index that is already built (the stable merge of
    voxel_hash.hip meets tied points that arrive in different batches), then ObsModel at lattice states: identity rotations, the
    position and the extrinsic offset on the lattice, so every transformed point is a lattice point again.  As
    test_gpu_lio.py::test_obs_model_matches_oracle, the valid-point count exact; residuals_ and point_selected_surf_ equal in the
    reference's semantics."""
    from oracle import Oracle
    scan, submap, T, info = lattice_pair(*PAIR)
    n = len(scan)
    body = (scan.astype(np.float64) - LIO_OFF_T).astype(np.float32)
    assert np.array_equal(body + (T[:3, 3] + LIO_OFF_T).astype(np.float32), info["scan_world"])
    kw = dict(voxel_resolution=0.5, num_neighbors=27)
    o = Oracle("P2PLANE", "GN", **kw)
    o.set_lio_reference_semantics(reference_semantics)
    g = pcm.P2PlaneRegistration(0, sort_source=sort_source, flags=pcm.capi.PCM_FLAG_LIO_REFERENCE_SEMANTICS if reference_semantics else 0, **kw)
    ident = (0.0, 0.0, 0.0, 1.0)
    step = np.array([0.0625, 0.0, -0.0625])        # a second lattice state: other ties
    states = ((T[:3, 3], True), (T[:3, 3] + step, False), (T[:3, 3] + step, True))
    lo = 0
    for k, size in enumerate(LIO_BATCHES):
        batch = submap[lo:lo + size]; lo += size
        if k == 0:
            o.set_input_target(batch); g.set_input_target(batch)
            o.set_input_source(body); g.set_input_source(body)
        else:
            o.target_insert(batch); g.target_insert(batch)
        assert np.array_equal(g.get_target(), o.get_target())
        for pos, conv in (states if lo == len(submap) else states[:1]):
            for extrinsic in (False, True):
                st = (ident, pos, ident, LIO_OFF_T)
                H0, h0, n0, s0 = o.obs_model(*st, extrinsic, conv)
                H1, h1, n1, s1, valid = g.obs_model(*st, extrinsic, conv)
                print("batch %d: n_eff %d / %d  rel_err HTH %.2e HTh %.2e" % (k, n1, n0, rel_err(H1, H0), rel_err(h1, h0)))
                assert n1 == n0 and valid and n0 > (1000 if lo == len(submap) else 300)
                assert rel_err(H1, H0) < HB_RTOL and rel_err(h1, h0) < HB_RTOL and abs(s1 - s0) <= HB_RTOL * s0
                if not extrinsic:
                    assert not H1[6:, :].any() and not h1[6:].any()
                if reference_semantics:
                    _, res_o, sel_o = o.get_lio_members(n)
                    res_g, sel_g = g.get_lio_members(n)
                    assert np.array_equal(sel_g, sel_o)
                    assert np.array_equal(_bits(res_g), _bits(res_o))
    assert lo == len(submap)


NDT_PAIR = (0, 4000, 40000, 1.0 / 16, 60.0)       # NDT voxels need > 6 points: a denser submap


@pytest.mark.parametrize("model", ["NDT_P2D", "NDT_D2D"])
@pytest.mark.parametrize("res", [1.0, 0.5])
@pytest.mark.parametrize("nn", [1, 7, 27])
def test_ndt_boundary_points(pcm, model, res, nn):
    """floorf(v / res - 0.5f): thousands of map and scan points sit exactly on a boundary of the Gaussian voxels.  Inliers exact,
    sums within the tolerances of test_gpu_ndt.py; the neighbour rows (16) change nothing against the cell lookups (64)."""
    from oracle import Oracle
    scan, submap, T, info = lattice_pair(*NDT_PAIR)
    assert info["boundary"]["floor_half", res][0] > 500 and info["boundary"]["floor_half", res][1] > 5000
    o = Oracle(model, "LM", voxel_resolution=res, num_neighbors=nn)
    o.set_input_target(submap); o.set_input_source(scan)
    regs = {f: pcm.NdtRegistration(0, model=model, optimizer="LM", voxel_resolution=res, num_neighbors=nn, flags=f) for f in (TILE, LISTS)}
    for g in regs.values():
        g.set_input_target(submap); g.set_input_source(scan)
    c0, H0, b0 = o.linearize(T)
    T2 = T.copy(); T2[:3, 3] += [0.02, -0.01, 0.01]       # trial pose on the remembered correspondences
    e0 = o.compute_error(T2)
    got = {}
    for f, g in regs.items():
        c1, H1, b1, inl = got[f] = g.evaluate_cost(T)
        print("flags %d: inliers %d / %d  rel_err H %.2e b %.2e" % (f, inl, o.num_inliers, rel_err(H1, H0), rel_err(b1, b0)))
        assert inl == o.num_inliers and inl > 0
        assert rel_err(H1, H0) < HB_RTOL and rel_err(b1, b0) < HB_RTOL and abs(c1 - c0) <= HB_RTOL * abs(c0)
        got[f] += (g.compute_error(T2),)
        assert abs(got[f][4] - e0) <= HB_RTOL * abs(e0)
    ra, rb = got[LISTS], got[TILE]
    assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2]) and ra[3] == rb[3] and ra[4] == rb[4]


@pytest.mark.parametrize("res", [1.0, 0.5])
@pytest.mark.parametrize("nn", [0, 1, 7, 27])      # 0 = KDTREE
def test_pclndt_boundary_points(pcm, res, nn):
    """pclomp NDT: floorf(v * inv) builds the leaves, floorf(x / res) finds the neighbourhood; most lattice points sit on a leaf
    boundary.  computeDerivatives (float, default, double Hessian) and calculateScore within the tolerances of test_gpu_pclndt.py;
    the neighbour-leaf lists (16) change nothing against the cell lookups (64)."""
    from oracle import Oracle
    scan, submap, T, info = lattice_pair(*NDT_PAIR)
    assert info["boundary"]["floor", res][0] > 1000 and info["boundary"]["floor", res][1] > 10000
    regs = {f: pcm.PclNdtRegistration(0, voxel_resolution=res, num_neighbors=nn, flags=f) for f in (TILE, LISTS)}
    cfg = regs[TILE].config
    o = Oracle("NDT_OMP", "LM", voxel_resolution=cfg.voxel_resolution, num_neighbors=nn, translation_eps=cfg.translation_eps,
               max_iterations=cfg.max_iterations, ndt_step_size=float(cfg.ndt_step_size), ndt_outlier_ratio=float(cfg.ndt_outlier_ratio))
    o.set_input_target(submap); o.set_input_source(scan)
    for g in regs.values():
        g.set_input_target(submap); g.set_input_source(scan)
    pv = np.concatenate([T[:3, 3], np.zeros(3)])       # (x, y, z, roll, pitch, yaw) of the lattice pose
    s0, g0, H0 = o.ndt_derivatives(pv)
    Hd0 = o.ndt_hessian(pv)
    sc0 = o.ndt_score(T)
    for f, g in regs.items():
        s1, g1, H1 = g.ndt_derivatives(pv, "float")
        print("flags %d: score %.6f / %.6f  rel_err g %.2e H %.2e" % (f, s1, s0, rel_err(g1, g0), rel_err(H1, H0)))
        assert s0 != 0 and abs(s1 - s0) <= 1e-6 * abs(s0)
        assert rel_err(g1, g0) < 1e-5 and rel_err(H1, H0) < 1e-5
        s2, g2, _ = g.ndt_derivatives(pv, None)
        assert abs(s2 - s0) <= 1e-6 * abs(s0) and rel_err(g2, g0) < 1e-5
        _, _, Hd1 = g.ndt_derivatives(pv, "double")
        assert rel_err(Hd1, Hd0) < 1e-9
        sc1 = g.ndt_score(T)
        assert sc0 != 0 and abs(sc1 - sc0) <= 1e-12 * abs(sc0)
    for kind in ("float", None, "double"):
        ra, rb = regs[LISTS].ndt_derivatives(pv, kind), regs[TILE].ndt_derivatives(pv, kind)
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    assert regs[LISTS].ndt_score(T) == regs[TILE].ndt_score(T)
