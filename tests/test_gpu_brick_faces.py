"""Every kernel that finds a voxel through the brick table (csrc/brick_table.h), on a map centred on the origin: voxel and brick
coordinates of both signs, and for most scan points a brick face between their cell and one of its 26 neighbours.  One linearize at
the ground-truth pose per case, compared with the reference exactly as that model's own test compares it (helpers and tolerances of
test_gpu_lattice.py, test_gpu_ndt.py, test_gpu_pclndt.py, test_gpu_gicp.py, test_gpu_loam.py).  Run on the MI355X box with ``-m gpu``.
"""
import types

import numpy as np
import pytest

from helpers import HB_RTOL, rel_err

pytestmark = pytest.mark.gpu

TILE, NO_LDS, LISTS, REF_ORDER = 64, 1, 16, 32
N_SCAN, N_MAP = 2000, 20000
RES = 0.5                     # a brick is 8 voxels = 4 m
# (cell size, voxel of a coordinate) of every map the cases build: the conventions of pcm_device.h's CoordMode
GRIDS = ((RES, np.round),                             # P2PLANE and GICP's search grid at 0.5 m (COORD_ROUND)
         (1.0, lambda x: np.floor(x - 0.5)),          # NDT P2D and VGICP at 1 m (COORD_FLOOR_HALF, _D)
         (1.0, np.floor))                             # pclomp NDT at 1 m and LOAM's search grid at its default search_cell of 1 m (COORD_FLOOR_MUL)
_pairs = {}


def centred_pair(synth, density=None):
    """synth.make_pair with scan world and map moved by one vector, so that the map's centroid is the origin; the preconditions of
    this file are asserted on it with numpy alone, for every grid the cases use (GRIDS)."""
    if density not in _pairs:
        p = synth.make_pair(0, N_SCAN, N_MAP) if density is None else synth.make_pair(0, N_SCAN, N_MAP, density=density)
        c = p.submap[:, :3].astype(np.float64).mean(axis=0)
        submap = p.submap.copy()
        submap[:, :3] = (p.submap[:, :3].astype(np.float64) - c).astype(np.float32)
        T = p.T_gt.copy()
        T[:3, 3] -= c
        world = p.scan[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        for res, cell in GRIDS:
            bricks = cell(submap[:, :3] / res).astype(np.int64) >> 3
            assert (bricks.min(axis=0) < 0).all() and (bricks.max(axis=0) >= 0).all()
            v = cell(world / res).astype(np.int64)
            faces = (((v - 1) >> 3) != ((v + 1) >> 3)).any(axis=1)       # the 27-cell neighbourhood spans two or more bricks
            assert faces.mean() >= 0.25, faces.mean()
        scan_world = p.scan.copy()
        scan_world[:, :3] = world.astype(np.float32)
        for a in (submap, T, scan_world):
            a.setflags(write=False)
        _pairs[density] = types.SimpleNamespace(scan=p.scan, submap=submap, T_gt=T, scan_world=scan_world)
    return _pairs[density]


@pytest.mark.parametrize("flags", [TILE | NO_LDS, LISTS, REF_ORDER])
def test_p2plane(pcm, synth, flags):
    """knn_global (64|1), the candidate lists (16) and the reference-order kernel (32): per point against the oracle."""
    from oracle import Oracle
    from test_gpu_lattice import _check_per_point, _reg
    p = centred_pair(synth)
    n = len(p.scan)
    order, rtol = ("libstdcxx", 1e-9) if flags == REF_ORDER else ("ascending", HB_RTOL)
    o = Oracle("P2PLANE", "GN", voxel_resolution=RES, num_neighbors=27)
    o.set_knn_order(order)
    o.set_input_target(p.submap); o.set_input_source(p.scan)
    c, H, b = o.linearize(p.T_gt)
    pl, sel = o.get_planes(n)
    g = _reg(pcm, p.submap, p.scan, sort_source=0, flags=flags, voxel_resolution=RES, num_neighbors=27)
    _check_per_point(g, p.T_gt, n, (pl, sel, c, H, b, o.num_inliers), rtol)


@pytest.mark.parametrize("nn", [7, 27])
def test_ndt_p2d(pcm, synth, nn):
    """k_ndt's cell lookups (64) and its neighbour rows (16), as test_gpu_lattice.test_ndt_boundary_points."""
    from oracle import Oracle
    p = centred_pair(synth, 60.0)
    o = Oracle("NDT_P2D", "LM", voxel_resolution=1.0, num_neighbors=nn)
    o.set_input_target(p.submap); o.set_input_source(p.scan)
    c0, H0, b0 = o.linearize(p.T_gt)
    got = {}
    for f in (TILE, LISTS):
        g = pcm.NdtRegistration(0, model="NDT_P2D", optimizer="LM", voxel_resolution=1.0, num_neighbors=nn, flags=f)
        g.set_input_target(p.submap); g.set_input_source(p.scan)
        c1, H1, b1, inl = got[f] = g.evaluate_cost(p.T_gt)
        print("flags %d: inliers %d / %d  rel_err H %.2e b %.2e" % (f, inl, o.num_inliers, rel_err(H1, H0), rel_err(b1, b0)))
        assert inl == o.num_inliers and inl > 0
        assert rel_err(H1, H0) < HB_RTOL and rel_err(b1, b0) < HB_RTOL and abs(c1 - c0) <= HB_RTOL * abs(c0)
    ra, rb = got[LISTS], got[TILE]
    assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2]) and ra[3] == rb[3]


@pytest.mark.parametrize("nn", [7, 27, 0])      # 0 = KDTREE
def test_pclndt(pcm, synth, nn):
    """neighbour_leaves cell by cell (64) and through the leaf lists (16), as test_gpu_pclndt.test_derivatives_match_oracle."""
    from oracle import Oracle
    from test_gpu_pclndt import _pvec
    p = centred_pair(synth, 60.0)
    regs = {f: pcm.PclNdtRegistration(0, voxel_resolution=1.0, num_neighbors=nn, flags=f) for f in (TILE, LISTS)}
    cfg = regs[TILE].config
    o = Oracle("NDT_OMP", "LM", voxel_resolution=cfg.voxel_resolution, num_neighbors=nn, translation_eps=cfg.translation_eps,
               max_iterations=cfg.max_iterations, ndt_step_size=float(cfg.ndt_step_size), ndt_outlier_ratio=float(cfg.ndt_outlier_ratio))
    o.set_input_target(p.submap); o.set_input_source(p.scan)
    for g in regs.values():
        g.set_input_target(p.submap); g.set_input_source(p.scan)
    pv = _pvec(p.T_gt)
    s0, g0, H0 = o.ndt_derivatives(pv)
    Hd0 = o.ndt_hessian(pv)
    for f, g in regs.items():
        s1, g1, H1 = g.ndt_derivatives(pv, "float")
        print("flags %d: score %.6f / %.6f  rel_err g %.2e H %.2e" % (f, s1, s0, rel_err(g1, g0), rel_err(H1, H0)))
        assert s0 != 0 and abs(s1 - s0) <= 1e-6 * abs(s0)
        assert rel_err(g1, g0) < 1e-5 and rel_err(H1, H0) < 1e-5
        _, _, Hd1 = g.ndt_derivatives(pv, "double")
        assert rel_err(Hd1, Hd0) < 1e-9
    ra, rb = regs[LISTS].ndt_derivatives(pv, "float"), regs[TILE].ndt_derivatives(pv, "float")
    assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])


@pytest.mark.parametrize("model,kw", [("GICP", {}), ("VGICP", {"num_neighbors": 7})])
def test_gicp(pcm, synth, model, kw):
    """scan_box / the segment loop behind the covariances and the nearest neighbour (GICP), the voxel look-ups of VGICP: as
    test_gpu_gicp.test_covariances_match_oracle and test_linearize_matches_oracle."""
    from test_gpu_gicp import _both
    p = centred_pair(synth)
    o, g = _both(pcm, model, "LM", p, **kw)
    if model == "GICP":
        for target in (False, True):
            c0, c1 = o.covariances(target), g.get_covariances(target)
            assert c1.shape == c0.shape
            bad = np.abs(c1 - c0).reshape(len(c0), -1).max(axis=1) > 1e-9 * max(1.0, np.abs(c0).max())
            assert bad.sum() <= max(2, len(c0) // 20000), int(bad.sum())
    c0, H0, b0 = o.linearize(p.T_gt)
    c1, H1, b1, inl = g.evaluate_cost(p.T_gt)
    print("inliers %d / %d  rel_err H %.2e b %.2e" % (inl, o.num_inliers, rel_err(H1, H0), rel_err(b1, b0)))
    assert inl > 0 and abs(inl - o.num_inliers) <= 2
    assert rel_err(H1, H0) < 1e-4 and rel_err(b1, b0) < 1e-4 and abs(c1 - c0) <= 1e-4 * abs(c0)


def test_loam_knn_walk(pcm, synth):
    """The 5-NN of k_loam_pass at the identity pose, the centred scan as features: equal to the kd-tree's wherever the 5th neighbour
    is within distance 1, as test_gpu_loam.test_per_point_parity.  The maps' grid is the default search_cell = 1.0 m, floor(p * 1.0):
    the last of GRIDS."""
    import loam_ref as R
    p = centred_pair(synth)
    corner_map, surf_map = np.ascontiguousarray(p.submap[::4]), p.submap
    corner, surf = np.ascontiguousarray(p.scan_world[::4]), p.scan_world
    g = pcm.LoamRegistration(0)
    g.set_input_target(corner_map, surf_map)
    g.set_input_source(corner, surf)
    x = np.zeros(6, np.float32)
    cn, sn = g.neighbours(x)
    ref = R.Problem(corner_map, surf_map, corner, surf).one_pass(x)
    for nn, want_nn, d2 in ((cn, ref.corner_nn, ref.corner_d2), (sn, ref.surf_nn, ref.surf_d2)):
        full = d2[:, 4] < 1.0
        print("%d of %d features with five neighbours within 1 m" % (full.sum(), len(full)))
        assert full.sum() > len(full) // 4
        assert np.array_equal(nn[full], want_nn[full])
