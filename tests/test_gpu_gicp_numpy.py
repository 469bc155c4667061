"""The GICP / VGICP kernels (csrc/gicp.hip: k_covariances + regularize_cov, k_vgicp_voxels, k_gicp<VG, TRIAL> with nearest1, vg_lookup and
the DIRECT7 table) against the independent numpy reference of gicp_numpy_ref.py.  The CPU oracle is not loaded here.

Inputs: gicp_numpy_ref.build_fixture -- synth.make_pair(3, 600, 3000) less the 1 scan and 4 map points at which a float32 search could
legitimately differ from an exact one (margins in test_gicp_numpy_ref.py), so nothing below excuses a point, an inlier or a digit:
covariances per point, H, b, the cost and compute_error to 1e-9 relative (the project's bar for double quantities), counts exact.
What these inputs can and cannot see is pinned by test_gicp_numpy_ref.test_fixture_sees_the_misreading.
Measured on an MI355X, largest relative deviation from numpy: covariances 2.7e-14 (all six regularisations, k = 5 / 20 / 33, both
clouds, 0 points above 1e-9); H 9.3e-15; b, cost and compute_error 4.0e-13 (MULTIPLICATIVE voxels at 0.5 m, 1e-14 elsewhere); every count
equal; the kernel's derivative discrepancy equals the reference's truncation term to three digits (1.16e-8 ... 3.14e-7).
"""
import numpy as np
import pytest

import gicp_numpy_ref as R
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def fx(synth):
    return R.build_fixture(synth)


@pytest.fixture(scope="module")
def fxc(synth):
    return R.build_fixture(synth, centred=True)


def _both(pcm, model, scan, submap, **kw):
    g = (pcm.GicpRegistration if model == "GICP" else pcm.VgicpRegistration)(0, optimizer="LM", **kw)
    g.set_input_target(submap); g.set_input_source(scan)
    cfg = g.config
    assert cfg.max_corr_dist == np.float32(kw.get("max_corr_dist", R.FLT_MAX)) and cfg.k_correspondences == kw.get("k_correspondences", 20)
    r = R.Reference(scan, submap, model, **kw)
    return r, g


def _check_at(r, g, T, n_expected=None):
    """evaluate_cost at T (k_gicp<., false>), then compute_error at the shifted pose (k_gicp<., true>), against the reference."""
    c0, H0, b0, n0 = r.linearize(T)
    c1, H1, b1, n1 = g.evaluate_cost(T)
    print("count %d %d  H %.2e  b %.2e  cost %.2e" % (n1, n0, rel_err(H1, H0), rel_err(b1, b0), abs(c1 - c0) / abs(c0)))
    assert n1 == n0 and n0 > 0
    if n_expected is not None:
        assert n0 == n_expected
    assert rel_err(H1, H0) < TOL and rel_err(b1, b0) < TOL and abs(c1 - c0) <= TOL * abs(c0)
    T2 = T.copy(); T2[:3, 3] += R.SHIFT
    e0, e1 = r.compute_error(T2), g.compute_error(T2)
    print("compute_error %.2e" % (abs(e1 - e0) / abs(e0)))
    assert abs(e1 - e0) <= TOL * abs(e0) and abs(e0 - c0) > 1e-3 * abs(c0)
    return b1


def _check_derivative(g, T, b, name, pose):
    """The kernel's own compute_error differentiated on the correspondences of its last evaluate_cost(T): 2 b, within 10 x the truncation
    term measured on the reference (gicp_numpy_ref.DERIV_MEASURED, test_reference_b_is_half_the_gradient)."""
    d = R.derivative_discrepancy(g.compute_error, T, b)
    print("derivative %s %s %.2e (reference %.2e)" % (name, pose, d, R.DERIV_MEASURED[name, pose]))
    assert d <= 10.0 * R.DERIV_MEASURED[name, pose], d


def _deriv_name(model, kw):
    for name, (m, k) in R.DERIV_CASES.items():
        if m == model and k == {a: v for a, v in kw.items() if not (a == "regularization" and v == "PLANE") and not (a == "voxel_mode" and v == 0)}:
            return name
    return None


# ---- covariances -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("reg", R.REGULARIZATIONS)
def test_covariances(pcm, fx, reg, k):
    """k = 5 and 20 run k_covariances<20>, k = 33 k_covariances<64> (other launch bounds, LDS size and merge area); the fixture's
    neighbour and eigenvalue gaps hold for all three k."""
    g = pcm.GicpRegistration(0, regularization=reg, k_correspondences=k)
    g.set_input_target(fx.submap); g.set_input_source(fx.scan)
    for target in (False, True):
        c0 = R.covariances(fx.submap if target else fx.scan, k, reg)
        c1 = g.get_covariances(target)
        assert c1.shape == c0.shape
        per_point = np.abs(c1 - c0).reshape(len(c0), -1).max(axis=1) / np.abs(c0).max()
        print(reg, k, target, "%.2e" % per_point.max())
        assert (per_point <= TOL).all(), (int((per_point > TOL).sum()), float(per_point.max()))


# ---- evaluate_cost, compute_error, derivative ------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", R.THRESHOLDS, ids=["default", "0.3", "1.0"])
def test_gicp(pcm, fx, thr):
    kw = {} if thr == R.FLT_MAX else {"max_corr_dist": thr}
    r, g = _both(pcm, "GICP", fx.scan, fx.submap, **kw)
    for pose, T in zip(("guess", "T_gt"), fx.poses):
        b = _check_at(r, g, T)
        if not kw:
            _check_derivative(g, T, b, "gicp", pose)
    if thr < 1.0:
        assert 0 < r.search.kept.sum() < len(fx.scan)


@pytest.mark.parametrize("res,nn,mode,reg", R.VGICP_CASES)
def test_vgicp(pcm, fx, res, nn, mode, reg):
    kw = dict(voxel_resolution=res, num_neighbors=nn, voxel_mode=mode, regularization=reg)
    r, g = _both(pcm, "VGICP", fx.scan, fx.submap, **kw)
    name = _deriv_name("VGICP", kw)
    for pose, T in zip(("guess", "T_gt"), fx.poses):
        b = _check_at(r, g, T)
        if name:
            _check_derivative(g, T, b, name, pose)


def test_derivative_cases_are_run():
    assert _deriv_name("GICP", {}) == "gicp"
    names = {_deriv_name("VGICP", dict(voxel_resolution=res, num_neighbors=nn, voxel_mode=mode, regularization=reg)) for res, nn, mode, reg in R.VGICP_CASES}
    assert names - {None} == {"vgicp_1.0_7_0", "vgicp_0.5_27_2"}


# ---- centred: voxel, brick and cell coordinates of both signs --------------------------------------------------------------------
@pytest.mark.parametrize("model,kw", [("GICP", {}), ("VGICP", dict(voxel_resolution=1.0, num_neighbors=7)),
                                      ("VGICP", dict(voxel_resolution=0.5, num_neighbors=27, voxel_mode=2))], ids=["gicp", "vgicp_1.0_7_0", "vgicp_0.5_27_2"])
def test_centred(pcm, fxc, model, kw):
    R.assert_both_signs(fxc)
    r, g = _both(pcm, model, fxc.scan, fxc.submap, **kw)
    for T in fxc.poses:
        _check_at(r, g, T)


# ---- tails -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,kw", [("GICP", {}), ("VGICP", dict(voxel_resolution=1.0, num_neighbors=7))], ids=["gicp", "vgicp"])
def test_scan_head_of_257_points(pcm, fx, model, kw):
    """One full workgroup of k_gicp and one lane of the next; the head is a cloud of its own, so its 20-NN margins are asserted here."""
    head = fx.scan[:257]
    assert len(R.violations_knn_gap(head, 20)) == 0 and len(R.violations_plane_gap(head, 20)) == 0
    r, g = _both(pcm, model, head, fx.submap, **kw)
    assert rel_err(g.get_covariances(False), r.covariances(False)) < TOL
    _check_at(r, g, fx.guess)


@pytest.mark.parametrize("model,kw", [("GICP", {}), ("VGICP", dict(voxel_resolution=1.0, num_neighbors=27))], ids=["gicp", "vgicp"])
def test_scan_head_of_one_point(pcm, fx, model, kw):
    """A single scan point (one lane of one wave).  A one-point cloud has no 20 neighbours, so its covariance is handed in: the row the
    whole scan gives that point."""
    cs = R.covariances(fx.scan, 20, "PLANE")[:1]
    r, g = _both(pcm, model, fx.scan[:1], fx.submap, **kw)
    r.set_covariances(cs, False); g.set_covariances(cs, False)
    _check_at(r, g, fx.guess, n_expected=1 if model == "GICP" else None)


@pytest.mark.parametrize("mode,reg", [(0, "PLANE"), (2, "MIN_EIG")])
def test_voxels_of_exactly_one_point(pcm, fx, mode, reg):
    """A target made of the map points that are alone in their 0.5 m voxel: every voxel distribution is one point and its covariance
    (mode 2: (C^-1)^-1 and C C^-1 x), every weight sqrt(1).  The covariances of both clouds are handed in (the rows of the whole
    clouds), as a cloud this sparse has other neighbour sets."""
    res = 0.5
    vm = R.voxel_map(R.widen(fx.submap), R.covariances(fx.submap, 20, reg), res, mode)
    alone = np.nonzero(vm.n[vm.of_point] == 1)[0]
    assert len(alone) >= 100
    target, ct, cs = fx.submap[alone], R.covariances(fx.submap, 20, reg)[alone], R.covariances(fx.scan, 20, reg)
    kw = dict(voxel_resolution=res, num_neighbors=27, voxel_mode=mode, regularization=reg)
    r, g = _both(pcm, "VGICP", fx.scan, target, **kw)
    for x in (r, g):
        x.set_covariances(cs, False); x.set_covariances(ct, True)
    assert (r.voxels().n == 1).all()
    _check_at(r, g, fx.guess)


def test_scan_point_with_an_empty_neighbourhood(pcm, fx):
    """A scan point whose 27 cells are all empty adds no correspondence and nothing to the sums: with it the count and H are what they
    are without it."""
    T = fx.guess
    far_world = R.widen(fx.submap).max(axis=0) + np.array([7.3, 5.2, 9.1])
    far = np.linalg.inv(T) @ np.append(far_world, 1.0)
    scan = np.concatenate([fx.scan[:64], fx.scan[:1]])
    scan[64, :3] = far[:3].astype(np.float32)
    assert len(R.violations_voxel_edge(R.transform(T, R.widen(scan[64:])), 1.0)) == 0
    cs = np.concatenate([R.covariances(fx.scan, 20, "PLANE")[:64], 0.01 * np.eye(3)[None]])
    kw = dict(voxel_resolution=1.0, num_neighbors=27)
    r, g = _both(pcm, "VGICP", scan, fx.submap, **kw)
    r.set_covariances(cs, False); g.set_covariances(cs, False)
    _check_at(r, g, T)
    assert (r.corr.src != 64).all()
    n_with = len(r.corr.src)
    r2, g2 = _both(pcm, "VGICP", scan[:64], fx.submap, **kw)
    r2.set_covariances(cs[:64], False); g2.set_covariances(cs[:64], False)
    c2, H2, b2, n2 = g2.evaluate_cost(T)
    c1, H1, b1, n1 = g.evaluate_cost(T)
    assert n1 == n2 == n_with and rel_err(H1, H2) < 1e-12 and abs(c1 - c2) <= 1e-12 * abs(c2)


# ---- swapped roles, covariances of the caller ------------------------------------------------------------------------------------
def test_swap_source_and_target(pcm, fx):
    """swapSourceAndTarget (fast_gicp_impl.hpp:50-58): the map is registered to the scan, at guess^-1; 2996 queries (12 workgroups) against a
    599-point target."""
    r, g = _both(pcm, "GICP", fx.scan, fx.submap)
    _check_at(r, g, fx.guess)
    r.swap_source_and_target(); g.swap_source_and_target()
    _check_at(r, g, fx.swapped_pose, n_expected=len(fx.submap))
    assert rel_err(g.get_covariances(False), R.covariances(fx.submap, 20, "PLANE")) < TOL


@pytest.mark.parametrize("model,kw", [("GICP", {}), ("VGICP", dict(voxel_resolution=1.0, num_neighbors=7))], ids=["gicp", "vgicp"])
def test_covariances_of_the_caller(pcm, fx, model, kw):
    """setSourceCovariances / setTargetCovariances (fast_gicp_impl.hpp:93-110) with the computed matrices deformed, as
    test_gpu_gicp.test_covariances_handed_in_by_the_caller deforms them."""
    r, g = _both(pcm, model, fx.scan, fx.submap, **kw)
    c_def = r.linearize(fx.guess)[0]
    D = np.diag([1.0, 2.0, 0.5])
    cs2 = D @ r.covariances(False) @ D.T + 0.01 * np.eye(3)
    ct2 = 1.5 * r.covariances(True) + 0.02 * np.eye(3)
    cs2, ct2 = 0.5 * (cs2 + cs2.transpose(0, 2, 1)), 0.5 * (ct2 + ct2.transpose(0, 2, 1))     # exactly symmetric: the library keeps one triangle
    for x in (r, g):
        x.set_covariances(cs2, False); x.set_covariances(ct2, True)
    assert np.array_equal(g.get_covariances(False), cs2) and np.array_equal(g.get_covariances(True), ct2)
    for T in fx.poses:
        _check_at(r, g, T)
    assert abs(r.linearize(fx.guess)[0] - c_def) > 1e-3 * abs(c_def)
