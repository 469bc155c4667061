"""The CPU oracle's GICP / VGICP (oracle/orc_gicp.c) against the independent numpy reference (gicp_numpy_ref.py), the preconditions of
the shared fixture, the sensitivity of the fixture to misreadings of the reference headers, and the derivative property b = grad / 2.

The fixture is synth.make_pair(3, 600, 3000) (and the same with the map's centroid moved to the origin) with the points removed that
violate a margin for any k in (5, 20, 33), any threshold in (FLT_MAX, 0.3f, 1.0), any resolution in (1.0, 0.75, 0.5), at the poses
guess and T_gt and with the roles swapped at guess^-1.  Measured on both variants:

  removed                                     1 of 600 scan points, 4 of 3000 map points (0.17 % / 0.13 %), in two rounds (1 + 3, then 0 + 1)
  smallest k-NN gap (d2[k+1] - d2[k]) / d2[k+1]  scan 1.8e-4 / 8.8e-5 / 3.9e-5, map 1.8e-5 / 3.6e-5 / 1.3e-5  (k = 5 / 20 / 33; limit 1e-5)
  smallest PLANE eigenvalue gap               scan 0.16 / 0.018 / 0.35, map 0.073 / 0.015 / 0.0094              (limit 1e-4)
  first against second nearest target         1.7e-3 relative
  threshold margin                            5.9e-3 relative at 0.3 m, 0.69 at 1.0 m
  nearest voxel boundary                      2.4e-5 of a cell (centred: 1.9e-6; limit 1e-9)

Oracle against numpy, largest relative deviation: covariances 2.7e-14 (FROBENIUS, k = 5; NONE is bit-equal); GICP H / b / cost /
compute_error 1.1e-14; VGICP 1.4e-14 in modes 0 and 1, 4.5e-13 in mode 2 at 0.5 m (two more inversions); every count equal.
"""
import numpy as np
import pytest

import gicp_numpy_ref as R
from helpers import rel_err

TOL = 1e-9      # the project's bar for double-precision quantities


@pytest.fixture(scope="module", params=[False, True], ids=["synth", "centred"])
def fx(request, synth):
    return R.build_fixture(synth, centred=request.param)


@pytest.fixture(scope="module")
def fx0(synth):
    return R.build_fixture(synth)


def _oracle(fx, model, **kw):
    from oracle import Oracle
    if model == "GICP":
        kw.setdefault("voxel_resolution", 0.5)     # sizes the oracle's search grid only
    o = Oracle(model, "LM", **kw)
    o.set_input_target(fx.submap); o.set_input_source(fx.scan)
    return o


# ---- preconditions ---------------------------------------------------------------------------------------------------------------
def test_fixture_has_no_violation_and_lost_under_one_percent(fx):
    bad_s, bad_m = R.all_violations(fx.scan, fx.submap, fx.poses, **fx.kw)
    assert len(bad_s) == 0 and len(bad_m) == 0
    assert len(fx.rounds) <= 3
    assert 0 <= fx.removed_scan <= 0.01 * 600 and 0 <= fx.removed_map <= 0.01 * 3000
    assert len(fx.scan) == 600 - fx.removed_scan and len(fx.submap) == 3000 - fx.removed_map
    m = R.margins(fx)
    print(fx.rounds, fx.removed_scan, fx.removed_map, m)
    assert min(v for k, v in m.items() if k.startswith("knn_gap")) >= R.GAP_KNN
    assert min(v for k, v in m.items() if k.startswith("plane_gap")) >= R.GAP_PLANE
    assert m["voxel_edge"] >= R.VOXEL_EDGE


def test_centred_fixture_has_voxel_coordinates_of_both_signs(synth):
    fx = R.build_fixture(synth, centred=True)
    R.assert_both_signs(fx)


@pytest.mark.parametrize("k", R.KS)
def test_tree_knn_equals_brute_force(fx0, k):
    for cloud in (fx0.scan, fx0.submap):
        x = R.widen(cloud)
        rows = np.arange(0, len(x), 5)
        idx, d2, gap = R.knn_self(x, k)
        assert np.array_equal(idx[rows], R.knn_brute(x, k, rows))        # no ties on the fixture: the order is determined too
        assert (idx[:, 0] == np.arange(len(x))).all() and (np.diff(d2, axis=1) > 0).all()


def test_reference_regularisations_on_a_known_matrix():
    """What each regularisation makes of diag(4, 1, 1e-4) rotated: the definitions, by hand."""
    Q = R.so3_exp([0.3, -0.2, 0.5])
    C = (Q @ np.diag([4.0, 1.0, 1e-4]) @ Q.T)[None]
    want = {"NONE": [4.0, 1.0, 1e-4], "PLANE": [1.0, 1.0, 1e-3], "MIN_EIG": [4.0, 1.0, 1e-3], "NORMALIZED_MIN_EIG": [1.0, 0.25, 1e-3]}
    lam = np.array([4.0, 1.0, 1e-4]) + 1e-3
    want["FROBENIUS"] = list(lam * np.sqrt((1.0 / lam ** 2).sum()))           # |C^-1|_F C
    for reg, vals in want.items():
        assert rel_err(R.regularize(C, reg)[0], Q @ np.diag(vals) @ Q.T) < 1e-11, reg     # two inversions at condition 4e3 in FROBENIUS


# ---- the oracle against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("reg", R.REGULARIZATIONS)
def test_oracle_covariances(fx, reg, k):
    o = _oracle(fx, "GICP", regularization=reg, k_correspondences=k)
    for target in (False, True):
        c0 = R.covariances(fx.submap if target else fx.scan, k, reg)
        c1 = o.covariances(target)
        assert c1.shape == c0.shape
        per_point = np.abs(c1 - c0).reshape(len(c0), -1).max(axis=1)
        assert (per_point <= TOL * np.abs(c0).max()).all(), (int((per_point > TOL * np.abs(c0).max()).sum()), per_point.max())


def _linearize_case(fx, model, **kw):
    o = _oracle(fx, model, **kw)
    r = R.Reference(fx.scan, fx.submap, model, **kw)
    for T in fx.poses:
        c0, H0, b0, n0 = r.linearize(T)
        c1, H1, b1 = o.linearize(T)
        assert n0 > 0 and o.num_inliers == n0
        assert rel_err(H1, H0) < TOL and rel_err(b1, b0) < TOL and abs(c1 - c0) <= TOL * abs(c0)
        T2 = T.copy(); T2[:3, 3] += R.SHIFT
        e0 = r.compute_error(T2)
        assert abs(o.compute_error(T2) - e0) <= TOL * abs(e0) and abs(e0 - c0) > 1e-3 * abs(c0)
    return r


@pytest.mark.parametrize("thr", R.THRESHOLDS, ids=["default", "0.3", "1.0"])
def test_oracle_gicp(fx, thr):
    r = _linearize_case(fx, "GICP", max_corr_dist=thr)
    if thr < 1.0:
        assert 0 < r.search.kept.sum() < len(fx.scan)          # the threshold really cuts


@pytest.mark.parametrize("res,nn,mode,reg", R.VGICP_CASES)
def test_oracle_vgicp(fx, res, nn, mode, reg):
    _linearize_case(fx, "VGICP", voxel_resolution=res, num_neighbors=nn, voxel_mode=mode, regularization=reg)


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
VG7 = dict(voxel_resolution=1.0, num_neighbors=7)
SENSITIVITY = [
    ("weight_n", "VGICP", VG7),
    ("floor_no_half", "VGICP", VG7),
    ("div_k_minus_1", "COV", "NONE"),
    ("div_k_minus_1", "GICP", dict(regularization="MIN_EIG")),
    ("plane_largest", "COV", "PLANE"),
    ("plane_largest", "GICP", {}),
    ("neg_skew", "GICP", {}),
    ("neg_skew", "VGICP", VG7),
    ("mode2_no_inverse", "VGICP", dict(voxel_resolution=1.0, num_neighbors=7, voxel_mode=2, regularization="MIN_EIG")),
    ("frobenius_no_norm", "COV", "FROBENIUS"),
    ("frobenius_no_norm", "GICP", dict(regularization="FROBENIUS")),
]


@pytest.mark.parametrize("mutation,what,case", SENSITIVITY, ids=["%s-%s" % (m, w) for m, w, _ in SENSITIVITY])
def test_fixture_sees_the_misreading(fx0, mutation, what, case):
    """A deliberate misreading put into the reference must move it at least 1e-6 (1000 x the bar) away from the oracle, in H, b, the cost
    or a covariance, on the very inputs the GPU tests use: otherwise agreement on them would prove nothing about that reading.

    The DIRECT7 row order is the one listed misreading these inputs cannot see, here or on the GPU: H, b and the cost are sums over the
    correspondences, and swapping two rows of the offsets table only permutes the terms (test_direct7_row_swap_only_permutes).  Seeing
    it needs a per-correspondence output: the (scan point, offset slot) -> voxel table, which neither the oracle nor the library hands
    out."""
    fx = fx0
    if what == "COV":
        o = _oracle(fx, "GICP", regularization=case)
        dev = max(rel_err(R.covariances(c, 20, case, mutation), o.covariances(t)) for c, t in ((fx.scan, False), (fx.submap, True)))
    else:
        o = _oracle(fx, what, **case)
        r = R.Reference(fx.scan, fx.submap, what, mutation=mutation, **case)
        dev = 0.0
        for T in fx.poses:
            c0, H0, b0, _ = r.linearize(T)
            c1, H1, b1 = o.linearize(T)
            dev = max(dev, rel_err(H0, H1), rel_err(b0, b1), abs(c0 - c1) / abs(c1))
    assert dev >= 1e-6, dev


def test_direct7_row_swap_only_permutes(fx0):
    """Rows +x and -x of the DIRECT7 table swapped: the correspondence list changes its order, the sums do not."""
    fx = fx0
    a = R.Reference(fx.scan, fx.submap, "VGICP", **VG7)
    b = R.Reference(fx.scan, fx.submap, "VGICP", mutation="direct7_swap", **VG7)
    ca, Ha, ba, na = a.linearize(fx.guess)
    cb, Hb, bb, nb = b.linearize(fx.guess)
    assert na == nb and not np.array_equal(a.corr.which, b.corr.which)
    assert np.array_equal(np.sort(a.corr.src * 10 ** 6 + a.corr.which), np.sort(b.corr.src * 10 ** 6 + b.corr.which))
    assert rel_err(Hb, Ha) < 1e-12 and rel_err(bb, ba) < 1e-12 and abs(cb - ca) <= 1e-12 * abs(ca)


# ---- derivative ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.DERIV_CASES))
def test_reference_b_is_half_the_gradient(fx0, name):
    """With the correspondences and M frozen, d cost(exp(eps) T) / d eps = 2 b for the left perturbation in (rotation, translation)
    order.  h = 1e-4: the discrepancy is the h^2 truncation term (it scales 100 x per decade of h from 1e-3 to 1e-5; rounding takes
    over below 1e-6 at ~2e-10).  Measured per case and pose in gicp_numpy_ref.DERIV_MEASURED (1.2e-8 ... 3.1e-7); the bound is 10 x."""
    model, kw = R.DERIV_CASES[name]
    r = R.Reference(fx0.scan, fx0.submap, model, **kw)
    for pose, T in zip(("guess", "T_gt"), fx0.poses):
        _, _, b, _ = r.linearize(T)
        d = R.derivative_discrepancy(r.compute_error, T, b)
        print(name, pose, d)
        assert d <= 10.0 * R.DERIV_MEASURED[name, pose], d
        assert d >= 0.1 * R.DERIV_MEASURED[name, pose], d      # the record is the truncation term of this fixture, not a stale figure
