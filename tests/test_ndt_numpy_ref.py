"""The CPU oracle's float models (oracle/orc_models_gauss.c, oracle/orc_pclndt.c) against the independent numpy reference
(ndt_numpy_ref.py), the preconditions of the shared fixture, the rounding-noise table the tolerances come from, the sensitivity of the
fixture to misreadings of the sources, and the derivative properties of the reference itself.  Figures: see DESIGN.md section 5.
"""
import numpy as np
import pytest

import ndt_numpy_ref as N
from ndt_numpy_ref import F32, F64, rel_err


def _name(case):
    return N.case_name(*case)


# ---- building both sides ---------------------------------------------------------------------------------------------------------
def kndt_oracle(ci, model, nn, res):
    from oracle import Oracle
    o = Oracle(model, "LM", voxel_resolution=res, num_neighbors=7 if isinstance(nn, str) else nn)
    if isinstance(nn, str):
        o.set_neighbor_radius(float(nn[1:]))
    o.set_input_target(ci.target); o.set_input_source(ci.scan)
    return o


def kndt_reference(ci, model, nn, res, covs=None, dtype=F64, mutation=None):
    r = N.NdtReference(ci.scan, ci.target, model, voxel_resolution=res, num_neighbors=nn, dtype=dtype, mutation=mutation)
    if model == "VGICP_CUDA":
        r.set_covariances(covs[0], False); r.set_covariances(covs[1], True)
    if ci.swapped:
        r.swap_source_and_target()
    return r


def _kndt_both(synth, case):
    model, nn, res, variant = case
    ci = N.case_inputs(synth, variant, N.kndt_family(res))
    o = kndt_oracle(ci, model, nn, res)
    covs = (o.covariances(False), o.covariances(True)) if model == "VGICP_CUDA" else None     # data: the estimators are pinned elsewhere
    if ci.swapped:
        o.swap_source_and_target()
    return ci, o, (lambda dtype=F64, mutation=None: kndt_reference(ci, model, nn, res, covs, dtype, mutation))


def pcl_reference(ci, nn, res, dtype=F64, mutation=None):
    r = N.PclNdtReference(ci.scan, ci.target, voxel_resolution=res, num_neighbors=nn, dtype=dtype, mutation=mutation)
    if ci.swapped:
        r.swap_source_and_target()
    return r


def _pcl_both(synth, case):
    from oracle import Oracle
    nn, res, variant = case
    ci = N.case_inputs(synth, variant)
    o = Oracle("NDT_OMP", "LM", voxel_resolution=res, num_neighbors=nn)
    o.set_input_target(ci.target); o.set_input_source(ci.scan)
    if ci.swapped:
        o.swap_source_and_target()
    return ci, o, (lambda dtype=F64, mutation=None: pcl_reference(ci, nn, res, dtype, mutation))


def _dev(a, b):
    return abs(a - b) / abs(b) if np.ndim(b) == 0 else rel_err(a, b)


# ---- preconditions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["wide", "dense"])
@pytest.mark.parametrize("centred", [False, True], ids=["synth", "centred"])
def test_fixture_has_no_violation_and_lost_under_one_percent(synth, centred, family):
    fx = N.build_fixture(synth, centred, family)
    bad_s, bad_m = N.all_violations(fx.scan, fx.submap, fx.poses, (fx.swapped_pose,))
    assert len(bad_s) == 0 and len(bad_m) == 0 and len(fx.rounds) <= 3
    assert 0 <= fx.removed_scan <= 0.01 * N.N_SCAN and 0 <= fx.removed_map <= 0.01 * N.N_MAP
    m = N.margins(fx)
    print(fx.rounds, fx.removed_scan, fx.removed_map, m)
    assert m["cell_ndt_over_slack"] > 1.0 and m["cell_pcl_over_slack"] > 1.0 and m["kdtree_radius_relative"] > N.KD_MARGIN


def test_an_unfiltered_pair_has_violations(synth):
    p = synth.make_pair(N.PAIR_ID, N.N_SCAN, N.N_MAP, density=N.DENSITY["wide"])
    g = p.guess.astype(F64)
    bad_s, bad_m = N.all_violations(p.scan, p.submap, (g, p.T_gt), (np.linalg.inv(g),))
    assert len(bad_s) + len(bad_m) > 0


def test_fixture_population(synth):
    """What the cases rely on.  Wide scene: at 1.0 m every scan point falls into a populated (> 6 points) cell at both poses; the pclomp rule at
    0.5 m leaves part of the scan without a leaf of 6 points (the empty-neighbourhood path).  Both scenes: the D2D source has several voxels at
    the resolution it is used at, beyond one wave's worth of nothing but element 0; single_voxel is a real subset.  Centred: cells of both signs."""
    fx = N.build_fixture(synth)
    tv = N.gauss_voxels(fx.submap[:, :3], 1.0)
    for T in fx.poses:
        pos, hit = N._lookup(tv.keys, N._cell_key(N.ndt_cells(N.transform_search(T, fx.scan[:, :3]), 1.0)))
        assert (hit & (tv.n[pos] > 6)).all()
        r = N.PclNdtReference(fx.scan, fx.submap, voxel_resolution=0.5, num_neighbors=1)
        i, _ = r.neighbourhood(N.transform_point_cloud_f32(N.pose_matrix_f32(N.pose_vector(T)), r.src32))
        assert 0 < len(i) < len(fx.scan)
    L = N.pcl_leaves(fx.submap[:, :3], 0.5)
    assert (L.n != -1).all() and (L.count == 6).any() and (L.count == 5).any()      # no rejected leaf; leaves on both sides of the minimum
    # D2D source voxels (scan), target voxels (map), and the map's voxels as the source of the swapped case
    fd = N.build_fixture(synth, family="dense")
    sv1, sv5 = N.gauss_voxels(fx.scan[:, :3], 1.0), N.gauss_voxels(fd.scan[:, :3], 0.5)
    print("source voxels", len(sv1.n), len(sv5.n), int((sv5.n > 6).sum()), "extent", np.ptp(fx.scan[:, :3], axis=0), np.ptp(fd.scan[:, :3], axis=0))
    assert len(sv1.n) == 11 and len(sv5.n) == 11 and (sv5.n > 6).sum() == 7
    assert len(tv.n) == 120 and len(N.gauss_voxels(fd.submap[:, :3], 0.5).n) >= 150
    one = N.case_inputs(synth, "single_voxel")
    assert 6 < len(one.scan) < len(fx.scan) / 2 and len(N.gauss_voxels(one.scan[:, :3], 1.0).n) == 1
    # centred: the dense scene at 0.5 m and the wide one for pclomp have cells of both signs on every axis (both are 2 m high: -2 ... 1 in z)
    xk = np.ascontiguousarray(N.build_fixture(synth, centred=True, family="dense").submap[:, :3])
    xp = np.ascontiguousarray(N.build_fixture(synth, centred=True).submap[:, :3])
    for cells in (N.ndt_cells(xk, 0.5), N.pcl_cells_of_map(xp, 0.5)):
        assert (cells.min(axis=0) < 0).all() and (cells.max(axis=0) > 0).all()
    cells = N.pcl_cells_of_map(xp, 1.0)
    assert (cells.min(axis=0) < 0).all() and (cells.max(axis=0) >= 0).all()
    tv5 = N.gauss_voxels(N.case_inputs(synth, "sparse20", "dense").target[:, :3], 0.5)
    assert (tv5.n == 6).any() and (tv5.n > 6).any() and (tv5.n == 1).any()         # sparse20: voxels on both sides of n > 6, and of one point


# ---- the oracle against the reference, and the noise table -----------------------------------------------------------------------
def _check_quantities(case_key, got, want, ratios):
    for q, w in want.items():
        d, noise, tol = _dev(got[q], w[0]), N.NOISE_MEASURED[case_key][q], N.tolerance(case_key, q)
        meas = _dev(w[1], w[0])
        print("%-40s %-14s oracle %.2e  noise %.2e (recorded %.2e)  tolerance %.2e" % (case_key, q, d, meas, noise, tol))
        assert noise / 2.0 <= meas <= noise * 2.0, (case_key, q, meas, noise)        # the recorded table describes these inputs
        assert d <= tol, (case_key, q, d, tol)
        ratios.append(d / noise)


@pytest.mark.parametrize("case", N.all_kndt_cases(), ids=_name)
def test_oracle_kndt(synth, case):
    ci, o, make = _kndt_both(synth, case)
    ratios = []
    for pose, T in ci.poses.items():
        key = N.case_name(*case, pose)
        want, n0 = N.measure_kndt(make, T)
        c1, H1, b1 = o.linearize(T)
        assert o.num_inliers == n0 == N.NOISE_MEASURED[key]["count"] and n0 > 0
        got = {"cost": c1, "H": H1, "b": b1, "compute_error": o.compute_error(N.TRIAL(T))}
        _check_quantities(key, got, want, ratios)
    assert max(ratios) <= N.ORACLE_RATIO_MEASURED * 1.0001, max(ratios)
    if case[3] == "sparse20" and case[0] == "VGICP_CUDA":
        r = make(); r.linearize(ci.fx.guess)
        assert (r.corr.n_b == 1).any()                  # a correspondence reaches a voxel of one point
    if case[3] == "single_voxel":
        assert len(make().source_elements()[0]) == 1


def test_oracle_sparse_targets(synth):
    """The count-0 cases of the GPU file, which need no device: P2D against a map of at most 6 points per voxel, pclomp with at most 5 points
    per leaf on both sides, before and after the swap: oracle and reference find nothing."""
    from oracle import Oracle
    ci = N.case_inputs(synth)
    ci.target = N.thin_for_p2d(ci.target)
    o = kndt_oracle(ci, "NDT_P2D", 27, 1.0)
    c1, H1, b1 = o.linearize(ci.fx.guess)
    assert kndt_reference(ci, "NDT_P2D", 27, 1.0).linearize(ci.fx.guess)[3] == 0 and o.num_inliers == 0 and c1 == 0.0 and not H1.any() and not b1.any()
    ci = N.case_inputs(synth)
    ci.target, ci.scan = N.thin_for_pcl(ci.target), N.thin_for_pcl(ci.scan)
    o = Oracle("NDT_OMP", "LM", voxel_resolution=1.0, num_neighbors=27)
    o.set_input_target(ci.target); o.set_input_source(ci.scan)
    r = pcl_reference(ci, 27, 1.0)
    for T in (ci.fx.guess, ci.fx.swapped_pose):
        p = N.pose_vector(T)
        s1, g1, H1 = o.ndt_derivatives(p)
        assert r.derivatives(p, "float")[3] == 0 and s1 == 0.0 and not g1.any() and not H1.any()
        assert o.ndt_score(T) == r.score(N.pose_f32(T)) == 0.0
        o.swap_source_and_target(); r.swap_source_and_target()


@pytest.mark.parametrize("case", N.all_pcl_cases(), ids=_name)
def test_oracle_pcl(synth, case):
    ci, o, make = _pcl_both(synth, case)
    ratios = []
    for pose, T in ci.poses.items():
        key = N.case_name("NDT_OMP", *case, pose)
        p = N.pose_vector(T)
        want, n0 = N.measure_pcl(make, T)
        assert n0 == N.NOISE_MEASURED[key]["count"] and n0 > 0
        s1, g1, H1 = o.ndt_derivatives(p)
        _check_quantities(key, {"score": s1, "gradient": g1, "H_float": H1}, want, ratios)
        s2, g2, _ = o.ndt_derivatives(p, False)
        assert abs(s2 - s1) <= 1e-12 * abs(s1) and rel_err(g2, g1) < 1e-12          # the same terms, summed by other threads
        r = make()
        Hd, sc = r.derivatives(p, "double")[2], r.score(N.pose_f32(T))
        dh, ds = rel_err(o.ndt_hessian(p), Hd), abs(o.ndt_score(T) - sc) / abs(sc)
        print("%-40s double Hessian %.2e  calculateScore %.2e" % (key, dh, ds))
        assert dh < N.DOUBLE_TOL and ds < N.DOUBLE_TOL and sc != 0
    assert max(ratios) <= N.ORACLE_RATIO_MEASURED * 1.0001, max(ratios)


def test_margin_is_four_times_the_largest_oracle_ratio():
    assert N.MARGIN == max(4.0, 4.0 * N.ORACLE_RATIO_MEASURED)
    for key, row in N.NOISE_MEASURED.items():
        for q in row:
            if q != "count":
                assert N.tolerance(key, q) <= N.HB_RTOL


# ---- the reference against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nn,res", [(7, 1.0), (0, 0.5)])
def test_pcl_gradient_and_hessian_are_derivatives_of_the_score(synth, nn, res):
    """Over the frozen neighbourhood and with the pose applied in float64, central differences (h = 1e-5) of the score give the gradient
    and of the gradient the DOUBLE Hessian and the float-pass Hessian WITHOUT the (+sy) entry; with it the float-pass Hessian differs in
    entry (pitch, pitch) alone.  Truncation + rounding of the difference: < 1e-7 relative observed (2e-9 ... 3e-8)."""
    ci = N.case_inputs(synth)
    r = pcl_reference(ci, nn, res)
    h = 1e-5
    for T in ci.poses.values():
        p = N.pose_vector(T)
        r.derivatives(p, None)
        fz = r.last_neighbourhood
        s0, g0, H0, _ = r.derivatives(p, "float", quirk=False, frozen=fz, exact=True)
        Hd = r.derivatives(p, "double", frozen=fz, exact=True)[2]
        gn, Hn = np.zeros(6), np.zeros((6, 6))
        for k in range(6):
            a = r.derivatives(p + h * np.eye(6)[k], None, frozen=fz, exact=True)
            b = r.derivatives(p - h * np.eye(6)[k], None, frozen=fz, exact=True)
            gn[k], Hn[k] = (a[0] - b[0]) / (2 * h), (a[1] - b[1]) / (2 * h)
        print(nn, res, rel_err(g0, gn), rel_err(H0, Hn), rel_err(Hd, Hn))
        assert rel_err(g0, gn) < 1e-7 and rel_err(H0, Hn) < 1e-7 and rel_err(Hd, Hn) < 1e-7
        Hq = r.derivatives(p, "float", quirk=True, frozen=fz, exact=True)[2]
        diff = np.abs(Hq - H0)
        assert diff[4, 4] > 1e-6 * np.abs(H0).max() and np.count_nonzero(diff) == 1


@pytest.mark.parametrize("model,nn,res", [("NDT_P2D", 7, 1.0), ("NDT_D2D", 27, 0.5), ("VGICP_CUDA", 7, 1.0)])
def test_kndt_b_is_half_the_gradient_less_the_weight_term(synth, model, nn, res):
    """d compute_error(exp(eps) T) / d eps = 2 b + cauchy_gradient_term() on the remembered correspondences: b is the Gauss-Newton vector
    with the weight held fixed, and the Cauchy weight of P2D / D2D depends on e (VGICP_CUDA: the term is zero).  h = DERIV_H; the
    discrepancy is the h^2 truncation term, recorded per case and pose in DERIV_MEASURED."""
    ci, o, make = _kndt_both(synth, (model, nn, res, "main"))
    r = make()
    for pose, T in ci.poses.items():
        _, _, b, _ = r.linearize(T)
        d = N.derivative_discrepancy(r.compute_error, T, b, r.cauchy_gradient_term())
        rec = N.DERIV_MEASURED[N.case_name(model, nn, res, pose)]
        print(model, nn, res, pose, d, rec)
        assert rec / 10.0 <= d <= rec * 10.0
        if model != "VGICP_CUDA":
            assert N.derivative_discrepancy(r.compute_error, T, b, np.zeros(6)) > 100.0 * d          # the term is needed


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
KNDT_SENSITIVITY = [("floor_no_half", ("NDT_P2D", 7, 1.0)), ("n_ge_6", ("NDT_P2D", 27, 0.5)), ("div_n_minus_1", ("NDT_P2D", 7, 1.0)),
                    ("no_min_eig", ("NDT_P2D", 7, 0.5)), ("cauchy_width_1", ("NDT_P2D", 7, 0.5)), ("weight_n", ("VGICP_CUDA", 7, 1.0)),
                    ("neg_skew", ("NDT_P2D", 7, 1.0)), ("d2d_no_source_cov", ("NDT_D2D", 7, 1.0)), ("trial_rotation", ("NDT_D2D", 7, 1.0)),
                    ("trial_rotation", ("VGICP_CUDA", 7, 1.0))]
PCL_SENSITIVITY = [("no_identity", (7, 1.0)), ("no_n_minus_1", (7, 1.0)), ("min_points_7", (7, 0.5)),
                   ("floor_minus_half", (7, 1.0)), ("d1_d2_swapped", (7, 1.0)), ("kdtree_cell_centre", (0, 1.0)),
                   ("drop_d2R_roll_roll", (7, 1.0)), ("score_not_per_cell", (7, 1.0))]


def _worst(effects):
    """The largest effect / tolerance over the compared quantities."""
    return max(e / t for e, t in effects)


@pytest.mark.parametrize("mutation,case", KNDT_SENSITIVITY, ids=["%s-%s" % (m, c[0]) for m, c in KNDT_SENSITIVITY])
def test_fixture_sees_the_kndt_misreading(synth, mutation, case):
    """A misreading put into the reference moves at least one compared quantity by at least 10 x the tolerance it is compared at, on the
    inputs the GPU tests use.  trial_rotation moves compute_error alone (the rotated TRIAL pose): its size is printed."""
    variant = "sparse20" if mutation == "n_ge_6" else "main"      # the target with voxels of exactly 6 points
    ci, o, make = _kndt_both(synth, case + (variant,))
    r, m = make(), make(mutation=mutation)
    effects = []
    for pose, T in ci.poses.items():
        key = N.case_name(*case, variant, pose)
        a, b = r.linearize(T), m.linearize(T)
        if a[3] != b[3]:
            effects.append((1.0, 0.1))                          # counts are compared exactly
        for q, x, y in (("cost", a[0], b[0]), ("H", a[1], b[1]), ("b", a[2], b[2]), ("compute_error", r.compute_error(N.TRIAL(T)), m.compute_error(N.TRIAL(T)))):
            effects.append((_dev(y, x), N.tolerance(key, q)))
            if mutation == "trial_rotation":
                print(case[0], pose, q, "%.2e" % _dev(y, x))
                assert q == "compute_error" or _dev(y, x) == 0.0
    print(mutation, case, "%.1f x tolerance" % _worst(effects))
    assert _worst(effects) >= 10.0


@pytest.mark.parametrize("mutation,case", PCL_SENSITIVITY, ids=[m for m, _ in PCL_SENSITIVITY])
def test_fixture_sees_the_pclomp_misreading(synth, mutation, case):
    ci = N.case_inputs(synth)
    r, m = pcl_reference(ci, *case), pcl_reference(ci, *case, mutation=mutation)
    effects = []
    for pose, T in ci.poses.items():
        key = N.case_name("NDT_OMP", *case, "main", pose)
        p = N.pose_vector(T)
        a, b = r.derivatives(p, "float"), m.derivatives(p, "float")
        for q, k in (("score", 0), ("gradient", 1), ("H_float", 2)):
            effects.append((_dev(b[k], a[k]), N.tolerance(key, q)))
        effects.append((rel_err(m.derivatives(p, "double")[2], r.derivatives(p, "double")[2]), N.DOUBLE_TOL))
        effects.append((_dev(m.score(N.pose_f32(T)), r.score(N.pose_f32(T))), N.DOUBLE_TOL))
    print(mutation, case, "%.1f x tolerance" % _worst(effects))
    assert _worst(effects) >= 10.0


def test_invisible_misreadings_are_listed(synth):
    """`<=` for `<` in the radius test changes nothing on these inputs, by construction (KD_MARGIN); it is listed with its reason."""
    ci = N.case_inputs(synth)
    r, m = pcl_reference(ci, 0, 1.0), pcl_reference(ci, 0, 1.0, mutation="radius_le")
    p = N.pose_vector(ci.fx.guess)
    a, b = r.derivatives(p, "float"), m.derivatives(p, "float")
    assert a[0] == b[0] and np.array_equal(a[2], b[2]) and "radius_le" in N.INVISIBLE and "direct7_order" in N.INVISIBLE
    # the inflation to 1 % never acts here: the identity the covariance starts from leaves every eigenvalue above (n - 1) / n^2, which with
    # at most ~100 points per leaf is more than 1 % of the largest -- 0.001 for 0.01 changes no leaf
    L = N.pcl_leaves(ci.target[:, :3], 1.0)
    assert np.array_equal(L.icov, N.pcl_leaves(ci.target[:, :3], 1.0, "inflation_0.001").icov) and "inflation_0.001" in N.INVISIBLE
    assert set(m for m, _ in KNDT_SENSITIVITY + PCL_SENSITIVITY) | {"radius_le", "inflation_0.001"} == set(N.MUTATIONS)
