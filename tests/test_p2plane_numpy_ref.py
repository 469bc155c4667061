"""The CPU oracle's P2PLANE model and ObsModel (oracle/pcm_oracle.c) against the independent numpy reference (p2plane_numpy_ref.py), the
preconditions of the shared fixtures, the rounding-noise table the tolerances come from, the sensitivity of the fixtures to misreadings
of the sources, and the derivative properties of the reference itself.  Figures: see DESIGN.md section 5.
"""
import numpy as np
import pytest

import p2plane_numpy_ref as P
from p2plane_numpy_ref import F64


def _oracle(ci, res, nn, max_range, optimizer="LM"):
    from oracle import Oracle
    o = Oracle("P2PLANE", optimizer, voxel_resolution=res, num_neighbors=nn, max_range=max_range)
    o.set_input_target(ci.target); o.set_input_source(ci.scan)
    return o


# ---- preconditions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centred", [False, True], ids=["synth", "centred"])
def test_fixture_has_no_violation_and_lost_under_one_percent(synth, centred):
    fx = P.build_fixture(synth, centred)
    bad_s, bad_m = P.all_violations(fx.scan, fx.submap, tuple(fx.poses.values()), fx.cases)
    assert len(bad_s) == 0 and len(bad_m) == 0 and len(fx.rounds) <= 3
    assert 0 <= fx.removed_scan <= 0.01 * P.PAIR[1] and 0 <= fx.removed_map <= 0.01 * P.PAIR[2]
    m = fx.margins
    print(fx.rounds, fx.removed_scan, fx.removed_map, m)
    assert m["cell"] > P.CELL_SLACK and m["knn_gap"] > 1.0 and m["range"] > 1.0
    assert m["threshold"] > P.THRESHOLD_SLACK and m["point_test"] > P.POINT_TEST_SLACK
    if centred:
        P.assert_both_signs(fx)


def test_an_unfiltered_pair_has_violations(synth):
    p = synth.make_pair(*P.PAIR)
    bad_s, bad_m = P.all_violations(p.scan, p.submap, (p.guess.astype(F64), p.T_gt), P.search_cases())
    assert 0 < len(bad_s) + len(bad_m) <= 6


def test_fixture_population(synth):
    """What the cases rely on: both plane paths (m = 5, and m = 3 or 4) and the no-plane exit are taken; the binding range makes
    queries lose candidates and drop below 5 and below 3; the lone-voxel target has one point per voxel; the far point's 27 cells are
    empty."""
    ci = P.case_inputs(synth)
    for res, lo, hi in ((0.5, 440, 480), (0.25, 370, 420)):
        for T in ci.poses.values():
            r = P.make_reference(ci, res, 27, P.MAX_RANGE)
            n = r.linearize(T)[3]
            m = r.found.m
            print(res, n, int((m == 5).sum()), int(((m >= 3) & (m < 5)).sum()), int((m < 3).sum()), int((~r.found.ok).sum()))
            assert lo <= n <= hi and (m == 5).sum() > 100 and (~r.found.ok).sum() > 50
            if res == 0.25:
                assert ((m >= 3) & (m < 5)).sum() > 200 and (m < 3).sum() > 100
    wide, tight = P.make_reference(ci, 0.5, 27, P.MAX_RANGE), P.make_reference(ci, 0.5, 27, P.BINDING_RANGE)
    q = wide.transform(P.round32(ci.fx.guess)[:3, :3], P.round32(ci.fx.guess)[:3, 3])
    mw, mt = wide.search(q)[2], tight.search(q)[2]
    assert (mt < mw).sum() > 100 and ((mw == 5) & (mt < 5) & (mt >= 3)).sum() > 50 and ((mw >= 3) & (mt < 3)).sum() > 100 and (mt == 5).sum() > 5
    lone = P.case_inputs(synth, "lone")
    v = P.voxel_coords(P.widen(lone.target), 0.25)
    assert len(np.unique(v, axis=0)) == len(v) >= 500 and len(lone.scan) >= 0.99 * len(ci.scan)
    e = P.case_inputs(synth, "empty")
    r = P.make_reference(e, 0.5, 27, P.MAX_RANGE)
    r.linearize(e.fx.guess)
    assert r.found.m[64] == 0 and not r.selected[64] and (r.geometry(r.q)[1][64] == 99).all()


# ---- the oracle against the reference, and the noise table -----------------------------------------------------------------------
def _check_quantities(key, got, want, ratios):
    for q, w in want.items():
        d, noise, tol = P.deviation(got[q], w[0], q), P.NOISE_MEASURED[key][q], P.tolerance(key, q)
        meas = P.deviation(w[1], w[0], q)
        print("%-28s %-14s oracle %.2e  noise %.2e (recorded %.2e)  tolerance %.2e" % (key, q, d, meas, noise, tol))
        assert noise / 2.0 <= meas <= noise * 2.0 or meas == noise == 0.0, (key, q, meas, noise)      # the recorded table describes these inputs
        assert d <= tol, (key, q, d, tol)
        if noise > 0.0:
            ratios.append(d / noise)


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: P.case_name(*c))
def test_oracle_p2plane(synth, case):
    variant, res, nn, rng = case
    ci = P.case_inputs(synth, variant)
    o = _oracle(ci, res, nn, rng)
    ratios = [0.0]
    for pose, T in ci.poses.items():
        key = P.case_name(*case, pose)
        want, n0, r64 = P.measure(ci, res, nn, rng, T)
        c1, H1, b1 = o.linearize(T)
        pl, sel = o.get_planes(len(ci.scan))
        assert o.num_inliers == n0 == P.NOISE_MEASURED[key]["count"] and np.array_equal(sel, r64.selected)
        got = {"planes": np.where(sel[:, None], pl, np.nan), "cost": c1, "H": H1, "b": b1, "compute_error": o.compute_error(P.shifted(T))}
        _check_quantities(key, got, want, ratios)
        if n0:
            # the two cannot be confused: they differ by more than 10 x the tolerance either is compared at
            assert abs(want["compute_error"][0] - want["cost"][0]) > 10.0 * P.HB_RTOL * want["cost"][0]
    assert max(ratios) <= P.ORACLE_RATIO_MEASURED * 1.0001, max(ratios)
    if variant == "empty":
        assert not r64.selected[64] and r64.found.m[64] == 0
        ci2 = P.types.SimpleNamespace(scan=ci.scan[:64], target=ci.target)
        a, b = P.make_reference(ci2, res, nn, rng).linearize(T), P.make_reference(ci, res, nn, rng).linearize(T)
        assert a[3] == b[3] and a[0] == b[0] and np.array_equal(a[1], b[1])          # the far point adds nothing


@pytest.mark.parametrize("case", P.LIO_CASES, ids=lambda c: P.lio_case_name(*c))
def test_oracle_obs_model(synth, case):
    """converge True, False (the stored planes at a shifted state), True, clean semantics."""
    res, ext = case
    ci = P.case_inputs(synth)
    o = _oracle(ci, res, 27, P.MAX_RANGE, "GN")
    ratios = []
    for k, (st, (want, n0)) in enumerate(zip(P.lio_states(ci), P.measure_lio(ci, res, ext))):
        key = P.lio_case_name(res, ext, k)
        H1, h1, n1, s1 = o.obs_model(*st, ext, P.LIO_STEPS[k][2])
        assert n1 == n0 == P.NOISE_MEASURED[key]["count"] and n0 > 300
        _check_quantities(key, {"HTH": H1, "HTh": h1, "sum_h2": s1}, want, ratios)
        assert bool(want["HTH"][0][6:, :].any()) == ext and bool(want["HTh"][0][6:].any()) == ext
    assert max(ratios) <= P.ORACLE_RATIO_MEASURED * 1.0001, max(ratios)


def test_margin_is_four_times_the_largest_oracle_ratio():
    assert P.MARGIN == max(4.0, 4.0 * P.ORACLE_RATIO_MEASURED) and P.PLANE_CAP == 4.0 * P.ORACLE_PLANE_DEVIATION_MEASURED
    for key, row in P.NOISE_MEASURED.items():
        for q in row:
            if q != "count":
                assert P.tolerance(key, q) <= (P.PLANE_CAP if q == "planes" else P.HB_RTOL)


# ---- the reference against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,nn", [(0.5, 27), (0.25, 19)])
def test_b_is_half_the_gradient_of_the_cost(synth, res, nn):
    """d compute_error(exp(eps) T) / d eps = 2 b on the frozen selected set and planes (pose not rounded): e is linear in the
    translation and the truncation term of the rotation is h^2 / 6; observed 1e-9 ... 2e-8."""
    ci = P.case_inputs(synth)
    r = P.make_reference(ci, res, nn, P.MAX_RANGE)
    for T in ci.poses.values():
        b = r.linearize(T)[2]
        d = P.derivative_discrepancy(lambda X: r.compute_error(X, exact=True), P.round32(T), b)
        print(res, nn, d)
        assert d < 1e-6


@pytest.mark.parametrize("ext", [False, True])
def test_lio_row_is_the_derivative_of_the_residual(synth, ext):
    """The 12 columns are d e / d (pos; rot, right: rot exp(d); off_R, right: off_R exp(d); off_T), by central differences of the
    reference's own residual with planes and set frozen: frame and sign of every block.  extrinsic_est_en off: the last six are zero
    although the derivative is not."""
    ci = P.case_inputs(synth)
    r = P.make_reference(ci, 0.5, 27, P.MAX_RANGE)
    rot, pos, oR, oT = P.lio_state(ci.fx.guess)
    r.obs_model(rot, pos, oR, oT, ext, True)
    rows = r.lio_rows(r.selected, rot, oR, oT, True, exact=True)
    h = 1e-5
    num = np.zeros_like(rows)

    def at(k, s):
        d = np.zeros(12); d[k] = s * h
        rot2 = (P.Rotation.from_quat(rot) * P.Rotation.from_rotvec(d[3:6])).as_quat()
        oR2 = (P.Rotation.from_quat(oR) * P.Rotation.from_rotvec(d[6:9])).as_quat()
        return r.lio_residual(rot2, pos + d[0:3], oR2, oT + d[9:12])
    for k in range(12):
        num[:, k] = (at(k, 1.0) - at(k, -1.0)) / (2.0 * h)
    print(np.abs(rows - num).max(axis=0) / np.abs(num).max(axis=0))
    assert (np.abs(rows - num).max(axis=0) <= 1e-7 * np.abs(num).max(axis=0)).all() and (np.abs(num).max(axis=0) > 0.1).all()
    used = r.lio_rows(r.selected, rot, oR, oT, ext)
    assert P.rel_err(used[:, :6], rows[:, :6]) < 1e-6 and (P.rel_err(used[:, 6:], rows[:, 6:]) < 1e-6 if ext else not used[:, 6:].any())


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
# (mutation, (variant, res, nn, max_range)) -- each on a case of the GPU file
SENSITIVITY = [("floor", ("main", 0.5, 27, P.MAX_RANGE)), ("no_centre_26", ("main", 0.5, 27, P.MAX_RANGE)), ("no_centre_18", ("main", 0.25, 19, P.MAX_RANGE)),
               ("nine", ("main", 0.5, 27, P.MAX_RANGE)), ("n_cross_q", ("main", 0.5, 27, P.MAX_RANGE)), ("d_is_norm", ("main", 0.5, 27, P.MAX_RANGE)),
               ("min_knn_5", ("main", 0.25, 27, P.MAX_RANGE)), ("h_plus", ("main", 0.5, 27, P.MAX_RANGE))]


@pytest.mark.parametrize("mutation,case", SENSITIVITY, ids=[m for m, _ in SENSITIVITY])
def test_fixture_sees_the_misreading(synth, mutation, case):
    """A misreading put into the reference changes a count (compared exactly) or moves a compared quantity by at least 10 x the tolerance
    it is compared at, on the inputs the GPU tests use."""
    variant, res, nn, rng = case
    ci = P.case_inputs(synth, variant)
    r, m = P.make_reference(ci, res, nn, rng), P.make_reference(ci, res, nn, rng, mutation=mutation)
    worst, counts = 0.0, False
    if mutation == "h_plus":
        st = P.lio_state(ci.fx.guess)
        a, b = r.obs_model(*st, True, True), m.obs_model(*st, True, True)
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and a[3] == b[3]                      # the sign of h shows in H^T h alone
        worst = P.rel_err(b[1], a[1]) / P.tolerance(P.lio_case_name(res, True, 0), "HTh")
    else:
        for pose, T in ci.poses.items():
            key = P.case_name(*case, pose)
            a, b = r.linearize(T), m.linearize(T)
            counts |= a[3] != b[3] or not np.array_equal(r.selected, m.selected)
            pairs = {"cost": (a[0], b[0]), "H": (a[1], b[1]), "b": (a[2], b[2]), "compute_error": (r.compute_error(P.shifted(T)), m.compute_error(P.shifted(T)))}
            if np.array_equal(r.selected, m.selected):
                pairs["planes"] = (r.planes(), m.planes())
            worst = max([worst] + [P.deviation(y, x, q) / P.tolerance(key, q) for q, (x, y) in pairs.items()])
    print(mutation, case, "counts differ" if counts else "", "%.1f x tolerance" % worst)
    assert worst >= 10.0
    if mutation in ("floor", "no_centre_26", "no_centre_18", "nine", "min_knn_5"):
        assert counts


def test_invisible_misreadings_are_listed(synth):
    """`<=` for `<` in the range test and `>=` for `>` in the threshold test change nothing on these inputs, by construction (the
    removal rule keeps every distance and every plane away from equality); they are listed with their reason, as are the neighbours'
    row order and the cells' visiting order."""
    ci = P.case_inputs(synth)
    for mutation, rng in (("range_le", P.BINDING_RANGE), ("threshold_ge", P.MAX_RANGE)):
        r, m = P.make_reference(ci, 0.5, 27, rng), P.make_reference(ci, 0.5, 27, rng, mutation=mutation)
        a, b = r.linearize(ci.fx.guess), m.linearize(ci.fx.guess)
        assert a[0] == b[0] and a[3] == b[3] and np.array_equal(a[1], b[1]) and mutation in P.INVISIBLE
    assert set(m for m, _ in SENSITIVITY) | {"range_le", "threshold_ge"} == set(P.MUTATIONS)
    assert {"neighbour_row_order", "cell_visit_order"} <= set(P.INVISIBLE)
