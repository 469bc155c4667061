"""The P2PLANE kernels (k_linearize with the LDS grid and with per-lane probing, k_linearize_counted, k_linearize_lists and its following-lists
variant, linearize_reforder.hip) and the LIO twins (k_linearize<., LIO>, k_lio_lists) against the independent numpy reference of
p2plane_numpy_ref.py.  The CPU oracle is not loaded here.

Inputs: p2plane_numpy_ref.build_fixture / case_inputs -- synth.make_pair(3, 600, 3000) less the points at which a float32 search could
legitimately differ from an exact one (margins in test_p2plane_numpy_ref.py), so nothing below excuses a point, an inlier or a digit:
with sort_source = 0 the selection mask per point, every selected plane, the inlier count, H, b, the cost and compute_error at a shifted
pose; with sort_source = 1 (the device re-orders the scan) the count and the sums.  Tolerances: p2plane_numpy_ref.tolerance(), never from
a kernel's result.  What these inputs can and cannot see is pinned by test_p2plane_numpy_ref.test_fixture_sees_the_misreading.
Measured on an MI355X, largest deviation from numpy over every path (flags 64, 64|1, 8, 16, 32, 128, default; sort_source 0 and 1): planes
2.2e-5 (tolerance 8.9e-5), cost 4.5e-6, compute_error 3.7e-6, H 1.5e-6, b 7.6e-6, H^T H 5.1e-7, H^T h 7.7e-6, sum h^2 2.8e-6 (tolerance 1e-5);
every mask and count equal.  The CPU oracle shows the same figures to three digits.
"""
import numpy as np
import pytest

import p2plane_numpy_ref as P

pytestmark = pytest.mark.gpu

TILE, TILE_GLOBAL, COUNTED, LISTS, REF_ORDER, FOLLOW, DEFAULT = 64, 64 | 1, 8, 16, 32, 128, 0
PATHS = (TILE, TILE_GLOBAL, COUNTED, LISTS, REF_ORDER, FOLLOW, DEFAULT)


def _reg(pcm, ci, res, nn, max_range, flags, sort_source=0):
    g = pcm.P2PlaneRegistration(0, optimizer="LM", voxel_resolution=res, num_neighbors=nn, flags=flags, sort_source=sort_source)
    if max_range != P.MAX_RANGE:
        g.set_max_range(max_range)
    if flags == FOLLOW:          # the target in two parts, so that the lists really follow
        half = len(ci.target) // 2
        g.set_input_target(ci.target[:half]); g.set_input_source(ci.scan)
        g.evaluate_cost(next(iter(ci.poses.values())))
        g.target_insert(ci.target[half:])
    else:
        g.set_input_target(ci.target); g.set_input_source(ci.scan)
    return g


def _check_path(g, flags, evaluations):
    """The kernel that was meant ran: lists exist for the lists paths (the default builds them at a target's second registration), and
    only for them; following lists were updated by the insert."""
    info = g.neighbour_list_info()
    if flags in (LISTS, FOLLOW) or (flags == DEFAULT and evaluations >= 2):
        assert info["lists"] > 0, info
    if flags in (TILE, TILE_GLOBAL, COUNTED, REF_ORDER):
        assert info["lists"] == 0, info
    if flags == FOLLOW:
        assert info["updates"] + info["rebuilds"] >= 1, info


def _check_at(g, r, key, T, per_point, worst):
    c0, H0, b0, n0 = r.linearize(T)
    c1, H1, b1, n1 = g.evaluate_cost(T)
    e0, e1 = r.compute_error(P.shifted(T)), g.compute_error(P.shifted(T))
    got, want = {"cost": c1, "H": H1, "b": b1, "compute_error": e1}, {"cost": c0, "H": H0, "b": b0, "compute_error": e0}
    if per_point:
        pl = g.get_planes(len(r.src))
        assert np.array_equal(~np.isnan(pl[:, 0]), r.selected), key
        got["planes"], want["planes"] = pl, r.planes()
    dev = {q: P.deviation(got[q], want[q], q) for q in want}
    print("%-28s count %d %d  " % (key, n1, n0) + "  ".join("%s %.2e" % kv for kv in dev.items()))
    assert n1 == n0 == P.NOISE_MEASURED[key]["count"], key
    for q, d in dev.items():
        worst[q] = max(worst.get(q, 0.0), d)
        assert d <= P.tolerance(key, q), (key, q, d, P.tolerance(key, q))
    if n0:
        assert abs(e0 - c0) > 10.0 * P.HB_RTOL * c0          # compute_error and the cost cannot be confused at these tolerances


def _run_case(pcm, synth, case, flags, sort_source=0):
    variant, res, nn, rng = case
    ci = P.case_inputs(synth, variant)
    r = P.make_reference(ci, res, nn, rng)
    g = _reg(pcm, ci, res, nn, rng, flags, sort_source)
    worst, k = {}, 1 if flags == FOLLOW else 0
    for pose, T in ci.poses.items():
        _check_at(g, r, P.case_name(*case, pose), T, sort_source == 0, worst)
        k += 1
        _check_path(g, flags, k)
    if flags == DEFAULT and len(ci.poses) == 1:         # the second registration: now on the lists
        _check_at(g, r, P.case_name(*case, "guess"), ci.fx.guess, sort_source == 0, worst)
        _check_path(g, flags, 2)
    print("worst", {q: "%.2e" % v for q, v in worst.items()})
    return r, g


# ---- every kernel path, neighbourhoods 1 / 7 / 19 / 27, both resolutions, both poses ---------------------------------------------
@pytest.mark.parametrize("res", P.RESOLUTIONS)
@pytest.mark.parametrize("flags", PATHS, ids=["tile", "tile_global", "counted", "lists", "reforder", "following", "default"])
def test_paths(pcm, synth, flags, res):
    for nn in P.NEIGHBOURS:
        _run_case(pcm, synth, ("main", res, nn, P.MAX_RANGE), flags)


@pytest.mark.parametrize("flags", (TILE, LISTS, DEFAULT), ids=["tile", "lists", "default"])
def test_sorted_source(pcm, synth, flags):
    """sort_source = 1: the device re-orders the scan (the tile kernel then stages tiles in LDS), so counts and sums only."""
    for res in P.RESOLUTIONS:
        r, g = _run_case(pcm, synth, ("main", res, 27, P.MAX_RANGE), flags, sort_source=1)
    if flags == TILE:
        g.set_profiling(2); g.align(P.case_inputs(synth).fx.guess.astype(np.float32))
        st = g.stats()
        assert st["tiles"] > 0 and st["tiles_lds_grid"] > 0, st


# ---- centred, the binding range, tails, lone voxels, the empty neighbourhood -----------------------------------------------------
SPECIAL = [c for c in P.CASES if not (c[0] == "main" and c[3] == P.MAX_RANGE)]


@pytest.mark.parametrize("flags", (TILE, COUNTED, LISTS), ids=["tile", "counted", "lists"])
@pytest.mark.parametrize("case", SPECIAL, ids=lambda c: P.case_name(*c))
def test_special(pcm, synth, case, flags):
    r, g = _run_case(pcm, synth, case, flags)
    if case[0] == "centred":
        P.assert_both_signs(P.build_fixture(synth, centred=True))
    if case[0] == "empty":                              # the point whose 27 cells are empty adds nothing: count and sums of the 64 others
        ci = P.case_inputs(synth, "empty")
        T = ci.fx.guess
        g2 = _reg(pcm, P.types.SimpleNamespace(scan=ci.scan[:64], target=ci.target, poses=ci.poses), case[1], case[2], case[3], flags)
        a, b = g.evaluate_cost(T), g2.evaluate_cost(T)
        assert a[3] == b[3] and a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert np.isnan(g.get_planes(65)[64, 0]) and r.found.m[64] == 0


# ---- the LIO measurement model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", (TILE, LISTS), ids=["tile", "lists"])
@pytest.mark.parametrize("case", P.LIO_CASES, ids=lambda c: P.lio_case_name(*c))
def test_obs_model(pcm, synth, case, flags):
    """converge True, False (the stored planes at a shifted state), True; extrinsic_est_en off and on; k_linearize<., LIO> and k_lio_lists."""
    res, ext = case
    ci = P.case_inputs(synth)
    r = P.make_reference(ci, res, 27, P.MAX_RANGE)
    g = _reg(pcm, ci, res, 27, P.MAX_RANGE, flags)
    worst = {}
    for k, st in enumerate(P.lio_states(ci)):
        key = P.lio_case_name(res, ext, k)
        H0, h0, n0, s0 = r.obs_model(*st, ext, P.LIO_STEPS[k][2])
        H1, h1, n1, s1, valid = g.obs_model(*st, ext, P.LIO_STEPS[k][2])
        dev = {q: P.deviation(a, b, q) for q, a, b in (("HTH", H1, H0), ("HTh", h1, h0), ("sum_h2", s1, s0))}
        print("%-24s count %d %d  " % (key, n1, n0) + "  ".join("%s %.2e" % kv for kv in dev.items()))
        assert valid and n1 == n0 == P.NOISE_MEASURED[key]["count"]
        for q, d in dev.items():
            worst[q] = max(worst.get(q, 0.0), d)
            assert d <= P.tolerance(key, q), (key, q, d, P.tolerance(key, q))
        assert bool(H1[6:, :].any()) == ext and bool(h1[6:].any()) == ext
    print("worst", {q: "%.2e" % v for q, v in worst.items()})
    assert g.lio_search_path() == ((2, 0) if flags == LISTS else (0, 2))          # two matching calls, on the kernel that was meant
