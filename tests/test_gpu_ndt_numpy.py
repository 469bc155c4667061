"""The float kernels -- k_ndt<KIND, TRIAL> with k_gauss_voxels / k_vgc_voxels (csrc/ndt.hip, voxel_hash.hip, gicp.hip) and the pclomp NDT
passes (csrc/pclndt.hip: k_pclndt_leaves, k_pclndt_derivatives<HESS>, k_pclndt_hessian, k_pclndt_score) -- against the independent numpy
reference of ndt_numpy_ref.py.  The CPU oracle is not loaded here.

Inputs: ndt_numpy_ref.build_fixture -- make_pair(3, 1100, 12000) at density 60 for pclomp NDT and the Gaussian-voxel cases at 1.0 m, at
density 150 for the Gaussian-voxel cases at 0.5 m (why: ndt_numpy_ref.DENSITY), less the points at which a float cell decision could
legitimately differ from an exact one; every context is built on them.  Counts exact; the pclomp double Hessian and calculateScore to
1e-9; every other quantity to tolerance(case, quantity) = min(MARGIN x the rounding noise measured on the CPU, HB_RTOL): the kernel is
never used to set its own tolerance.  Every deviation is printed.
Observed on an MI355X, largest relative deviation from numpy (its multiple of that quantity's rounding noise): k_ndt cost 8.5e-7 (58 x, P2D
swapped: noise 1.5e-8), H 2.1e-6 (3.0 x), b 5.9e-6 (1.4 x; P2D 27 at 0.5 m centred), compute_error 8.1e-7 (9.3 x); pclomp score 3.5e-8,
gradient 2.4e-7 (2.6 x), float Hessian 2.0e-7; pclomp double Hessian 8.4e-15, calculateScore 4.6e-16; every count equal; the kernel's
derivative discrepancy equals the reference's truncation term to two digits (3.3e-4 ... 2.7e-3; VGICP_CUDA at T_gt 5.9e-6 against 6.8e-6).
"""
import numpy as np
import pytest

import ndt_numpy_ref as N
from ndt_numpy_ref import F64, rel_err

pytestmark = pytest.mark.gpu


def _name(case):
    return N.case_name(*case)


def _dev(a, b):
    return abs(a - b) / abs(b) if np.ndim(b) == 0 else rel_err(a, b)


def _kndt_both(pcm, ci, model, nn, res, flags=None):
    kw = dict(voxel_resolution=res)
    if isinstance(nn, str):
        kw["neighbor_search_radius"] = float(nn[1:])
    else:
        kw["num_neighbors"] = nn
    if flags is not None:
        kw["flags"] = flags
    if model == "VGICP_CUDA":
        g = pcm.VgicpCudaRegistration(0, optimizer="LM", **kw)
    else:
        g = pcm.NdtRegistration(0, model=model, optimizer="LM", **kw)
    g.set_input_target(ci.target); g.set_input_source(ci.scan)
    r = N.NdtReference(ci.scan, ci.target, model, voxel_resolution=res, num_neighbors=nn)
    if model == "VGICP_CUDA":        # data: what the device holds (the estimators are pinned elsewhere)
        r.set_covariances(g.get_covariances(False), False); r.set_covariances(g.get_covariances(True), True)
    if ci.swapped:
        g.swap_source_and_target(); r.swap_source_and_target()
    return r, g


def _check_kndt(r, g, T, key):
    c0, H0, b0, n0 = r.linearize(T)
    c1, H1, b1, n1 = g.evaluate_cost(T)
    e0, e1 = r.compute_error(N.TRIAL(T)), g.compute_error(N.TRIAL(T))
    assert n1 == n0 == N.NOISE_MEASURED[key]["count"] and n0 > 0
    bad = []
    for q, x, y in (("cost", c1, c0), ("H", H1, H0), ("b", b1, b0), ("compute_error", e1, e0)):
        d, tol = _dev(x, y), N.tolerance(key, q)
        print("%-40s %-14s %.2e  (tolerance %.2e, noise %.2e)" % (key, q, d, tol, N.NOISE_MEASURED[key][q]))
        if not d <= tol:
            bad.append((q, d, tol))
    assert not bad, bad
    assert abs(e0 - c0) > 1e-4 * abs(c0)          # the trial pose is another pose
    return b1


# ---- k_ndt -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.all_kndt_cases(), ids=_name)
def test_kndt(pcm, synth, case):
    model, nn, res, variant = case
    ci = N.case_inputs(synth, variant, N.kndt_family(res))
    r, g = _kndt_both(pcm, ci, model, nn, res)
    for pose, T in ci.poses.items():
        _check_kndt(r, g, T, N.case_name(*case, pose))
    if variant == "sparse20" and model == "VGICP_CUDA":
        assert (r.corr.n_b == 1).any()                  # a correspondence reaches a voxel of one point
    if variant == "single_voxel":
        assert len(r.source_elements()[0]) == 1


@pytest.mark.parametrize("flags", [16, 64])
@pytest.mark.parametrize("model", N.MODELS)
def test_kndt_neighbour_rows(pcm, synth, model, flags):
    """flags = 16: k_ndt reads the neighbour voxel rows; 64: every cell is looked up.  Each path against the reference."""
    ci = N.case_inputs(synth)
    r, g = _kndt_both(pcm, ci, model, 27, 1.0, flags=flags)
    for pose, T in ci.poses.items():
        _check_kndt(r, g, T, N.case_name(model, 27, 1.0, "main", pose))


@pytest.mark.parametrize("model,nn,res", [("NDT_P2D", 7, 1.0), ("NDT_D2D", 27, 0.5), ("VGICP_CUDA", 7, 1.0)])
def test_kndt_derivative(pcm, synth, model, nn, res):
    """The kernel's own compute_error differentiated around T on the correspondences of its last evaluate_cost(T): 2 b plus the weight
    term the Gauss-Newton b leaves out (ndt_numpy_ref.NdtReference.cauchy_gradient_term; zero for VGICP_CUDA), within 10 x the
    truncation term measured on the reference."""
    ci = N.case_inputs(synth, "main", N.kndt_family(res))
    r, g = _kndt_both(pcm, ci, model, nn, res)
    for pose, T in ci.poses.items():
        r.linearize(T)
        _, _, b, _ = g.evaluate_cost(T)
        d = N.derivative_discrepancy(g.compute_error, T, b, r.cauchy_gradient_term())
        rec = N.DERIV_MEASURED[N.case_name(model, nn, res, pose)]
        print("derivative %s %s %.2e (reference %.2e)" % (model, pose, d, rec))
        assert d <= 10.0 * rec, d


def test_p2d_sparse_target_has_no_correspondence(pcm, synth):
    """A target thinned to at most 6 points per voxel (every 20th map point still leaves voxels of up to 17): P2D finds nothing: count 0,
    sums 0."""
    ci = N.case_inputs(synth)
    ci.target = N.thin_for_p2d(ci.target)
    assert N.gauss_voxels(ci.target[:, :3], 1.0).n.max() == 6
    r, g = _kndt_both(pcm, ci, "NDT_P2D", 27, 1.0)
    c0, H0, b0, n0 = r.linearize(ci.fx.guess)
    c1, H1, b1, n1 = g.evaluate_cost(ci.fx.guess)
    assert n0 == n1 == 0 and c0 == c1 == 0.0 and not H1.any() and not b1.any()


# ---- pclomp ----------------------------------------------------------------------------------------------------------------------
def _pcl_both(pcm, ci, nn, res, flags=None):
    kw = {} if flags is None else {"flags": flags}
    g = pcm.PclNdtRegistration(0, voxel_resolution=res, num_neighbors=nn, **kw)
    g.set_input_target(ci.target); g.set_input_source(ci.scan)
    r = N.PclNdtReference(ci.scan, ci.target, voxel_resolution=res, num_neighbors=nn, outlier_ratio=float(g.config.ndt_outlier_ratio))
    if ci.swapped:
        g.swap_source_and_target(); r.swap_source_and_target()
    return r, g


def _check_pcl(r, g, T, key):
    p = N.pose_vector(T)
    s0, g0, H0, n0 = r.derivatives(p, "float")
    assert n0 == N.NOISE_MEASURED[key]["count"] and n0 > 0
    s1, g1, H1 = g.ndt_derivatives(p, "float")
    s2, g2, _ = g.ndt_derivatives(p, None)
    bad = []
    for q, x, y in (("score", s1, s0), ("gradient", g1, g0), ("H_float", H1, H0), ("score", s2, s0), ("gradient", g2, g0)):
        d, tol = _dev(x, y), N.tolerance(key, q)
        print("%-40s %-14s %.2e  (tolerance %.2e, noise %.2e)" % (key, q, d, tol, N.NOISE_MEASURED[key][q]))
        if not d <= tol:
            bad.append((q, d, tol))
    Hd0 = r.derivatives(p, "double")[2]
    _, _, Hd1 = g.ndt_derivatives(p, "double")
    sc0, sc1 = r.score(N.pose_f32(T)), g.ndt_score(T)
    print("%-40s double Hessian %.2e  calculateScore %.2e" % (key, rel_err(Hd1, Hd0), abs(sc1 - sc0) / abs(sc0)))
    assert not bad, bad
    assert rel_err(Hd1, Hd0) < N.DOUBLE_TOL and sc0 != 0 and abs(sc1 - sc0) <= N.DOUBLE_TOL * abs(sc0)


@pytest.mark.parametrize("case", N.all_pcl_cases(), ids=_name)
def test_pclomp(pcm, synth, case):
    nn, res, variant = case
    ci = N.case_inputs(synth, variant)
    r, g = _pcl_both(pcm, ci, nn, res)
    for pose, T in ci.poses.items():
        _check_pcl(r, g, T, N.case_name("NDT_OMP", *case, pose))


@pytest.mark.parametrize("case", [c + ("main",) for c in N.pcl_cases()], ids=_name)
def test_pclomp_neighbour_leaf_lists(pcm, synth, case):
    """flags = 16: the passes read the grid's neighbour-leaf lists; against the reference, not only against the other path."""
    nn, res, variant = case
    ci = N.case_inputs(synth, variant)
    r, g = _pcl_both(pcm, ci, nn, res, flags=16)
    for pose, T in ci.poses.items():
        _check_pcl(r, g, T, N.case_name("NDT_OMP", *case, pose))


def test_pclomp_sparse_on_both_sides(pcm, synth):
    """Map and scan thinned to at most 5 points per leaf: no leaf takes part, whichever of the two is the target: no term, score and sums
    zero, before and after swap_source_and_target()."""
    ci = N.case_inputs(synth)
    ci.target, ci.scan = N.thin_for_pcl(ci.target), N.thin_for_pcl(ci.scan)
    assert N.pcl_leaves(ci.target[:, :3], 1.0).count.max() == 5 and N.pcl_leaves(ci.scan[:, :3], 1.0).count.max() == 5
    r, g = _pcl_both(pcm, ci, 27, 1.0)
    for T in (ci.fx.guess, ci.fx.swapped_pose):
        p = N.pose_vector(T)
        s0, g0, H0, n0 = r.derivatives(p, "float")
        s1, g1, H1 = g.ndt_derivatives(p, "float")
        assert n0 == 0 and s0 == s1 == 0.0 and not g1.any() and not H1.any()
        assert g.ndt_score(T) == r.score(N.pose_f32(T)) == 0.0
        r.swap_source_and_target(); g.swap_source_and_target()
