"""GPU checks of point-to-point ICP (PCM_MODEL_ICP, csrc/icp.hip) against the numpy restatement of its rules (tests/icp_ref.py) on the
cases of tests/icp_cases.py: the smallest clouds at which the pair kernel, the block-order reduction and the step can go wrong.

Equalities: the stop reason, the iteration count, `converged` and the pair count N of every iteration.  The inputs keep every
discrete decision away from a tie -- in every iteration every query's nearest and second-nearest squared distance differ by at
least 1e-4 relative, and no threshold comparison lies within 1e-9 relative of equality (one deliberate exact equality aside) --
which is asserted here on the reference's trace, not assumed.

Bound on the 16 entries of T: the device adds the pair terms in another order than numpy and takes the SVD by two-sided Jacobi
instead of LAPACK, all in double, so the double poses differ by rounding; the float result follows, and moves by one more float
ulp where the double pose lies that near a rounding boundary.  Measured on an MI355X over every case below: largest
|T64 - T64_ref| = 1.63e-14 (n257), largest |T - T_ref| = 1.47e-14 (no entry crossed a float rounding boundary).  DESIGN.md
section 37."""
import ctypes as C

import numpy as np
import pytest

import icp_cases as K
import icp_ref as R

pytestmark = pytest.mark.gpu

# 100 x the measured 1.63e-14 for the summation order; the float result may add one float ulp of the pose's largest entry
# (below 4 in every case: 2.4e-7 at most), which keeps the bound under the float resolution of 1e-6 it may never pass.
T64_BOUND = 1.7e-12


def t_bound(T_ref):
    b = T64_BOUND + float(np.spacing(np.float32(np.abs(T_ref).max())))
    assert b <= 1e-6
    return b


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make(pcm, name, device_inputs=False):
    from pointcloud_slam_amd import icp
    src, tgt, guess, params = K.inputs(name)
    g = icp.IterativeClosestPoint(0, **params)
    keep = None
    if device_inputs:
        import torch
        pad = np.zeros((len(src), 4), np.float32)
        pad[:, :3] = src
        keep = (torch.tensor(pad, device="cuda:0"), torch.tensor(np.array(tgt), device="cuda:0"))
        g.set_input_target(keep[1])
        g.set_input_source(keep[0])
    else:
        g.set_input_target(tgt)
        g.set_input_source(src)
    return g, guess, keep


def conditions(name):
    ref = K.reference(name)
    assert ref["min_gap"] >= K.MIN_GAP, (name, ref["min_gap"])
    assert ref["min_margin"] >= K.MIN_MARGIN, (name, ref["min_margin"])
    assert ref["exact_ties"] == (1 if name == "threshold_kept" else 0)
    return ref


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case_equals_reference(pcm, name):
    from pointcloud_slam_amd import icp
    ref = conditions(name)
    g, guess, _ = make(pcm, name)
    r = g.align(guess)
    N, mse = g.trace()
    want_N = [t["N"] for t in ref["trace"]]
    print(name, "iterations", r.iterations, "stop", r.stop_reason, "N", list(N)[:4], "worst |T - T_ref|", np.abs(r.T - ref["T"]).max(),
          "worst |T64 - T64_ref|", np.abs(r.T64 - ref["T64"]).max())
    assert r.stop_reason == icp.STOP_REASON[ref["stop"]]
    assert (r.iterations, r.converged) == (ref["iterations"], ref["converged"])
    assert list(N) == want_N and r.num_pairs == ref["num_pairs"]
    assert np.abs(r.T - ref["T"]).max() <= t_bound(ref["T"])
    assert np.abs(r.T64 - ref["T64"]).max() <= T64_BOUND
    ref_mse = np.array([t["mse"] for t in ref["trace"]])
    assert np.allclose(mse, ref_mse, rtol=1e-9, atol=1e-30) or name == "mirrored"   # mirrored: an exact fit, mse is rounding residue
    assert np.array_equal(g.get_final_transformation(), r.T) and g.has_converged() == r.converged
    # pcm_fitness_score after align equals the reference's at the same float pose (n double additions in another order)
    if ref["iterations"] > 0:
        src, tgt, _, _ = K.inputs(name)
        want = R.fitness(src, tgt, r.T)
        assert abs(g.get_fitness_score() - want) <= 1e-12 * max(want, 1e-30)


def test_lattice_recovers_the_known_pose(pcm):
    """i <-> i from the first iteration on: N = 7 throughout, and the known SE(3) comes back from a non-identity guess"""
    ref = conditions("lattice")
    g, guess, _ = make(pcm, "lattice")
    assert not np.array_equal(guess, np.eye(4, dtype=np.float32))
    r = g.align(guess)
    assert list(g.trace()[0]) == [7] * r.iterations
    assert np.abs(r.T64 - K.T_LATTICE).max() < 1e-5   # the source is the float32 image of the exact one: 1e-6 m per coordinate
    assert np.abs(ref["T64"] - K.T_LATTICE).max() < 1e-5


def test_every_stop_reason_is_reached(pcm):
    from pointcloud_slam_amd import icp
    seen = set()
    for name in ("lattice_transform_stop", "lattice_abs_mse_stop", "n63_rel_mse_stop", "lattice_no_pairs", "n257_three_iterations"):
        g, guess, _ = make(pcm, name)
        seen.add(g.align(guess).stop_reason)
    assert seen == set(icp.STOP_REASON.values()) - {"none"}


def test_iteration_cap_counts_as_converged(pcm):
    ref = conditions("n257_three_iterations")
    assert K.reference("n257")["iterations"] > 3   # the pair needs more
    g, guess, _ = make(pcm, "n257_three_iterations")
    r = g.align(guess)
    assert (r.iterations, r.converged, r.stop_reason) == (3, True, "iterations") and ref["stop"] == R.STOP_ITERATIONS


def test_threshold_is_inclusive(pcm):
    """d2 = 25 exactly against max_correspondence_distance = 5 is a pair; against 4.999 it is not"""
    for name, n in (("threshold_kept", 4), ("threshold_dropped", 3)):
        conditions(name)
        g, guess, _ = make(pcm, name)
        g.align(guess)
        assert list(g.trace()[0]) == [n], name


def test_too_few_pairs_leave_the_guess(pcm):
    for name, n in (("lattice_no_pairs", 0), ("two_pairs", 2)):
        conditions(name)
        g, guess, _ = make(pcm, name)
        r = g.align(guess)
        assert (r.stop_reason, r.converged, r.iterations, r.num_pairs) == ("no_correspondences", False, 0, n)
        assert np.array_equal(bits(r.T), bits(guess)) and list(g.trace()[0]) == [n]


def test_non_finite_points_are_dropped(pcm):
    ref = conditions("bad_points")
    g, guess, _ = make(pcm, "bad_points")
    r = g.align(guess)
    assert set(g.trace()[0]) == {60} and r.num_pairs == 60 and np.isfinite(r.T).all() and ref["num_pairs"] == 60


@pytest.mark.parametrize("name", ["n257", "n1000", "lattice"])
def test_host_and_device_inputs_and_two_runs_give_the_same_bytes(pcm, name):
    """n1000 runs 20 iterations: chunk boundaries after the 8th and the 16th fall inside the run"""
    from pointcloud_slam_amd import capi
    g, guess, _ = make(pcm, name)
    a = g.align(guess)
    b = g.align(guess)
    gd, _, keep = make(pcm, name, device_inputs=True)
    c = gd.align(guess)
    for o in (b, c):
        assert np.array_equal(a.T64.view(np.uint64), o.T64.view(np.uint64)) and np.array_equal(bits(a.T), bits(o.T))
        assert (a.iterations, a.converged, a.stop_reason, a.num_pairs, a.mse) == (o.iterations, o.converged, o.stop_reason, o.num_pairs, o.mse)
    assert np.array_equal(g.trace()[1], gd.trace()[1])
    if name == "n1000":
        assert a.iterations > 2 * capi.PCM_ICP_CHUNK_ITERATIONS
    assert g.get_fitness_score() == gd.get_fitness_score()
    del keep


def test_parameters_and_errors(pcm):
    from pointcloud_slam_amd import capi, icp
    g = icp.IterativeClosestPoint(0)
    assert g.params == dict(R.DEFAULTS)
    g.set_maximum_iterations(100); g.set_max_correspondence_distance(150.0); g.set_transformation_epsilon(1e-6)
    g.set_euclidean_fitness_epsilon(1e-6); g.set_transformation_rotation_epsilon(0.5)
    assert g.params == dict(R.DEFAULTS, max_iterations=100, max_correspondence_distance=150.0, transformation_epsilon=1e-6, euclidean_fitness_epsilon=1e-6,
                            rotation_epsilon=0.5)
    for call in (lambda: g.set_maximum_iterations(0), lambda: g.set_max_correspondence_distance(0.0), lambda: g.set_transformation_epsilon(float("nan"))):
        with pytest.raises(capi.PcmError) as e:
            call()
        assert e.value.code == capi.PCM_ERR_INVALID_ARGUMENT
    assert g.params["max_iterations"] == 100
    with pytest.raises(capi.PcmError) as e:
        g.align()
    assert e.value.code == capi.PCM_ERR_NO_INPUT
    with pytest.raises(KeyError):
        icp.IterativeClosestPoint(0, no_such_field=1)
    # the ICP calls on a context of another model, and the calls ICP has no use for
    other = pcm.GicpRegistration(0)
    p = capi.PcmIcpParams()
    other._L.pcm_icp_default_params(C.byref(p))
    assert other._L.pcm_icp_set_params(other.handle, C.byref(p)) == capi.PCM_ERR_UNSUPPORTED
    info = capi.PcmIcpInfo()
    assert other._L.pcm_icp_last(other.handle, C.byref(info)) == capi.PCM_ERR_UNSUPPORTED
    src, tgt, guess, _ = K.inputs("lattice")
    g.set_input_target(tgt); g.set_input_source(src)
    T = np.eye(4)
    assert g._L.pcm_linearize(g.handle, T.ctypes.data, None, None, None, None) == capi.PCM_ERR_UNSUPPORTED
