"""A context that lives through growth, shrink and swap computes what a fresh context computes.

Every device array of a context is grow-only and capacity-managed: a context that has seen a larger cloud runs the next, smaller
one inside the allocations it kept.  The tests drive one context through 400 -> 4000 -> 400 target points (the sizes cross every
capacity once, then run below it) and compare each step, bit for bit, with a fresh context given the same pair; then the target
log's growth through pcm_target_insert, the resize semantics of the LIO per-point members, and the destruction of every context.
Run on the MI355X box with ``-m gpu``."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODELS = ["P2PlaneRegistration", "GicpRegistration", "VgicpRegistration", "VgicpCudaRegistration", "NdtRegistration", "PclNdtRegistration"]
SIZES = (400, 4000, 400)
SHIFT = np.array([0.05, -0.03, 0.02, 0.0], np.float32)


@pytest.fixture(scope="module")
def clouds(synth):
    """target of n points and its source (every 4th point, shifted), for every size of the sequence; read-only"""
    out = {}
    for n in sorted(set(SIZES)):
        tgt = synth.sample_submap(synth.scene_for_points(77, n, 8.0), n, 78)
        src = np.ascontiguousarray(tgt[::4] + SHIFT)
        tgt.setflags(write=False); src.setflags(write=False)
        out[n] = (tgt, src)
    return out


def _make(pcm, name):
    return getattr(pcm, name)(0, max_iterations=3)


def _bits(*arrays):
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


def _outcome(pcm, reg, with_linearize):
    """everything an align reports, as bytes (NaNs compare too); for the least-squares models also the normal equations
    (cost, H, b, inliers) at the final pose"""
    try:
        r = reg.align(np.eye(4, dtype=np.float32))
    except pcm.PcmError as e:
        return ("error", e.code)
    out = _bits(r.T, r.T64, r.H, np.float64(r.cost)) + (r.iterations, r.status, r.converged, r.num_inliers, r.num_linearize, r.num_compute_error)
    if with_linearize:
        cost, H, b, inl = reg.evaluate_cost(r.T64)
        out += _bits(np.float64(cost), H, b) + (inl,)
    return out


@pytest.mark.parametrize("name", MODELS)
def test_reused_context_equals_fresh(pcm, clouds, name):
    lsq = name != "PclNdtRegistration"   # pclomp NDT has no pcm_linearize
    reused = _make(pcm, name)
    for step, n in enumerate(SIZES):
        tgt, src = clouds[n]
        reused.set_input_target(tgt); reused.set_input_source(src)
        fresh = _make(pcm, name)
        fresh.set_input_target(tgt); fresh.set_input_source(src)
        a, b = _outcome(pcm, reused, lsq), _outcome(pcm, fresh, lsq)
        assert a[0] != "error", (name, step, a)
        assert a == b, (name, step, n)
        if n == max(SIZES):
            # swap on the grown context: equal to a fresh one given the pair the other way round
            reused.swap_source_and_target()
            other = _make(pcm, name)
            other.set_input_target(src); other.set_input_source(tgt)
            a, b = _outcome(pcm, reused, lsq), _outcome(pcm, other, lsq)
            assert a == b, (name, "swap")
            other.__del__()
        fresh.__del__()
    reused.__del__()
    gc.collect()


@pytest.mark.parametrize("first_target", ["host", "device", "borrowed"])
def test_target_log_growth(pcm, synth, clouds, first_target):
    """three inserts of 300 points onto a 400-point target: the log (400 slots) grows on the first; the points stay in order.
    device: the first target is a device tensor of stride 16; borrowed: it is used in place (it came in as a zero-copy source
    and was swapped into the target's place), so the first insert copies it into an owned log"""
    import torch
    tgt, src = clouds[400]
    more = synth.sample_submap(synth.scene_for_points(77, 900, 8.0), 900, 79)
    parts = [tgt] + [more[300 * k:300 * (k + 1)] for k in range(3)]
    g = _make(pcm, "P2PlaneRegistration")
    dev = None if first_target == "host" else torch.from_numpy(np.array(tgt)).cuda()   # kept alive to the end
    if first_target == "borrowed":
        g.set_input_source(dev); g.set_input_target(src)
        g.swap_source_and_target()
    else:
        g.set_input_target(tgt if dev is None else dev)
        g.set_input_source(src)
    for p in parts[1:]:
        g.target_insert(p)
    whole = np.concatenate(parts)
    assert np.array_equal(g.get_target(), whole[:, :3])
    fresh = _make(pcm, "P2PlaneRegistration")
    fresh.set_input_target(whole); fresh.set_input_source(src)
    a, b = _outcome(pcm, g, False), _outcome(pcm, fresh, False)
    assert a[0] != "error" and a == b
    g.__del__(); fresh.__del__()
    del dev


def test_lio_members_survive_a_larger_scan(pcm, synth):
    """residuals_.resize(n, 0); point_selected_surf_.resize(n, true): the entries of the old scan stay, new ones take the defaults"""
    tgt = synth.sample_submap(synth.scene_for_points(77, 20000, 8.0), 20000, 80)
    scan = np.ascontiguousarray(tgt[::4][:1500] + SHIFT)
    g = pcm.P2PlaneRegistration(0, flags=pcm.capi.PCM_FLAG_LIO_REFERENCE_SEMANTICS)
    g.set_input_target(tgt)
    g.set_input_source(scan[:500])
    ident = ((0, 0, 0, 1.0), (0, 0, 0), (0, 0, 0, 1.0), (0, 0, 0))
    g.obs_model(*ident, True, True)
    res0, sel0 = g.get_lio_members(500)
    assert np.count_nonzero(res0) > 50          # the call left residuals behind
    g.set_input_source(scan)
    res1, sel1 = g.get_lio_members(1500)
    assert np.array_equal(res1[:500].view(np.uint32), res0.view(np.uint32)) and np.array_equal(sel1[:500], sel0)
    assert not res1[500:].any() and sel1[500:].all()
    g.__del__()
