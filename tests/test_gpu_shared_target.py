"""pcm_share_target: several contexts registering against one built target.

A context that shares a target computes, bit for bit, what a context owning a copy of that target computes -- single aligns,
the normal equations at a fixed pose, batches, two contexts driven from two threads on their own streams -- for every model of
the core context; the holder count follows share / detach / destroy; the target outlives its first owner; what would change a
shared target is refused and changes nothing; and a sharing context takes no device memory for the target.
Shapes: a 20 000-point target and 2 000-point scans (the memory test: 524 288 points, see there).
Run on the MI355X box with ``-m gpu``."""
import ctypes as C
import gc
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
N_TGT, N_SCAN = 20000, 2000
SHIFT = np.array([0.05, -0.03, 0.02, 0.0], F)
LISTS = 16        # PCM_FLAG_NEIGHBOUR_LISTS
UNSUPPORTED, INVALID, NO_INPUT = -4, -1, -2
# (front class, configuration): every model of the core context; P2PLANE on the tile kernel's policy and with the lists from the start
MODELS = {
    "p2plane": ("P2PlaneRegistration", {}),
    "p2plane_lists": ("P2PlaneRegistration", {"flags": LISTS}),
    "gicp": ("GicpRegistration", {}),
    "vgicp": ("VgicpRegistration", {}),
    "vgicp_cuda": ("VgicpCudaRegistration", {}),
    "ndt_p2d": ("NdtRegistration", {"model": "NDT_P2D"}),
    "ndt_d2d": ("NdtRegistration", {}),
    "ndt_omp": ("PclNdtRegistration", {}),
}
POSE6 = np.array([0.04, -0.02, 0.03, 0.01, -0.005, 0.02])   # the fixed pose of the pclomp NDT derivatives


@pytest.fixture(scope="module")
def clouds(synth):
    """the target, a second target, and four scans of 2 000 points (every 10th target point from four offsets, shifted); read-only"""
    tgt = synth.sample_submap(synth.scene_for_points(77, N_TGT, 8.0), N_TGT, 78)
    other = synth.sample_submap(synth.scene_for_points(91, N_TGT, 8.0), N_TGT, 92)
    scans = [np.ascontiguousarray(tgt[k::10][:N_SCAN] + SHIFT * (1.0 + 0.25 * k)) for k in range(4)]
    for a in [tgt, other] + scans:
        a.setflags(write=False)
    return {"tgt": tgt, "other": other, "scans": scans}


def fixed_T():
    T = np.eye(4)
    T[:3, 3] = [0.03, -0.02, 0.01]
    return T


def make(pcm, key, **extra):
    name, cfg = MODELS[key]
    kw = dict(max_iterations=6)
    kw.update(cfg); kw.update(extra)
    return getattr(pcm, name)(0, **kw)


def destroy(*regs):
    for r in regs:
        r.__del__()
    gc.collect()


def align_bits(pcm, reg, guess=None):
    """the pcm_result record of one pcm_align, as bytes"""
    g = np.eye(4, dtype=F) if guess is None else np.ascontiguousarray(guess, dtype=F)
    res = pcm.capi.PcmResult()
    rc = pcm.load_library().pcm_align(reg.handle, g.ctypes.data, C.byref(res))
    assert rc in (0, pcm.capi.PCM_ERR_NOT_CONVERGED), (rc, pcm.load_library().pcm_last_error(reg.handle))
    return bytes(res)


def fresh_align_bits(pcm, reg, scan, guess=None):
    """a new scan on the context, then one align (the scan's device order is fixed by the first align's guess)"""
    reg.set_input_source(scan)
    return align_bits(pcm, reg, guess)


def linearize_bits(reg, key):
    """H, b (gradient) and cost at a fixed pose, as bytes"""
    if key == "ndt_omp":
        score, g, H = reg.ndt_derivatives(POSE6)
        return (np.float64(score).tobytes(), np.ascontiguousarray(g).tobytes(), np.ascontiguousarray(H).tobytes())
    cost, H, b, inl = reg.evaluate_cost(fixed_T())
    return (np.float64(cost).tobytes(), np.ascontiguousarray(H).tobytes(), np.ascontiguousarray(b).tobytes(), inl)


def error_of(L, h):
    return (L.pcm_last_error(h) or b"").decode()


# ---- 1. equality, per model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(MODELS))
def test_sharer_owner_and_independent_context_agree(pcm, clouds, key):
    a, b, c = make(pcm, key), make(pcm, key), make(pcm, key)
    a.set_input_target(clouds["tgt"])
    b.share_target(a)
    c.set_input_target(clouds["tgt"])
    assert a.target_share_count == 2 and b.target_share_count == 2 and c.target_share_count == 1
    scan = clouds["scans"][0]
    aligned = [fresh_align_bits(pcm, r, scan) for r in (a, b, c)]
    assert aligned[0] == aligned[1] == aligned[2]
    assert np.frombuffer(aligned[0], np.int32)[-6] > 0        # iterations: the registration ran
    lin = [linearize_bits(r, key) for r in (a, b, c)]
    assert lin[0] == lin[1] == lin[2]
    assert np.isfinite(np.frombuffer(lin[0][0], np.float64)[0])
    destroy(a, b, c)


# ---- 2. batch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["p2plane_lists", "gicp", "ndt_omp"])
def test_batch_over_sharers_equals_batch_over_owners(pcm, clouds, key):
    guesses = np.stack([np.eye(4, dtype=F)] * 4)

    def batch(regs):
        L = pcm.load_library()
        for r, s in zip(regs, clouds["scans"]):
            r.set_input_source(s)
        arr = (C.c_void_p * 4)(*[r.handle for r in regs])
        out = (pcm.capi.PcmResult * 4)()
        rc = L.pcm_align_batch(arr, 4, guesses.ctypes.data, out, None)
        assert rc in (0, pcm.capi.PCM_ERR_NOT_CONVERGED), (rc, error_of(L, regs[0].handle))
        return [bytes(out[i]) for i in range(4)]

    sharers = [make(pcm, key) for _ in range(4)]
    sharers[0].set_input_target(clouds["tgt"])
    for r in sharers[1:]:
        r.share_target(sharers[0])
    assert [r.target_share_count for r in sharers] == [4] * 4
    owners = [make(pcm, key) for _ in range(4)]
    for r in owners:
        r.set_input_target(clouds["tgt"])
    got, want = batch(sharers), batch(owners)
    assert got == want
    assert len(set(got)) == 4                                  # four different scans: four different results
    destroy(*(sharers + owners))


# ---- 3. two streams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["p2plane_lists", "vgicp"])
def test_two_sharers_on_two_threads_equal_the_serial_run(pcm, clouds, key):
    """every context has a stream of its own (pcm_create); the two threads run 8 alignments each at the same time"""
    a, b = make(pcm, key), make(pcm, key)
    a.set_input_target(clouds["tgt"])
    b.share_target(a)
    jobs = {a: [(clouds["scans"][k % 4], k) for k in range(8)], b: [(clouds["scans"][(k + 1) % 4], k + 3) for k in range(8)]}

    def guess(k):
        g = np.eye(4, dtype=F)
        g[:3, 3] = [0.01 * k, -0.005 * k, 0.002 * k]
        return g

    def run(reg, out):
        try:
            for scan, k in jobs[reg]:
                out.append(fresh_align_bits(pcm, reg, scan, guess(k)))
        except BaseException as e:   # reported by the assertion below
            out.append(e)

    serial = {a: [], b: []}
    for reg in (a, b):
        run(reg, serial[reg])
    threaded = {a: [], b: []}
    threads = [threading.Thread(target=run, args=(reg, threaded[reg])) for reg in (a, b)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for reg in (a, b):
        assert len(threaded[reg]) == 8 and all(isinstance(x, bytes) for x in threaded[reg]), threaded[reg][-1]
        assert threaded[reg] == serial[reg]
    assert len(set(serial[a])) == 8
    destroy(a, b)


# ---- 4. lifetime --------------------------------------------------------------------------------------------------------------------
def test_count_and_lifetime(pcm, clouds):
    key = "p2plane_lists"
    scan = clouds["scans"][0]
    a, b, c = make(pcm, key), make(pcm, key), make(pcm, key)
    a.set_input_target(clouds["tgt"])
    assert a.target_share_count == 1
    b.share_target(a)
    assert a.target_share_count == 2
    c.share_target(b)                                          # through a sharer: the same target
    assert [r.target_share_count for r in (a, b, c)] == [3, 3, 3]
    b.share_target(a)                                          # again: nothing changes
    assert a.target_share_count == 3
    before = fresh_align_bits(pcm, b, scan)
    assert fresh_align_bits(pcm, c, scan) == before
    destroy(a)                                                 # the first owner goes
    assert [r.target_share_count for r in (b, c)] == [2, 2]
    assert fresh_align_bits(pcm, b, scan) == before and fresh_align_bits(pcm, c, scan) == before
    # another cloud on one sharer: that sharer only
    c.set_input_target(clouds["other"])
    assert b.target_share_count == 1 and c.target_share_count == 1
    ref = make(pcm, key)
    ref.set_input_target(clouds["other"])
    on_other = fresh_align_bits(pcm, c, scan)
    assert on_other == fresh_align_bits(pcm, ref, scan) and on_other != before
    assert fresh_align_bits(pcm, b, scan) == before
    # clear on a sharer detaches it; clear on the last holder leaves no target
    c.share_target(b)
    assert b.target_share_count == 2
    c.clear_target()
    assert b.target_share_count == 1 and c.target_share_count == 1
    assert fresh_align_bits(pcm, b, scan) == before
    b.clear_target()
    for reg in (b, c):
        with pytest.raises(pcm.PcmError) as e:
            reg.align(np.eye(4, dtype=F))
        assert e.value.code == NO_INPUT and "setInputTarget" in str(e.value)
    destroy(b, c, ref)


# ---- 5. refused calls -----------------------------------------------------------------------------------------------------------------
def test_mutations_of_a_shared_target_are_refused(pcm, clouds):
    L = pcm.load_library()
    scan = clouds["scans"][0]
    extra = np.ascontiguousarray(clouds["other"][:500])
    a, b = make(pcm, "p2plane"), make(pcm, "p2plane")
    a.set_input_target(clouds["tgt"])
    b.share_target(a)
    before = (fresh_align_bits(pcm, a, scan), fresh_align_bits(pcm, b, scan))
    ident = ((0, 0, 0, 1.0), (0, 0, 0), (0, 0, 0, 1.0), (0, 0, 0))
    lio_state = pcm.capi.PcmLioState()
    lio_state.rot[3] = lio_state.off_R[3] = 1.0
    calls = {
        "pcm_target_insert": lambda r: r.target_insert(extra),
        "pcm_map_incremental": lambda r: r.map_incremental(*ident, 0.5),
        "pcm_lio_frame_end": lambda r: r._check(L.pcm_lio_frame_end(r.handle, C.byref(lio_state), C.c_float(0.5), 1, None)),
        "pcm_swap_source_and_target": lambda r: r.swap_source_and_target(),
        "pcm_set_config": lambda r: r.set_resolution(1.0),
    }
    for name, call in calls.items():
        for reg in (a, b):
            with pytest.raises(pcm.PcmError) as e:
                call(reg)
            assert e.value.code == UNSUPPORTED, name
            assert error_of(L, reg.handle) and "shared" in error_of(L, reg.handle), name
            assert reg.target_share_count == 2
    assert a.config.voxel_resolution == 0.5 and b.config.voxel_resolution == 0.5
    for reg in (a, b):                                         # solver settings stay free
        reg.set_max_iterations(7); reg.set_max_iterations(6)
    assert (fresh_align_bits(pcm, a, scan), fresh_align_bits(pcm, b, scan)) == before
    # pcm_set_covariances(target) is an entry point of the GICP family
    ga, gb = make(pcm, "gicp"), make(pcm, "gicp")
    ga.set_input_target(clouds["tgt"])
    gb.share_target(ga)
    gbefore = (fresh_align_bits(pcm, ga, scan), fresh_align_bits(pcm, gb, scan))
    covs = np.tile(np.eye(3), (N_TGT, 1, 1))
    for reg in (ga, gb):
        with pytest.raises(pcm.PcmError) as e:
            reg.set_covariances(covs, target=True)
        assert e.value.code == UNSUPPORTED and "shared" in error_of(L, reg.handle)
    gb.set_covariances(np.tile(np.eye(3), (N_SCAN, 1, 1)), target=False)   # the source side is the context's own
    gb.set_input_source(scan)                                   # ... and is dropped with the scan
    assert (fresh_align_bits(pcm, ga, scan), fresh_align_bits(pcm, gb, scan)) == gbefore
    # the other holder detaches: the same insert goes through
    b.clear_target()
    assert a.target_share_count == 1
    a.target_insert(extra)
    assert len(a.get_target()) == N_TGT + 500
    whole = make(pcm, "p2plane")
    whole.set_input_target(np.concatenate([clouds["tgt"], extra]))
    assert fresh_align_bits(pcm, a, scan) == fresh_align_bits(pcm, whole, scan)
    destroy(a, b, ga, gb, whole)


# ---- 6. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors(pcm, clouds):
    L = pcm.load_library()
    a = make(pcm, "p2plane")
    a.set_input_target(clouds["tgt"])

    def refused(dst, src, code, *words):
        rc = L.pcm_share_target(dst.handle, src.handle)
        msg = error_of(L, dst.handle)
        assert rc == code and msg and all(w in msg for w in words), (rc, msg)
        assert all(L.pcm_target_share_count(r.handle) == 1 for r in (dst, src))

    coarse = make(pcm, "p2plane", voxel_resolution=1.0)
    refused(coarse, a, INVALID, "voxel_resolution")
    nn7 = make(pcm, "p2plane", num_neighbors=7)
    refused(nn7, a, INVALID, "num_neighbors")
    lists = make(pcm, "p2plane_lists")
    refused(lists, a, INVALID, "flags")
    gicp = make(pcm, "gicp")
    refused(gicp, a, INVALID, "model")
    g10 = make(pcm, "gicp", k_correspondences=10)
    gicp.set_input_target(clouds["tgt"])
    refused(g10, gicp, INVALID, "k_correspondences")
    empty = make(pcm, "p2plane")
    refused(a, empty, INVALID, "no target")
    refused(a, a, INVALID, "itself")
    loam = pcm.LoamRegistration(0)
    refused(loam, a, UNSUPPORTED, "LOAM")
    refused(a, loam, UNSUPPORTED, "LOAM")
    with pytest.raises(pcm.PcmError) as e:
        coarse.share_target(a)
    assert e.value.code == INVALID and "voxel_resolution" in str(e.value)
    # nothing above touched the target
    other = make(pcm, "p2plane")
    other.set_input_target(clouds["tgt"])
    scan = clouds["scans"][1]
    assert fresh_align_bits(pcm, a, scan) == fresh_align_bits(pcm, other, scan)
    destroy(a, coarse, nn7, lists, gicp, g10, empty, loam, other)


# ---- 7. memory --------------------------------------------------------------------------------------------------------------------------
def test_a_sharer_takes_no_memory_for_the_target(pcm, synth):
    """A condition of the layout, not a measured ratio: an owning context holds at least its copy of the target's points,
    16 B x 524 288 = 8 MiB (well above the allocation granularity), which a sharing one does not; the voxel map and the lists
    come on top.  G_own / G_share: growth of the used device memory from adding one context of each kind, after one align."""
    import torch
    n = 524288
    tgt = synth.sample_submap(synth.scene_for_points(55, n, 8.0), n, 56)
    scan = np.ascontiguousarray(tgt[::256][:N_SCAN] + SHIFT)

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    def add(share_from):
        r = make(pcm, "p2plane_lists")
        if share_from is None:
            r.set_input_target(tgt)
        else:
            r.share_target(share_from)
        fresh_align_bits(pcm, r, scan)
        return r

    first = add(None)          # what a process pays once (runtime, code objects, pools) is paid here
    u0 = used()
    owner = add(None)
    u1 = used()
    sharer = add(first)
    u2 = used()
    g_own, g_share = u1 - u0, u2 - u1
    print("G_own = %d B, G_share = %d B" % (g_own, g_share))
    assert first.target_share_count == 2 and owner.target_share_count == 1
    assert g_share <= g_own - 16 * n, (g_own, g_share)
    destroy(first, owner, sharer)
