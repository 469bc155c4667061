"""pcm_loam_tile_share / pcm_loam_tile_share_count / pcm_loam_dynmap_crop_batch without a GPU: the symbols are exported, declared and
bound and the ABI version stays; a context without a device answers with the library's readable error; the layout arithmetic of a
batched crop (csrc/loam_dynmap.h through tests/loam_dynmap_batch_hooks.cpp, g++) maps every workgroup back to its context and keeps
the count slices aligned and disjoint; and the holder rules -- share, detach by clear, last release, refused mutation -- run their
sequences in a stand-alone program built with -fsanitize=address,undefined (tests/tile_share_check.cpp; nothing sanitized is loaded
into Python)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloud-slam_amd", "csrc")
NEW = ("pcm_loam_tile_share", "pcm_loam_tile_share_count", "pcm_loam_dynmap_crop_batch")


def test_symbols_are_exported_declared_and_bound(pcm):
    pcm.build_library()
    L = pcm.load_library()
    version_script = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    dynsyms = subprocess.check_output(["nm", "-D", "--defined-only", pcm.capi.library_path()]).decode()
    hdr = open(os.path.join(ROOT, "include", "pcm_amd.h")).read()
    for name in NEW:
        assert re.search(r"\b%s;" % name, version_script), name + " is not in exports.map"
        assert name in pcm.capi.SYMBOLS
        assert (" T " + name + "\n") in dynsyms, name
        assert ("int " + name + "(") in hdr
        assert getattr(L, name).argtypes is not None   # a prototype, not ctypes' default
    vp = C.c_void_p
    assert L.pcm_loam_tile_share.argtypes == [vp, vp] and L.pcm_loam_tile_share_count.argtypes == [vp]
    assert L.pcm_loam_dynmap_crop_batch.argtypes == [C.POINTER(vp), C.c_int32, C.POINTER(pcm.capi.PcmLoamDynmapParams), vp,
                                                     C.POINTER(pcm.capi.PcmLoamDynmapCropResult)]
    assert "#define PCM_ABI_VERSION 3\n" in hdr and pcm.capi.PCM_ABI_VERSION == 3
    assert L.pcm_abi_version() == 3                    # added entry points: the ABI version stays


def test_python_surface(pcm):
    """The fleet calls are functions of the ``loam`` module, beside ``loam_align_batch``."""
    import inspect
    from pointcloud_slam_amd import loam
    assert list(inspect.signature(loam.loam_share_tiles).parameters) == ["reg", "other"]
    assert list(inspect.signature(loam.loam_tile_share_count).parameters) == ["reg"]
    assert list(inspect.signature(loam.loam_crop_map_batch).parameters) == ["regs", "poses6", "params"]


def test_no_device_fails_with_the_readable_error(pcm):
    """A context of a device that does not exist is kept so that the caller can read why; the three calls refuse it."""
    L = pcm.load_library()
    cfg = pcm.capi.PcmConfig()
    L.pcm_default_config(C.byref(cfg))
    cfg.model = pcm.capi.MODEL["LOAM"]
    a, b = L.pcm_create(9999, C.byref(cfg)), L.pcm_create(9999, C.byref(cfg))
    assert a and b
    try:
        arr = (C.c_void_p * 2)(a, b)
        poses = np.zeros((2, 6), np.float32)
        out = (pcm.capi.PcmLoamDynmapCropResult * 2)()
        for rc in (L.pcm_loam_tile_share(a, b), L.pcm_loam_tile_share(b, a), L.pcm_loam_tile_share_count(a),
                   L.pcm_loam_dynmap_crop_batch(arr, 2, None, poses.ctypes.data, out)):
            assert rc == -3                            # PCM_ERR_HIP, as pcm_loam_dynmap_crop and the rest answer on such a context
        assert L.pcm_loam_tile_share(None, a) == -1 and L.pcm_loam_tile_share_count(None) == -1
        assert L.pcm_loam_dynmap_crop_batch(None, 2, None, poses.ctypes.data, out) == -1
        assert L.pcm_loam_dynmap_crop_batch(arr, 0, None, poses.ctypes.data, out) == -1
        assert L.pcm_loam_dynmap_crop_batch(arr, 2, None, None, out) == -1
        assert L.pcm_loam_dynmap_crop_batch(arr, 2, None, poses.ctypes.data, None) == -1
        assert b"no CPU fallback" in L.pcm_last_error(a) and b"no CPU fallback" in L.pcm_last_error(b)
    finally:
        L.pcm_destroy(a)
        L.pcm_destroy(b)


# ---- the layout of a batched crop ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dynmap_batch_hooks") / "loam_dynmap_batch_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC,
                    os.path.join(ROOT, "tests", "loam_dynmap_batch_hooks.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.dynmap_batch_hook_layout.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.dynmap_batch_hook_context_of.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.dynmap_batch_hook_context_of.restype = C.c_uint32
    return L


def layout(H, nb):
    nb = np.ascontiguousarray(nb, np.uint32)
    sl = np.zeros((len(nb), 4), np.uint32)
    tot = np.zeros(3, np.uint32)
    ok = H.dynmap_batch_hook_layout(nb.ctypes.data, len(nb), sl.ctypes.data, tot.ctypes.data)
    return bool(ok), sl, tot


NB_LISTS = [[0], [1], [255, 256, 257], [0, 3, 0, 700], [3, 0], [0, 0, 5, 0, 0], [256] * 5, [1] * 33, [65536, 1, 65537]]


@pytest.mark.parametrize("nb", NB_LISTS, ids=lambda v: "-".join(map(str, v)))
def test_batch_layout_maps_every_block_back(H, nb):
    chunk = H.dynmap_batch_hook_chunk()
    assert chunk == 256 and H.dynmap_batch_hook_block() == 256
    ok, sl, tot = layout(H, nb)
    assert ok
    n = len(nb)
    block0, slot0, chunk0, nchunks = (sl[:, k].astype(np.int64) for k in range(4))
    # the grid is the contexts' workgroups one after the other
    assert list(block0) == list(np.concatenate([[0], np.cumsum(nb)[:-1]])) and tot[0] == sum(nb)
    # slices: whole scan blocks, aligned, in order, disjoint; a context without workgroups owns nothing
    assert list(nchunks) == [-(-v // chunk) for v in nb]
    assert (slot0 == chunk0 * chunk).all() and (slot0 % chunk == 0).all()
    assert list(chunk0) == list(np.concatenate([[0], np.cumsum(nchunks)[:-1]]))
    assert tot[2] == nchunks.sum() and tot[1] == tot[2] * chunk
    owner = -np.ones(int(tot[1]), np.int64)
    for i in range(n):
        assert (owner[slot0[i]:slot0[i] + nchunks[i] * chunk] == -1).all()
        owner[slot0[i]:slot0[i] + nchunks[i] * chunk] = i
        assert nb[i] <= nchunks[i] * chunk < nb[i] + chunk
    assert (owner >= 0).all()
    assert all(nchunks[i] == 0 for i in range(n) if nb[i] == 0)
    # every workgroup finds its context and its local index
    want = np.repeat(np.arange(n), nb)
    b0 = np.ascontiguousarray(sl[:, 0])
    blocks = range(int(tot[0])) if tot[0] <= 2000 else sorted({0, 1, 65535, 65536, 65537, int(tot[0]) - 1} | set(range(0, int(tot[0]), 997)))
    for b in blocks:
        i = H.dynmap_batch_hook_context_of(b0.ctypes.data, n, b)
        assert i == want[b], (b, i)
        assert 0 <= b - block0[i] < nb[i]


def test_batch_layout_limits(H):
    ok, _, tot = layout(H, [0x7fffffff])
    assert not ok                                         # the padded count array would pass 2^31 - 1 slots
    ok, _, tot = layout(H, [0x7fffff00])
    assert ok and tot[0] == 0x7fffff00 and tot[1] == 0x7fffff00
    assert not layout(H, [0x40000000, 0x40000000])[0]    # the grid itself
    assert not layout(H, [0x7fffff00, 1])[0]


def test_holder_sequences_under_the_sanitizers(tmp_path):
    """share then destroy the owner first / the sharer first, detach by clear, a chain A -> B -> C, a refused mutation, an empty
    store: the counts, the selection reset, and the release hook exactly once per store (tests/tile_share_check.cpp)."""
    exe = str(tmp_path / "tile_share_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "tile_share_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"tile_share_check ok" in out.stdout, out.stdout.decode()
