"""CPU checks of the LOAM scan-to-map arithmetic (pointcloud-slam_amd/csrc/loam_step.h, compiled with g++ through
tests/loam_step_hooks.cpp) against the numpy restatement (tests/loam_ref.py), of the restatement itself against numpy.linalg and
the synthetic ground truth, and of the pcm_loam_* struct layouts against the ctypes binding.  No GPU."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loam_ref as R  # noqa: E402

F = np.float32


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("loam_hooks") / "loam_step_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "pointcloud-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "loam_step_hooks.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    for f in (L.loam_hook_sym_eigen6, L.loam_hook_sym_eigen3):
        f.argtypes = [C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
    L.loam_hook_solve6.argtypes = [C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
    L.loam_hook_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.loam_hook_coeff.argtypes = [C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.loam_hook_jacobian.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
    L.loam_hook_step.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                 C.c_double, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
    return L


def _spd(rng, n, rank=6, scale=1e4):
    Q, _ = np.linalg.qr(rng.normal(size=(n, 6, 6)))
    ev = rng.uniform(1.0, scale, (n, 6))
    ev[:, rank:] = 0.0
    return np.einsum("nij,nj,nkj->nik", Q, ev, Q)


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                                                  b.view(np.uint64 if b.dtype == np.float64 else np.uint32))


@pytest.mark.parametrize("rank", [6, 5, 3])
def test_eigen_and_solve_match_restatement_and_numpy(H, rank):
    rng = np.random.default_rng(rank)
    n = 300
    A = np.ascontiguousarray(_spd(rng, n, rank))
    b = np.ascontiguousarray(rng.normal(size=(n, 6)) * 100)
    w = np.zeros((n, 6)); E = np.zeros((n, 6, 6)); x = np.zeros((n, 6))
    H.loam_hook_sym_eigen6(n, _p(A), _p(w), _p(E))
    H.loam_hook_solve6(n, _p(A), _p(b), _p(x))
    wr, Er = R.sym_eigen(A)
    assert _bits_equal(w, wr) and _bits_equal(E, Er)
    for i in range(0, n, 7):
        assert _bits_equal(x[i], np.array(R.solve6_qr(A[i], b[i])))
    # the restatement is an eigen-decomposition: descending eigenvalues of numpy, orthonormal rows, A E^T = E^T diag(w)
    ref = np.sort(np.linalg.eigvalsh(A), axis=1)[:, ::-1]
    tol = 1e-9 * np.abs(ref).max(axis=1, keepdims=True)
    assert np.all(np.abs(w - ref) <= tol)
    assert np.allclose(np.einsum("nij,nkj->nik", E, E), np.eye(6), atol=1e-12)
    assert np.allclose(np.einsum("nij,nkj->nik", A, E), np.einsum("nkj,nk->njk", E, w), atol=1e-7 * np.abs(ref).max())
    if rank == 6:
        assert np.allclose(x, np.linalg.solve(A, b[..., None])[..., 0], rtol=1e-8, atol=1e-10)


def _run_step(H, x6, sums, it=0, degenerate=0, P=None, iter_num=30, rot=0.01, trans=0.05, thr=100.0):
    x = np.array(x6, F)
    itc, dg = C.c_int(it), C.c_int(degenerate)
    Pm = np.zeros(36) if P is None else np.array(P, np.float64).reshape(36)
    eig = np.zeros(6); fit = np.zeros(2)
    conv, done = C.c_int(0), C.c_int(0)
    H.loam_hook_step(_p(x), C.byref(itc), C.byref(dg), _p(Pm), _p(np.ascontiguousarray(sums, np.float64)), iter_num, rot, trans, thr, _p(eig),
                     C.byref(conv), C.byref(done), _p(fit))
    return dict(x=x, iter=itc.value, degenerate=bool(dg.value), P=Pm.reshape(6, 6), eig=eig, converged=bool(conv.value), done=bool(done.value), fit=fit)


def _sums_for(AtA, AtB, n_rows=200, fit=(12.0, 40, 30.0, 150)):
    s = np.zeros(33)
    t = 0
    for i in range(6):
        for j in range(i, 6):
            s[t] = AtA[i, j]
            t += 1
    s[21:27] = AtB
    s[27], s[28] = n_rows // 4, n_rows - n_rows // 4
    s[29:33] = fit
    return s


@pytest.mark.parametrize("rank", [6, 4])
def test_step_matches_restatement(H, rank):
    """Full LM step of iteration 0 (eigen-decomposition, degeneracy projector) and of a later iteration, device header vs restatement."""
    rng = np.random.default_rng(10 + rank)
    for case in range(40):
        A = _spd(rng, 1, rank, scale=1e5)[0]
        A += np.diag(rng.uniform(0.0, 50.0, 6)) if rank < 6 else 0.0   # small eigenvalues below the threshold of 100
        b = rng.normal(size=6) * 10
        sums = _sums_for(A, b)
        x0 = rng.normal(size=6).astype(F) * F(0.3)
        got = _run_step(H, x0, sums)
        s = R.State(x=x0.copy(), eig=np.zeros(6), P=np.zeros((6, 6)))
        R.step(s, sums, R.Params())
        assert _bits_equal(got["x"], s.x) and got["degenerate"] == s.degenerate and got["converged"] == s.converged
        assert _bits_equal(got["eig"], s.eig) and _bits_equal(got["P"], s.P)
        # the projector is that of the eigenvectors kept, whatever their signs
        w, V = np.linalg.eigh(A)
        order = np.argsort(w)[::-1]
        V = V[:, order]
        n_small = 0
        for i in range(5, -1, -1):
            if s.eig[i] < 100.0:
                n_small += 1
            else:
                break
        Pn = V[:, :6 - n_small] @ V[:, :6 - n_small].T
        assert np.allclose(s.P, Pn, atol=1e-6)
        assert s.degenerate == (n_small > 0)
        # a later iteration re-uses P and never re-decomposes
        got2 = _run_step(H, got["x"], sums, it=1, degenerate=int(got["degenerate"]), P=got["P"])
        s.done = False
        R.step(s, sums, R.Params())
        assert _bits_equal(got2["x"], s.x) and got2["iter"] == s.iter == 2
    assert got["fit"][0] == 12.0 / 40 and got["fit"][1] == 30.0 / 150


def test_step_rules_at_their_edges(H):
    """< 50 rows: no update; fitness with <= 1 point: DBL_MAX; both convergence thresholds just inside / outside."""
    A = np.eye(6) * 1e6
    s = _sums_for(A, np.ones(6), n_rows=49, fit=(0.5, 1, 0.0, 0))
    got = _run_step(H, np.zeros(6, F), s)
    assert np.all(got["x"] == 0) and got["iter"] == 1 and not got["converged"] and not got["done"]
    assert got["fit"][0] == R.DBL_MAX and got["fit"][1] == R.DBL_MAX
    last = _run_step(H, np.zeros(6, F), s, it=29)
    assert last["done"] and last["iter"] == 30 and not last["converged"]
    for rot_thr in (0.01, 0.05):
        for factor, want in ((0.999, True), (1.001, False)):
            d = math.radians(rot_thr * factor)
            b = np.array([d, 0, 0, 0.0004, 0, 0]) * 1e6
            got = _run_step(H, np.zeros(6, F), _sums_for(A, b), rot=rot_thr)
            st = R.State(x=np.zeros(6, F), eig=np.zeros(6), P=np.zeros((6, 6)))
            R.step(st, _sums_for(A, b), R.Params(rot_conv_deg=rot_thr))
            assert got["converged"] == st.converged == want, (rot_thr, factor)
    for factor, want in ((0.999, True), (1.001, False)):
        b = np.array([0, 0, 0, 0, 0.0005 * factor, 0]) * 1e6
        got = _run_step(H, np.zeros(6, F), _sums_for(A, b))
        assert got["converged"] == want


def test_pose_and_per_point_arithmetic_match_restatement(H):
    rng = np.random.default_rng(5)
    for _ in range(20):
        x6 = (rng.normal(size=6) * [0.3, 0.3, 2.0, 20, 20, 2]).astype(F)
        T = np.zeros(12, F); trig = np.zeros(6, F)
        H.loam_hook_pose(_p(x6), _p(T), _p(trig))
        Tr, tr = R.pose_matrix(x6)
        assert _bits_equal(T, Tr.reshape(12)) and _bits_equal(trig, tr)
        ref = R.__dict__["pose_matrix"](x6)[0].astype(np.float64)
        import importlib
        synth_loam = importlib.import_module("pointcloud-slam_amd.synth_loam")
        assert np.allclose(ref, synth_loam.pose_matrix(x6)[:3], atol=1e-5)
    n = 4000
    # edge-like (points along a line), plane-like and random neighbourhoods, query points around them
    centre = rng.uniform(-50, 50, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = rng.uniform(-0.5, 0.5, (n, 5))
    line = centre[:, None, :] + t[..., None] * d[:, None, :] + rng.normal(0, 0.02, (n, 5, 3))
    u = np.cross(d, rng.normal(size=(n, 3))); u /= np.linalg.norm(u, axis=1, keepdims=True)
    plane = line + rng.uniform(-0.4, 0.4, (n, 5))[..., None] * u[:, None, :]
    rand = centre[:, None, :] + rng.normal(0, 0.3, (n, 5, 3))
    q = (centre + rng.normal(0, 0.3, (n, 3))).astype(F)
    for kind, nb in ((0, line), (0, rand), (1, plane), (1, rand)):
        nb = np.ascontiguousarray(nb, F)
        out = np.zeros((n, 4), F); sel = np.zeros(n, np.int32)
        H.loam_hook_coeff(kind, n, _p(nb), _p(q), _p(out), _p(sel))
        co, s = (R.edge_coeff if kind == 0 else R.plane_coeff)(nb, q)
        assert np.array_equal(sel.astype(bool), s)
        assert _bits_equal(out[s], co[s])
        assert s.any()
    body = rng.uniform(-30, 30, (n, 3)).astype(F)
    co = rng.normal(size=(n, 4)).astype(F)
    rows = np.zeros((n, 7), F)
    H.loam_hook_jacobian(_p(trig), n, _p(body), _p(co), _p(rows))
    assert _bits_equal(rows, R.jacobian_rows(trig, body, co))


def test_edge_eigen_matches_numpy():
    rng = np.random.default_rng(3)
    M = rng.normal(size=(500, 3, 3)); M = M @ np.transpose(M, (0, 2, 1))
    w, E = R.sym_eigen(M)
    assert np.allclose(w, np.sort(np.linalg.eigvalsh(M), axis=1)[:, ::-1], rtol=1e-10, atol=1e-12)
    assert np.allclose(np.einsum("nij,nkj->nki", M, E), E * w[..., None], atol=1e-9)


def test_restatement_recovers_ground_truth():
    """The yardstick works: from a 0.3 m / 3 deg perturbation the restatement lands on the pose the scan was taken at."""
    import importlib
    synth_loam = importlib.import_module("pointcloud-slam_amd.synth_loam")
    fr = synth_loam.make_frame(1, n_corner_map=8000, n_surf_map=40000, n_corner=600, n_surf=2500)
    prob = R.Problem(fr.corner_map, fr.surf_map, fr.corner, fr.surf)
    st = R.scan2map(prob, fr.x_guess)
    assert st.iter >= 2 and not st.degenerate
    assert np.abs(st.x[3:] - fr.x_gt[3:]).max() < 0.03, (st.x, fr.x_gt)
    assert np.abs(st.x[:3] - fr.x_gt[:3]).max() < math.radians(0.3), (st.x, fr.x_gt)
    assert st.n_corner > 50 and st.n_surf > 500 and st.fit[0] < 0.05 and st.fit[1] < 0.05


def test_corridor_is_degenerate_in_the_restatement():
    import importlib
    synth_loam = importlib.import_module("pointcloud-slam_amd.synth_loam")
    fr = synth_loam.make_corridor(2)
    st = R.scan2map(R.Problem(fr.corner_map, fr.surf_map, fr.corner, fr.surf), fr.x_guess)
    assert st.degenerate and st.eig[-1] < 100.0 <= st.eig[0]


def test_loam_struct_layouts_match_binding(tmp_path):
    import pointcloud_slam_amd as pcm
    capi = pcm.capi
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "pcm_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(pcm_loam_params), sizeof(pcm_loam_result), offsetof(pcm_loam_params, rot_conv_deg),
         offsetof(pcm_loam_params, search_cell), offsetof(pcm_loam_result, eigenvalues), offsetof(pcm_loam_result, corner_fitness),
         offsetof(pcm_loam_result, maps_built), offsetof(pcm_loam_result, num_corner), (int)PCM_MODEL_LOAM, (int)PCM_ERR_TOO_FEW_FEATURES);
  return 0;
}
''')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(capi.PcmLoamParams), C.sizeof(capi.PcmLoamResult), capi.PcmLoamParams.rot_conv_deg.offset, capi.PcmLoamParams.search_cell.offset,
            capi.PcmLoamResult.eigenvalues.offset, capi.PcmLoamResult.corner_fitness.offset, capi.PcmLoamResult.maps_built.offset,
            capi.PcmLoamResult.num_corner.offset, capi.MODEL["LOAM"], capi.PCM_ERR_TOO_FEW_FEATURES]
    assert got == want


def test_loam_parameters_default_to_the_reference():
    import pointcloud_slam_amd as pcm
    L = pcm.load_library()
    p = pcm.capi.PcmLoamParams()
    L.pcm_loam_default_params(C.byref(p))
    assert (p.iter_num, p.edge_min_valid, p.surf_min_valid) == (30, 10, 100)
    assert (p.rot_conv_deg, p.trans_conv_cm, p.degeneracy_threshold, p.search_cell) == (0.01, 0.05, 100.0, 1.0)
