"""An independent double-precision statement of the GICP and VGICP models, in numpy / scipy only.

Written from the mathematics of fast_gicp's impl/fast_gicp_impl.hpp, impl/fast_vgicp_impl.hpp and fast_vgicp_voxel.hpp (and pclomp's
gicp_omp_impl.hpp for PCM_REG_PCLOMP), not from the project's CPU oracle or its kernels: nothing here imports `oracle`, and every
decomposition is numpy.linalg (eigh, inv, norm).  Everything runs in float64 on the float32 inputs widened exactly.

  cloud in itself      exact k nearest neighbours (the point itself is one of them), cKDTree checked against brute force
  covariance           the k neighbours centred on their mean, cov = X X^T / k, then one of
                         NONE                cov
                         FROBENIUS           C = cov + 1e-3 I,  ((C^-1) / |C^-1|_F)^-1
                         PLANE               U diag(1, 1, 1e-3) V^T,        singular values largest first
                         MIN_EIG             U diag(max(s, 1e-3)) V^T
                         NORMALIZED_MIN_EIG  U diag(max(s / s_max, 1e-3)) V^T
                         PCLOMP              raw second moments (float products, added nearest first), cov = S / k - m m^T,
                                             then sum_k v_k u_k u_k^T with v = (1, 1, 1e-3)
                       cov is symmetric positive semi-definite, so U = V are its eigenvectors and s its eigenvalues: a spectral function
  GICP at a pose T     for every scan point p: the nearest target point B of T_f p (the pose rounded to float, as the search sees it), kept
                       when d^2 < max_corr_dist^2;  M = (C_B + R C_A R^T)^-1,  e = p_B - T p,  J = [skew(T p), -I];
                       H = sum J^T M J,  b = sum J^T M e,  cost = sum e^T M e
  VGICP voxel map      cell = floor(x / res - 0.5);  modes 0, 1: mean of the points and of the covariances;  mode 2: sum C_i^-1 and
                       sum C_i^-1 x_i, then cov = (sum C_i^-1)^-1 and mean = cov sum C_i^-1 x_i;  n points per voxel
  VGICP at a pose T    one correspondence per occupied cell among cell(T p) + offsets (1, 7 or 27 of them), weight sqrt(n), B = the voxel
  compute_error(T2)    the cost of the remembered correspondences and M at another pose

The precondition functions report the points at which a comparison with a float32 search would be ambiguous; build_fixture() removes
them from a synth pair before either side sees it.
"""
from __future__ import annotations

import types

import numpy as np
from scipy.spatial import cKDTree

FLT_MAX = float(np.finfo(np.float32).max)
REGULARIZATIONS = ("NONE", "FROBENIUS", "PLANE", "MIN_EIG", "NORMALIZED_MIN_EIG", "PCLOMP")
MUTATIONS = ("weight_n", "floor_no_half", "direct7_swap", "div_k_minus_1", "plane_largest", "neg_skew", "mode2_no_inverse", "frobenius_no_norm")
EPS32 = 2.0 ** -24

# neighbour cells of fast_vgicp_voxel.hpp: the cell itself; + the six face neighbours (+x, -x, +y, -y, +z, -z); the 3 x 3 x 3 block, x slowest
OFFSETS = {
    1: np.array([[0, 0, 0]], np.int64),
    7: np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.int64),
    27: np.array([[i - 1, j - 1, k - 1] for i in range(3) for j in range(3) for k in range(3)], np.int64),
}


def widen(cloud) -> np.ndarray:
    """(N, 3) float64 of an (N, >= 3) float32 cloud, exactly."""
    a = np.asarray(cloud)
    assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] >= 3
    return a[:, :3].astype(np.float64)


# ---- exact k-NN of a cloud in itself ---------------------------------------------------------------------------------------------
_knn_cache = {}


def _key(x: np.ndarray):
    return (x.shape, hash(np.ascontiguousarray(x).tobytes()))


def knn_self(x: np.ndarray, k: int):
    """(idx (N, k) nearest first, d2 (N, k + 1), gap (N,)): the k nearest points of every point of x in x (itself included), their
    squared distances and the next one's, and the relative gap (d2[k] - d2[k-1]) / d2[k] between the k-th and the (k+1)-th."""
    key = (_key(x), k)
    if key not in _knn_cache:
        assert len(x) > k
        _, idx = cKDTree(x).query(x, k=k + 1)
        d2 = ((x[idx] - x[:, None, :]) ** 2).sum(axis=2)
        order = np.argsort(d2, axis=1, kind="stable")             # the tree sorted by its own distances; sort by ours
        idx, d2 = np.take_along_axis(idx, order, 1), np.take_along_axis(d2, order, 1)
        gap = (d2[:, k] - d2[:, k - 1]) / d2[:, k]
        for a in (idx, d2, gap):
            a.setflags(write=False)
        _knn_cache[key] = (idx[:, :k], d2, gap)
    return _knn_cache[key]


def knn_brute(x: np.ndarray, k: int, rows):
    """The same neighbour sets by brute force, for the rows given: (len(rows), k) indices, nearest first."""
    d2 = ((x[None, :, :] - x[rows][:, None, :]) ** 2).sum(axis=2)
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


# ---- covariances -----------------------------------------------------------------------------------------------------------------
_cov_cache = {}


def raw_covariances(x: np.ndarray, idx: np.ndarray, mutation=None) -> np.ndarray:
    k = idx.shape[1]
    nb = x[idx]
    c = nb - nb.mean(axis=1, keepdims=True)
    return np.einsum("nka,nkb->nab", c, c) / ((k - 1) if mutation == "div_k_minus_1" else k)


def regularize(cov: np.ndarray, method: str, mutation=None) -> np.ndarray:
    """fast_gicp_impl.hpp:264-294 on (N, 3, 3) symmetric positive semi-definite matrices."""
    if method == "NONE":
        return cov.copy()
    if method == "FROBENIUS":
        ci = np.linalg.inv(cov + 1e-3 * np.eye(3))
        if mutation != "frobenius_no_norm":
            ci = ci / np.linalg.norm(ci, axis=(1, 2))[:, None, None]
        return np.linalg.inv(ci)
    w, v = np.linalg.eigh(cov)                 # ascending: singular value j (largest first) is w[:, 2 - j], with U = V = its eigenvector
    if method == "PLANE":
        val = np.broadcast_to([1.0, 1.0, 1e-3] if mutation == "plane_largest" else [1e-3, 1.0, 1.0], w.shape)
    elif method == "MIN_EIG":
        val = np.maximum(w, 1e-3)
    elif method == "NORMALIZED_MIN_EIG":
        val = np.maximum(w / w[:, 2:3], 1e-3)
    else:
        raise KeyError(method)
    return np.einsum("nak,nk,nbk->nab", v, val, v)


def pclomp_covariances(x32: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """gicp_omp_impl.hpp:48-122: the products pt.x * pt.y are float, the sums double and run over the neighbours nearest first."""
    k = idx.shape[1]
    n = len(idx)
    mean = np.zeros((n, 3))
    s = np.zeros((n, 3, 3))
    for j in range(k):
        p = x32[idx[:, j]]
        mean += p.astype(np.float64)
        for a in range(3):
            for b in range(a + 1):
                s[:, a, b] += (p[:, a] * p[:, b]).astype(np.float64)    # float32 product, widened
    mean /= float(k)
    cov = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(a + 1):
            cov[:, a, b] = s[:, a, b] / float(k) - mean[:, a] * mean[:, b]
            cov[:, b, a] = cov[:, a, b]
    _, v = np.linalg.eigh(cov)
    return np.einsum("nak,k,nbk->nab", v, np.array([1e-3, 1.0, 1.0]), v)


def covariances(cloud, k: int = 20, regularization: str = "PLANE", mutation=None) -> np.ndarray:
    """(N, 3, 3) regularised k-NN covariances of an (N, >= 3) float32 cloud, input order; cached per (cloud, k, regularisation)."""
    x32 = np.ascontiguousarray(np.asarray(cloud)[:, :3])
    key = (_key(x32), k, regularization, mutation)
    if key not in _cov_cache:
        x = widen(x32)
        idx, _, _ = knn_self(x, k)
        if regularization == "PCLOMP":
            out = pclomp_covariances(x32, idx)
        else:
            out = regularize(raw_covariances(x, idx, mutation), regularization, mutation)
        out.setflags(write=False)
        _cov_cache[key] = out
    return _cov_cache[key]


def plane_eigen_gap(cloud, k: int = 20) -> np.ndarray:
    """(N,) relative gap (w1 - w0) / w1 between the two smallest eigenvalues of the unregularised covariance."""
    x = widen(cloud)
    w = np.linalg.eigvalsh(raw_covariances(x, knn_self(x, k)[0]))
    return (w[:, 1] - w[:, 0]) / w[:, 1]


# ---- poses -----------------------------------------------------------------------------------------------------------------------
def skew(v: np.ndarray) -> np.ndarray:
    """(..., 3, 3) with skew(v) w = v x w."""
    out = np.zeros(v.shape[:-1] + (3, 3))
    out[..., 0, 1], out[..., 0, 2] = -v[..., 2], v[..., 1]
    out[..., 1, 0], out[..., 1, 2] = v[..., 2], -v[..., 0]
    out[..., 2, 0], out[..., 2, 1] = -v[..., 1], v[..., 0]
    return out


def so3_exp(w) -> np.ndarray:
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    if th < 1e-300:
        return np.eye(3)
    K = skew(w / th)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def left_step(T: np.ndarray, d) -> np.ndarray:
    """delta * T with delta.linear = exp(d[:3]), delta.translation = d[3:]: how lsq_registration_impl.hpp applies a step."""
    D = np.eye(4)
    D[:3, :3] = so3_exp(d[:3])
    D[:3, 3] = d[3:]
    return D @ np.asarray(T, np.float64)


def transform(T: np.ndarray, x: np.ndarray) -> np.ndarray:
    return x @ T[:3, :3].T + T[:3, 3]


def transform_f32(T: np.ndarray, x32: np.ndarray) -> np.ndarray:
    """trans.cast<float>() * p in float32 arithmetic, widened: the point the nearest-neighbour search is given."""
    Tf = np.asarray(T, np.float64).astype(np.float32)
    q = (x32[:, None, :3] * Tf[None, :3, :3]).sum(axis=2, dtype=np.float32) + Tf[:3, 3]
    assert q.dtype == np.float32
    return q.astype(np.float64)


def transform_f32_bound(T: np.ndarray, x: np.ndarray) -> np.ndarray:
    """(N,) bound of the float32 evaluation error of T_f p per coordinate: 4 * 2^-24 * (|R| |p| + |t|), max norm."""
    T = np.asarray(T, np.float64)
    return 4.0 * EPS32 * (np.abs(x) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])).max(axis=1)


# ---- voxel map -------------------------------------------------------------------------------------------------------------------
def voxel_coords(x: np.ndarray, res: float, mutation=None) -> np.ndarray:
    """(N, 3) int64 cell of every point: floor(x / res - 0.5)  (fast_vgicp_voxel.hpp:158-160)."""
    return np.floor(x / res - (0.0 if mutation == "floor_no_half" else 0.5)).astype(np.int64)


def _cell_key(c: np.ndarray) -> np.ndarray:
    b = c + (1 << 20)
    assert (b >= 0).all() and (b < (1 << 21)).all()
    return (b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2]


def voxel_map(x: np.ndarray, covs: np.ndarray, res: float, mode: int, mutation=None):
    """The Gaussian voxel map of a cloud: namespace(keys sorted, coords, mean (V, 3), cov (V, 3, 3), n (V,), of_point (N,))."""
    coords = voxel_coords(x, res, mutation)
    keys, first, inv = np.unique(_cell_key(coords), return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    nv = len(keys)
    n = np.bincount(inv, minlength=nv)
    mean = np.zeros((nv, 3))
    cov = np.zeros((nv, 3, 3))
    if mode in (0, 1):                                   # AdditiveGaussianVoxel :105-122
        np.add.at(mean, inv, x)
        np.add.at(cov, inv, covs)
        mean /= n[:, None]
        cov /= n[:, None, None]
    elif mode == 2:                                      # MultiplicativeGaussianVoxel :79-102
        ci = np.linalg.inv(covs)
        np.add.at(cov, inv, ci)
        np.add.at(mean, inv, np.einsum("nab,nb->na", ci, x))
        if mutation != "mode2_no_inverse":
            cov = np.linalg.inv(cov)
            mean = np.einsum("vab,vb->va", cov, mean)
    else:
        raise KeyError(mode)
    return types.SimpleNamespace(keys=keys, coords=coords[first], mean=mean, cov=cov, n=n, of_point=inv)


# ---- the two models --------------------------------------------------------------------------------------------------------------
class Reference:
    """FastGICP / FastVGICP (CPU semantics) on a scan and a target, in float64."""

    def __init__(self, scan, target, model="GICP", *, k_correspondences=20, regularization="PLANE", max_corr_dist=FLT_MAX,
                 voxel_resolution=1.0, num_neighbors=1, voxel_mode=0, mutation=None):
        assert model in ("GICP", "VGICP") and mutation in (None,) + MUTATIONS
        self.model, self.k, self.reg, self.max_corr_dist = model, int(k_correspondences), regularization, float(max_corr_dist)
        self.res, self.nn, self.mode, self.mutation = float(voxel_resolution), int(num_neighbors), int(voxel_mode), mutation
        self.src32 = np.ascontiguousarray(np.asarray(scan)[:, :3])
        self.tgt32 = np.ascontiguousarray(np.asarray(target)[:, :3])
        self._cov = {}
        self._vox = None
        self.corr = None

    # clouds and covariances
    @property
    def src(self): return widen(self.src32)

    @property
    def tgt(self): return widen(self.tgt32)

    def covariances(self, target=False) -> np.ndarray:
        if target not in self._cov:
            self._cov[target] = covariances(self.tgt32 if target else self.src32, self.k, self.reg, self.mutation)
        return self._cov[target]

    def set_covariances(self, covs, target=False):
        covs = np.asarray(covs, np.float64)
        assert covs.shape == (len(self.tgt32 if target else self.src32), 3, 3)
        self._cov[target] = covs
        if target:
            self._vox = None

    def swap_source_and_target(self):
        self.src32, self.tgt32 = self.tgt32, self.src32
        self._cov = {(not t): c for t, c in self._cov.items()}
        self._vox = None
        self.corr = None

    def voxels(self):
        if self._vox is None:
            self._vox = voxel_map(self.tgt, self.covariances(True), self.res, self.mode, self.mutation)
        return self._vox

    # correspondences
    def _gicp_correspondences(self, T):
        tgt = self.tgt
        qf = transform_f32(T, self.src32)
        d, j = cKDTree(tgt).query(qf, k=2)
        d2 = ((tgt[j] - qf[:, None, :]) ** 2).sum(axis=2)
        swap = d2[:, 1] < d2[:, 0]
        j[swap], d2[swap] = j[swap][:, ::-1], d2[swap][:, ::-1]
        keep = d2[:, 0] < self.max_corr_dist * self.max_corr_dist
        i = np.nonzero(keep)[0]
        self.search = types.SimpleNamespace(d2_first=d2[:, 0], d2_second=d2[:, 1], nearest=j[:, 0], kept=keep)
        return i, tgt[j[i, 0]], self.covariances(True)[j[i, 0]], np.ones(len(i)), j[i, 0]

    def _vgicp_correspondences(self, T):
        vm = self.voxels()
        off = OFFSETS[self.nn]
        if self.mutation == "direct7_swap" and self.nn == 7:
            off = off[[0, 2, 1, 3, 4, 5, 6]]
        cell = voxel_coords(transform(T, self.src), self.res, self.mutation)
        want = _cell_key(cell[:, None, :] + off[None, :, :])                  # (N, nn): point-major, offsets in table order
        pos = np.minimum(np.searchsorted(vm.keys, want), len(vm.keys) - 1)
        hit = vm.keys[pos] == want
        i, o = np.nonzero(hit)
        v = pos[i, o]
        w = vm.n[v].astype(np.float64)
        return i, vm.mean[v], vm.cov[v], (w if self.mutation == "weight_n" else np.sqrt(w)), v

    def linearize(self, T):
        """(cost, H (6, 6), b (6,), count) at the pose T; the correspondences and M are remembered for compute_error."""
        T = np.asarray(T, np.float64)
        i, mean_b, cov_b, w, which = (self._gicp_correspondences if self.model == "GICP" else self._vgicp_correspondences)(T)
        R = T[:3, :3]
        M = np.linalg.inv(cov_b + np.einsum("ab,nbc,dc->nad", R, self.covariances(False)[i], R))
        self.corr = types.SimpleNamespace(src=i, mean_b=mean_b, M=M, w=w, which=which)
        q = transform(T, self.src[i])
        e = mean_b - q
        J = np.concatenate([skew(q) * (-1.0 if self.mutation == "neg_skew" else 1.0), np.broadcast_to(-np.eye(3), (len(i), 3, 3))], axis=2)
        H = np.einsum("n,nar,nab,nbs->rs", w, J, M, J)
        b = np.einsum("n,nar,nab,nb->r", w, J, M, e)
        cost = float(np.einsum("n,na,nab,nb->", w, e, M, e))
        return cost, H, b, len(i)

    def compute_error(self, T2) -> float:
        c = self.corr
        e = c.mean_b - transform(np.asarray(T2, np.float64), self.src[c.src])
        return float(np.einsum("n,na,nab,nb->", c.w, e, c.M, e))


# ---- preconditions ---------------------------------------------------------------------------------------------------------------
GAP_KNN = 1e-5        # (a): float32 distances, a few 2^-24 of relative error, cannot flip an order across this
GAP_PLANE = 1e-4      # (b): PLANE's result has error ~ eps / gap
VOXEL_EDGE = 1e-9     # (e): of a cell


def violations_knn_gap(cloud, k):
    """(a) points whose k-th and (k+1)-th neighbour are closer than GAP_KNN relative."""
    return np.nonzero(knn_self(widen(cloud), k)[2] < GAP_KNN)[0]


def violations_plane_gap(cloud, k):
    """(b) points whose two smallest covariance eigenvalues are closer than GAP_PLANE relative."""
    return np.nonzero(plane_eigen_gap(cloud, k) < GAP_PLANE)[0]


def nearest_margins(queries, target, T, max_corr_dist):
    """For every query p: the two nearest target points of T_f p and the slack 4 delta sqrt(d2) + GAP_KNN d2 the float32 search may be off
    by (delta: transform_f32_bound; the second term covers the float32 evaluation of the distance itself)."""
    x32 = np.ascontiguousarray(np.asarray(queries)[:, :3])
    tgt = widen(target)
    qf = transform_f32(T, x32)
    _, j = cKDTree(tgt).query(qf, k=2)
    d2 = np.sort(((tgt[j] - qf[:, None, :]) ** 2).sum(axis=2), axis=1)
    delta = transform_f32_bound(T, widen(x32))
    thr2 = float(max_corr_dist) ** 2
    return types.SimpleNamespace(d2_first=d2[:, 0], d2_second=d2[:, 1], slack_second=4.0 * delta * np.sqrt(d2[:, 1]) + GAP_KNN * d2[:, 1],
                                 slack_first=4.0 * delta * np.sqrt(d2[:, 0]) + GAP_KNN * d2[:, 0], thr2=thr2)


def violations_nearest(queries, target, T, max_corr_dist):
    """(c) the nearest target is ambiguous, (d) the nearest distance sits on the threshold."""
    m = nearest_margins(queries, target, T, max_corr_dist)
    c = m.d2_second - m.d2_first <= m.slack_second
    d = np.abs(m.d2_first - m.thr2) <= m.slack_first
    return np.nonzero(c | d)[0]


def violations_voxel_edge(x: np.ndarray, res: float):
    """(e) a voxel coordinate x / res - 0.5 within VOXEL_EDGE of an integer; x: (N, 3) float64 positions in the map's frame."""
    u = x / res - 0.5
    return np.nonzero((np.abs(u - np.round(u)) < VOXEL_EDGE).any(axis=1))[0]


def all_violations(scan, submap, poses, *, ks, thresholds, resolutions, swapped_poses=()):
    """(scan rows, map rows) that violate a margin in any of the cases."""
    bad_s, bad_m = set(), set()
    for k in ks:
        bad_s.update(violations_knn_gap(scan, k)); bad_m.update(violations_knn_gap(submap, k))
        bad_s.update(violations_plane_gap(scan, k)); bad_m.update(violations_plane_gap(submap, k))
    for res in resolutions:
        bad_m.update(violations_voxel_edge(widen(submap), res))
        for T in poses:
            bad_s.update(violations_voxel_edge(transform(T, widen(scan)), res))
    for T in poses:
        for thr in thresholds:
            bad_s.update(violations_nearest(scan, submap, T, thr))
    for T in swapped_poses:                            # after swap_source_and_target: map points look for their nearest scan point
        bad_m.update(violations_nearest(submap, scan, T, FLT_MAX))
        for res in resolutions:
            bad_s.update(violations_voxel_edge(widen(scan), res))
            bad_m.update(violations_voxel_edge(transform(T, widen(submap)), res))
    return np.array(sorted(bad_s), np.int64), np.array(sorted(bad_m), np.int64)


# ---- fixture ---------------------------------------------------------------------------------------------------------------------
KS = (5, 20, 33)
THRESHOLDS = (FLT_MAX, float(np.float32(0.3)), 1.0)
VGICP_CASES = ((1.0, 1, 0, "PLANE"), (1.0, 7, 0, "PLANE"), (1.0, 27, 0, "PLANE"), (0.75, 27, 1, "PLANE"), (1.0, 7, 2, "MIN_EIG"), (0.5, 27, 2, "PLANE"))
RESOLUTIONS = (1.0, 0.75, 0.5)
SHIFT = np.array([0.02, -0.01, 0.01])
REMOVED_CAP = 0.01
_fixtures = {}


def build_fixture(synth, centred=False):
    """synth.make_pair(3, 600, 3000) with the points removed that violate a precondition in any case of the two test files (k = 5, 20,
    33; the three thresholds; the three resolutions; the poses guess and T_gt; the swapped roles at guess^-1).  centred: the map and the
    poses moved by the map's centroid, so that voxel coordinates take both signs.  At most three rounds; the result has no violation
    and at most 1 % of either cloud removed, or this raises."""
    if centred not in _fixtures:
        p = synth.make_pair(3, 600, 3000)
        scan, submap = p.scan.copy(), p.submap.copy()
        guess, T_gt = p.guess.astype(np.float64), p.T_gt.copy()
        if centred:
            c = widen(submap).mean(axis=0)
            submap[:, :3] = (widen(submap) - c).astype(np.float32)
            guess[:3, 3] -= c
            T_gt[:3, 3] -= c
        n_scan, n_map = len(scan), len(submap)
        poses = (guess, T_gt)
        swapped = (np.linalg.inv(guess),)
        kw = dict(ks=KS, thresholds=THRESHOLDS, resolutions=RESOLUTIONS, swapped_poses=swapped)
        rounds = []
        for _ in range(3):
            bad_s, bad_m = all_violations(scan, submap, poses, **kw)
            rounds.append((len(bad_s), len(bad_m)))
            if not len(bad_s) and not len(bad_m):
                break
            scan, submap = np.delete(scan, bad_s, axis=0), np.delete(submap, bad_m, axis=0)
        bad_s, bad_m = all_violations(scan, submap, poses, **kw)
        if len(bad_s) or len(bad_m):
            raise AssertionError("violations left after three rounds: %d scan, %d map" % (len(bad_s), len(bad_m)))
        removed = (n_scan - len(scan), n_map - len(submap))
        if removed[0] > REMOVED_CAP * n_scan or removed[1] > REMOVED_CAP * n_map:
            raise AssertionError("more than 1 %% of a cloud removed: %r" % (removed,))
        for a in (scan, submap, guess, T_gt):
            a.setflags(write=False)
        _fixtures[centred] = types.SimpleNamespace(scan=scan, submap=submap, guess=guess, T_gt=T_gt, poses=poses, swapped_pose=swapped[0],
                                                   removed_scan=removed[0], removed_map=removed[1], rounds=rounds, kw=kw)
    return _fixtures[centred]


def margins(fx):
    """The measured margins of a fixture (smallest over all cases), for the record."""
    out = {}
    for name, cloud in (("scan", fx.scan), ("map", fx.submap)):
        for k in KS:
            out["knn_gap_%s_k%d" % (name, k)] = float(knn_self(widen(cloud), k)[2].min())
            out["plane_gap_%s_k%d" % (name, k)] = float(plane_eigen_gap(cloud, k).min())
    first_second, thr = [], {t: [] for t in THRESHOLDS[1:]}
    for T in fx.poses:
        m = nearest_margins(fx.scan, fx.submap, T, FLT_MAX)
        first_second.append(((m.d2_second - m.d2_first) / m.d2_second).min())
        for t in thr:
            thr[t].append((np.abs(m.d2_first - t * t) / (t * t)).min())
    out["nearest_first_second_gap"] = float(min(first_second))
    for t in thr:
        out["threshold_margin_%.1f" % t] = float(min(thr[t]))
    edge = []
    for res in RESOLUTIONS:
        for x in [widen(fx.submap)] + [transform(T, widen(fx.scan)) for T in fx.poses]:
            u = x / res - 0.5
            edge.append(np.abs(u - np.round(u)).min())
    out["voxel_edge"] = float(min(edge))
    return out


# ---- derivative property ---------------------------------------------------------------------------------------------------------
DERIV_H = 1e-4
DERIV_CASES = {
    "gicp": ("GICP", {}),
    "vgicp_1.0_7_0": ("VGICP", dict(voxel_resolution=1.0, num_neighbors=7)),
    "vgicp_0.5_27_2": ("VGICP", dict(voxel_resolution=0.5, num_neighbors=27, voxel_mode=2)),
}
# derivative_discrepancy of this reference on build_fixture(synth) at DERIV_H, per (case, pose): the h^2 truncation term
DERIV_MEASURED = {
    ("gicp", "guess"): 3.14e-07,
    ("gicp", "T_gt"): 1.16e-08,
    ("vgicp_1.0_7_0", "guess"): 8.19e-08,
    ("vgicp_1.0_7_0", "T_gt"): 2.74e-07,
    ("vgicp_0.5_27_2", "guess"): 2.32e-07,
    ("vgicp_0.5_27_2", "T_gt"): 3.58e-08,
}


def derivative_discrepancy(compute_error, T, b, h=DERIV_H) -> float:
    """max_k |central difference of compute_error(exp(+-h e_k) T) - 2 b_k| / max |2 b|, correspondences and M frozen."""
    g = np.array([(compute_error(left_step(T, h * np.eye(6)[k])) - compute_error(left_step(T, -h * np.eye(6)[k]))) / (2.0 * h) for k in range(6)])
    return float(np.abs(g - 2.0 * np.asarray(b)).max() / np.abs(2.0 * np.asarray(b)).max())


def assert_both_signs(fx):
    """The centred fixture: the map's voxel coordinates take both signs on every axis; the scan's cells at the poses (one corner of the
    map) are negative somewhere on every axis and straddle zero on at least one."""
    for res in RESOLUTIONS:
        c = voxel_coords(widen(fx.submap), res)
        assert (c.min(axis=0) < 0).all() and (c.max(axis=0) > 0).all(), (res, c.min(axis=0), c.max(axis=0))
        for T in fx.poses:
            c = voxel_coords(transform(T, widen(fx.scan)), res)
            assert (c.min(axis=0) < 0).all() and ((c.min(axis=0) < 0) & (c.max(axis=0) > 0)).any(), (res, c.min(axis=0), c.max(axis=0))
