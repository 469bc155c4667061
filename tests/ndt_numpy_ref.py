"""An independent statement of the float models -- NDT P2D / D2D and VGICP_CUDA (csrc/ndt.hip, k_gauss_voxels, k_vgc_voxels) and
pclomp NDT (csrc/pclndt.hip) -- in numpy / scipy only.

Written from the mathematics of fast_gicp's src/fast_gicp/cuda/{ndt_compute_derivatives, compute_derivatives, gaussian_voxelmap,
covariance_regularization, find_voxel_correspondences, ndt_cuda}.cu and include/fast_gicp/cuda/vector3_hash.cuh, and of pclomp's
ndt_omp_impl.hpp and voxel_grid_covariance_omp_impl.hpp; not from the project's CPU oracle or its kernels: nothing here imports
`oracle` or the package, and every decomposition is numpy.linalg (eigh, inv).  Small helpers are shared with gicp_numpy_ref.py.

Every model takes a dtype.  float64 is the reference proper: every quantity in double on the float32 inputs widened exactly.  float32
forms every per-correspondence quantity in numpy float32 arrays, in numpy's own operation order, and still sums over the
correspondences in float64; it is never compared with a kernel -- rel_err(Q32, Q64) measures how far float rounding alone moves a
result on these inputs (NOISE_MEASURED), and the tolerance of a comparison is MARGIN times that (tolerance()).

Two things the kernels do in float decide WHICH terms exist, not their value, and are evaluated here as the sources state them, in
both runs: the pose rounded to float32 before the search, and the cell rule on the float transformed point (floor(q / res - 0.5) of
vector3_hash.cuh for the Gaussian voxels, floor(q / leaf) of getNeighborhoodAtPoint for pclomp).  The precondition functions report
the points at which that decision is within rounding of flipping; build_fixture() removes them before either side sees the clouds.

  Gaussian voxels      cell = floor(x / res - 0.5);  mean = sum x / n;  cov = (sum x x^T - mean sum x^T) / n;  MIN_EIG as a spectral
                       function: V max(L, 1e-3) V^T;  n per voxel;  a target voxel takes part only with n > 6
  neighbourhoods       1 / 7 / 27 offsets, or DIRECT_RADIUS r: every offset of the cube with |offset| <= r + 1e-3 (19 at r = 1.5)
  P2D at a pose T      one term per (scan point p, occupied neighbour voxel B):  e = mean_B - T p,  M = C_B^-1,
                       w = res^2 / (res^2 + |e|^2),  J = [skew(T p), -I];  H = sum w J^T M J,  b = sum w J^T M e,  cost = sum w e^T M e
  D2D                  the source elements are the scan's own Gaussian voxels (all of them);  M = (C_B + R C_A R^T)^-1 with R the
                       rotation of the LINEARISATION pose, also in a trial pass
  VGICP_CUDA           the same with w = sqrt(n_B), voxels with n > 0;  voxel = mean of its points and of their covariances; the
                       per-point covariances are data (handed in)
  compute_error(T2)    the cost of the remembered correspondences at another pose; R stays that of the linearisation pose

  pclomp leaves        cell = floor(x * (1 / leaf)) in float;  cov starts as the IDENTITY and takes sum x x^T on top:
                       cov = (I + sum x x^T - 2 sum x mean^T) / n + mean mean^T, times (n - 1) / n;  fewer than 6 points: no
                       covariance;  eigenvalues below 1 % of the largest raised to it through V L V^-1;  icov = cov^-1;  a leaf with
                       a negative eigenvalue or an infinite icov is rejected;  the centroid is the float32 sum in input order / n
  pclomp neighbours    DIRECT1 / 7 / 26 (27 cells) around floor(xt / leaf), leaves with >= 6 points;  KDTREE (0): the leaves with
                       >= 6 points whose float centroid is strictly within one resolution of xt (float squared distance)
  d1, d2, d3           eq. 6.8 from the outlier ratio and the (float) resolution
  pclomp score         xt = the float32 transformed point (pcl::transformPointCloud = m00 x + (m01 y + (m02 z + m03)) in float, the
                       choice DESIGN.md section 5 states, PCL not being in the tree);  per (point, leaf):  d = xt - mean,
                       e = exp(-d2 d^T icov d / 2),  score += -d1 e;  with e' = d2 e admissible when 0 <= e' <= 1:
                       g_i += d1 e' d^T icov dT_i,  H_ij += d1 e' (-d2 (d^T icov dT_i)(d^T icov dT_j) + d^T icov d2T_ij + dT_j^T icov dT_i)
                       dT_i, d2T_ij: derivatives of Rx(roll) Ry(pitch) Rz(yaw) x + t, obtained here by differentiating the three axis
                       rotations (R' = c K + s K^2, R'' = -s K + c K^2), not from the source's 8- and 15-row tables
  calculateScore       sum over points of sum over its m leaves of (-d1 e - d3) / m, over the number of points

The source's FLOAT Hessian table carries (+sy) in the z-coefficient of d^2 T_x / d pitch^2 where its double table (and the derivative)
have (-sy) (ndt_omp_impl.hpp:354 against :332).  The float pass of computeDerivatives therefore is not the Hessian of its score; the
reference states this as PITCH2_SIGN_QUIRK, applied to the float pass only, and the tests show both facts: without it the float
Hessian equals the central difference of the gradient, with it it equals what the source's tables produce.

What no test of sums can see: the order of the DIRECT7 rows (it permutes the terms), and `<=` for `<` in the radius test (the
fixture keeps every centroid KD_MARGIN away from the radius, or the comparison with a float kernel would be ambiguous).
"""
from __future__ import annotations

import types

import numpy as np
from scipy.spatial import cKDTree

from gicp_numpy_ref import EPS32, OFFSETS, _cell_key, left_step, skew, so3_exp, transform, widen

F32, F64 = np.float32, np.float64
MODELS = ("NDT_P2D", "NDT_D2D", "VGICP_CUDA")
MUTATIONS_KNDT = ("floor_no_half", "n_ge_6", "div_n_minus_1", "no_min_eig", "cauchy_width_1", "weight_n", "neg_skew", "d2d_no_source_cov",
                  "trial_rotation")
MUTATIONS_PCL = ("no_identity", "no_n_minus_1", "min_points_7", "inflation_0.001", "floor_minus_half", "d1_d2_swapped", "kdtree_cell_centre",
                 "radius_le", "drop_d2R_roll_roll", "score_not_per_cell")
MUTATIONS = MUTATIONS_KNDT + MUTATIONS_PCL
INVISIBLE = {"radius_le": "differs only where a float squared distance EQUALS the squared radius; the fixture keeps every centroid KD_MARGIN away from it",
             "inflation_0.001": "the identity start keeps every eigenvalue above (n - 1) / n^2, more than 1 % of the largest on leaves of ~100 points or fewer: the inflation never acts on this fixture",
             "direct7_order": "permutes the terms of a sum (not a mutation of this module: see gicp_numpy_ref.direct7_swap)"}


def rel_err(a, b):
    a = np.asarray(a, F64); b = np.asarray(b, F64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def radius_offsets(radius: float) -> np.ndarray:
    """ndt_cuda.cu DIRECT_RADIUS: the offsets of the cube [-ceil(r), ceil(r)]^3 with |offset| <= r + 1e-3."""
    k = int(np.ceil(radius))
    g = np.array([[i, j, l] for i in range(-k, k + 1) for j in range(-k, k + 1) for l in range(-k, k + 1)], np.int64)
    return g[np.sqrt((g * g).sum(axis=1).astype(F64)) <= radius + 1e-3]


def offsets_of(nn):
    return radius_offsets(float(nn[1:])) if isinstance(nn, str) else OFFSETS[nn]


def pose_f32(T) -> np.ndarray:
    return np.asarray(T, F64).astype(F32)


def transform_search(T, x32: np.ndarray) -> np.ndarray:
    """(N, 3) float32: trans.cast<float>() * p in float32 arithmetic -- the point whose cell is looked up."""
    Tf = pose_f32(T)
    q = (x32[:, None, :3] * Tf[None, :3, :3]).sum(axis=2, dtype=F32) + Tf[:3, 3]
    assert q.dtype == F32
    return q


def ndt_cells(q32: np.ndarray, res: float, mutation=None) -> np.ndarray:
    """calc_voxel_coord (vector3_hash.cuh): floor(x / resolution - 0.5) on float32 coordinates, in float32."""
    assert q32.dtype == F32
    u = q32 / F32(res)
    if mutation != "floor_no_half":
        u = u - F32(0.5)
    return np.floor(u).astype(np.int64)


def pcl_cells_of_map(x32: np.ndarray, leaf: float, mutation=None) -> np.ndarray:
    """applyFilter's first pass: floor(x * inverse_leaf_size) in float32."""
    assert x32.dtype == F32
    u = x32 * (F32(1.0) / F32(leaf))
    if mutation == "floor_minus_half":
        u = u - F32(0.5)
    return np.floor(u).astype(np.int64)


def pcl_cells_of_query(xt32: np.ndarray, leaf: float, mutation=None) -> np.ndarray:
    """getNeighborhoodAtPoint: floor(x / leaf_size) on the float32 transformed point."""
    assert xt32.dtype == F32
    u = xt32 / F32(leaf)
    if mutation == "floor_minus_half":
        u = u - F32(0.5)
    return np.floor(u).astype(np.int64)


def _lookup(keys, want):
    pos = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    return pos, keys[pos] == want


# ---- Gaussian voxels -------------------------------------------------------------------------------------------------------------
def gauss_voxels(x32: np.ndarray, res: float, dt=F64, mutation=None):
    """gaussian_voxelmap.cu + covariance_regularization_mineig: namespace(keys sorted, coords, mean, cov, n, of_point); mean and cov in dt.
    The sums over a voxel's points run in float64 in both runs (float32: on float32 products, and the covariance is rounded to float32
    before the float32 eigendecomposition)."""
    x32 = np.ascontiguousarray(x32[:, :3])
    coords = ndt_cells(x32, res, mutation)
    keys, first, inv = np.unique(_cell_key(coords), return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    nv = len(keys)
    n = np.bincount(inv, minlength=nv)
    x = x32.astype(F64)
    outer = np.einsum("na,nb->nab", x32, x32).astype(F64) if dt == F32 else np.einsum("na,nb->nab", x, x)
    sx, sxx = np.zeros((nv, 3)), np.zeros((nv, 3, 3))
    np.add.at(sx, inv, x)
    np.add.at(sxx, inv, outer)
    mean = sx / n[:, None]
    div = np.maximum(n - 1, 1) if mutation == "div_n_minus_1" else n
    cov = ((sxx - np.einsum("va,vb->vab", mean, sx)) / div[:, None, None]).astype(dt)
    if mutation != "no_min_eig":
        cov = 0.5 * (cov + cov.transpose(0, 2, 1))
        w, v = np.linalg.eigh(cov)
        cov = np.einsum("vak,vk,vbk->vab", v, np.maximum(w, dt(1e-3)), v)
    assert cov.dtype == dt
    return types.SimpleNamespace(keys=keys, coords=coords[first], mean=mean.astype(dt), cov=cov, n=n, of_point=inv)


def vgc_voxels(x32: np.ndarray, covs: np.ndarray, res: float, dt=F64):
    """GaussianVoxelMap::create_voxelmap(points, covariances): voxel mean = mean of its points, covariance = mean of theirs."""
    x32 = np.ascontiguousarray(x32[:, :3])
    coords = ndt_cells(x32, res)
    keys, first, inv = np.unique(_cell_key(coords), return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    nv = len(keys)
    n = np.bincount(inv, minlength=nv)
    sx, sc = np.zeros((nv, 3)), np.zeros((nv, 3, 3))
    np.add.at(sx, inv, x32.astype(F64))
    np.add.at(sc, inv, np.asarray(covs, F64))
    return types.SimpleNamespace(keys=keys, coords=coords[first], mean=(sx / n[:, None]).astype(dt), cov=(sc / n[:, None, None]).astype(dt), n=n, of_point=inv)


class NdtReference:
    """NDTCuda (P2D / D2D) and the VGICP_CUDA core on a scan and a target."""

    def __init__(self, scan, target, model, *, voxel_resolution=1.0, num_neighbors=7, dtype=F64, mutation=None):
        assert model in MODELS and mutation in (None,) + MUTATIONS_KNDT and dtype in (F32, F64)
        self.model, self.res, self.nn, self.dt, self.mutation = model, float(voxel_resolution), num_neighbors, dtype, mutation
        self.src32 = np.ascontiguousarray(np.asarray(scan)[:, :3])
        self.tgt32 = np.ascontiguousarray(np.asarray(target)[:, :3])
        assert self.src32.dtype == F32 and self.tgt32.dtype == F32
        self._cov = {}
        self._reset()

    def _reset(self):
        self._tv = self._sv = self.corr = None

    def set_covariances(self, covs, target=False):
        covs = np.asarray(covs, F64)
        assert covs.shape == (len(self.tgt32 if target else self.src32), 3, 3)
        self._cov[bool(target)] = covs
        self._reset()

    def swap_source_and_target(self):
        self.src32, self.tgt32 = self.tgt32, self.src32
        self._cov = {(not t): c for t, c in self._cov.items()}
        self._reset()

    def target_voxels(self):
        if self._tv is None:
            self._tv = (vgc_voxels(self.tgt32, self._cov[True], self.res, self.dt) if self.model == "VGICP_CUDA"
                        else gauss_voxels(self.tgt32, self.res, self.dt, self.mutation))
        return self._tv

    def source_elements(self):
        """(position (N, 3) dt, position float32 for the search, covariance (N, 3, 3) dt or None)."""
        if self.model == "NDT_D2D":
            if self._sv is None:
                self._sv = gauss_voxels(self.src32, self.res, self.dt, self.mutation)
            sv = self._sv
            cov = None if self.mutation == "d2d_no_source_cov" else sv.cov
            return sv.mean, sv.mean.astype(F32), cov
        cov = self._cov[False].astype(self.dt) if self.model == "VGICP_CUDA" else None
        return self.src32.astype(self.dt), self.src32, cov

    def _terms(self, T, R_lin):
        """Per remembered correspondence at the pose T: (q, e, M, w)."""
        c, dt = self.corr, self.dt
        Td = (pose_f32(T) if dt == F32 else np.asarray(T, F64)).astype(dt)      # float32 run: the pose as the float model holds it
        q = np.einsum("ab,nb->na", Td[:3, :3], c.pa) + Td[:3, 3]
        e = c.mean_b - q
        C = c.cov_b
        if c.cov_a is not None:
            Rl = (pose_f32(R_lin) if dt == F32 else np.asarray(R_lin, F64)).astype(dt)[:3, :3]
            C = C + np.einsum("ab,nbc,dc->nad", Rl, c.cov_a, Rl)
        M = np.linalg.inv(C) if len(C) else C
        if self.model == "VGICP_CUDA":
            w = c.n_b.astype(dt) if self.mutation == "weight_n" else np.sqrt(c.n_b.astype(dt))
        else:
            k2 = dt(1.0) if self.mutation == "cauchy_width_1" else dt(self.res) * dt(self.res)
            w = k2 / (k2 + np.einsum("na,na->n", e, e))
        assert q.dtype == dt and M.dtype == dt and w.dtype == dt
        return q, e, M, w

    def linearize(self, T):
        """(cost, H (6, 6), b (6,), count) at the pose T; the correspondences are remembered for compute_error."""
        T = np.asarray(T, F64)
        tv = self.target_voxels()
        pa, pa32, cov_a = self.source_elements()
        off = offsets_of(self.nn)
        cell = ndt_cells(transform_search(T, pa32), self.res, self.mutation)
        pos, hit = _lookup(tv.keys, _cell_key(cell[:, None, :] + off[None, :, :]))
        if self.model == "VGICP_CUDA":
            hit &= tv.n[pos] > 0
        else:
            hit &= (tv.n[pos] >= 6) if self.mutation == "n_ge_6" else (tv.n[pos] > 6)
        i, o = np.nonzero(hit)
        v = pos[i, o]
        self.corr = types.SimpleNamespace(src=i, vox=v, pa=pa[i], cov_a=None if cov_a is None else cov_a[i], mean_b=tv.mean[v], cov_b=tv.cov[v],
                                          n_b=tv.n[v], T_lin=T)
        q, e, M, w = self._terms(T, T)
        sgn = self.dt(-1.0 if self.mutation == "neg_skew" else 1.0)
        J = np.concatenate([sgn * skew(q).astype(self.dt), np.broadcast_to(-np.eye(3, dtype=self.dt), (len(i), 3, 3))], axis=2)
        Ht = np.einsum("n,nar,nab,nbs->nrs", w, J, M, J)
        bt = np.einsum("n,nar,nab,nb->nr", w, J, M, e)
        ct = np.einsum("n,na,nab,nb->n", w, e, M, e)
        assert Ht.dtype == self.dt and ct.dtype == self.dt
        return float(ct.astype(F64).sum()), Ht.astype(F64).sum(axis=0), bt.astype(F64).sum(axis=0), len(i)

    def cauchy_gradient_term(self) -> np.ndarray:
        """d cost / d eps - 2 b at the linearisation pose, float64: the Cauchy weight of P2D / D2D is a function of e, which the
        source's b (Gauss-Newton on w fixed) leaves out:  w = k^2 / (k^2 + |e|^2),  dw = -(w^2 / k^2) 2 e^T J d eps,  so the term is
        -2 sum (w^2 / k^2) (e^T M e) J^T e.  Zero for VGICP_CUDA (w = sqrt(n))."""
        if self.model == "VGICP_CUDA":
            return np.zeros(6)
        T = self.corr.T_lin
        q, e, M, w = (a.astype(F64) for a in self._terms(T, T))
        J = np.concatenate([skew(q), np.broadcast_to(-np.eye(3), (len(q), 3, 3))], axis=2)
        return -2.0 * np.einsum("n,n,nar,na->r", w * w / (self.res * self.res), np.einsum("na,nab,nb->n", e, M, e), J, e)

    def compute_error(self, T2) -> float:
        R_lin = T2 if self.mutation == "trial_rotation" else self.corr.T_lin
        _, e, M, w = self._terms(np.asarray(T2, F64), R_lin)
        return float(np.einsum("n,na,nab,nb->n", w, e, M, e).astype(F64).sum())


# ---- pclomp NDT ------------------------------------------------------------------------------------------------------------------
def pose_vector(T) -> np.ndarray:
    """p = (x, y, z, roll, pitch, yaw) with T = Translation * Rx(roll) Ry(pitch) Rz(yaw)."""
    from scipy.spatial.transform import Rotation
    T = np.asarray(T, F64)
    return np.concatenate([T[:3, 3], Rotation.from_matrix(T[:3, :3]).as_euler("XYZ")])


def _axis_rotation(c, s, axis, order=0):
    """R, dR / da or d^2 R / da^2 of the rotation by a about a coordinate axis, with c = cos a, s = sin a: R = I + s K + (1 - c) K^2."""
    K = skew(np.eye(3)[axis])
    K2 = K @ K
    return (np.eye(3) + s * K + (1.0 - c) * K2, c * K + s * K2, -s * K + c * K2)[order]


def angle_derivatives(p, mutation=None):
    """(dR (3, 3, 3), d2R (3, 3, 3, 3)): the first and second derivatives of Rx Ry Rz by (roll, pitch, yaw), by the product rule.
    computeAngleDerivatives takes cos = 1, sin = 0 for an angle below 10e-5 in magnitude; so does this."""
    cs = [(1.0, 0.0) if abs(a) < 10e-5 else (np.cos(a), np.sin(a)) for a in np.asarray(p, F64)[3:6]]

    def prod(orders):
        return np.linalg.multi_dot([_axis_rotation(cs[k][0], cs[k][1], k, orders[k]) for k in range(3)])
    dR = np.stack([prod([int(k == i) for k in range(3)]) for i in range(3)])
    d2R = np.stack([np.stack([prod([int(k == i) + int(k == j) for k in range(3)]) for j in range(3)]) for i in range(3)])
    if mutation == "drop_d2R_roll_roll":
        d2R[0, 0] = 0.0
    return dR, d2R


def pose_matrix_f32(p) -> np.ndarray:
    """final_transformation_ = Translation(p[:3]) * AngleAxisf(roll, X) * AngleAxisf(pitch, Y) * AngleAxisf(yaw, Z), a float32 4 x 4.
    Stated choice (Eigen/Geometry): AngleAxisf::toRotationMatrix of a unit coordinate axis has (1 - c) + c on the axis' diagonal entry, c on
    the other two and +-s off the diagonal; cos and sin of the float angle are rounded to float once; the 3 x 3 products are float32."""
    p = np.asarray(p, F64)
    Rs = []
    for k in range(3):
        a = F32(p[3 + k])
        c, s = F32(np.cos(F64(a))), F32(np.sin(F64(a)))
        R = np.zeros((3, 3), F32)
        i, j = (k + 1) % 3, (k + 2) % 3
        R[k, k] = (F32(1.0) - c) + c
        R[i, i] = R[j, j] = c
        R[i, j], R[j, i] = -s, s
        Rs.append(R)
    mul = lambda A, B: np.array([[(A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j] for j in range(3)] for i in range(3)], F32)
    T = np.eye(4, dtype=F32)
    T[:3, :3] = mul(mul(Rs[0], Rs[1]), Rs[2])
    T[:3, 3] = p[:3].astype(F32)
    return T


def transform_point_cloud_f32(Tf: np.ndarray, x32: np.ndarray) -> np.ndarray:
    """pcl::transformPointCloud in float32.  Stated choice (PCL is not in the tree): m00 x + (m01 y + (m02 z + m03)), as
    PCL >= 1.10 writes it -- the three float32 lines below."""
    assert Tf.dtype == F32 and x32.dtype == F32
    u = Tf[None, :3, 2] * x32[:, 2:3] + Tf[None, :3, 3]
    u = Tf[None, :3, 1] * x32[:, 1:2] + u
    u = Tf[None, :3, 0] * x32[:, 0:1] + u
    assert u.dtype == F32
    return u


def gauss_constants(outlier_ratio: float, resolution: float, mutation=None):
    """eq. 6.8 [Magnusson 2009], ndt_omp_impl.hpp:77-82; resolution_ is a float."""
    r = float(F32(resolution))
    c1, c2 = 10.0 * (1.0 - outlier_ratio), outlier_ratio / r ** 3
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2.0 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    return (d2, d1, d3) if mutation == "d1_d2_swapped" else (d1, d2, d3)


def pcl_leaves(x32: np.ndarray, leaf: float, mutation=None):
    """VoxelGridCovariance::applyFilter: namespace(keys, coords, n (after the rejection rules: -1), mean, icov, centroid float32, count)."""
    x32 = np.ascontiguousarray(x32[:, :3])
    coords = pcl_cells_of_map(x32, leaf, mutation)
    keys, first, inv = np.unique(_cell_key(coords), return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    nv = len(keys)
    count = np.bincount(inv, minlength=nv)
    x = x32.astype(F64)
    s, sxx, csum = np.zeros((nv, 3)), np.zeros((nv, 3, 3)), np.zeros((nv, 3), F32)
    if mutation != "no_identity":
        sxx += np.eye(3)
    np.add.at(s, inv, x)
    np.add.at(sxx, inv, np.einsum("na,nb->nab", x, x))
    np.add.at(csum, inv, x32)                                    # float32, a leaf's points in input order
    centroid = csum / count[:, None].astype(F32)
    mean = s / count[:, None]
    min_points = 7 if mutation == "min_points_7" else 6
    big = count >= min_points
    n = count.astype(np.int64)
    nn = count[:, None, None].astype(F64)
    cov = (sxx - 2.0 * np.einsum("va,vb->vab", s, mean)) / nn + np.einsum("va,vb->vab", mean, mean)
    if mutation != "no_n_minus_1":
        cov = cov * ((nn - 1.0) / nn)
    icov = np.zeros((nv, 3, 3))
    if big.any():
        w, V = np.linalg.eigh(cov[big])
        bad = (w[:, 0] < 0) | (w[:, 1] < 0) | (w[:, 2] <= 0)
        floor_ = (0.001 if mutation == "inflation_0.001" else 0.01) * w[:, 2:3]
        w2 = np.maximum(w, floor_)
        infl = np.einsum("vak,vk,vkb->vab", V, w2, np.linalg.inv(V))      # evecs * eigen_val * evecs.inverse()
        c = np.where((w[:, 0:1] < floor_)[:, :, None], infl, cov[big])
        ic = np.zeros_like(c)
        ic[~bad] = np.linalg.inv(c[~bad])
        bad |= ~np.isfinite(ic).all(axis=(1, 2))
        ic[bad] = 0.0
        icov[big] = ic
        idx = np.nonzero(big)[0]
        n[idx[bad]] = -1
    return types.SimpleNamespace(keys=keys, coords=coords[first], n=n, count=count, mean=mean, icov=icov, centroid=centroid, min_points=min_points,
                                 in_centroids=big)


PITCH2_SIGN_QUIRK = True      # the float pass of the source: see the module docstring


class PclNdtReference:
    """pclomp::NormalDistributionsTransform: computeDerivatives, computeHessian and calculateScore."""

    def __init__(self, scan, target, *, voxel_resolution=1.0, num_neighbors=7, outlier_ratio=0.55, dtype=F64, mutation=None):
        assert num_neighbors in (0, 1, 7, 27) and mutation in (None,) + MUTATIONS_PCL and dtype in (F32, F64)
        self.res, self.nn, self.dt, self.mutation = float(F32(voxel_resolution)), num_neighbors, dtype, mutation
        self.outlier_ratio = float(outlier_ratio)
        self.src32 = np.ascontiguousarray(np.asarray(scan)[:, :3])
        self.tgt32 = np.ascontiguousarray(np.asarray(target)[:, :3])
        self._leaves = None

    def swap_source_and_target(self):
        self.src32, self.tgt32 = self.tgt32, self.src32
        self._leaves = None

    def leaves(self):
        if self._leaves is None:
            self._leaves = pcl_leaves(self.tgt32, self.res, self.mutation)
        return self._leaves

    def neighbourhood(self, xt32):
        """(point index, leaf index) of every (point, neighbour leaf), point-major; kd: the float32 squared distances of KDTREE."""
        L = self.leaves()
        ok = L.n >= L.min_points
        if self.nn == 0:
            cand = np.nonzero(L.in_centroids)[0]
            if self.mutation == "kdtree_cell_centre":
                c32 = ((L.coords[cand].astype(F64) + 0.5) * self.res).astype(F32)
            else:
                c32 = L.centroid[cand]
            pairs = cKDTree(c32.astype(F64)).query_ball_point(xt32.astype(F64), self.res * 1.001)
            i = np.repeat(np.arange(len(xt32)), [len(a) for a in pairs])
            j = np.array([b for a in pairs for b in sorted(a)], np.int64)
            d = xt32[i] - c32[j]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert d2.dtype == F32
            r2 = F32(self.res * self.res)
            keep = (d2 <= r2) if self.mutation == "radius_le" else (d2 < r2)
            self.kd = types.SimpleNamespace(d2=d2.astype(F64), r2=float(r2))
            return i[keep], cand[j[keep]]
        off = OFFSETS[self.nn]
        cell = pcl_cells_of_query(xt32, self.res, self.mutation)
        pos, hit = _lookup(L.keys, _cell_key(cell[:, None, :] + off[None, :, :]))
        hit &= ok[pos]
        i, o = np.nonzero(hit)
        return i, pos[i, o]

    def _terms(self, Tf, dt, frozen=None, exact_p=None):
        xt32 = transform_point_cloud_f32(Tf, self.src32)
        i, v = self.neighbourhood(xt32) if frozen is None else frozen
        self.last_neighbourhood = (i, v)
        L = self.leaves()
        xt = xt32.astype(F64)
        if exact_p is not None:        # the derivative tests only: the pose applied in float64, so that a central difference is smooth
            Rm = np.linalg.multi_dot([_axis_rotation(np.cos(a), np.sin(a), k) for k, a in enumerate(exact_p[3:6])])
            xt = self.src32.astype(F64) @ Rm.T + exact_p[:3]
        d = (xt[i] - L.mean[v]).astype(dt)                          # x_trans -= cell->getMean() in double, then the float 4-vector
        C = L.icov[v].astype(dt)
        return i, v, d, C

    def derivatives(self, p, hessian="float", quirk=PITCH2_SIGN_QUIRK, frozen=None, exact=False):
        """(score, gradient (6,), Hessian (6, 6) or None, count) at p.  hessian "float" / None: computeDerivatives with updateDerivatives'
        per-term quantities in self.dt; "double": computeHessian / updateHessian, always in float64 (score and gradient None).
        frozen: the (point, leaf) pairs of another call (last_neighbourhood) instead of a search; exact: the pose applied in float64."""
        p = np.asarray(p, F64)
        dt = F64 if hessian == "double" else self.dt
        d1, d2, _ = gauss_constants(self.outlier_ratio, self.res, self.mutation)
        i, v, d, C = self._terms(pose_matrix_f32(p), dt, frozen, p if exact else None)
        dR, d2R = angle_derivatives(p, self.mutation)
        if hessian == "float" and quirk:
            sy = 0.0 if abs(p[4]) < 10e-5 else np.sin(p[4])
            d2R = d2R.copy()
            d2R[1, 1, 0, 2] = sy                                   # ndt_omp_impl.hpp:354; the derivative is -sy
        x = self.src32[i].astype(dt)
        n = len(i)
        pg = np.zeros((n, 3, 6), dt)                              # d T(x, p) / d p
        pg[:, :, :3] = np.eye(3, dtype=dt)
        pg[:, :, 3:] = np.einsum("kab,nb->nak", dR.astype(dt), x)
        ph = np.einsum("klab,nb->nakl", d2R.astype(dt), x)         # d^2 T / d angle_k d angle_l
        d2t, d1t = dt(d2), dt(d1)
        dC = np.einsum("na,nab->nb", d, C)
        q = np.einsum("na,na->n", dC, d)
        e = np.exp(-d2t * q * dt(0.5))
        score_t = -d1t * e
        e2 = d2t * e
        self.e_x_cov_x = e2.astype(F64)
        ok = ~((e2 > 1) | (e2 < 0) | np.isnan(e2))
        e2 = np.where(ok, e2 * d1t, dt(0))
        xg = np.einsum("nb,nbj->nj", dC, pg)
        count = int(ok.sum())
        if hessian == "double":
            score = g = None
        else:
            score = float(np.where(ok, score_t, dt(0)).astype(F64).sum())
            g = (e2[:, None] * xg).astype(F64).sum(axis=0)
        H = None
        if hessian is not None:
            Ht = -d2t * np.einsum("ni,nj->nij", xg, xg) + np.einsum("nai,nab,nbj->nij", pg, C, pg)
            Ht[:, 3:, 3:] += np.einsum("nb,nbkl->nkl", dC, ph)
            Ht = e2[:, None, None] * Ht
            assert Ht.dtype == dt
            H = Ht.astype(F64).sum(axis=0)
        return score, g, H, count

    def score(self, T32) -> float:
        """calculateScore of the scan transformed by the float32 pose T32, in float64."""
        T32 = np.asarray(T32)
        assert T32.dtype == F32
        d1, d2, d3 = gauss_constants(self.outlier_ratio, self.res, self.mutation)
        i, v, d, C = self._terms(T32, F64)
        e = np.exp(-d2 * np.einsum("na,nab,nb->n", d, C, d) / 2.0)
        m = np.bincount(i, minlength=len(self.src32)).astype(F64)
        per = (-d1 * e - d3) / (1.0 if self.mutation == "score_not_per_cell" else m[i])
        self.score_count = len(i)
        return float(per.sum() / len(self.src32))


# ---- preconditions ---------------------------------------------------------------------------------------------------------------
CELL_ULPS = 8         # a transformed coordinate this many float32 ulps (of |R| |p| + |t|) from a cell boundary may fall either way
KD_MARGIN = 1e-5      # relative, of the squared radius
EXCOV_MARGIN = 1e-5   # of e_x_cov_x to its bounds 0 and 1


def _coordinate_slack(T, x):
    T = np.asarray(T, F64)
    return CELL_ULPS * 2.0 * EPS32 * (np.abs(x) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3]))


def cell_boundary_distance(T, x, res, rule):
    """(N, 3) distance of every coordinate of T x (exact, float64) to the nearest cell boundary of the rule, in metres:
    "ndt": boundaries at (k + 0.5) res;  "pcl": at k res."""
    q = transform(np.asarray(T, F64), x)
    u = q / res - (0.5 if rule == "ndt" else 0.0)
    return np.abs(u - np.round(u)) * res


def violations_cell(T, x, res, rule):
    """Rows of x with a transformed coordinate within CELL_ULPS float32 ulps of a cell boundary."""
    return np.nonzero((cell_boundary_distance(T, x, res, rule) <= _coordinate_slack(T, x)).any(axis=1))[0]


def violations_kdtree(scan, target, T, res):
    """Scan rows with a leaf centroid within KD_MARGIN (relative, squared) of the search radius."""
    r = PclNdtReference(scan, target, voxel_resolution=res, num_neighbors=0)
    xt32 = transform_point_cloud_f32(pose_matrix_f32(pose_vector(T)), r.src32)
    L = r.leaves()
    cand = L.centroid[L.in_centroids].astype(F64)
    pairs = cKDTree(cand).query_ball_point(xt32.astype(F64), r.res * 1.01)
    bad = []
    for k, a in enumerate(pairs):
        if a:
            d2 = ((cand[a] - xt32[k].astype(F64)) ** 2).sum(axis=1)
            if (np.abs(d2 - r.res ** 2) <= KD_MARGIN * r.res ** 2).any():
                bad.append(k)
    return np.array(bad, np.int64)


def violations_e_x_cov_x(scan, target, T, res, nn):
    r = PclNdtReference(scan, target, voxel_resolution=res, num_neighbors=nn)
    p = pose_vector(T)
    r.derivatives(p, None)
    i, _ = r.neighbourhood(transform_point_cloud_f32(pose_matrix_f32(p), r.src32))
    e = r.e_x_cov_x
    near = np.abs(e - 1.0) <= EXCOV_MARGIN          # the bound 0 is reached only by underflow, and 0 is admissible: no decision there
    return np.unique(i[near])


RESOLUTIONS = (1.0, 0.5)


def all_violations(scan, submap, poses, swapped_poses):
    """(scan rows, map rows) that violate a margin in any case of the two test files."""
    bad_s, bad_m = set(), set()
    xs, xm = widen(scan), widen(submap)
    for res in RESOLUTIONS:
        for rule in ("ndt", "pcl"):
            for T in poses:
                bad_s.update(violations_cell(T, xs, res, rule))
            for T in swapped_poses:
                bad_m.update(violations_cell(T, xm, res, rule))
        # D2D: the source elements are voxel means; a mean near a boundary takes its whole voxel out
        for cloud, x32, Ts, bad in ((scan, scan[:, :3], poses, bad_s), (submap, submap[:, :3], swapped_poses, bad_m)):
            sv = gauss_voxels(np.ascontiguousarray(x32), res)
            for T in Ts:
                vb = violations_cell(T, sv.mean, res, "ndt")
                bad.update(np.nonzero(np.isin(sv.of_point, vb))[0])
        for T in poses:
            bad_s.update(violations_kdtree(scan, submap, T, res))
            bad_s.update(violations_e_x_cov_x(scan, submap, T, res, 27))
    return np.array(sorted(bad_s), np.int64), np.array(sorted(bad_m), np.int64)


# ---- fixture ---------------------------------------------------------------------------------------------------------------------
SHIFT = np.array([0.02, -0.01, 0.01])
TRIAL_ROTATION = np.array([0.02, -0.02, 0.02])
REMOVED_CAP = 0.01
N_SCAN, N_MAP, PAIR_ID = 1100, 12000, 3
# Points per square metre of the synthetic scene (its area goes with 1 / density^2, and the scan's extent with the scene's).
#   wide   60: 7.3 x 5.5 x 2.2 m, scan 1.3 x 1.8 x 2.1 m.  pclomp NDT (leaves of fewer than 6 points and scan points without a leaf exist
#              here) and every Gaussian-voxel case at 1.0 m, with the swapped, head and single-voxel cases: 120 target voxels, 11 D2D source
#              voxels (11 / 60 / 147 correspondences at 1 / 7 / 27).
#   dense 150: 3.2 x 2.4 x 2.1 m, scan 0.56 x 0.79 x 1.1 m.  The Gaussian-voxel cases at 0.5 m: 169 target voxels (164 with n > 6), 11 D2D
#              source voxels (7 with n > 6; 11 / 54 / 123 correspondences).
# Why not 60 at 0.5 m: gaussian_voxelmap.cu forms x x^T in float and subtracts mean sum x^T, and covariance_regularization leaves an
# eigenvalue just above 1e-3 unclamped; the 0.5 m voxels of the wide scene are thin patches 10 m off the origin whose smallest eigenvalue sits at
# that clamp, the float products alone move C_B^-1 of such voxels by 1e-4 and b of P2D 1 / 27 / r1.5 and D2D 7 by 1.0e-5 ... 1.5e-5 (twelve seeds
# tried: 2.0e-5 ... 4.5e-4) -- above HB_RTOL, on the CPU oracle and on the MI355X alike, so ill-conditioned inputs by the rule of tolerance().
# The CPU oracle's largest deviation from the double statement over the 0.5 m grid, by density: 60: 1.5e-5, 90: 3.0e-5 (centred), 110: 7.7e-6,
# 130: 9.2e-5, 150: 4.4e-6, 200: 1.2e-5 (centred), 300: 3.0e-6 -- erratic, b being a sum of cancelling terms; 300 and above shrink the scan
# to one to three source voxels, so 150 it is.  The centred cases run at 27 cells / 0.5 m on the dense scene: on the wide one centred P2D lies
# 3.7e-5 ... 9.4e-5 off at 1.0 m.
DENSITY = {"wide": 60.0, "dense": 150.0}
_fixtures = {}


def TRIAL(T) -> np.ndarray:
    """The trial pose of a linearisation pose T: T composed with a rotation of about 0.02 rad on each axis, plus the translation shift.
    A rotated trial pose separates R of the trial pose from R of the linearisation pose in D2D / VGICP_CUDA."""
    T2 = left_step(np.asarray(T, F64), np.concatenate([TRIAL_ROTATION, np.zeros(3)]))
    T2[:3, 3] = np.asarray(T, F64)[:3, 3] + SHIFT
    return T2


def build_fixture(synth, centred=False, family="wide"):
    """synth.make_pair(3, 1100, 12000, density=DENSITY[family]) less the points that violate a precondition; centred: the map and the poses
    moved by the map's centroid.  At most three rounds, at most 1 % of either cloud removed, or this raises."""
    key = (centred, family)
    if key not in _fixtures:
        p = synth.make_pair(PAIR_ID, N_SCAN, N_MAP, density=DENSITY[family])
        scan, submap = p.scan.copy(), p.submap.copy()
        guess, T_gt = p.guess.astype(F64), p.T_gt.copy()
        if centred:
            c = widen(submap).mean(axis=0)
            submap[:, :3] = (widen(submap) - c).astype(F32)
            guess[:3, 3] -= c
            T_gt[:3, 3] -= c
        # both poses exactly representable in float32: the float models round the pose they are given, and at T_gt, where b is a sum of
        # cancelling terms, that rounding alone moved b by more than HB_RTOL (measured: 1.2e-5 ... 1.8e-5) -- an ill-conditioned input
        guess, T_gt = guess.astype(F32).astype(F64), T_gt.astype(F32).astype(F64)
        n_scan, n_map = len(scan), len(submap)
        poses, swapped = (guess, T_gt), (np.linalg.inv(guess),)
        rounds = []
        for _ in range(3):
            bad_s, bad_m = all_violations(scan, submap, poses, swapped)
            rounds.append((len(bad_s), len(bad_m)))
            if not len(bad_s) and not len(bad_m):
                break
            scan, submap = np.delete(scan, bad_s, axis=0), np.delete(submap, bad_m, axis=0)
        bad_s, bad_m = all_violations(scan, submap, poses, swapped)
        if len(bad_s) or len(bad_m):
            raise AssertionError("violations left after three rounds: %d scan, %d map" % (len(bad_s), len(bad_m)))
        removed = (n_scan - len(scan), n_map - len(submap))
        if removed[0] > REMOVED_CAP * n_scan or removed[1] > REMOVED_CAP * n_map:
            raise AssertionError("more than 1 %% of a cloud removed: %r" % (removed,))
        for a in (scan, submap, guess, T_gt):
            a.setflags(write=False)
        _fixtures[key] = types.SimpleNamespace(scan=scan, submap=submap, guess=guess, T_gt=T_gt, poses=poses, swapped_pose=swapped[0],
                                                   removed_scan=removed[0], removed_map=removed[1], rounds=rounds, centred=centred)
    return _fixtures[key]


def margins(fx):
    """The smallest margin left per rule: cell boundaries as a multiple of the allowed slack (> 1), the KDTREE radius relative."""
    out = {}
    xs, xm = widen(fx.scan), widen(fx.submap)
    for rule in ("ndt", "pcl"):
        m = []
        for res in RESOLUTIONS:
            for T, x in [(T, xs) for T in fx.poses] + [(fx.swapped_pose, xm)]:
                m.append((cell_boundary_distance(T, x, res, rule) / _coordinate_slack(T, x)).min())
        out["cell_%s_over_slack" % rule] = float(min(m))
    kd = []
    for res in RESOLUTIONS:
        for T in fx.poses:
            r = PclNdtReference(fx.scan, fx.submap, voxel_resolution=res, num_neighbors=0)
            r.neighbourhood(transform_point_cloud_f32(pose_matrix_f32(pose_vector(T)), r.src32))
            kd.append((np.abs(r.kd.d2 - r.kd.r2) / r.kd.r2).min())
    out["kdtree_radius_relative"] = float(min(kd))
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------
POSES = ("guess", "T_gt")


def kndt_cases():
    """(model, neighbourhood, resolution) of the main grid: 1 / 7 / 27 on all three, DIRECT_RADIUS 1.5 on P2D and VGICP_CUDA."""
    out = []
    for model in MODELS:
        for nn in (1, 7, 27) + (("r1.5",) if model != "NDT_D2D" else ()):
            for res in RESOLUTIONS:
                out.append((model, nn, res))
    return out


def pcl_cases():
    return [(nn, res) for nn in (0, 1, 7, 27) for res in RESOLUTIONS]


def case_name(*parts):
    return "/".join(str(x) for x in parts)


# the cases beside the main grid: (model, neighbourhood, resolution, variant); every variant but "centred" is evaluated at one pose
KNDT_SPECIAL = [("NDT_P2D", 27, 0.5, "centred"), ("NDT_D2D", 27, 0.5, "centred"), ("VGICP_CUDA", 27, 0.5, "centred"),
                ("NDT_P2D", 7, 1.0, "swapped"), ("NDT_D2D", 7, 1.0, "swapped"),
                ("NDT_P2D", 7, 1.0, "head257"), ("NDT_P2D", 7, 1.0, "head1"), ("NDT_D2D", 7, 1.0, "single_voxel"),
                ("VGICP_CUDA", 27, 0.5, "sparse20"), ("NDT_P2D", 27, 0.5, "sparse20")]      # sparse20 P2D: voxels of exactly 6 points
PCL_SPECIAL = [(7, 1.0, "centred"), (7, 1.0, "swapped"), (7, 1.0, "head257"), (7, 1.0, "head1")]


def kndt_family(res) -> str:
    """The scene a Gaussian-voxel case of that resolution runs on (see DENSITY)."""
    return "dense" if res == 0.5 else "wide"


def case_inputs(synth, variant="main", family="wide"):
    """namespace(scan, target, poses {name: T}, swapped) of a variant.  swapped: the caller builds both sides on (scan, target) and calls
    swap_source_and_target() on them; the pose is guess^-1."""
    fx = build_fixture(synth, centred=(variant == "centred"), family=family)
    scan, target, poses, swapped = fx.scan, fx.submap, dict(zip(POSES, fx.poses)), False
    if variant == "swapped":
        poses, swapped = {"guess_inv": fx.swapped_pose}, True
    elif variant == "head257":
        scan, poses = fx.scan[:257], {"guess": fx.guess}
    elif variant == "head1":
        scan, poses = fx.scan[:1], {"guess": fx.guess}
    elif variant == "single_voxel":                      # the scan points of the fullest 1.0 m source voxel: one D2D source element
        sv = gauss_voxels(np.ascontiguousarray(fx.scan[:, :3]), 1.0)
        scan, poses = fx.scan[sv.of_point == int(np.argmax(sv.n))], {"guess": fx.guess}
        assert len(sv.n) > 1 and 6 < len(scan) < len(fx.scan)
    elif variant == "sparse20":                          # every 20th map point: voxels of one point, of exactly 6 and of more
        target, poses = fx.submap[::20], {"guess": fx.guess}
    else:
        assert variant in ("main", "centred")
    return types.SimpleNamespace(scan=scan, target=target, poses=poses, swapped=swapped, fx=fx)


def at_most_per_cell(cloud, of_point, cap):
    """The points of a cloud less those beyond the first `cap` of their cell (input order)."""
    order = np.argsort(of_point, kind="stable")
    start = np.r_[0, np.nonzero(np.diff(of_point[order]))[0] + 1]
    rank = np.arange(len(order)) - np.repeat(start, np.diff(np.r_[start, len(order)]))
    return cloud[np.sort(order[rank < cap])]


def thin_for_p2d(cloud, res=1.0):
    """At most 6 points per Gaussian voxel: no voxel takes part (n > 6).  (Every 20th map point still leaves voxels of 17.)"""
    return at_most_per_cell(cloud, gauss_voxels(np.ascontiguousarray(cloud[:, :3]), res).of_point, 6)


def thin_for_pcl(cloud, leaf=1.0):
    """At most 5 points per pclomp leaf: no leaf takes part (>= 6)."""
    x = np.ascontiguousarray(cloud[:, :3])
    L = pcl_leaves(x, leaf)
    return at_most_per_cell(cloud, np.searchsorted(L.keys, _cell_key(pcl_cells_of_map(x, leaf))), 5)


def all_kndt_cases():
    return [c + ("main",) for c in kndt_cases()] + KNDT_SPECIAL


def all_pcl_cases():
    return [c + ("main",) for c in pcl_cases()] + PCL_SPECIAL


def measure_kndt(make, T):
    """make(dtype) -> NdtReference.  {quantity: (Q64, Q32)} at T and TRIAL(T)."""
    out = {}
    r64, r32 = make(F64), make(F32)
    a, b = r64.linearize(T), r32.linearize(T)
    assert a[3] == b[3]
    out["cost"], out["H"], out["b"] = (a[0], b[0]), (a[1], b[1]), (a[2], b[2])
    out["compute_error"] = (r64.compute_error(TRIAL(T)), r32.compute_error(TRIAL(T)))
    return out, a[3]


def measure_pcl(make, T):
    out = {}
    r64, r32 = make(F64), make(F32)
    p = pose_vector(T)
    a, b = r64.derivatives(p, "float"), r32.derivatives(p, "float")
    assert a[3] == b[3]
    out["score"], out["gradient"], out["H_float"] = (a[0], b[0]), (a[1], b[1]), (a[2], b[2])
    return out, a[3]


def noise_of(pairs):
    return {k: (abs(b - a) / abs(a) if np.ndim(a) == 0 else rel_err(b, a)) for k, (a, b) in pairs.items()}


# ---- tolerances ------------------------------------------------------------------------------------------------------------------
HB_RTOL = 1e-5        # tests/helpers.py: the bar these kernels are held to against the oracle
DOUBLE_TOL = 1e-9     # the project's bar for double quantities: the pclomp double Hessian pass and calculateScore
# Chosen once from tests/test_ndt_numpy_ref.py::test_oracle_*: the CPU oracle performs the float operations in the kernels' order; the
# largest rel_err(oracle, Q64) / noise(Q) seen over every case and quantity is ORACLE_RATIO_MEASURED, and MARGIN = max(4, 4 x that).
ORACLE_RATIO_MEASURED = 62.73      # NDT_P2D/7/1.0/head1/guess cost (a sum of 5 terms: its noise, 1.6e-9, is one draw); with MARGIN = 4 x this, most tolerances are the HB_RTOL cap
MARGIN = max(4.0, 4.0 * ORACLE_RATIO_MEASURED)
NOISE_MEASURED = {
    'NDT_P2D/1/1.0/main/guess': {'count': 1098, 'cost': 1.57e-07, 'H': 1.17e-07, 'b': 9.66e-08, 'compute_error': 4e-07},
    'NDT_P2D/1/1.0/main/T_gt': {'count': 1098, 'cost': 1.49e-07, 'H': 1.15e-07, 'b': 9.72e-07, 'compute_error': 4.34e-07},
    'NDT_P2D/1/0.5/main/guess': {'count': 1100, 'cost': 3.16e-07, 'H': 4.62e-08, 'b': 3.48e-07, 'compute_error': 4.78e-07},
    'NDT_P2D/1/0.5/main/T_gt': {'count': 1100, 'cost': 1.91e-07, 'H': 5.95e-08, 'b': 1.56e-06, 'compute_error': 1.25e-07},
    'NDT_P2D/7/1.0/main/guess': {'count': 5845, 'cost': 3.69e-08, 'H': 9.13e-08, 'b': 5.89e-07, 'compute_error': 1.67e-08},
    'NDT_P2D/7/1.0/main/T_gt': {'count': 5789, 'cost': 2.91e-08, 'H': 8.47e-08, 'b': 6.46e-07, 'compute_error': 2.01e-08},
    'NDT_P2D/7/0.5/main/guess': {'count': 5591, 'cost': 4.83e-07, 'H': 7.8e-08, 'b': 2.39e-07, 'compute_error': 4.98e-07},
    'NDT_P2D/7/0.5/main/T_gt': {'count': 5501, 'cost': 4.42e-08, 'H': 4.7e-08, 'b': 1.88e-06, 'compute_error': 8.99e-09},
    'NDT_P2D/27/1.0/main/guess': {'count': 14241, 'cost': 3.13e-08, 'H': 7.67e-08, 'b': 4.38e-07, 'compute_error': 6.19e-08},
    'NDT_P2D/27/1.0/main/T_gt': {'count': 14073, 'cost': 3.52e-09, 'H': 6.98e-08, 'b': 4.41e-07, 'compute_error': 2.91e-08},
    'NDT_P2D/27/0.5/main/guess': {'count': 12669, 'cost': 8.26e-08, 'H': 5.24e-08, 'b': 3.11e-07, 'compute_error': 9.9e-08},
    'NDT_P2D/27/0.5/main/T_gt': {'count': 12532, 'cost': 2.37e-08, 'H': 4.07e-08, 'b': 8.84e-07, 'compute_error': 2.74e-08},
    'NDT_P2D/r1.5/1.0/main/guess': {'count': 12045, 'cost': 4.23e-08, 'H': 7.71e-08, 'b': 5.93e-07, 'compute_error': 7.74e-08},
    'NDT_P2D/r1.5/1.0/main/T_gt': {'count': 11877, 'cost': 1.41e-08, 'H': 7.01e-08, 'b': 5.86e-07, 'compute_error': 4.45e-08},
    'NDT_P2D/r1.5/0.5/main/guess': {'count': 11027, 'cost': 1.53e-07, 'H': 5.47e-08, 'b': 2.52e-07, 'compute_error': 1.73e-07},
    'NDT_P2D/r1.5/0.5/main/T_gt': {'count': 10787, 'cost': 5.37e-08, 'H': 4.5e-08, 'b': 1.46e-06, 'compute_error': 4.6e-08},
    'NDT_D2D/1/1.0/main/guess': {'count': 11, 'cost': 1.29e-07, 'H': 1.58e-07, 'b': 1.01e-06, 'compute_error': 7.96e-07},
    'NDT_D2D/1/1.0/main/T_gt': {'count': 11, 'cost': 1.15e-07, 'H': 1.03e-07, 'b': 3.15e-06, 'compute_error': 5.74e-07},
    'NDT_D2D/1/0.5/main/guess': {'count': 11, 'cost': 3.14e-08, 'H': 5.57e-08, 'b': 1.3e-06, 'compute_error': 2.62e-07},
    'NDT_D2D/1/0.5/main/T_gt': {'count': 11, 'cost': 3.23e-07, 'H': 7.03e-08, 'b': 4.23e-06, 'compute_error': 1.08e-07},
    'NDT_D2D/7/1.0/main/guess': {'count': 60, 'cost': 9.83e-08, 'H': 1.25e-07, 'b': 8.32e-07, 'compute_error': 4.38e-08},
    'NDT_D2D/7/1.0/main/T_gt': {'count': 60, 'cost': 5.63e-08, 'H': 1.21e-07, 'b': 5.45e-07, 'compute_error': 4.26e-08},
    'NDT_D2D/7/0.5/main/guess': {'count': 55, 'cost': 2.65e-07, 'H': 7.76e-08, 'b': 1.07e-06, 'compute_error': 1.93e-07},
    'NDT_D2D/7/0.5/main/T_gt': {'count': 54, 'cost': 2.32e-07, 'H': 5.44e-08, 'b': 2.59e-06, 'compute_error': 1.78e-07},
    'NDT_D2D/27/1.0/main/guess': {'count': 147, 'cost': 7.49e-08, 'H': 9.99e-08, 'b': 5.28e-07, 'compute_error': 1.04e-08},
    'NDT_D2D/27/1.0/main/T_gt': {'count': 147, 'cost': 9.11e-08, 'H': 1.38e-07, 'b': 4.57e-07, 'compute_error': 5.32e-08},
    'NDT_D2D/27/0.5/main/guess': {'count': 123, 'cost': 7.3e-08, 'H': 4.63e-08, 'b': 1.71e-06, 'compute_error': 4.14e-08},
    'NDT_D2D/27/0.5/main/T_gt': {'count': 118, 'cost': 1.14e-07, 'H': 4.85e-08, 'b': 8.96e-07, 'compute_error': 9e-08},
    'VGICP_CUDA/1/1.0/main/guess': {'count': 1098, 'cost': 2.49e-07, 'H': 4.04e-08, 'b': 1.18e-06, 'compute_error': 3.82e-07},
    'VGICP_CUDA/1/1.0/main/T_gt': {'count': 1098, 'cost': 1.51e-07, 'H': 1.39e-07, 'b': 1.52e-06, 'compute_error': 4.16e-07},
    'VGICP_CUDA/1/0.5/main/guess': {'count': 1100, 'cost': 1.25e-07, 'H': 2.39e-07, 'b': 1.96e-07, 'compute_error': 1.41e-07},
    'VGICP_CUDA/1/0.5/main/T_gt': {'count': 1100, 'cost': 3.02e-08, 'H': 2.89e-07, 'b': 9.36e-07, 'compute_error': 2.15e-07},
    'VGICP_CUDA/7/1.0/main/guess': {'count': 5845, 'cost': 3.44e-08, 'H': 9.2e-08, 'b': 3.92e-06, 'compute_error': 1.11e-07},
    'VGICP_CUDA/7/1.0/main/T_gt': {'count': 5789, 'cost': 3.78e-08, 'H': 4.89e-08, 'b': 8.6e-07, 'compute_error': 6.45e-08},
    'VGICP_CUDA/7/0.5/main/guess': {'count': 5725, 'cost': 1.01e-09, 'H': 2.07e-07, 'b': 2.06e-07, 'compute_error': 3.85e-08},
    'VGICP_CUDA/7/0.5/main/T_gt': {'count': 5690, 'cost': 1.62e-08, 'H': 2.51e-07, 'b': 6.12e-07, 'compute_error': 9.97e-08},
    'VGICP_CUDA/27/1.0/main/guess': {'count': 14241, 'cost': 1.74e-08, 'H': 5.55e-08, 'b': 3.5e-07, 'compute_error': 8.37e-08},
    'VGICP_CUDA/27/1.0/main/T_gt': {'count': 14073, 'cost': 1.44e-08, 'H': 1.86e-08, 'b': 1.62e-07, 'compute_error': 5.55e-08},
    'VGICP_CUDA/27/0.5/main/guess': {'count': 13716, 'cost': 6.7e-09, 'H': 1.84e-07, 'b': 4.33e-07, 'compute_error': 5.12e-08},
    'VGICP_CUDA/27/0.5/main/T_gt': {'count': 13563, 'cost': 7.65e-10, 'H': 2.52e-07, 'b': 2.37e-07, 'compute_error': 4.26e-08},
    'VGICP_CUDA/r1.5/1.0/main/guess': {'count': 12045, 'cost': 3.73e-09, 'H': 5.62e-08, 'b': 6.69e-07, 'compute_error': 7.55e-08},
    'VGICP_CUDA/r1.5/1.0/main/T_gt': {'count': 11877, 'cost': 6.28e-09, 'H': 1.88e-08, 'b': 2.9e-07, 'compute_error': 4.62e-08},
    'VGICP_CUDA/r1.5/0.5/main/guess': {'count': 11622, 'cost': 4.24e-09, 'H': 1.86e-07, 'b': 2.55e-07, 'compute_error': 4.87e-08},
    'VGICP_CUDA/r1.5/0.5/main/T_gt': {'count': 11501, 'cost': 1.7e-09, 'H': 2.54e-07, 'b': 5.21e-07, 'compute_error': 5.5e-08},
    'NDT_P2D/27/0.5/centred/guess': {'count': 14004, 'cost': 1.59e-07, 'H': 5.36e-08, 'b': 5.68e-06, 'compute_error': 1.6e-07},
    'NDT_P2D/27/0.5/centred/T_gt': {'count': 13854, 'cost': 9.65e-09, 'H': 3.75e-08, 'b': 2.6e-06, 'compute_error': 8.27e-09},
    'NDT_D2D/27/0.5/centred/guess': {'count': 132, 'cost': 3.31e-08, 'H': 1.14e-07, 'b': 4.06e-07, 'compute_error': 3.65e-08},
    'NDT_D2D/27/0.5/centred/T_gt': {'count': 132, 'cost': 1.2e-08, 'H': 1.33e-07, 'b': 3.7e-07, 'compute_error': 7.55e-09},
    'VGICP_CUDA/27/0.5/centred/guess': {'count': 14004, 'cost': 3.19e-08, 'H': 7.43e-08, 'b': 1.63e-06, 'compute_error': 4.87e-08},
    'VGICP_CUDA/27/0.5/centred/T_gt': {'count': 13854, 'cost': 3.15e-09, 'H': 2.19e-07, 'b': 2e-06, 'compute_error': 1.17e-09},
    'NDT_P2D/7/1.0/swapped/guess_inv': {'count': 4212, 'cost': 7.86e-07, 'H': 4.78e-07, 'b': 6.07e-07, 'compute_error': 7.31e-07},
    'NDT_D2D/7/1.0/swapped/guess_inv': {'count': 56, 'cost': 1.39e-08, 'H': 2.53e-07, 'b': 1.18e-06, 'compute_error': 3.9e-07},
    'NDT_P2D/7/1.0/head257/guess': {'count': 1457, 'cost': 3.07e-08, 'H': 7.56e-08, 'b': 3.37e-07, 'compute_error': 5.73e-08},
    'NDT_P2D/7/1.0/head1/guess': {'count': 5, 'cost': 1.61e-09, 'H': 1.18e-07, 'b': 5.97e-07, 'compute_error': 1.07e-07},
    'NDT_D2D/7/1.0/single_voxel/guess': {'count': 6, 'cost': 1.4e-07, 'H': 1.49e-07, 'b': 6.19e-06, 'compute_error': 1.64e-07},
    'VGICP_CUDA/27/0.5/sparse20/guess': {'count': 12669, 'cost': 6.11e-07, 'H': 9.29e-08, 'b': 5.66e-07, 'compute_error': 5.58e-07},
    'NDT_P2D/27/0.5/sparse20/guess': {'count': 1591, 'cost': 5.29e-07, 'H': 2.26e-06, 'b': 1.59e-06, 'compute_error': 4.7e-07},
    'NDT_OMP/0/1.0/main/guess': {'count': 6126, 'score': 4.86e-08, 'gradient': 5.35e-08, 'H_float': 3.05e-08},
    'NDT_OMP/0/1.0/main/T_gt': {'count': 6322, 'score': 4.93e-08, 'gradient': 4.72e-08, 'H_float': 3.9e-08},
    'NDT_OMP/0/0.5/main/guess': {'count': 3232, 'score': 8.91e-09, 'gradient': 2.17e-08, 'H_float': 4.37e-08},
    'NDT_OMP/0/0.5/main/T_gt': {'count': 3174, 'score': 1e-08, 'gradient': 1.74e-08, 'H_float': 4.43e-08},
    'NDT_OMP/1/1.0/main/guess': {'count': 1077, 'score': 4.62e-08, 'gradient': 3.82e-08, 'H_float': 4.45e-08},
    'NDT_OMP/1/1.0/main/T_gt': {'count': 1073, 'score': 4.2e-08, 'gradient': 7.98e-08, 'H_float': 4.74e-08},
    'NDT_OMP/1/0.5/main/guess': {'count': 614, 'score': 1.45e-08, 'gradient': 3.66e-08, 'H_float': 4.65e-08},
    'NDT_OMP/1/0.5/main/T_gt': {'count': 507, 'score': 1.38e-08, 'gradient': 5.63e-08, 'H_float': 4.18e-08},
    'NDT_OMP/7/1.0/main/guess': {'count': 6512, 'score': 5.24e-08, 'gradient': 5.4e-08, 'H_float': 2.94e-08},
    'NDT_OMP/7/1.0/main/T_gt': {'count': 6230, 'score': 4.74e-08, 'gradient': 4.18e-08, 'H_float': 5.26e-08},
    'NDT_OMP/7/0.5/main/guess': {'count': 3786, 'score': 9.76e-09, 'gradient': 1.23e-08, 'H_float': 4.07e-08},
    'NDT_OMP/7/0.5/main/T_gt': {'count': 3282, 'score': 1.23e-08, 'gradient': 2.17e-08, 'H_float': 4.72e-08},
    'NDT_OMP/27/1.0/main/guess': {'count': 20496, 'score': 5.87e-08, 'gradient': 5.54e-08, 'H_float': 1.49e-08},
    'NDT_OMP/27/1.0/main/T_gt': {'count': 18947, 'score': 5.75e-08, 'gradient': 4.86e-08, 'H_float': 3.65e-08},
    'NDT_OMP/27/0.5/main/guess': {'count': 13154, 'score': 1.28e-08, 'gradient': 1.32e-08, 'H_float': 2.08e-08},
    'NDT_OMP/27/0.5/main/T_gt': {'count': 11451, 'score': 1.33e-08, 'gradient': 1.56e-08, 'H_float': 4.88e-08},
    'NDT_OMP/7/1.0/centred/guess': {'count': 5871, 'score': 5.14e-08, 'gradient': 7.67e-08, 'H_float': 1.47e-08},
    'NDT_OMP/7/1.0/centred/T_gt': {'count': 5810, 'score': 5.34e-08, 'gradient': 7.86e-08, 'H_float': 3.52e-08},
    'NDT_OMP/7/1.0/swapped/guess_inv': {'count': 2586, 'score': 4.14e-08, 'gradient': 5.57e-07, 'H_float': 6.6e-08},
    'NDT_OMP/7/1.0/head257/guess': {'count': 1583, 'score': 5.15e-08, 'gradient': 5.55e-08, 'H_float': 1.62e-08},
    'NDT_OMP/7/1.0/head1/guess': {'count': 7, 'score': 1.14e-07, 'gradient': 1.64e-07, 'H_float': 1.92e-07},
}


def tolerance(case: str, quantity: str) -> float:
    """min(MARGIN x the measured rounding noise of that quantity in that case, HB_RTOL)."""
    return min(MARGIN * NOISE_MEASURED[case][quantity], HB_RTOL)


# ---- derivative property ---------------------------------------------------------------------------------------------------------
# h = 1e-2: the kernels' compute_error is a sum of float terms, ~1e-7 relative, which a central difference divides by 2 h; at 1e-4 that
# rounding (1e-4 of |2 b| observed on an MI355X) hides the h^2 truncation term (3e-7), at 1e-2 it is 1e-6 against 1e-3
DERIV_H = 1e-2
DERIV_MEASURED = {'NDT_P2D/7/1.0/guess': 0.00274, 'NDT_P2D/7/1.0/T_gt': 0.000601, 'NDT_D2D/27/0.5/guess': 0.00186, 'NDT_D2D/27/0.5/T_gt': 0.000327, 'VGICP_CUDA/7/1.0/guess': 0.0007, 'VGICP_CUDA/7/1.0/T_gt': 6.82e-06}


def derivative_discrepancy(compute_error, T, b, extra, h=DERIV_H) -> float:
    """max_k |central difference of compute_error(exp(+-h e_k) T) - (2 b + extra)_k| / max |2 b|, correspondences and the linearisation
    pose frozen; extra: NdtReference.cauchy_gradient_term(), the part of the gradient that b leaves out by design."""
    g = np.array([(compute_error(left_step(T, h * np.eye(6)[k])) - compute_error(left_step(T, -h * np.eye(6)[k]))) / (2.0 * h) for k in range(6)])
    return float(np.abs(g - 2.0 * np.asarray(b) - np.asarray(extra)).max() / np.abs(2.0 * np.asarray(b)).max())
