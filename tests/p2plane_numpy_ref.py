"""An independent double-precision statement of the P2PLANE model and of the jueying_lio measurement model, in numpy / scipy only.

Written from the mathematics of jueying_lio's laser_mapping.cc:592-701 (ObsModel), ivox3d.h:132-235 and :283-286 (GetClosestPoint, the
nearby grids, Pos2Grid), ivox3d_node.hpp:140-205 (KNNPointByCondition) and common_lib.h:186-243 (esti_plane), not from the project's CPU
oracle or its kernels: nothing here imports `oracle` or the product, the search is brute force over the whole map, and the plane is
numpy.linalg.lstsq.  Everything runs in float64 on the float32 inputs widened exactly.

  voxel of a map point  round(p / res) per axis                                                      (Pos2Grid)
  query                 q = R p + t with the pose FIRST ROUNDED TO FLOAT32 -- the models cast the pose (R_wl, t_wl .cast<float>()), so
                        this is the definition, not an approximation -- then applied exactly
  candidates            the map points whose voxel v satisfies max |v - round(q / res)| <= 1 per axis and sum |v - round(q / res)| <= L:
                        L = 0 the centre (1 cell), 1 + the 6 faces (7), 2 + the 12 edges (19), 3 + the 8 corners (27);
                        kept when |c - q|^2 < max_range^2; the (up to) 5 nearest; m = how many; no plane when m < 3
  plane                 x = the least-squares solution of A x = -1 (A: the m neighbours, one per row), n = x / |x|, d = 1 / |x|;
                        rejected when any |n . p_j + d| > plane_threshold
  point test            selected when |p_body| > 81 e^2,  e = n . q + d
  linearize(T)          J = [(q x n)^T, n^T] (left perturbation, exp(delta) T),  H = sum J J^T,  b = sum J e,  cost = sum e^2,  count
  compute_error(T2)     sum e(T2)^2 over the selected set and the planes of the last linearize
  obs_model(state)      q from (rot, pos, off_R, off_T): the quaternion rot * off_R and the vector rot * off_T + pos rounded to float32,
                        q = v + 2 w (u x v) + 2 u x (u x v) + t (Eigen's quaternion * vector, which does not normalise); the same matcher;
                        h = -e; the 12-column row [n, point_this x C, p x (off_R^T C), C] with point_this = off_R p + off_T and
                        C = rot^T n, the last six columns zero unless extrinsic_est_en (laser_mapping.cc:674-698);
                        H^T H, H^T h, count, sum h^2.  converge = False: no new match, the stored planes at the new state, the point
                        test evaluated again.  DEFAULT (clean) SEMANTICS ONLY: PCM_FLAG_LIO_REFERENCE_SEMANTICS keeps residuals_ and
                        point_selected_surf_ across calls and frames; that mode is stateful and stays pinned to the CPU oracle alone
                        (tests/test_gpu_lio.py).

dtype = float32 is the reference's twin: every per-point quantity (transform, distances, lstsq on float32 input, residual, row) once
more in float32, the sums over the widened rows in float64.  It is never compared with a kernel: rel_err(Q32, Q64) is how far float
rounding alone moves that quantity on those inputs (NOISE_MEASURED), and a comparison's tolerance is min(MARGIN x that, cap), see
tolerance().

build_fixture() removes from a synth pair every point at which a correct float32 implementation may decide differently from an exact
one (scan_violations, cell_violations); nothing is masked in a comparison.  Margins left after removal: build_fixture().margins,
recorded in DESIGN.md section 5 with NOISE_MEASURED, MARGIN and the largest deviations of the CPU oracle and of an MI355X.

What these inputs cannot see (INVISIBLE): `<=` for `<` in the range test and `>=` for `>` in the threshold test differ from the
statement above only AT equality, which the removal rule keeps away by construction (tests/test_gpu_lattice.py owns exact ties); the
row order of the five neighbours, which no sum and no exact plane depends on (tests/test_gpu_reforder.py owns it); the visiting order of
the cells.
"""
from __future__ import annotations

import types

import numpy as np
from scipy.spatial.transform import Rotation

F32, F64 = np.float32, np.float64
EPS32 = 2.0 ** -24
KNN = 5
MIN_KNN = 3
LEVEL = {1: 0, 7: 1, 19: 2, 27: 3}       # largest sum |dv| of a neighbour cell: centre, faces, edges, corners
MUTATIONS = ("floor", "no_centre_26", "no_centre_18", "range_le", "threshold_ge", "nine", "n_cross_q", "d_is_norm", "min_knn_5", "h_plus")
INVISIBLE = {
    "range_le": "differs only where a squared distance EQUALS max_range^2; the fixture keeps every candidate range_slack away from it",
    "threshold_ge": "differs only where a neighbour's plane distance EQUALS the threshold; the fixture keeps every plane THRESHOLD_SLACK away from it",
    "neighbour_row_order": "no sum and no exact least-squares plane depends on the order of the five rows; tests/test_gpu_reforder.py owns it",
    "cell_visit_order": "the candidates are a set; the order in which the cells are visited only breaks exact ties (tests/test_gpu_lattice.py)",
}


def rel_err(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def widen(cloud) -> np.ndarray:
    """(N, 3) float64 of an (N, >= 3) float32 cloud, exactly."""
    a = np.asarray(cloud)
    assert a.dtype == F32 and a.ndim == 2 and a.shape[1] >= 3
    return a[:, :3].astype(F64)


# ---- poses and states ------------------------------------------------------------------------------------------------------------
def skew(v):
    """(3, 3) with skew(v) w = v x w."""
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_exp(w) -> np.ndarray:
    w = np.asarray(w, F64)
    th = float(np.linalg.norm(w))
    if th < 1e-300:
        return np.eye(3)
    K = skew(w / th)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def left_step(T, d) -> np.ndarray:
    """delta * T with delta.linear = exp(d[:3]), delta.translation = d[3:]: how lsq_registration_impl.hpp applies a step."""
    D = np.eye(4)
    D[:3, :3] = so3_exp(d[:3])
    D[:3, 3] = d[3:]
    return D @ np.asarray(T, F64)


def shifted(T) -> np.ndarray:
    T2 = np.array(T, F64)
    T2[:3, 3] += SHIFT
    return T2


def round32(a) -> np.ndarray:
    return np.asarray(a, F64).astype(F32).astype(F64)


def quat_matrix(q_xyzw) -> np.ndarray:
    """The matrix of v -> v + 2 w (u x v) + 2 u x (u x v), q = (u, w) as given (NOT normalised: Eigen's quaternion * vector)."""
    u, w = np.asarray(q_xyzw[:3], F64), float(q_xyzw[3])
    K = skew(u)
    return np.eye(3) + 2.0 * w * K + 2.0 * (K @ K)


def lio_state(T_wl, off_rpy=(0.01, -0.02, 0.03), off_t=(0.1713, 0.0, 0.05925)):
    """(rot xyzw, pos, off_R xyzw, off_T) of the IMU state whose lidar pose is T_wl under the extrinsic (off_rpy, off_t)."""
    off = Rotation.from_euler("xyz", off_rpy)
    Til = np.eye(4); Til[:3, :3] = off.as_matrix(); Til[:3, 3] = off_t
    Twi = np.asarray(T_wl, F64) @ np.linalg.inv(Til)
    return Rotation.from_matrix(Twi[:3, :3]).as_quat(), Twi[:3, 3].copy(), off.as_quat(), np.asarray(off_t, F64)


def lio_world_pose(rot, pos, off_R, off_T, exact=False):
    """(R_wl, t_wl) of a state: rot * off_R and rot * off_T + pos, rounded to float32 as a quaternion and a vector (:602-603)."""
    r, o = Rotation.from_quat(rot), Rotation.from_quat(off_R)
    q = (r * o).as_quat()
    t = r.apply(np.asarray(off_T, F64)) + np.asarray(pos, F64)
    if exact:
        return (r * o).as_matrix(), t
    return quat_matrix(round32(q)), round32(t)


# ---- the matcher -----------------------------------------------------------------------------------------------------------------
def voxel_coords(x, res, mutation=None) -> np.ndarray:
    """(N, 3) int32 round(x / res); x in float64 or float32 (the twin)."""
    u = x / x.dtype.type(res)
    return (np.floor(u) if mutation == "floor" else np.round(u)).astype(np.int32)


_geometry = {}


def fit_plane(P, dtype, mutation=None):
    """(plane (4,), largest |n . p_j + d|) of the rows P (m, 3), in dtype."""
    A = np.ascontiguousarray(P, dtype)
    x = np.linalg.lstsq(A, -np.ones(len(A), dtype), rcond=None)[0].astype(dtype)
    nrm = np.sqrt((x * x).sum(dtype=dtype))
    n = x / nrm
    d = nrm if mutation == "d_is_norm" else dtype(1.0) / nrm
    return np.append(n, d).astype(dtype), float(np.abs(A @ n + d).max())


class Reference:
    """jueying_lio's matcher under LsqRegistration::linearize / compute_error and under ObsModel, on a scan and a target."""

    def __init__(self, scan, target, *, voxel_resolution=0.5, num_neighbors=27, max_range=5.0, plane_threshold=0.1, dtype=F64, mutation=None):
        assert mutation in (None,) + MUTATIONS and num_neighbors in LEVEL and dtype in (F32, F64)
        self.res, self.nn, self.max_range, self.threshold = float(voxel_resolution), int(num_neighbors), float(max_range), float(plane_threshold)
        self.dtype, self.mutation = dtype, mutation
        self.src32 = np.ascontiguousarray(np.asarray(scan)[:, :3])
        self.tgt32 = np.ascontiguousarray(np.asarray(target)[:, :3])
        assert self.src32.dtype == F32 and self.tgt32.dtype == F32
        self.src, self.tgt = self.src32.astype(dtype), self.tgt32.astype(dtype)
        self.vt = voxel_coords(self.tgt, self.res, mutation)
        self.pn = np.sqrt((self.src * self.src).sum(axis=1, dtype=dtype))          # |p_body|
        self.found = None

    def transform(self, R, t):
        """R p + t in dtype (float64: exactly the definition; float32: what a float implementation computes)."""
        R, t = np.asarray(R, self.dtype), np.asarray(t, self.dtype)
        return (self.src[:, None, :] * R[None, :, :]).sum(axis=2, dtype=self.dtype) + t

    def geometry(self, q):
        """(d2 (N, M) squared distances in dtype, level (N, M) the sum |dv| of the map point's voxel about the query's, 99 = outside the 27)."""
        key = (q.dtype.str, hash(q.tobytes()), hash(self.tgt.tobytes()), self.res, self.mutation == "floor")
        if key not in _geometry:
            if len(_geometry) >= 4:
                _geometry.clear()
            d = self.tgt[None, :, :] - q[:, None, :]
            D = np.abs(self.vt[None, :, :] - voxel_coords(q, self.res, self.mutation)[:, None, :])
            _geometry[key] = ((d * d).sum(axis=2, dtype=self.dtype), np.where(D.max(axis=2) <= 1, D.sum(axis=2), 99).astype(np.int8))
        return _geometry[key]

    def in_cells(self, level):
        """(N, M) bool: the map point's voxel is one of the nn cells -- centre (level 0), faces (1), edges (2), corners (3)."""
        ok = level <= LEVEL[self.nn]
        if (self.mutation == "no_centre_26" and self.nn == 27) or (self.mutation == "no_centre_18" and self.nn == 19):
            ok &= level > 0
        return ok

    def search(self, q):
        """The (up to) 6 nearest kept candidates of every query: (idx (N, 6), -1 = none; d2 (N, 6), inf = none; m (N,) = min(kept, 5))."""
        d2, level = self.geometry(q)
        r2 = self.max_range * self.max_range
        kept = self.in_cells(level) & ((d2 <= r2) if self.mutation == "range_le" else (d2 < r2))
        d2 = np.where(kept, d2, np.inf)
        idx = np.argsort(d2, axis=1, kind="stable")[:, :KNN + 1]
        d2 = np.take_along_axis(d2, idx, 1)
        idx = np.where(np.isfinite(d2), idx, -1)
        if idx.shape[1] < KNN + 1:
            pad = KNN + 1 - idx.shape[1]
            idx, d2 = np.pad(idx, ((0, 0), (0, pad)), constant_values=-1), np.pad(d2, ((0, 0), (0, pad)), constant_values=np.inf)
        return idx, d2, np.minimum(kept.sum(axis=1), KNN)

    def match(self, q):
        """Neighbours and planes of the queries q: namespace(idx, d2, m, plane (N, 4) NaN = none, residual (N,) the largest neighbour
        distance from the plane, NaN when m < min_knn, ok (N,))."""
        idx, d2, m = self.search(q)
        n = len(q)
        plane, residual, ok = np.full((n, 4), np.nan, self.dtype), np.full(n, np.nan), np.zeros(n, bool)
        min_knn = KNN if self.mutation == "min_knn_5" else MIN_KNN
        for i in np.nonzero(m >= min_knn)[0]:
            pl, r = fit_plane(self.tgt[idx[i, :m[i]]], self.dtype, self.mutation)
            residual[i] = r
            if (r >= self.threshold) if self.mutation == "threshold_ge" else (r > self.threshold):
                continue
            plane[i], ok[i] = pl, True
        self.found = types.SimpleNamespace(idx=idx, d2=d2, m=m, plane=plane, residual=residual, ok=ok)
        return self.found

    def residuals(self, q):
        """(e (N,), valid (N,)) of the stored planes at the queries q: e = n . q + d, valid = plane & |p_body| > 81 e^2."""
        f = self.found
        pl = np.where(f.ok[:, None], f.plane, 0).astype(self.dtype)
        e = (pl[:, :3] * q).sum(axis=1, dtype=self.dtype) + pl[:, 3]
        k = self.dtype(9.0 if self.mutation == "nine" else 81.0)
        return e, f.ok & (self.pn > k * e * e)

    # -- LsqRegistration ------------------------------------------------------------------------------------------------------------
    def rows(self, q, sel):
        n = self.found.plane[sel, :3]
        qs = q[sel]
        c = np.cross(n, qs) if self.mutation == "n_cross_q" else np.cross(qs, n)
        return np.concatenate([c.astype(self.dtype), n], axis=1)

    def linearize(self, T):
        """(cost, H (6, 6), b (6,), count) at the pose T; the selected set and the planes are remembered for compute_error."""
        Tf = round32(T)
        q = self.transform(Tf[:3, :3], Tf[:3, 3])
        self.match(q)
        e, sel = self.residuals(q)
        self.selected, self.q = sel, q
        J, e = self.rows(q, sel).astype(F64), e[sel].astype(F64)
        return float(e @ e), J.T @ J, J.T @ e, int(sel.sum())

    def planes(self) -> np.ndarray:
        """(N, 4) the planes of the selected points of the last linearize, NaN rows elsewhere (what get_planes returns)."""
        return np.where(self.selected[:, None], self.found.plane, np.nan)

    def compute_error(self, T2, exact=False) -> float:
        """sum e(T2)^2 over the selected set and planes of the last linearize; exact: the pose is not rounded (for derivatives)."""
        Tf = np.asarray(T2, F64) if exact else round32(T2)
        q = self.transform(Tf[:3, :3], Tf[:3, 3])
        pl = self.found.plane[self.selected]
        e = ((pl[:, :3] * q[self.selected]).sum(axis=1, dtype=self.dtype) + pl[:, 3]).astype(F64)
        return float(e @ e)

    # -- ObsModel -------------------------------------------------------------------------------------------------------------------
    def lio_rows(self, sel, rot, off_R, off_T, extrinsic_est_en, exact=False):
        """(k, 12) rows of the selected points (laser_mapping.cc:670-694)."""
        cast = (lambda a: np.asarray(a, F64)) if exact else round32
        dt = self.dtype
        oR = cast(Rotation.from_quat(off_R).as_matrix()).astype(dt)
        ot = cast(off_T).astype(dt)
        Rt = cast(Rotation.from_quat(rot).as_matrix().T).astype(dt)
        p, n = self.src[sel], self.found.plane[sel, :3]
        mv = lambda M, v: (v[:, None, :] * M[None, :, :]).sum(axis=2, dtype=dt)
        point_this = mv(oR, p) + ot
        Cv = mv(Rt, n)
        A = np.cross(point_this, Cv).astype(dt)
        out = np.zeros((len(p), 12), dt)
        out[:, 0:3], out[:, 3:6] = n, A
        if extrinsic_est_en:
            out[:, 6:9], out[:, 9:12] = np.cross(p, mv(oR.T, Cv)).astype(dt), Cv
        return out

    def obs_model(self, rot, pos, off_R, off_T, extrinsic_est_en=False, converge=True):
        """(H^T H (12, 12), H^T h (12,), count, sum h^2) at the state."""
        R, t = lio_world_pose(rot, pos, off_R, off_T)
        q = self.transform(R, t)
        if converge:
            self.match(q)
        e, sel = self.residuals(q)
        self.selected, self.q = sel, q
        Hx = self.lio_rows(sel, rot, off_R, off_T, extrinsic_est_en).astype(F64)
        h = e[sel].astype(F64) * (1.0 if self.mutation == "h_plus" else -1.0)
        return Hx.T @ Hx, Hx.T @ h, int(sel.sum()), float(h @ h)

    def lio_residual(self, rot, pos, off_R, off_T):
        """(k,) e of the selected points at an unrounded state, planes and set frozen: the function the 12 columns differentiate."""
        R, t = lio_world_pose(rot, pos, off_R, off_T, exact=True)
        pl = self.found.plane[self.selected].astype(F64)
        return (pl[:, :3] * (self.src[self.selected].astype(F64) @ R.T + t)).sum(axis=1) + pl[:, 3]


# ---- preconditions ---------------------------------------------------------------------------------------------------------------
CELL_SLACK = 4.0           # x the float32 evaluation error of the coordinate
THRESHOLD_SLACK = 1e-4     # absolute, of max |n . p_j + d| to plane_threshold: n . p + d evaluated in float32 on coordinates of up to 64 m is
                           # off by ~4 x 2^-24 x 64 = 1.5e-5, and a backward-stable float fit moves the residuals by as much again
POINT_TEST_SLACK = 1e-3    # relative, of |p_body| - 81 e^2 to 0: d(81 e^2) / |p| = 18 de / sqrt|p| at the boundary; de ~ 3e-5, |p| >= 1 m -> 5e-4


def coordinate_error(R, t, x):
    """(N,) the order of the float32 evaluation error of a coordinate of R p + t: one ulp of its largest term, 2^-23 (|R| |p| + |t|)."""
    return 2.0 * EPS32 * (np.abs(x) @ np.abs(np.asarray(R, F64)).T + np.abs(np.asarray(t, F64))).max(axis=1)


def range_slack(d2, u):
    """The absolute float32 error of a squared distance d2 between coordinates known to u, times 4: the three differences are off by u
    each, so d2 by 2 sqrt(3 d2) u, and the squares and sums add 3 x 2^-24 d2."""
    return 4.0 * (2.0 * np.sqrt(3.0 * d2) * u + 3.0 * EPS32 * d2)


def cell_violations(x, res, u):
    """Rows of x (N, 3) with a coordinate within CELL_SLACK u of a cell boundary (k + 1/2) res."""
    w = x / res - 0.5
    return np.nonzero((np.abs(w - np.round(w)) * res <= CELL_SLACK * np.reshape(u, (-1, 1))).any(axis=1))[0]


def scan_violations(scan, target, T, res, nn, max_range, margins=None):
    """Scan rows at which a float32 implementation may decide differently from the exact one at the pose T (and at shifted(T), where
    compute_error and a converge = False call evaluate the point test again)."""
    r = Reference(scan, target, voxel_resolution=res, num_neighbors=nn, max_range=max_range)
    Tf = round32(T)
    q = r.transform(Tf[:3, :3], Tf[:3, 3])
    u = np.maximum(coordinate_error(Tf[:3, :3], Tf[:3, 3], r.src), 2.0 * EPS32 * np.abs(r.tgt).max())
    bad = set(cell_violations(q, res, u))
    f = r.match(q)
    has6 = np.isfinite(f.d2[:, KNN])
    gap = np.where(has6, f.d2[:, KNN] - np.where(has6, f.d2[:, KNN - 1], 0.0), np.inf)
    gap_slack = range_slack(np.where(has6, f.d2[:, KNN], 0.0), u)
    bad.update(np.nonzero(gap <= gap_slack)[0])
    # every candidate in the cells, kept or not, against the range
    d2, level = r.geometry(q)
    d2 = np.where(r.in_cells(level), d2, np.inf)
    r2 = max_range * max_range
    near = np.abs(d2 - r2) <= range_slack(np.where(np.isfinite(d2), d2, 0.0), u[:, None])
    bad.update(np.nonzero(near.any(axis=1))[0])
    thr = np.abs(f.residual - r.threshold)
    bad.update(np.nonzero(thr <= THRESHOLD_SLACK)[0])
    pt = []
    for Tx in (Tf, round32(shifted(T))):
        e, _ = r.residuals(r.transform(Tx[:3, :3], Tx[:3, 3]))
        rel = np.where(f.ok, np.abs(r.pn - 81.0 * e * e) / r.pn, np.inf)
        bad.update(np.nonzero(rel <= POINT_TEST_SLACK)[0])
        pt.append(rel.min())
    if margins is not None:
        w = q / res - 0.5
        margins.append(dict(cell=float((np.abs(w - np.round(w)) * res / u[:, None]).min()), knn_gap=float((gap / np.maximum(gap_slack, 1e-300)).min()),
                            range=float((np.abs(d2 - r2) / np.maximum(range_slack(np.where(np.isfinite(d2), d2, 0.0), u[:, None]), 1e-300)).min()),
                            threshold=float(np.nanmin(thr)) if np.isfinite(thr).any() else np.inf, point_test=float(min(pt))))
    return np.array(sorted(bad), np.int64)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
PAIR = (3, 600, 3000)
RESOLUTIONS = (0.5, 0.25)
NEIGHBOURS = (1, 7, 19, 27)
MAX_RANGE = 5.0
BINDING_RANGE = 0.3                       # at 0.5 m: some queries lose candidates, some drop below 5 and below 3
SHIFT = np.array([0.02, -0.01, 0.01])
REMOVED_CAP = 0.01
_fixtures = {}


FAR = np.array([0.01, -0.015, 0.02, 0.08, -0.06, 0.05])     # the centred fixture's poses: left_step(guess, FAR), left_step(T_gt, -FAR)


def search_cases(centred=False):
    """(res, nn, max_range) of every search a fixture is used with."""
    if centred:
        return [(res, 27, MAX_RANGE) for res in RESOLUTIONS]
    return [(res, nn, MAX_RANGE) for res in RESOLUTIONS for nn in NEIGHBOURS] + [(0.5, nn, BINDING_RANGE) for nn in (7, 27)]


def all_violations(scan, submap, poses, cases, margins=None):
    bad_m = set()
    for res in RESOLUTIONS:
        bad_m.update(cell_violations(widen(submap), res, 2.0 * EPS32 * np.abs(widen(submap)).max(axis=1)))
    bad_s = set()
    for T in poses:
        for res, nn, rng in cases:
            bad_s.update(scan_violations(scan, submap, T, res, nn, rng, margins))
    return np.array(sorted(bad_s), np.int64), np.array(sorted(bad_m), np.int64)


def build_fixture(synth, centred=False):
    """synth.make_pair(3, 600, 3000) less the points that violate a precondition in any search case at the fixture's poses: guess and T_gt.
    centred: the map and the poses moved by the map's centroid, so that voxel coordinates take both signs, and the poses stepped away
    from the optimum by FAR (why: DESIGN.md section 5 -- about the centroid b has no lever arm, at guess and T_gt it is a cancelled sum
    of magnitude 4 ... 10, and the float plane fit's rounding alone moves it by 1.2e-5 and 2.6e-5 of that: not a well-posed quantity at
    HB_RTOL).  At most three rounds; the result has no violation and at most 1 % of either cloud removed, or this raises.  The margins
    left are those of the last, clean round: cell, knn_gap and range in units of their slack (> 1), threshold absolute
    (> THRESHOLD_SLACK), point_test relative (> POINT_TEST_SLACK)."""
    if centred not in _fixtures:
        p = synth.make_pair(*PAIR)
        scan, submap = p.scan.copy(), p.submap.copy()
        guess, T_gt = p.guess.astype(F64), p.T_gt.copy()
        names = ("guess", "T_gt")
        if centred:
            c = widen(submap).mean(axis=0)
            submap[:, :3] = (widen(submap) - c).astype(F32)
            guess[:3, 3] -= c
            T_gt[:3, 3] -= c
            guess, T_gt, names = left_step(guess, FAR), left_step(T_gt, -FAR), ("far", "far_back")
        n_scan, n_map = len(scan), len(submap)
        poses, cases = (guess, T_gt), search_cases(centred)
        rounds = []
        for _ in range(4):
            rows = []
            bad_s, bad_m = all_violations(scan, submap, poses, cases, rows)
            rounds.append((len(bad_s), len(bad_m)))
            if not len(bad_s) and not len(bad_m):
                break
            scan, submap = np.delete(scan, bad_s, axis=0), np.delete(submap, bad_m, axis=0)
        if rounds[-1] != (0, 0):
            raise AssertionError("violations left after three rounds: %r" % (rounds,))
        removed = (n_scan - len(scan), n_map - len(submap))
        if removed[0] > REMOVED_CAP * n_scan or removed[1] > REMOVED_CAP * n_map:
            raise AssertionError("more than 1 %% of a cloud removed: %r" % (removed,))
        for a in (scan, submap, guess, T_gt):
            a.setflags(write=False)
        _fixtures[centred] = types.SimpleNamespace(scan=scan, submap=submap, guess=guess, T_gt=T_gt, poses=dict(zip(names, poses)), cases=cases,
                                                   removed_scan=removed[0], removed_map=removed[1], rounds=rounds[:-1],
                                                   margins={k: min(r[k] for r in rows) for k in rows[0]})
    return _fixtures[centred]


def assert_both_signs(fx):
    """The centred fixture: the map's voxel coordinates take both signs on every axis; the scan's cells at the poses (one corner of the
    map) are negative somewhere on every axis and straddle zero on at least one."""
    for res in RESOLUTIONS:
        c = voxel_coords(widen(fx.submap), res)
        assert (c.min(axis=0) < 0).all() and (c.max(axis=0) > 0).all(), (res, c.min(axis=0), c.max(axis=0))
        for T in fx.poses.values():
            Tf = round32(T)
            c = voxel_coords(widen(fx.scan) @ Tf[:3, :3].T + Tf[:3, 3], res)
            assert (c.min(axis=0) < 0).all() and ((c.min(axis=0) < 0) & (c.max(axis=0) > 0)).any(), (res, c.min(axis=0), c.max(axis=0))


# ---- cases -----------------------------------------------------------------------------------------------------------------------
_inputs = {}


def lone_voxel_target(submap, res=0.25):
    """The map points that are alone in their voxel."""
    v = voxel_coords(widen(submap), res)
    _, inv, cnt = np.unique(v, axis=0, return_inverse=True, return_counts=True)
    return submap[cnt[inv.reshape(-1)] == 1]


def case_inputs(synth, variant="main"):
    """namespace(scan, target, poses {name: T}, fx) of a variant: main, centred, head1 / head255 / head257 (scan heads against the whole
    map), lone (the target made of the map points alone in their 0.25 m voxel; the scan less the points that violate a precondition
    against THAT target, at most 1 %), empty (64 scan points and one whose 27 cells are all empty)."""
    if variant not in _inputs:
        fx = build_fixture(synth, centred=variant == "centred")
        scan, target, poses = fx.scan, fx.submap, dict(fx.poses)
        if variant.startswith("head"):
            scan, poses = fx.scan[:int(variant[4:])], {"guess": fx.guess}
        elif variant == "lone":
            target, poses = lone_voxel_target(fx.submap), {"guess": fx.guess}
            bad = scan_violations(scan, target, fx.guess, 0.25, 27, MAX_RANGE)
            assert len(bad) <= REMOVED_CAP * len(scan), len(bad)
            scan = np.delete(scan, bad, axis=0)
            assert len(scan_violations(scan, target, fx.guess, 0.25, 27, MAX_RANGE)) == 0
        elif variant == "empty":
            far_world = widen(fx.submap).max(axis=0) + np.array([7.3, 5.2, 9.1])
            far = np.linalg.inv(round32(fx.guess)) @ np.append(far_world, 1.0)
            scan = np.concatenate([fx.scan[:64], fx.scan[:1]])
            scan[64, :3] = far[:3].astype(F32)
            poses = {"guess": fx.guess}
        _inputs[variant] = types.SimpleNamespace(scan=scan, target=target, poses=poses, fx=fx)
    return _inputs[variant]


# (variant, res, nn, max_range)
CASES = ([("main", res, nn, MAX_RANGE) for res in RESOLUTIONS for nn in NEIGHBOURS]
         + [("centred", res, 27, MAX_RANGE) for res in RESOLUTIONS]      # at the poses far and far_back
         + [("main", 0.5, nn, BINDING_RANGE) for nn in (7, 27)]
         + [("head1", 0.5, 27, MAX_RANGE), ("head255", 0.5, 27, MAX_RANGE), ("head257", 0.5, 27, MAX_RANGE), ("head257", 0.25, 27, MAX_RANGE),
            ("lone", 0.25, 27, MAX_RANGE), ("empty", 0.5, 27, MAX_RANGE)])
LIO_CASES = [(res, ext) for res in RESOLUTIONS for ext in (False, True)]
LIO_STEPS = (("guess", False, True), ("guess", True, False), ("T_gt", False, True))      # (pose, shifted, converge): True, False, True


def case_name(variant, res, nn, max_range, pose=None):
    s = "%s/%.2f/%d" % (variant, res, nn) + ("" if max_range == MAX_RANGE else "/r%.1f" % max_range)
    return s if pose is None else s + "/" + pose


def lio_case_name(res, ext, step=None):
    s = "lio/%.2f/ext%d" % (res, int(ext))
    return s if step is None else s + "/step%d" % step


def make_reference(ci, res, nn, max_range, dtype=F64, mutation=None):
    return Reference(ci.scan, ci.target, voxel_resolution=res, num_neighbors=nn, max_range=max_range, dtype=dtype, mutation=mutation)


def plane_deviation(got, want) -> float:
    """The largest per-point max |got - want| / max |want| over the rows of want that hold a plane (the masks are compared apart)."""
    ok = ~np.isnan(want[:, 0])
    if not ok.any():
        return 0.0
    g, w = np.asarray(got, F64)[ok], np.asarray(want, F64)[ok]
    return float((np.abs(g - w).max(axis=1) / np.abs(w).max(axis=1)).max())


def measure(ci, res, nn, max_range, T):
    """({quantity: (Q64, Q32)}, count, r64) at T and shifted(T); the twin's decisions equal the exact ones, or the fixture is wrong."""
    r64, r32 = make_reference(ci, res, nn, max_range, F64), make_reference(ci, res, nn, max_range, F32)
    a, b = r64.linearize(T), r32.linearize(T)
    assert a[3] == b[3] and np.array_equal(r64.selected, r32.selected) and np.array_equal(r64.found.m, r32.found.m)
    assert np.array_equal(np.sort(r64.found.idx[:, :KNN], axis=1), np.sort(r32.found.idx[:, :KNN], axis=1))
    out = {"planes": (r64.planes(), r32.planes()), "cost": (a[0], b[0]), "H": (a[1], b[1]), "b": (a[2], b[2]),
           "compute_error": (r64.compute_error(shifted(T)), r32.compute_error(shifted(T)))}
    return out, a[3], r64


def lio_states(ci):
    """The states of LIO_STEPS."""
    return [lio_state(shifted(ci.poses[pose]) if shift else ci.poses[pose]) for pose, shift, _ in LIO_STEPS]


def measure_lio(ci, res, ext):
    """[({quantity: (Q64, Q32)}, count)] over LIO_STEPS, the two references carried through the sequence."""
    r64, r32 = make_reference(ci, res, 27, MAX_RANGE, F64), make_reference(ci, res, 27, MAX_RANGE, F32)
    out = []
    for st, (_, _, conv) in zip(lio_states(ci), LIO_STEPS):
        a, b = r64.obs_model(*st, ext, conv), r32.obs_model(*st, ext, conv)
        assert a[2] == b[2] and np.array_equal(r64.selected, r32.selected)
        out.append(({"HTH": (a[0], b[0]), "HTh": (a[1], b[1]), "sum_h2": (a[3], b[3])}, a[2]))
    return out


def deviation(got, want, quantity) -> float:
    if quantity == "planes":
        return plane_deviation(got, want)
    return abs(got - want) / max(abs(want), 1e-300) if np.ndim(want) == 0 else rel_err(got, want)


def noise_of(pairs):
    return {k: deviation(b, a, k) for k, (a, b) in pairs.items()}


# ---- tolerances ------------------------------------------------------------------------------------------------------------------
HB_RTOL = 1e-5        # tests/helpers.py: the bar the kernels are held to against the oracle; the cap of every sum
# Chosen once from tests/test_p2plane_numpy_ref.py::test_oracle_*: the CPU oracle fits the plane of 5 neighbours in float32 (Householder QR, as
# esti_plane<float> does), the twin only rounds a double solution, so the oracle is 3.4e-6 ... 2.2e-5 from the reference on plane
# coefficients where the twin's noise is 1e-7: with MARGIN = 4 x the largest ratio every tolerance below is its cap
ORACLE_RATIO_MEASURED = 259.99      # empty/0.50/27/guess planes
MARGIN = max(4.0, 4.0 * ORACLE_RATIO_MEASURED)
ORACLE_PLANE_DEVIATION_MEASURED = 2.22e-5      # main/0.50/19/guess: the largest oracle-against-reference plane deviation on the CPU
PLANE_CAP = 4.0 * ORACLE_PLANE_DEVIATION_MEASURED
NOISE_MEASURED = {
    'main/0.50/1/guess': {'count': 151, 'planes': 7.9e-08, 'cost': 1.94e-07, 'H': 5.1e-08, 'b': 5.23e-07, 'compute_error': 3.31e-07},
    'main/0.50/1/T_gt': {'count': 126, 'planes': 7.9e-08, 'cost': 5.25e-07, 'H': 2.51e-08, 'b': 1.77e-06, 'compute_error': 8.35e-07},
    'main/0.50/7/guess': {'count': 517, 'planes': 1.13e-07, 'cost': 6.44e-07, 'H': 2.48e-08, 'b': 1.4e-06, 'compute_error': 6.16e-07},
    'main/0.50/7/T_gt': {'count': 511, 'planes': 1.13e-07, 'cost': 8.19e-07, 'H': 1.16e-08, 'b': 3.71e-06, 'compute_error': 1.46e-06},
    'main/0.50/19/guess': {'count': 467, 'planes': 1.07e-07, 'cost': 4.11e-07, 'H': 3.84e-09, 'b': 7.97e-07, 'compute_error': 8.23e-07},
    'main/0.50/19/T_gt': {'count': 451, 'planes': 1.07e-07, 'cost': 1.19e-06, 'H': 5.9e-09, 'b': 5.45e-07, 'compute_error': 1.19e-06},
    'main/0.50/27/guess': {'count': 464, 'planes': 1.07e-07, 'cost': 3.77e-07, 'H': 4.15e-09, 'b': 7.45e-07, 'compute_error': 7.82e-07},
    'main/0.50/27/T_gt': {'count': 449, 'planes': 1.07e-07, 'cost': 1.04e-06, 'H': 6.31e-09, 'b': 4.6e-07, 'compute_error': 1e-06},
    'main/0.25/1/guess': {'count': 0, 'planes': 0.0, 'cost': 0.0, 'H': 0.0, 'b': 0.0, 'compute_error': 0.0},
    'main/0.25/1/T_gt': {'count': 0, 'planes': 0.0, 'cost': 0.0, 'H': 0.0, 'b': 0.0, 'compute_error': 0.0},
    'main/0.25/7/guess': {'count': 216, 'planes': 9.28e-08, 'cost': 3.8e-07, 'H': 2.87e-08, 'b': 2.13e-06, 'compute_error': 3.15e-07},
    'main/0.25/7/T_gt': {'count': 202, 'planes': 9.28e-08, 'cost': 1.29e-06, 'H': 3.55e-08, 'b': 6.93e-06, 'compute_error': 8.54e-07},
    'main/0.25/19/guess': {'count': 384, 'planes': 8.71e-08, 'cost': 1e-06, 'H': 3.92e-09, 'b': 7.54e-07, 'compute_error': 1.18e-06},
    'main/0.25/19/T_gt': {'count': 407, 'planes': 8.71e-08, 'cost': 9.25e-07, 'H': 1.23e-08, 'b': 6.09e-07, 'compute_error': 8.88e-07},
    'main/0.25/27/guess': {'count': 385, 'planes': 8.71e-08, 'cost': 1.31e-06, 'H': 2.25e-09, 'b': 5.92e-07, 'compute_error': 1.41e-06},
    'main/0.25/27/T_gt': {'count': 403, 'planes': 8.71e-08, 'cost': 9.94e-07, 'H': 9.18e-09, 'b': 9.18e-07, 'compute_error': 8.41e-07},
    'centred/0.50/27/far': {'count': 522, 'planes': 1.15e-07, 'cost': 9.51e-07, 'H': 9.05e-09, 'b': 6.63e-07, 'compute_error': 8.8e-07},
    'centred/0.50/27/far_back': {'count': 543, 'planes': 1.15e-07, 'cost': 8.81e-07, 'H': 1.14e-08, 'b': 6.78e-07, 'compute_error': 8.41e-08},
    'centred/0.25/27/far': {'count': 412, 'planes': 9.59e-08, 'cost': 1.49e-06, 'H': 8.94e-09, 'b': 1.04e-06, 'compute_error': 7.16e-07},
    'centred/0.25/27/far_back': {'count': 462, 'planes': 9.59e-08, 'cost': 3.63e-07, 'H': 7.47e-09, 'b': 4.35e-07, 'compute_error': 4.06e-07},
    'main/0.50/7/r0.3/guess': {'count': 151, 'planes': 1.07e-07, 'cost': 4.65e-07, 'H': 1.07e-08, 'b': 1.19e-06, 'compute_error': 8.87e-09},
    'main/0.50/7/r0.3/T_gt': {'count': 147, 'planes': 9.38e-08, 'cost': 1.14e-07, 'H': 1.85e-08, 'b': 3.3e-06, 'compute_error': 7.94e-07},
    'main/0.50/27/r0.3/guess': {'count': 175, 'planes': 1.26e-07, 'cost': 7.5e-07, 'H': 1.53e-08, 'b': 1.52e-06, 'compute_error': 7.08e-08},
    'main/0.50/27/r0.3/T_gt': {'count': 164, 'planes': 1.26e-07, 'cost': 3.67e-07, 'H': 1.12e-08, 'b': 5.33e-06, 'compute_error': 5.96e-07},
    'head1/0.50/27/guess': {'count': 1, 'planes': 2.37e-08, 'cost': 3.93e-07, 'H': 5.67e-08, 'b': 1.68e-07, 'compute_error': 8.96e-07},
    'head255/0.50/27/guess': {'count': 177, 'planes': 1.07e-07, 'cost': 2.2e-07, 'H': 1.7e-08, 'b': 4.68e-07, 'compute_error': 6.21e-07},
    'head257/0.50/27/guess': {'count': 179, 'planes': 1.07e-07, 'cost': 2.06e-07, 'H': 1.71e-08, 'b': 5.89e-07, 'compute_error': 6.09e-07},
    'head257/0.25/27/guess': {'count': 168, 'planes': 8.71e-08, 'cost': 1.61e-06, 'H': 2.59e-09, 'b': 1.03e-06, 'compute_error': 1.72e-06},
    'lone/0.25/27/guess': {'count': 261, 'planes': 8.88e-08, 'cost': 1.49e-07, 'H': 1.68e-08, 'b': 9.65e-07, 'compute_error': 5.13e-07},
    'empty/0.50/27/guess': {'count': 48, 'planes': 8.53e-08, 'cost': 2.96e-07, 'H': 2.84e-08, 'b': 2.71e-06, 'compute_error': 6.88e-07},
    'lio/0.50/ext0/step0': {'count': 464, 'HTH': 6.19e-08, 'HTh': 2.51e-06, 'sum_h2': 6.98e-07},
    'lio/0.50/ext0/step1': {'count': 464, 'HTH': 6.27e-08, 'HTh': 2.09e-06, 'sum_h2': 1.16e-06},
    'lio/0.50/ext0/step2': {'count': 449, 'HTH': 6.56e-08, 'HTh': 1.32e-05, 'sum_h2': 1.01e-06},
    'lio/0.50/ext1/step0': {'count': 464, 'HTH': 6.19e-08, 'HTh': 2.46e-06, 'sum_h2': 6.98e-07},
    'lio/0.50/ext1/step1': {'count': 464, 'HTH': 6.27e-08, 'HTh': 2.09e-06, 'sum_h2': 1.16e-06},
    'lio/0.50/ext1/step2': {'count': 449, 'HTH': 6.56e-08, 'HTh': 1.32e-05, 'sum_h2': 1.01e-06},
    'lio/0.25/ext0/step0': {'count': 385, 'HTH': 7.56e-08, 'HTh': 2.11e-06, 'sum_h2': 1.34e-06},
    'lio/0.25/ext0/step1': {'count': 384, 'HTH': 7.55e-08, 'HTh': 1.64e-06, 'sum_h2': 1.9e-06},
    'lio/0.25/ext0/step2': {'count': 403, 'HTH': 7.72e-08, 'HTh': 7.52e-06, 'sum_h2': 6.25e-07},
    'lio/0.25/ext1/step0': {'count': 385, 'HTH': 7.56e-08, 'HTh': 2.11e-06, 'sum_h2': 1.34e-06},
    'lio/0.25/ext1/step1': {'count': 384, 'HTH': 7.55e-08, 'HTh': 1.64e-06, 'sum_h2': 1.9e-06},
    'lio/0.25/ext1/step2': {'count': 403, 'HTH': 7.72e-08, 'HTh': 7.5e-06, 'sum_h2': 6.25e-07},
}


def tolerance(case: str, quantity: str) -> float:
    """min(MARGIN x the measured rounding noise of that quantity in that case, the cap): HB_RTOL for the sums, PLANE_CAP for planes."""
    return min(MARGIN * NOISE_MEASURED[case][quantity], PLANE_CAP if quantity == "planes" else HB_RTOL)


# ---- derivative property ---------------------------------------------------------------------------------------------------------
DERIV_H = 1e-4


def derivative_discrepancy(compute_error, T, b, h=DERIV_H) -> float:
    """max_k |central difference of compute_error(exp(+-h e_k) T) - 2 b_k| / max |2 b|, selected set and planes frozen."""
    g = np.array([(compute_error(left_step(T, h * np.eye(6)[k])) - compute_error(left_step(T, -h * np.eye(6)[k]))) / (2.0 * h) for k in range(6)])
    return float(np.abs(g - 2.0 * np.asarray(b)).max() / np.abs(2.0 * np.asarray(b)).max())
