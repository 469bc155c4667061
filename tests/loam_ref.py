"""CPU restatement of the LOAM scan-to-map optimisation (jueying_slam mapOptmization.cpp:1255-1586) for the tests.

numpy float32 per-point arithmetic in the reference's operation order, an exact 5-NN through scipy's cKDTree (ties ordered by
(d^2, map index), d^2 = (dx^2 + dy^2) + dz^2 in float), the plane solve through the oracle's ColPivHouseholderQR restatement
(oracle/orc_eigen.h), and the reduction / step rule of the device written out again in plain Python doubles: rows summed per
64-row block by a halving tree, blocks summed in order, 6x6 Householder solve and cyclic Jacobi eigen-decomposition in double,
the step rounded to float.  It shares no code with csrc/loam_step.h."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np
from scipy.spatial import cKDTree

F = np.float32
LANES = 64
NSUMS = 33
DBL_MAX = float(np.finfo(np.float64).max)


@dataclasses.dataclass
class Params:
    iter_num: int = 30
    edge_min_valid: int = 10
    surf_min_valid: int = 100
    rot_conv_deg: float = 0.01
    trans_conv_cm: float = 0.05
    degeneracy_threshold: float = 100.0


# ---- pose ---------------------------------------------------------------------------------------------------------------
def sinf(a) -> np.float32:
    return F(math.sin(float(a)))


def cosf(a) -> np.float32:
    return F(math.cos(float(a)))


def pose_matrix(x):
    """pcl::getTransformation in float (3x4 row-major, float32) and (srx, crx, sry, cry, srz, crz)."""
    x = np.asarray(x, F)
    A, B, Cc, D, E, Fv = cosf(x[2]), sinf(x[2]), cosf(x[1]), sinf(x[1]), cosf(x[0]), sinf(x[0])
    DE, DF = D * E, D * Fv
    T = np.array([[A * Cc, A * DF - B * E, B * Fv + A * DE, x[3]],
                  [B * Cc, A * E + B * DF, B * DE - A * Fv, x[4]],
                  [-D, Cc * Fv, Cc * E, x[5]]], F)
    return T, np.array([D, Cc, B, A, Fv, E], F)


def to_map(T, p):
    p = np.asarray(p, F)
    return np.stack([T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1] + T[a, 2] * p[:, 2] + T[a, 3] for a in range(3)], axis=1)


# ---- 5-NN -----------------------------------------------------------------------------------------------------------------
class Map:
    def __init__(self, pts):
        self.p = np.ascontiguousarray(np.asarray(pts, F)[:, :3])
        self.tree = cKDTree(self.p.astype(np.float64)) if len(self.p) else None

    def knn5(self, q):
        """(idx (n,5) int64, d2 (n,5) float32) of the 5 nearest with d2 <= 1 by (d2, index); -1 / inf pad."""
        n = len(q)
        idx = np.full((n, 5), -1, np.int64)
        d2 = np.full((n, 5), np.inf, F)
        if self.tree is None or n == 0:
            return idx, d2
        K = min(24, len(self.p))
        _, cand = self.tree.query(q.astype(np.float64), k=K, distance_upper_bound=1.001)
        cand = cand.reshape(n, K)
        full = cand[:, -1] < len(self.p)
        rows = [list(c[c < len(self.p)]) for c in cand]
        if full.any():
            for r, lst in zip(np.nonzero(full)[0], self.tree.query_ball_point(q[full].astype(np.float64), r=1.001)):
                rows[r] = lst
        for r in range(n):
            c = np.asarray(rows[r], np.int64)
            if c.size == 0:
                continue
            dx, dy, dz = self.p[c, 0] - q[r, 0], self.p[c, 1] - q[r, 1], self.p[c, 2] - q[r, 2]
            dd = dx * dx + dy * dy + dz * dz
            keep = dd <= F(1.0)
            c, dd = c[keep], dd[keep]
            o = np.lexsort((c, dd))[:5]
            idx[r, :o.size] = c[o]
            d2[r, :o.size] = dd[o]
        return idx, d2


# ---- symmetric eigen-decomposition (cyclic Jacobi, double), vectorised over matrices -----------------------------------------
def sym_eigen(M):
    """M (n,N,N) float64 -> w (n,N) descending (first index on ties), E (n,N,N) rows = eigenvectors."""
    a = np.array(M, np.float64, copy=True)
    n, N, _ = a.shape
    v = np.broadcast_to(np.eye(N), (n, N, N)).copy()
    active = np.ones(n, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for _ in range(64):
            if not active.any():
                break
            rotated = np.zeros(n, bool)
            for p in range(N - 1):
                for q in range(p + 1, N):
                    apq = a[:, p, q].copy()
                    app, aqq = a[:, p, p].copy(), a[:, q, q].copy()
                    nz = active & (apq != 0.0)
                    small = nz & (np.abs(apq) <= 1e-18 * (np.abs(app) + np.abs(aqq)))
                    a[small, p, q] = 0.0
                    a[small, q, p] = 0.0
                    rot = nz & ~small
                    if not rot.any():
                        continue
                    theta = (aqq - app) / (2.0 * apq)
                    t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    t = np.where(theta < 0.0, -t, t)
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    cr, sr = c[rot, None], s[rot, None]
                    akp, akq = a[rot, :, p].copy(), a[rot, :, q].copy()
                    a[rot, :, p] = cr * akp - sr * akq
                    a[rot, :, q] = sr * akp + cr * akq
                    apk, aqk = a[rot, p, :].copy(), a[rot, q, :].copy()
                    a[rot, p, :] = cr * apk - sr * aqk
                    a[rot, q, :] = sr * apk + cr * aqk
                    a[rot, p, q] = 0.0
                    a[rot, q, p] = 0.0
                    vkp, vkq = v[rot, :, p].copy(), v[rot, :, q].copy()
                    v[rot, :, p] = cr * vkp - sr * vkq
                    v[rot, :, q] = sr * vkp + cr * vkq
                    rotated |= rot
            active &= rotated
    d = np.diagonal(a, axis1=1, axis2=2)
    w = np.empty((n, N))
    E = np.empty((n, N, N))
    used = np.zeros((n, N), bool)
    ar = np.arange(n)
    for k in range(N):
        best = np.full(n, -1)
        for i in range(N):
            take = ~used[:, i] & ((best < 0) | (d[:, i] > d[ar, np.maximum(best, 0)]))
            best = np.where(take, i, best)
        used[ar, best] = True
        w[:, k] = d[ar, best]
        E[:, k, :] = v[ar, :, best]
    return w, E


def solve6_qr(A, b):
    """Householder QR solve of the 6x6 system in Python doubles (zero pivot -> zero component)."""
    A = [[float(A[i][j]) for j in range(6)] for i in range(6)]
    b = [float(t) for t in b]
    v = [0.0] * 6
    for k in range(6):
        nrm2 = 0.0
        for i in range(k, 6):
            nrm2 += A[i][k] * A[i][k]
        nrm = math.sqrt(nrm2)
        if nrm == 0.0:
            continue
        alpha = -nrm if A[k][k] > 0.0 else nrm
        vtv = 0.0
        for i in range(k, 6):
            v[i] = A[k][k] - alpha if i == k else A[i][k]
            vtv += v[i] * v[i]
        if vtv == 0.0:
            continue
        for j in range(k, 6):
            dot = 0.0
            for i in range(k, 6):
                dot += v[i] * A[i][j]
            f = (2.0 * dot) / vtv
            for i in range(k, 6):
                A[i][j] -= f * v[i]
        dot = 0.0
        for i in range(k, 6):
            dot += v[i] * b[i]
        f = (2.0 * dot) / vtv
        for i in range(k, 6):
            b[i] -= f * v[i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = b[i]
        for j in range(i + 1, 6):
            s -= A[i][j] * x[j]
        x[i] = s / A[i][i] if A[i][i] != 0.0 else 0.0
    return x


# ---- per-point coefficients -------------------------------------------------------------------------------------------
def edge_coeff(nb, q):
    """nb (n,5,3) float32 neighbours, q (n,3) float32 -> coeff (n,4) float32, selected (n,) bool  (:1273-1343)."""
    n = len(q)
    if n == 0:
        return np.zeros((0, 4), F), np.zeros(0, bool)
    cx, cy, cz = (np.zeros(n, F) for _ in range(3))
    for j in range(5):
        cx = cx + nb[:, j, 0]; cy = cy + nb[:, j, 1]; cz = cz + nb[:, j, 2]
    five = F(5.0)
    cx, cy, cz = cx / five, cy / five, cz / five
    a = [np.zeros(n, F) for _ in range(6)]
    for j in range(5):
        ax, ay, az = nb[:, j, 0] - cx, nb[:, j, 1] - cy, nb[:, j, 2] - cz
        a[0] = a[0] + ax * ax; a[1] = a[1] + ax * ay; a[2] = a[2] + ax * az
        a[3] = a[3] + ay * ay; a[4] = a[4] + ay * az; a[5] = a[5] + az * az
    a11, a12, a13, a22, a23, a33 = (t / five for t in a)
    M = np.stack([a11, a12, a13, a12, a22, a23, a13, a23, a33], axis=1).astype(np.float64).reshape(n, 3, 3)
    w, E = sym_eigen(M)
    l0, l1 = w[:, 0].astype(F), w[:, 1].astype(F)
    ok = l0 > F(3.0) * l1
    v0, v1, v2 = E[:, 0, 0].astype(F), E[:, 0, 1].astype(F), E[:, 0, 2].astype(F)
    x0, y0, z0 = q[:, 0], q[:, 1], q[:, 2]
    x1 = (cx.astype(np.float64) + 0.1 * v0.astype(np.float64)).astype(F)
    y1 = (cy.astype(np.float64) + 0.1 * v1.astype(np.float64)).astype(F)
    z1 = (cz.astype(np.float64) + 0.1 * v2.astype(np.float64)).astype(F)
    x2 = (cx.astype(np.float64) - 0.1 * v0.astype(np.float64)).astype(F)
    y2 = (cy.astype(np.float64) - 0.1 * v1.astype(np.float64)).astype(F)
    z2 = (cz.astype(np.float64) - 0.1 * v2.astype(np.float64)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)
        vv = (x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)
        t = (y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1)
        a012 = np.sqrt(u * u + vv * vv + t * t)
        l12 = np.sqrt((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2))
        la = ((y1 - y2) * u + (z1 - z2) * vv) / a012 / l12
        lb = (-((x1 - x2) * u - (z1 - z2) * t)) / a012 / l12
        lc = (-((x1 - x2) * vv + (y1 - y2) * t)) / a012 / l12
        ld2 = a012 / l12
    s = (1.0 - 0.9 * np.abs(ld2).astype(np.float64)).astype(F)
    co = np.stack([s * la, s * lb, s * lc, s * ld2], axis=1)
    sel = ok & (s.astype(np.float64) > 0.1)
    return co, sel


def _colpivqr(A):
    from oracle.loader import lib
    L = lib()
    n = len(A)
    A = np.ascontiguousarray(A, F)
    b = np.full((n, 5), -1.0, F)
    x = np.zeros((n, 3), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    L.orc_test_eig_colpivqr_f.argtypes = [C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.orc_test_eig_colpivqr_f.restype = None
    L.orc_test_eig_colpivqr_f(C.c_long(n), C.c_int(5), p(A), p(b), p(x))
    return x


def plane_coeff(nb, q):
    """(:1376-1415) with the float ColPivHouseholderQR of the oracle."""
    n = len(q)
    if n == 0:
        return np.zeros((0, 4), F), np.zeros(0, bool)
    X = _colpivqr(nb)
    pa, pb, pc = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        ps = np.sqrt(pa * pa + pb * pb + pc * pc)
        pa, pb, pc, pd = pa / ps, pb / ps, pc / ps, F(1.0) / ps
        ok = np.ones(n, bool)
        for j in range(5):
            r = pa * nb[:, j, 0] + pb * nb[:, j, 1] + pc * nb[:, j, 2] + pd
            ok &= ~(np.abs(r).astype(np.float64) > 0.2)
        pd2 = pa * q[:, 0] + pb * q[:, 1] + pc * q[:, 2] + pd
        rn = np.sqrt(np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]))
        s = (1.0 - 0.9 * np.abs(pd2).astype(np.float64) / rn.astype(np.float64)).astype(F)
    co = np.stack([s * pa, s * pb, s * pc, s * pd2], axis=1)
    sel = ok & (s.astype(np.float64) > 0.1)
    return co, sel


def jacobian_rows(trig, body, co):
    """(:1469-1504) rows (n,7) float32: arz, arx, ary, c.x, c.y, c.z, -intensity."""
    srx, crx, sry, cry, srz, crz = (F(t) for t in trig)
    px, py, pz = body[:, 1], body[:, 2], body[:, 0]
    cx, cy, cz = co[:, 1], co[:, 2], co[:, 0]
    arx = ((crx * sry * srz * px + crx * crz * sry * py - srx * sry * pz) * cx
           + (-srx * srz * px - crz * srx * py - crx * pz) * cy
           + (crx * cry * srz * px + crx * cry * crz * py - cry * srx * pz) * cz)
    ary = (((cry * srx * srz - crz * sry) * px + (sry * srz + cry * crz * srx) * py + crx * cry * pz) * cx
           + ((-cry * crz - srx * sry * srz) * px + (cry * srz - crz * srx * sry) * py - crx * sry * pz) * cz)
    arz = (((crz * srx * sry - cry * srz) * px + (-cry * crz - srx * sry * srz) * py) * cx
           + (crx * crz * px - crx * srz * py) * cy
           + ((sry * srz + cry * crz * srx) * px + (crz * sry - cry * srx * srz) * py) * cz)
    return np.stack([arz, arx, ary, cz, cx, cy, -co[:, 3]], axis=1).astype(F)


# ---- one pass -------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Pass:
    corner: np.ndarray     # (Nc,4) coefficients, NaN rows = not selected
    surf: np.ndarray       # (Ns,4)
    corner_nn: np.ndarray  # (Nc,5) map indices (-1 pads)
    surf_nn: np.ndarray
    corner_d2: np.ndarray  # (Nc,5)
    surf_d2: np.ndarray
    sums: np.ndarray       # (33,) as the step reads them


class Problem:
    def __init__(self, corner_map, surf_map, corner, surf):
        self.maps = (Map(corner_map), Map(surf_map))
        self.feats = (np.ascontiguousarray(np.asarray(corner, F)[:, :3]), np.ascontiguousarray(np.asarray(surf, F)[:, :3]))

    def one_pass(self, x) -> Pass:
        T, trig = pose_matrix(x)
        rows, coeffs, nns, d2s, fits = [], [], [], [], []
        for kind in (0, 1):
            body = self.feats[kind]
            q = to_map(T, body)
            idx, d2 = self.maps[kind].knn5(q)
            n = len(q)
            co = np.full((n, 4), np.nan, F)
            sel = np.zeros(n, bool)
            acc = d2[:, 4] < F(1.0)
            if acc.any():
                nb = self.maps[kind].p[idx[acc]]
                c, s = (edge_coeff if kind == 0 else plane_coeff)(nb, q[acc])
                sub = np.nonzero(acc)[0]
                co[sub[s]] = c[s]
                sel[sub[s]] = True
            r = np.zeros((n, 7), F)
            if sel.any():
                r[sel] = jacobian_rows(trig, body[sel], co[sel])
            f = d2[:, 0] <= F(1.0)
            extra = np.zeros((n, 6))
            extra[:, kind] = sel
            extra[:, 2 + 2 * kind] = np.where(f, d2[:, 0].astype(np.float64), 0.0)
            extra[:, 3 + 2 * kind] = f
            rows.append((r, extra))
            coeffs.append(co); nns.append(idx); d2s.append(d2)
        r = np.concatenate([rows[0][0], rows[1][0]])
        extra = np.concatenate([rows[0][1], rows[1][1]])
        rd = r.astype(np.float64)
        terms = [rd[:, a] * rd[:, c] for a in range(6) for c in range(a, 6)] + [rd[:, a] * rd[:, 6] for a in range(6)] + [extra[:, k] for k in range(6)]
        return Pass(coeffs[0], coeffs[1], nns[0], nns[1], d2s[0], d2s[1], reduce_rows(np.stack(terms, axis=1)))


def reduce_rows(terms):
    """(n, 33) -> the device's order: 64-row blocks by halving (lane i + lane i+off), block totals summed in block order."""
    n = len(terms)
    nb = max(1, -(-n // LANES))
    t = np.zeros((nb * LANES, terms.shape[1]))
    t[:n] = terms
    t = t.reshape(nb, LANES, -1)
    off = LANES // 2
    while off >= 1:
        t = t[:, :off] + t[:, off:2 * off]
        off //= 2
    blocks = t[:, 0, :]
    s = np.zeros(terms.shape[1])
    for b in range(nb):
        s = s + blocks[b]
    return s


# ---- the step and the loop --------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class State:
    x: np.ndarray
    iter: int = 0
    done: bool = False
    converged: bool = False
    degenerate: bool = False
    P: np.ndarray = None
    eig: np.ndarray = None
    n_corner: int = 0
    n_surf: int = 0
    fit: tuple = (DBL_MAX, DBL_MAX)
    last_step: np.ndarray = None   # the (projected) float step of the last update


def step(s: State, sums, p: Params):
    s.n_corner, s.n_surf = int(sums[27]), int(sums[28])
    s.fit = (sums[29] / sums[30] if sums[30] > 1.0 else DBL_MAX, sums[31] / sums[32] if sums[32] > 1.0 else DBL_MAX)
    it = s.iter
    s.iter = it + 1
    if s.n_corner + s.n_surf >= 50:
        AtA = np.zeros((6, 6))
        t = 0
        for i in range(6):
            for j in range(i, 6):
                AtA[i, j] = AtA[j, i] = sums[t]
                t += 1
        x = solve6_qr(AtA, sums[21:27])
        if it == 0:
            w, E = sym_eigen(AtA[None])
            w, E = w[0], E[0]
            s.eig = w
            E2 = E.copy()
            s.degenerate = False
            for i in range(5, -1, -1):
                if w[i] < p.degeneracy_threshold:
                    E2[i, :] = 0.0
                    s.degenerate = True
                else:
                    break
            P = np.zeros((6, 6))
            for r in range(6):
                for c in range(6):
                    acc = 0.0
                    for k in range(6):
                        acc += float(E[k, r]) * float(E2[k, c])
                    P[r, c] = acc
            s.P = P
        if s.degenerate:
            y = []
            for r in range(6):
                acc = 0.0
                for c in range(6):
                    acc += float(s.P[r, c]) * x[c]
                y.append(acc)
            x = y
        xf = np.array(x, np.float64).astype(F)
        s.x = (s.x + xf).astype(F)
        s.last_step = xf
        r = xf[:3] * F(57.29578)
        tt = xf[3:] * F(100.0)
        dR = F(math.sqrt(float(r[0]) * float(r[0]) + float(r[1]) * float(r[1]) + float(r[2]) * float(r[2])))
        dT = F(math.sqrt(float(tt[0]) * float(tt[0]) + float(tt[1]) * float(tt[1]) + float(tt[2]) * float(tt[2])))
        if float(dR) < p.rot_conv_deg and float(dT) < p.trans_conv_cm:
            s.converged = True
            s.done = True
    if s.iter >= p.iter_num:
        s.done = True


def scan2map(prob: Problem, x0, p: Params = Params()):
    """-> State (x, iter, converged, degenerate, eig, counts, fitness); iter 0 and x0 when there are too few features."""
    s = State(x=np.asarray(x0, F).copy(), eig=np.zeros(6), P=np.zeros((6, 6)))
    if not (len(prob.feats[0]) > p.edge_min_valid and len(prob.feats[1]) > p.surf_min_valid):
        return s
    while not s.done and s.iter < p.iter_num:
        step(s, prob.one_pass(s.x).sums, p)
    return s
