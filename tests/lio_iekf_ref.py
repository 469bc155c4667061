"""numpy / float64 restatement of jueying_lio's iterated Kalman update, esekf::update_iterated_dyn_share_modified
(IKFoM_toolkit/esekfom/esekfom.hpp:1526-1834) for state_ikfom (use-ikfom.hpp:14-15), with the manifold pieces of mtk/types/SOn.hpp,
mtk/types/S2.hpp (S2<double, 98090, 10000, 1>) and mtk/src/mtkmath.hpp it calls.  A literal transcription, both gain branches
included (`n > dof_Measurement` dense form and the information form); Eigen's general inverse() is numpy.linalg.inv.

The state is a dict of float64 arrays: pos(3) rot(4: x,y,z,w) off_R(4) off_T(3) vel(3) bg(3) ba(3) grav(3); DOF 23 in that order.
The measurement callback is  h(x, converge) -> dict(valid, HTH (12x12), HTh (12), n_eff, sum_h2[, h_x (m x 12), h (m)])."""
import math

import numpy as np

N = 23
TOL = 1e-11                      # MTK::tolerance<double>()
LENGTH = 98090.0 / 10000.0       # S2<double, 98090, 10000, 1>::length
KEYS = (("pos", 3), ("rot", 4), ("off_R", 4), ("off_T", 3), ("vel", 3), ("bg", 3), ("ba", 3), ("grav", 3))
SO3_STATE = (3, 6)
S2_STATE = (21,)
INIT_P_DIAG = np.array([1.0] * 6 + [1e-5] * 6 + [1.0] * 3 + [1e-4] * 3 + [1e-3] * 3 + [1e-5] * 2)   # imu_processing.hpp:154-161


def make_state(pos=(0, 0, 0), rot=(0, 0, 0, 1), off_R=(0, 0, 0, 1), off_T=(0, 0, 0), vel=(0, 0, 0), bg=(0, 0, 0), ba=(0, 0, 0), grav=(0, 0, -LENGTH)):
    loc = locals()
    return {k: np.array(loc[k], np.float64) for k, _ in KEYS}


def copy_state(x):
    return {k: x[k].copy() for k, _ in KEYS}


def state_to_vec(x):
    return np.concatenate([x[k] for k, _ in KEYS])


def vec_to_state(v):
    out, o = {}, 0
    for k, n in KEYS:
        out[k] = np.array(v[o:o + n], np.float64); o += n
    return out


# ---- small pieces ------------------------------------------------------------------------------------------------------------
def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def mat33_mul(A, B):
    C = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            C[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
    return C


def mat_vec3(A, v):   # rows of A (r x 3) times v, Eigen's order of additions
    return np.array([(A[i, 0] * v[0] + A[i, 1] * v[1]) + A[i, 2] * v[2] for i in range(A.shape[0])])


def quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def quat_to_rot(q):
    x, y, z, w = (float(t) for t in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def cos_sinc_sqrt(x2):   # mtkmath.hpp:149-180
    taylor_0_bound = float(np.finfo(np.float64).eps)
    taylor_2_bound = math.sqrt(taylor_0_bound)
    taylor_n_bound = math.sqrt(taylor_2_bound)
    if x2 >= taylor_n_bound:
        x = math.sqrt(x2)
        return math.cos(x), math.sin(x) / x
    inv = [1 / 3., 1 / 4., 1 / 5., 1 / 6., 1 / 7., 1 / 8., 1 / 9.]
    cosi, sinc = 1., 1.
    term = -1 / 2. * x2
    for i in range(3):
        cosi += term
        term *= inv[2 * i]
        sinc += term
        term *= -inv[2 * i + 1] * x2
    return cosi, sinc


def exp_quat(vec, scale):   # MTK::exp, mtkmath.hpp:248-254
    norm2 = (vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2]
    c, s = cos_sinc_sqrt(scale * scale * norm2)
    mult = s * scale
    return np.array([mult * vec[0], mult * vec[1], mult * vec[2], c])


def A_matrix(v):   # mtkmath.hpp:234-245
    squaredNorm = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    norm = math.sqrt(squaredNorm)
    if norm < TOL:
        return np.eye(3)
    H = hat(v)
    return (np.eye(3) + (1 - math.cos(norm)) / squaredNorm * H) + mat33_mul((1 - math.sin(norm) / norm) / squaredNorm * H, H)


def so3_boxplus(q, vec):   # SOn.hpp:210-213
    return quat_mul(q, exp_quat(vec, 1.0 / 2))


def so3_boxminus(q, other):   # SOn.hpp:214-216, mtkmath.hpp:266-284 with plus_minus_periodicity
    r = quat_mul(np.array([-other[0], -other[1], -other[2], other[3]]), q)
    nv = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if nv < TOL:
        nv = TOL
    s = 2.0 / nv * math.atan(nv / r[3])
    return s * r[:3]


def s2_Bx(vec):   # S2.hpp:188-199 (S2_typ == 1)
    if vec[0] + LENGTH > TOL:
        res = np.array([[-vec[1], -vec[2]],
                        [LENGTH - vec[1] * vec[1] / (LENGTH + vec[0]), -vec[2] * vec[1] / (LENGTH + vec[0])],
                        [-vec[2] * vec[1] / (LENGTH + vec[0]), LENGTH - vec[2] * vec[2] / (LENGTH + vec[0])]])
        return res / LENGTH
    res = np.zeros((3, 2))
    res[1, 1] = -1
    res[2, 0] = 1
    return res


def _bx_delta(B, d):
    return np.array([B[i, 0] * d[0] + B[i, 1] * d[1] for i in range(3)])


def s2_boxplus(vec, delta):   # S2.hpp:131-138
    Bu = _bx_delta(s2_Bx(vec), delta)
    return mat_vec3(quat_to_rot(exp_quat(Bu, 1.0 / 2)), vec)


def s2_boxminus(vec, other):   # S2.hpp:140-158
    hv = mat_vec3(hat(vec), other)
    v_sin = math.sqrt((hv[0] * hv[0] + hv[1] * hv[1]) + hv[2] * hv[2])
    v_cos = (vec[0] * other[0] + vec[1] * other[1]) + vec[2] * other[2]
    theta = math.atan2(v_sin, v_cos)
    if v_sin < TOL:
        return np.array([3.1415926, 0.0]) if abs(theta) > TOL else np.zeros(2)
    M1 = (theta / v_sin) * s2_Bx(other).T
    Ho = hat(other)
    M2 = np.array([[(M1[r, 0] * Ho[0, c] + M1[r, 1] * Ho[1, c]) + M1[r, 2] * Ho[2, c] for c in range(3)] for r in range(2)])
    return mat_vec3(M2, vec)


def s2_Nx_yy(vec):   # S2.hpp:225-229
    M1 = (1 / LENGTH / LENGTH) * s2_Bx(vec).T
    Hv = hat(vec)
    return np.array([[(M1[r, 0] * Hv[0, c] + M1[r, 1] * Hv[1, c]) + M1[r, 2] * Hv[2, c] for c in range(3)] for r in range(2)])


def s2_Mx(vec, delta):   # S2.hpp:231-242
    B = s2_Bx(vec)
    Hv = hat(vec)
    if math.sqrt(delta[0] * delta[0] + delta[1] * delta[1]) < TOL:
        M = -Hv
    else:
        Bu = _bx_delta(B, delta)
        Rm = quat_to_rot(exp_quat(Bu, float(1 // 2)))     # scalar(1 / 2): integer division
        M = mat33_mul(mat33_mul(-Rm, Hv), A_matrix(Bu).T.copy())
    return np.array([[(M[r, 0] * B[0, c] + M[r, 1] * B[1, c]) + M[r, 2] * B[2, c] for c in range(2)] for r in range(3)])


def s2_NxMx(vec_x, vec_prop, seg):
    Nx, Mx = s2_Nx_yy(vec_x), s2_Mx(vec_prop, seg)
    return np.array([[(Nx[r, 0] * Mx[0, c] + Nx[r, 1] * Mx[1, c]) + Nx[r, 2] * Mx[2, c] for c in range(2)] for r in range(2)])


def state_boxplus(x, d):   # build_manifold.hpp:195-197
    y = copy_state(x)
    y["pos"] = x["pos"] + d[0:3]
    y["rot"] = so3_boxplus(x["rot"], d[3:6])
    y["off_R"] = so3_boxplus(x["off_R"], d[6:9])
    y["off_T"] = x["off_T"] + d[9:12]
    y["vel"] = x["vel"] + d[12:15]
    y["bg"] = x["bg"] + d[15:18]
    y["ba"] = x["ba"] + d[18:21]
    y["grav"] = s2_boxplus(x["grav"], d[21:23])
    return y


def state_boxminus(x, o):   # build_manifold.hpp:201-203
    d = np.zeros(N)
    d[0:3] = x["pos"] - o["pos"]
    d[3:6] = so3_boxminus(x["rot"], o["rot"])
    d[6:9] = so3_boxminus(x["off_R"], o["off_R"])
    d[9:12] = x["off_T"] - o["off_T"]
    d[12:15] = x["vel"] - o["vel"]
    d[15:18] = x["bg"] - o["bg"]
    d[18:21] = x["ba"] - o["ba"]
    d[21:23] = s2_boxminus(x["grav"], o["grav"])
    return d


def sums_of(HTH, HTh, sum_h2, n_eff):
    """The 92 sums in the device's order: HTH upper triangle, HTh, sum h^2, count."""
    s = np.zeros(96)
    t = 0
    for a in range(12):
        for b in range(a, 12):
            s[t] = HTH[a, b]; t += 1
    s[78:90] = HTh
    s[90], s[91] = sum_h2, n_eff
    return s


# ---- one pass of the loop body (esekfom.hpp:1556-1733) and the closing block (:1736-1827) -------------------------------------------
def project(x, x_prop, dx, P_prop):
    """:1556-1601 -> (dx_new, P_)."""
    dx_new = dx.copy()
    P = P_prop.copy()
    for idx in SO3_STATE:
        res = A_matrix(dx[idx:idx + 3]).T.copy()
        dx_new[idx:idx + 3] = mat_vec3(res, dx_new[idx:idx + 3])
        P[idx:idx + 3, :] = res @ P[idx:idx + 3, :]
        P[:, idx:idx + 3] = P[:, idx:idx + 3] @ res.T
    for idx in S2_STATE:
        res = s2_NxMx(x["grav"], x_prop["grav"], dx[idx:idx + 2])
        dx_new[idx:idx + 2] = np.array([res[0, 0] * dx_new[idx] + res[0, 1] * dx_new[idx + 1], res[1, 0] * dx_new[idx] + res[1, 1] * dx_new[idx + 1]])
        P[idx:idx + 2, :] = res @ P[idx:idx + 2, :]
        P[:, idx:idx + 2] = P[:, idx:idx + 2] @ res.T
    return dx_new, P


def gain(P, R, m, dense=None):
    """:1618-1716 -> (K_h, K_x).  m: dict of the measurement; dense None = as the reference chooses (n > dof_Measurement)."""
    dof = int(m["n_eff"])
    if dense is None:
        dense = N > dof
    if dense:
        h_x_cur = np.zeros((dof, N))
        h_x_cur[:, :12] = m["h_x"]
        K_ = P @ h_x_cur.T @ np.linalg.inv(h_x_cur @ P @ h_x_cur.T / R + np.eye(dof)) / R
        return K_ @ m["h"], K_ @ h_x_cur
    P_temp = np.linalg.inv(P / R)
    P_temp[:12, :12] += m["HTH"]
    P_inv = np.linalg.inv(P_temp)
    K_h = P_inv[:, :12] @ m["HTh"]
    K_x = np.zeros((N, N))
    K_x[:, :12] = P_inv[:, :12] @ m["HTH"]
    return K_h, K_x


def final_cov(x, x_prop, dx_, P, K_x):
    """:1736-1827 with x the updated state -> P_."""
    P = P.copy(); K_x = K_x.copy()
    L = P.copy()
    for idx in SO3_STATE:
        res = A_matrix(dx_[idx:idx + 3]).T.copy()
        L[idx:idx + 3, :] = res @ P[idx:idx + 3, :]
        K_x[idx:idx + 3, :12] = res @ K_x[idx:idx + 3, :12]
        L[:, idx:idx + 3] = L[:, idx:idx + 3] @ res.T
        P[:, idx:idx + 3] = P[:, idx:idx + 3] @ res.T
    for idx in S2_STATE:
        res = s2_NxMx(x["grav"], x_prop["grav"], dx_[idx:idx + 2])
        L[idx:idx + 2, :] = res @ P[idx:idx + 2, :]
        K_x[idx:idx + 2, :12] = res @ K_x[idx:idx + 2, :12]
        L[:, idx:idx + 2] = L[:, idx:idx + 2] @ res.T
        P[:, idx:idx + 2] = P[:, idx:idx + 2] @ res.T
    return L - K_x[:, :12] @ P[:12, :]


def update(x0, P0, h, R=0.001, max_iter=4, limit=None, dense=None):
    """update_iterated_dyn_share_modified.  Returns dict(x, P, iterations, rematches, valid_calls, t, n_eff_last, sum_h2_last, trace);
    trace: per ObsModel call dict(x, converge, n_eff, HTH, HTh, dx_)."""
    limit = np.full(N, 0.001) if limit is None else np.asarray(limit, np.float64)
    converge = True
    t = 0
    x = copy_state(x0)
    x_prop = copy_state(x0)
    P = np.array(P0, np.float64).reshape(N, N).copy()
    P_prop = P.copy()
    out = dict(iterations=0, rematches=0, valid_calls=0, n_eff_last=0, sum_h2_last=0.0, trace=[])
    for i in range(-1, max_iter):
        m = h(x, converge)
        rec = dict(x=copy_state(x), converge=converge, n_eff=int(m["n_eff"]), HTH=np.array(m["HTH"]), HTh=np.array(m["HTh"]), dx_=np.zeros(N))
        out["trace"].append(rec)
        out["iterations"] += 1
        out["rematches"] += int(converge)
        out["n_eff_last"], out["sum_h2_last"] = int(m["n_eff"]), float(m["sum_h2"])
        if not m["valid"]:
            continue
        out["valid_calls"] += 1
        dx = state_boxminus(x, x_prop)
        dx_new, P = project(x, x_prop, dx, P_prop)
        K_h, K_x = gain(P, R, m, dense)
        dx_ = K_h + (K_x - np.eye(N)) @ dx_new
        rec["dx_"] = dx_.copy()
        x = state_boxplus(x, dx_)
        converge = True
        for k in range(N):
            if abs(dx_[k]) > limit[k]:
                converge = False
                break
        if converge:
            t += 1
        if (not t) and i == max_iter - 2:
            converge = True
        if t > 1 or i == max_iter - 1:
            P = final_cov(x, x_prop, dx_, P, K_x)
            break
    out.update(x=x, P=P, t=t)
    return out


# ---- measurement rows (laser_mapping.cc:669-698) in float32, for the dense branch ----------------------------------------------------
def lio_rows(scan, planes, selected, x, extrinsic_est_en):
    """h_x (m x 12) and h (m) of the points ObsModel keeps (clean semantics: a fitted plane and |p| > 81 pd2^2), float32 arithmetic in the
    reference's order, returned as float64."""
    F = np.float32
    qwl = quat_mul(x["rot"], x["off_R"])
    R = quat_to_rot(x["rot"])
    # Eigen _transformVector for the double translation, then the float casts
    q = x["rot"]; v = x["off_T"]
    uv = 2 * np.cross(q[:3], v)
    twl = v + q[3] * uv + np.cross(q[:3], uv)
    qf = qwl.astype(F); tf = (twl + x["pos"]).astype(F)
    Rt = R.T.astype(F); offR = quat_to_rot(x["off_R"]).astype(F); offt = x["off_T"].astype(F)
    rows, hs = [], []
    for i in np.nonzero(selected)[0]:
        p = scan[i].astype(F); pl = planes[i].astype(F)
        u = np.array([qf[1] * p[2] - qf[2] * p[1], qf[2] * p[0] - qf[0] * p[2], qf[0] * p[1] - qf[1] * p[0]], F)
        u = u + u
        c3 = np.array([qf[1] * u[2] - qf[2] * u[1], qf[2] * u[0] - qf[0] * u[2], qf[0] * u[1] - qf[1] * u[0]], F)
        qq = (p + qf[3] * u + c3) + tf
        pd2 = F(F(F(pl[0] * qq[0]) + F(pl[1] * qq[1])) + F(pl[2] * qq[2])) + pl[3]
        pn = np.sqrt(F(F(p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]))
        if not (pn > F(81.0) * pd2 * pd2):
            continue
        pt = np.array([(offR[a, 0] * p[0] + offR[a, 1] * p[1]) + offR[a, 2] * p[2] + offt[a] for a in range(3)], F)
        C = np.array([(Rt[a, 0] * pl[0] + Rt[a, 1] * pl[1]) + Rt[a, 2] * pl[2] for a in range(3)], F)
        A = np.array([(F(0) * C[0] + -pt[2] * C[1]) + pt[1] * C[2], (pt[2] * C[0] + F(0) * C[1]) + -pt[0] * C[2], (-pt[1] * C[0] + pt[0] * C[1]) + F(0) * C[2]], F)
        row = np.zeros(12, F)
        row[0:3] = pl[:3]; row[3:6] = A
        if extrinsic_est_en:
            S = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]], F)
            SM = np.array([[(S[a, 0] * offR[b, 0] + S[a, 1] * offR[b, 1]) + S[a, 2] * offR[b, 2] for b in range(3)] for a in range(3)], F)
            row[6:9] = [(SM[a, 0] * C[0] + SM[a, 1] * C[1]) + SM[a, 2] * C[2] for a in range(3)]
            row[9:12] = C
        rows.append(row.astype(np.float64)); hs.append(-float(pd2))
    if not rows:
        return np.zeros((0, 12)), np.zeros(0)
    return np.array(rows), np.array(hs)


def oracle_callback(o, scan, extrinsic_est_en, with_rows=False):
    """Measurement callback on the oracle's obs_model (clean semantics); with_rows adds h_x / h from lio_rows over the oracle's planes."""
    n = len(scan)

    def h(x, converge):
        HTH, HTh, n_eff, s2 = o.obs_model(x["rot"], x["pos"], x["off_R"], x["off_T"], extrinsic_est_en, converge)
        m = dict(valid=n_eff >= 1, HTH=HTH, HTh=HTh, n_eff=n_eff, sum_h2=s2)
        if with_rows:
            pl, sel = o.get_planes(n)
            m["h_x"], m["h"] = lio_rows(scan, pl, sel, x, extrinsic_est_en)
        return m
    return h
