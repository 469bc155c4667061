"""Point-to-point ICP as include/pcm_amd.h defines it (PCM_MODEL_ICP), in numpy, written from the rules and
not from csrc/icp.h: float32 for the transform and the squared distances with the stated expression order, a brute-force nearest
neighbour, float64 elsewhere, numpy.linalg.svd for the closed-form step.  ``align`` records a per-iteration trace (N, mse, the
step, the stop reason) and the margins the GPU tests demand of their inputs: the relative gap between every query's nearest
and second-nearest squared distance, and how far every threshold comparison that was evaluated lies from equality."""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
STOP_NONE, STOP_ITERATIONS, STOP_TRANSFORM, STOP_ABS_MSE, STOP_REL_MSE, STOP_NO_CORRESPONDENCES = 0, 1, 2, 3, 4, 5

DEFAULTS = dict(max_iterations=10, max_correspondence_distance=float(np.sqrt(np.float64(DBL_MAX))), transformation_epsilon=0.0, rotation_epsilon=0.0,
                euclidean_fitness_epsilon=-DBL_MAX, mse_absolute=1e-12)


def transform(Ff, s):
    """c = Ff s in float32 as m0*x + (m1*y + (m2*z + m3)), one IEEE operation per step."""
    Ff = np.asarray(Ff, np.float32)
    x, y, z = (np.asarray(s[:, k], np.float32) for k in range(3))
    with np.errstate(all="ignore"):
        return np.stack([Ff[a, 0] * x + (Ff[a, 1] * y + (Ff[a, 2] * z + Ff[a, 3])) for a in range(3)], axis=1).astype(np.float32)


def sq_dists(c, tgt):
    """(n, m) float32: (ex*ex + ey*ey) + ez*ez"""
    with np.errstate(all="ignore"):
        e = tgt[None, :, :].astype(np.float32) - c[:, None, :].astype(np.float32)
        return ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(np.float32)


def _rel_margin(a, b):
    """|a - b| relative to the larger magnitude; inf when one is infinite; 0 when both are below 1e-30 in magnitude (rounding
    residue against a zero threshold: one implementation's exact 0 is another's 1e-76)"""
    a, b = float(a), float(b)
    m = max(abs(a), abs(b))
    if not np.isfinite(m):
        return np.inf
    if m < 1e-30:
        return 0.0
    return abs(a - b) / m


def umeyama(sums):
    """The step of one sum row (sum c, sum q, sum q c^T, sum d2, N) -> (R, t, S2)."""
    N = sums["N"]
    cm, qm = sums["c"] / N, sums["q"] / N
    sigma = sums["qc"] / N - np.outer(qm, cm)
    U, _, Vt = np.linalg.svd(sigma)
    s2 = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = U @ np.diag([1.0, 1.0, s2]) @ Vt
    return R, qm - R @ cm, s2


def pair_sums(c, q, d2):
    c64, q64 = c.astype(np.float64), q.astype(np.float64)
    return dict(N=float(len(c)), c=c64.sum(0), q=q64.sum(0), qc=q64.T @ c64, d2=float(d2.astype(np.float64).sum()))


def align(src, tgt, guess=None, **params):
    P = dict(DEFAULTS, **params)
    src, tgt = np.asarray(src, np.float32)[:, :3], np.asarray(tgt, np.float32)[:, :3]
    F = np.eye(4) if guess is None else np.asarray(guess, np.float32).astype(np.float64).reshape(4, 4)
    max_sq = min(P["max_correspondence_distance"] ** 2, DBL_MAX)
    rot_thr = P["rotation_epsilon"] if P["rotation_epsilon"] > 0 else 1.0 - P["transformation_epsilon"]
    prev = DBL_MAX
    out = dict(iterations=0, converged=False, stop=STOP_NONE, trace=[], min_gap=np.inf, min_margin=np.inf, exact_ties=0, num_pairs=0, mse=0.0)
    k = 0
    while True:
        k += 1
        c = transform(F.astype(np.float32), src)
        finite = np.isfinite(c).all(1)
        D = sq_dists(c, tgt)
        D = np.where(np.isnan(D), np.float32(np.inf), D)
        j = np.argmin(D, axis=1)
        d2 = D[np.arange(len(c)), j]
        if tgt.shape[0] > 1:
            second = np.partition(D, 1, axis=1)[:, 1].astype(np.float64)
            with np.errstate(all="ignore"):
                gap = np.where(finite & np.isfinite(second), (second - d2.astype(np.float64)) / second, np.inf)
            out["min_gap"] = min(out["min_gap"], float(np.nanmin(gap)) if len(gap) else np.inf)
        keep = finite & (d2.astype(np.float64) <= max_sq)
        for v in d2[finite].astype(np.float64):   # step 3's comparison: an exact equality is a case of its own, a near one is refused
            if v == max_sq:
                out["exact_ties"] += 1
            else:
                out["min_margin"] = min(out["min_margin"], _rel_margin(v, max_sq))
        N = int(keep.sum())
        out["num_pairs"] = N
        if N < 3:
            out.update(converged=False, stop=STOP_NO_CORRESPONDENCES)
            out["trace"].append(dict(N=N, mse=0.0, delta=None, stop=STOP_NO_CORRESPONDENCES))
            break
        S = pair_sums(c[keep], tgt[j[keep]], d2[keep])
        R, t, s2 = umeyama(S)
        Dl = np.eye(4)
        Dl[:3, :3], Dl[:3, 3] = R, t
        F = Dl @ F
        mse = S["d2"] / S["N"]
        out["iterations"], out["mse"] = k, mse
        stop = STOP_NONE
        if k >= P["max_iterations"]:
            stop = STOP_ITERATIONS
        else:
            cos_angle, t2 = 0.5 * (np.trace(R) - 1.0), float(t @ t)
            # the conjunction is as far from flipping as its most decided false side, or, when both hold, as its least decided one
            sides = [(cos_angle >= rot_thr, _rel_margin(cos_angle, rot_thr)), (t2 <= P["transformation_epsilon"], _rel_margin(t2, P["transformation_epsilon"]))]
            false_sides = [m for ok, m in sides if not ok]
            out["min_margin"] = min(out["min_margin"], max(false_sides) if false_sides else min(m for _, m in sides))
            if cos_angle >= rot_thr and t2 <= P["transformation_epsilon"]:
                stop = STOP_TRANSFORM
            else:
                diff = abs(mse - prev)
                out["min_margin"] = min(out["min_margin"], _rel_margin(diff, P["mse_absolute"]))
                if diff < P["mse_absolute"]:
                    stop = STOP_ABS_MSE
                else:
                    out["min_margin"] = min(out["min_margin"], _rel_margin(diff / prev, P["euclidean_fitness_epsilon"]))
                    if diff / prev < P["euclidean_fitness_epsilon"]:
                        stop = STOP_REL_MSE
        out["trace"].append(dict(N=N, mse=mse, delta=Dl, stop=stop, s2=s2))
        if stop != STOP_NONE:
            out.update(converged=True, stop=stop)
            break
        prev = mse
    out["T64"] = F
    out["T"] = F.astype(np.float32)
    return out


def fitness(src, tgt, T, max_range=DBL_MAX):
    """pcl::Registration::getFitnessScore(max_range): the squared distance meets max_range itself."""
    c = transform(np.asarray(T, np.float32), np.asarray(src, np.float32)[:, :3])
    ok = np.isfinite(c).all(1)
    d2 = sq_dists(c[ok], np.asarray(tgt, np.float32)[:, :3]).min(1).astype(np.float64)
    d2 = d2[d2 <= max_range]
    return float(d2.sum() / len(d2)) if len(d2) else DBL_MAX


# ---- the pose algebra of performSCLoopClosure (mapOptmization.cpp:817-834), float64 except the float32 Euler extraction ----
def sc_pose_from(correction):
    """pcl::getTranslationAndEulerAngles of the float 4x4: (roll, pitch, yaw, x, y, z), each angle the double function rounded to float"""
    T = np.asarray(correction, np.float32).reshape(4, 4)
    f = np.float32
    roll = f(np.arctan2(np.float64(T[2, 1]), np.float64(T[2, 2])))
    pitch = f(np.arcsin(np.float64(-T[2, 0])))
    yaw = f(np.arctan2(np.float64(T[1, 0]), np.float64(T[0, 0])))
    return np.array([roll, pitch, yaw, T[0, 3], T[1, 3], T[2, 3]], np.float32).astype(np.float64)


def rzryrx(x, y, z):
    cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def sc_between(correction):
    """poseFrom.between(identity) = poseFrom^-1 as a 4x4 and its (roll, pitch, yaw, x, y, z)"""
    p = sc_pose_from(correction)
    Rf = rzryrx(p[0], p[1], p[2])
    B = np.eye(4)
    B[:3, :3] = Rf.T
    B[:3, 3] = Rf.T @ (-p[3:])
    b6 = np.array([np.arctan2(B[2, 1], B[2, 2]), np.arctan2(-B[2, 0], np.hypot(B[2, 1], B[2, 2])), np.arctan2(B[1, 0], B[0, 0]), B[0, 3], B[1, 3], B[2, 3]])
    return p, B, b6
