"""numpy restatement of jueying_slam's performLoopClosure after the two near clouds exist (mapOptmization.cpp:645-725): the size
gates (:652), the acceptance test (:693), tCorrect = correctionLidarFrame * tWrong (:711-713), pcl::getTranslationAndEulerAngles
(:714), Rot3::RzRyRx / Pose3 (:715-716) and poseFrom.between(poseTo) (:725).

Float where the reference is Eigen::Affine3f, double where it is GTSAM.  Every float step is a numpy float32 scalar operation
(one IEEE operation each, in the order pointcloud-slam_amd/csrc/loam_loop.h writes them); sin / cos / atan2 / asin are libm's
double functions (``math``) rounded to float32 where the reference calls them on floats -- the rule the header pins, since PCL,
Eigen and GTSAM are outside the reference tree.  ``dtype=np.float64`` evaluates the float part in double:
the yardstick of how much the float steps cost (tests/test_loam_loop.py)."""
import math

import numpy as np

ACCEPTED, REJECTED_SIZE, REJECTED_NOT_CONVERGED, REJECTED_FITNESS, NO_LOOP = 0, 1, 2, 3, 4
STATUS_NAMES = {ACCEPTED: "accepted", REJECTED_SIZE: "rejected_size", REJECTED_NOT_CONVERGED: "rejected_not_converged",
                REJECTED_FITNESS: "rejected_fitness", NO_LOOP: "no_loop"}

# the reference's values: utility.h:290-291, mapOptmization.cpp:652, :243 (mappingSurfLeafSize, utility.h:272), :684-686
DEFAULTS = dict(history_search_num=25, min_cur_points=300, min_prev_points=1000, wrt_key=-1, fitness_threshold=0.3, near_leaf=0.2,
                ndt_epsilon=0.01, ndt_resolution=1.0, ndt_num_neighbors=7)


def size_gate(n_cur, n_prev, min_cur=300, min_prev=1000):
    """:652 `if (cure->size() < 300 || prev->size() < 1000) return;` -> True when the pair goes on to NDT"""
    return not (n_cur < min_cur or n_prev < min_prev)


def accept_status(converged, fitness, threshold=0.3):
    """:693 `hasConverged() == false || getFitnessScore() > historyKeyframeFitnessScore` (a double against a float)"""
    if not converged:
        return REJECTED_NOT_CONVERGED
    if float(fitness) > float(np.float32(threshold)):
        return REJECTED_FITNESS
    return ACCEPTED


def _f(dtype, v):
    return dtype(v)


def affine_from_pose(pose6, dtype=np.float32):
    """pclPointToAffine3f = pcl::getTransformation(x, y, z, roll, pitch, yaw) from (roll, pitch, yaw, x, y, z): 4 x 4"""
    p = [dtype(v) for v in pose6]
    A, B = dtype(math.cos(float(p[2]))), dtype(math.sin(float(p[2])))
    Cc, D = dtype(math.cos(float(p[1]))), dtype(math.sin(float(p[1])))
    E, F = dtype(math.cos(float(p[0]))), dtype(math.sin(float(p[0])))
    DE, DF = D * E, D * F
    T = np.zeros((4, 4), dtype)
    T[0, 0] = A * Cc; T[0, 1] = A * DF - B * E; T[0, 2] = B * F + A * DE; T[0, 3] = p[3]
    T[1, 0] = B * Cc; T[1, 1] = A * E + B * DF; T[1, 2] = B * DE - A * F; T[1, 3] = p[4]
    T[2, 0] = -D; T[2, 1] = Cc * F; T[2, 2] = Cc * E; T[2, 3] = p[5]
    T[3, 3] = dtype(1)
    return T


def affine_mul(a, b, dtype=np.float32):
    """Eigen::Affine3f a * b: a row's three products summed left to right, the translation added last"""
    a = np.asarray(a, dtype); b = np.asarray(b, dtype)
    out = np.zeros((4, 4), dtype)
    for i in range(3):
        for j in range(3):
            out[i, j] = a[i, 0] * b[0, j] + a[i, 1] * b[1, j] + a[i, 2] * b[2, j]
        out[i, 3] = a[i, 0] * b[0, 3] + a[i, 1] * b[1, 3] + a[i, 2] * b[2, 3] + a[i, 3]
    out[3, 3] = dtype(1)
    return out


def _asin(v):
    return math.asin(v) if -1.0 <= v <= 1.0 else float("nan")   # libm's asin outside its domain (math.asin raises)


def pose_from_affine(T, dtype=np.float32):
    """pcl::getTranslationAndEulerAngles -> (roll, pitch, yaw, x, y, z)"""
    T = np.asarray(T, dtype)
    roll = dtype(math.atan2(float(T[2, 1]), float(T[2, 2])))
    pitch = dtype(_asin(float(-T[2, 0])))
    yaw = dtype(math.atan2(float(T[1, 0]), float(T[0, 0])))
    return np.array([roll, pitch, yaw, T[0, 3], T[1, 3], T[2, 3]], dtype)


def rzryrx(x, y, z):
    """gtsam::Rot3::RzRyRx(x = roll, y = pitch, z = yaw) = Rz(z) Ry(y) Rx(x), double"""
    cx, sx, cy, sy, cz, sz = math.cos(x), math.sin(x), math.cos(y), math.sin(y), math.cos(z), math.sin(z)
    ss_, cs_, sc_, cc_ = sx * sy, cx * sy, sx * cy, cx * cy
    c_s, s_s, _cs, _cc = cx * sz, sx * sz, cy * sz, cy * cz
    s_c, c_c, ssc, csc, sss, css = sx * cz, cx * cz, ss_ * cz, cs_ * cz, ss_ * sz, cs_ * sz
    return np.array([[_cc, -c_s + ssc, s_s + csc], [_cs, c_c + sss, -s_c + css], [-sy, sc_, cc_]], np.float64)


def between(from6, to6):
    """poseFrom.between(poseTo) = poseFrom^-1 * poseTo for (roll, pitch, yaw, x, y, z) doubles: (4 x 4, six numbers)"""
    f = [float(v) for v in from6]; t = [float(v) for v in to6]
    Rf, Rt = rzryrx(*f[:3]), rzryrx(*t[:3])
    d = [t[3] - f[3], t[4] - f[4], t[5] - f[5]]
    B = np.zeros((4, 4))
    for i in range(3):
        for j in range(3):
            B[i, j] = float(Rf[0, i]) * float(Rt[0, j]) + float(Rf[1, i]) * float(Rt[1, j]) + float(Rf[2, i]) * float(Rt[2, j])
        B[i, 3] = float(Rf[0, i]) * d[0] + float(Rf[1, i]) * d[1] + float(Rf[2, i]) * d[2]
    B[3, 3] = 1.0
    b6 = np.array([math.atan2(B[2, 1], B[2, 2]), math.atan2(-B[2, 0], math.sqrt(B[2, 1] * B[2, 1] + B[2, 2] * B[2, 2])),
                   math.atan2(B[1, 0], B[0, 0]), B[0, 3], B[1, 3], B[2, 3]])
    return B, b6


def loop_factor(correction, pose_cur, pose_pre, dtype=np.float32, swapped=False):
    """:706-725 -> dict(pose_from, pose_to, between, between6).  correction: ndt->getFinalTransformation() (4 x 4); the poses are
    the stored key poses (roll, pitch, yaw, x, y, z).  swapped=True is the deliberately wrong tWrong * correction."""
    Cm = np.asarray(correction, dtype).reshape(4, 4)
    tWrong = affine_from_pose(pose_cur, dtype)
    tCorrect = affine_mul(tWrong, Cm, dtype) if swapped else affine_mul(Cm, tWrong, dtype)
    pf = pose_from_affine(tCorrect, dtype).astype(np.float64)
    pt = np.asarray(pose_pre, dtype).astype(np.float64)
    B, b6 = between(pf, pt)
    return dict(pose_from=pf, pose_to=pt, between=B, between6=b6)


def perform_loop_closure(n_cur, n_prev, ndt, pose_cur, pose_pre, params=None):
    """:645-725 for one pair.  ndt: a callable returning (converged, iterations, correction 4 x 4 float32, fitness) -- it is called
    only when the size gates pass.  Returns a dict with the fields of pcm_loam_loop_result."""
    p = dict(DEFAULTS, **(params or {}))
    r = dict(status=REJECTED_SIZE, num_cur_points=int(n_cur), num_prev_points=int(n_prev), iterations=0, converged=False, fitness=0.0,
             noise_variance=0.0, correction=np.eye(4, dtype=np.float32), pose_from=np.zeros(6), pose_to=np.zeros(6),
             between=np.zeros((4, 4)), between6=np.zeros(6))
    if not size_gate(n_cur, n_prev, p["min_cur_points"], p["min_prev_points"]):
        return r
    converged, iterations, correction, fitness = ndt()
    r.update(iterations=int(iterations), converged=bool(converged), fitness=float(fitness), noise_variance=float(np.float32(fitness)),
             correction=np.asarray(correction, np.float32).reshape(4, 4))
    r["status"] = accept_status(converged, fitness, p["fitness_threshold"])
    if r["status"] == ACCEPTED:
        r.update(loop_factor(r["correction"], pose_cur, pose_pre))
    return r
