// lio_iekf.h -- arithmetic of jueying_lio's iterated error-state Kalman update, host + device, double precision throughout.
//
// Restates esekf::update_iterated_dyn_share_modified (jueying_lio/include/IKFoM_toolkit/esekfom/esekfom.hpp:1526-1834) for
// state_ikfom (use-ikfom.hpp:14-15: pos, rot, offset_R_L_I, offset_T_L_I, vel, bg, ba, grav; DOF 23) as a per-call state
// machine: one step() consumes the 92 sums of one ObsModel call (pcm_device.h kLioSums) and leaves the state, the covariance,
// the float pose of the next ObsModel call, its converge flag and a done flag.  The manifold pieces are those of
// mtk/types/SOn.hpp, mtk/types/S2.hpp (S2<double, 98090, 10000, 1>) and mtk/src/mtkmath.hpp, quirks included:
//   - S2_Mx scales its exponential with scalar(1 / 2) == 0: exp_delta is the identity                    S2.hpp:239
//   - S2::boxminus answers 3.1415926 (not pi) for antipodal vectors                                      S2.hpp:146
//   - cos_sinc_sqrt switches to its Taylor series below epsilon<double>^(1/4)                            mtkmath.hpp:153-160
//   - A_matrix is the identity below a norm of 1e-11                                                     mtkmath.hpp:238
//   - dx_new is re-projected, but the segments the projections are built from are read from dx         esekfom.hpp:1567,1586
//   - the closing covariance block reads dx_ (the update), not dx                                        esekfom.hpp:1744,1775
//   - P_ is a member: a loop that ends on an invalid call leaves the re-projected P_ of the last valid call
//   - SO3::boxminus goes through atan(nv / w) with nv clamped to 1e-11: a zero rotation gives 0 * vec    mtkmath.hpp:270-283
// Deliberate deviation: the `n > dof_Measurement` gain (esekfom.hpp:1618-1648) needs the rows of h_x; the information form of the
// else branch (:1685-1713) is used for every n_eff >= 1 (equal in exact arithmetic by the push-through identity).  K_h is
// P_inv(:, 0:12) * (h_x^T h) with the product h_x^T h summed by the reduction.
//
// A step is written for `lanes` cooperating lanes (the device: one 64-lane wave; a host caller: one) through an executor that
// supplies lane(), lanes() and sync().  Every small, state-sized piece is computed by all lanes alike in registers; the 23 x 23
// matrices live in the Work block (LDS on the device) and are spread over the lanes element-wise, row-wise or column-wise.
#pragma once

#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IEKF_HD __host__ __device__ inline
#else
#define IEKF_HD inline
#endif

namespace pcm {
namespace iekf {

constexpr int N = 23;             // state_ikfom::DOF
constexpr int NN = N * N;
constexpr int kMaxCalls = 16;     // ObsModel calls of one update: maximum_iter + 1 <= kMaxCalls
constexpr double kTol = 1e-11;    // MTK::tolerance<double>()
constexpr int kRot = 3, kOffR = 6, kGrav = 21;   // SO3_state = {3, 6}, S2_state = {21}

struct State {   // = pcm_lio_filter_state
  double pos[3], rot[4], off_R[4], off_T[3], vel[3], bg[3], ba[3], grav[3];
};
struct Params {
  double R;
  int32_t max_iter, extrinsic;
  double limit[N];
};
struct PoseF {   // = pcm::LioPose (pcm_device.h): the float state ObsModel reads, plus the converge flag of the call
  float q_wl[4], t_wl[3], off_t[3], off_R[9], Rt[9];
  int32_t rematch, pad;
};
struct Ctl {
  int32_t i;            // the loop variable of esekfom.hpp:1539 at the call about to be consumed (-1 first)
  int32_t t;
  int32_t converge;     // dyn_share.converge handed to the next ObsModel call
  int32_t done;
  int32_t iterations, rematches, valid_calls, n_eff_last;
  double sum_h2_last;
};
struct Trace {
  State x;              // the state the call was evaluated at
  int32_t converge, n_eff;
  double sums[90];      // HTH upper triangle (78) + HTh (12)
  double dx[N];         // dx_ of the call (zeros: invalid call)
};
struct Block {          // device-resident record of one update
  State x_prop;
  double P_prop[NN];
  Params prm;
  State x;              // x_
  double P[NN];         // P_
  Ctl ctl;
  Trace tr[kMaxCalls];
};
struct Work {           // scratch of a step (LDS on the device)
  double P[NN], T[NN], Pinv[NN], Kx[NN], L[NN];
  double dx_[N];
};

struct SerialExec {
  IEKF_HD int lane() const { return 0; }
  IEKF_HD int lanes() const { return 1; }
  IEKF_HD void sync() const {}
};

// ---- 3-vectors, quaternions (x, y, z, w), row-major 3 x 3 ---------------------------------------------------------------------
IEKF_HD void hat(const double* v, double* M) {
  M[0] = 0; M[1] = -v[2]; M[2] = v[1];
  M[3] = v[2]; M[4] = 0; M[5] = -v[0];
  M[6] = -v[1]; M[7] = v[0]; M[8] = 0;
}
IEKF_HD void mat33_mul(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[i * 3 + j] = (A[i * 3 + 0] * B[0 * 3 + j] + A[i * 3 + 1] * B[1 * 3 + j]) + A[i * 3 + 2] * B[2 * 3 + j];
}
IEKF_HD void mat33_vec(const double* A, const double* v, double* r) {
  for (int i = 0; i < 3; i++) r[i] = (A[i * 3 + 0] * v[0] + A[i * 3 + 1] * v[1]) + A[i * 3 + 2] * v[2];
}
IEKF_HD void quat_mul(const double* a, const double* b, double* r) {   // Eigen quaternion product
  r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
IEKF_HD void quat_rot(const double* q, const double* v, double* r) {   // Eigen _transformVector
  double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
  uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
  const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int a = 0; a < 3; a++) r[a] = v[a] + q[3] * uv[a] + c[a];
}
IEKF_HD void quat_to_rot(const double* q, double* R) {   // Eigen Quaternion::toRotationMatrix
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// ---- mtkmath.hpp ------------------------------------------------------------------------------------------------------------
IEKF_HD void cos_sinc_sqrt(double x2, double* cosi_out, double* sinc_out) {   // :149-180
  const double taylor_n_bound = 0.0001220703125;   // sqrt(sqrt(epsilon<double>())) = 2^-13
  if (x2 >= taylor_n_bound) {
    const double x = sqrt(x2);
    *cosi_out = cos(x);
    *sinc_out = sin(x) / x;
    return;
  }
  const double inv[7] = {1 / 3., 1 / 4., 1 / 5., 1 / 6., 1 / 7., 1 / 8., 1 / 9.};
  double cosi = 1., sinc = 1;
  double term = -1 / 2. * x2;
  for (int i = 0; i < 3; ++i) {
    cosi += term;
    term *= inv[2 * i];
    sinc += term;
    term *= -inv[2 * i + 1] * x2;
  }
  *cosi_out = cosi;
  *sinc_out = sinc;
}
IEKF_HD void exp_quat(const double* vec, double scale, double* q) {   // MTK::exp :248-254 -> (vec part, w)
  const double norm2 = (vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2];
  double c, s;
  cos_sinc_sqrt(scale * scale * norm2, &c, &s);
  const double mult = s * scale;
  q[0] = mult * vec[0]; q[1] = mult * vec[1]; q[2] = mult * vec[2];
  q[3] = c;
}
IEKF_HD void A_matrix(const double* v, double* A) {   // :234-245
  const double squaredNorm = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  const double norm = sqrt(squaredNorm);
  for (int k = 0; k < 9; k++) A[k] = (k % 4 == 0) ? 1.0 : 0.0;
  if (norm < kTol) return;
  double H[9], HH[9], H2[9];
  hat(v, H);
  const double c1 = (1 - cos(norm)) / squaredNorm, c2 = (1 - sin(norm) / norm) / squaredNorm;
  for (int k = 0; k < 9; k++) H2[k] = c2 * H[k];
  mat33_mul(H2, H, HH);
  for (int k = 0; k < 9; k++) A[k] = (A[k] + c1 * H[k]) + HH[k];
}

// ---- SO3 (SOn.hpp:210-216, 256-269) ------------------------------------------------------------------------------------------
IEKF_HD void so3_boxplus(double* q, const double* vec) {
  double d[4], r[4];
  exp_quat(vec, 1.0 / 2, d);
  quat_mul(q, d, r);
  for (int a = 0; a < 4; a++) q[a] = r[a];
}
IEKF_HD void so3_boxminus(const double* q, const double* other, double* res) {   // log(other.conjugate() * q), scale 2, +-periodic
  const double oc[4] = {-other[0], -other[1], -other[2], other[3]};
  double r[4];
  quat_mul(oc, q, r);
  double nv = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
  if (nv < kTol) nv = kTol;
  const double s = 2.0 / nv * atan(nv / r[3]);
  for (int a = 0; a < 3; a++) res[a] = s * r[a];
}

// ---- S2<double, 98090, 10000, 1> (S2.hpp) ------------------------------------------------------------------------------------
IEKF_HD double s2_length() { return 98090.0 / 10000.0; }
IEKF_HD void s2_Bx(const double* vec, double* B) {   // 3 x 2, the S2_typ == 1 branch :188-199
  const double length = s2_length();
  if (vec[0] + length > kTol) {
    B[0] = -vec[1]; B[1] = -vec[2];
    B[2] = length - vec[1] * vec[1] / (length + vec[0]); B[3] = -vec[2] * vec[1] / (length + vec[0]);
    B[4] = -vec[2] * vec[1] / (length + vec[0]); B[5] = length - vec[2] * vec[2] / (length + vec[0]);
    for (int k = 0; k < 6; k++) B[k] /= length;
  } else {
    for (int k = 0; k < 6; k++) B[k] = 0;
    B[1 * 2 + 1] = -1;
    B[2 * 2 + 0] = 1;
  }
}
IEKF_HD void s2_boxplus(double* vec, const double* delta) {   // :131-138
  double B[6], q[4], Rm[9], r[3];
  s2_Bx(vec, B);
  const double Bu[3] = {B[0] * delta[0] + B[1] * delta[1], B[2] * delta[0] + B[3] * delta[1], B[4] * delta[0] + B[5] * delta[1]};
  exp_quat(Bu, 1.0 / 2, q);
  quat_to_rot(q, Rm);
  mat33_vec(Rm, vec, r);
  for (int a = 0; a < 3; a++) vec[a] = r[a];
}
IEKF_HD void s2_boxminus(const double* vec, const double* other, double* res) {   // :140-158
  double Hv[9], hv[3];
  hat(vec, Hv);
  mat33_vec(Hv, other, hv);
  const double v_sin = sqrt((hv[0] * hv[0] + hv[1] * hv[1]) + hv[2] * hv[2]);
  const double v_cos = (vec[0] * other[0] + vec[1] * other[1]) + vec[2] * other[2];
  const double theta = atan2(v_sin, v_cos);
  if (v_sin < kTol) {
    if (fabs(theta) > kTol) { res[0] = 3.1415926; res[1] = 0; }
    else { res[0] = 0; res[1] = 0; }
    return;
  }
  double B[6], Ho[9], M1[6], M2[6];
  s2_Bx(other, B);
  hat(other, Ho);
  const double s = theta / v_sin;
  for (int r = 0; r < 2; r++) for (int c = 0; c < 3; c++) M1[r * 3 + c] = s * B[c * 2 + r];   // s * Bx^T
  for (int r = 0; r < 2; r++)
    for (int c = 0; c < 3; c++) M2[r * 3 + c] = (M1[r * 3 + 0] * Ho[0 * 3 + c] + M1[r * 3 + 1] * Ho[1 * 3 + c]) + M1[r * 3 + 2] * Ho[2 * 3 + c];
  for (int r = 0; r < 2; r++) res[r] = (M2[r * 3 + 0] * vec[0] + M2[r * 3 + 1] * vec[1]) + M2[r * 3 + 2] * vec[2];
}
IEKF_HD void s2_Nx_yy(const double* vec, double* Nx) {   // 2 x 3  :225-229
  const double length = s2_length();
  double B[6], Hv[9], M1[6];
  s2_Bx(vec, B);
  hat(vec, Hv);
  const double s = 1 / length / length;
  for (int r = 0; r < 2; r++) for (int c = 0; c < 3; c++) M1[r * 3 + c] = s * B[c * 2 + r];
  for (int r = 0; r < 2; r++)
    for (int c = 0; c < 3; c++) Nx[r * 3 + c] = (M1[r * 3 + 0] * Hv[0 * 3 + c] + M1[r * 3 + 1] * Hv[1 * 3 + c]) + M1[r * 3 + 2] * Hv[2 * 3 + c];
}
IEKF_HD void s2_Mx(const double* vec, const double* delta, double* Mx) {   // 3 x 2  :231-242
  double B[6], Hv[9];
  s2_Bx(vec, B);
  hat(vec, Hv);
  double M[9];
  if (sqrt(delta[0] * delta[0] + delta[1] * delta[1]) < kTol) {
    for (int k = 0; k < 9; k++) M[k] = -Hv[k];
  } else {
    const double Bu[3] = {B[0] * delta[0] + B[1] * delta[1], B[2] * delta[0] + B[3] * delta[1], B[4] * delta[0] + B[5] * delta[1]};
    double q[4], Rm[9], A[9], At[9], RH[9];
    exp_quat(Bu, (double)(1 / 2), q);   // integer division: scale 0, the identity rotation
    quat_to_rot(q, Rm);
    for (int k = 0; k < 9; k++) Rm[k] = -Rm[k];
    mat33_mul(Rm, Hv, RH);
    A_matrix(Bu, A);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) At[r * 3 + c] = A[c * 3 + r];
    mat33_mul(RH, At, M);
  }
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 2; c++) Mx[r * 2 + c] = (M[r * 3 + 0] * B[0 * 2 + c] + M[r * 3 + 1] * B[1 * 2 + c]) + M[r * 3 + 2] * B[2 * 2 + c];
}
IEKF_HD void s2_NxMx(const double* vec_x, const double* vec_prop, const double* seg, double* G) {   // res_temp_S2 = Nx * Mx, 2 x 2
  double Nx[6], Mx[6];
  s2_Nx_yy(vec_x, Nx);
  s2_Mx(vec_prop, seg, Mx);
  for (int r = 0; r < 2; r++)
    for (int c = 0; c < 2; c++) G[r * 2 + c] = (Nx[r * 3 + 0] * Mx[0 * 2 + c] + Nx[r * 3 + 1] * Mx[1 * 2 + c]) + Nx[r * 3 + 2] * Mx[2 * 2 + c];
}

// ---- state_ikfom (build_manifold.hpp:195-203) --------------------------------------------------------------------------------
IEKF_HD void state_boxplus(State& x, const double* d) {
  for (int a = 0; a < 3; a++) x.pos[a] += d[0 + a];
  so3_boxplus(x.rot, d + kRot);
  so3_boxplus(x.off_R, d + kOffR);
  for (int a = 0; a < 3; a++) { x.off_T[a] += d[9 + a]; x.vel[a] += d[12 + a]; x.bg[a] += d[15 + a]; x.ba[a] += d[18 + a]; }
  s2_boxplus(x.grav, d + kGrav);
}
IEKF_HD void state_boxminus(const State& x, const State& o, double* d) {
  for (int a = 0; a < 3; a++) {
    d[0 + a] = x.pos[a] - o.pos[a]; d[9 + a] = x.off_T[a] - o.off_T[a]; d[12 + a] = x.vel[a] - o.vel[a];
    d[15 + a] = x.bg[a] - o.bg[a]; d[18 + a] = x.ba[a] - o.ba[a];
  }
  so3_boxminus(x.rot, o.rot, d + kRot);
  so3_boxminus(x.off_R, o.off_R, d + kOffR);
  s2_boxminus(x.grav, o.grav, d + kGrav);
}

// the float state of an ObsModel call exactly as the reference casts it (laser_mapping.cc:602-603, 669-671)
IEKF_HD void pose_of(const State& s, PoseF* L) {
  double qwl[4], twl[3], Rd[9], ORd[9];
  quat_mul(s.rot, s.off_R, qwl);
  quat_rot(s.rot, s.off_T, twl);
  quat_to_rot(s.rot, Rd);
  quat_to_rot(s.off_R, ORd);
  for (int a = 0; a < 4; a++) L->q_wl[a] = (float)qwl[a];
  for (int a = 0; a < 3; a++) { L->t_wl[a] = (float)(twl[a] + s.pos[a]); L->off_t[a] = (float)s.off_T[a]; }
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { L->Rt[i * 3 + j] = (float)Rd[j * 3 + i]; L->off_R[i * 3 + j] = (float)ORd[i * 3 + j]; }
}

// ---- 23 x 23 inverse: LU with partial pivoting, then one column of the inverse per lane ----------------------------------------
// A (row-major, n x n) is overwritten by its factors; Inv receives A^-1.  Lanes: the pivot search is done by every lane alike (n
// broadcast reads), the row swap and the multipliers take one element per lane, the trailing update is spread element-wise over
// all lanes, and each column of the inverse is one lane's forward + back substitution (its column of Inv is its scratch).
template <class Ex>
IEKF_HD void lu_inverse(const Ex& ex, double* A, double* Inv, int n) {
  const int lane = ex.lane(), nl = ex.lanes();
  int8_t perm[N];
  for (int i = 0; i < n; i++) perm[i] = (int8_t)i;
  for (int k = 0; k < n; k++) {
    int p = k;
    double best = fabs(A[k * n + k]);
    for (int i = k + 1; i < n; i++) {
      const double v = fabs(A[i * n + k]);
      if (v > best) { best = v; p = i; }
    }
    ex.sync();   // every lane has read column k before a swap moves it
    if (p != k) {
      const int8_t tp = perm[k]; perm[k] = perm[p]; perm[p] = tp;
      for (int j = lane; j < n; j += nl) { const double tv = A[k * n + j]; A[k * n + j] = A[p * n + j]; A[p * n + j] = tv; }
      ex.sync();
    }
    const double piv = A[k * n + k];
    for (int i = k + 1 + lane; i < n; i += nl) A[i * n + k] /= piv;
    ex.sync();
    const int m = n - k - 1;
    for (int e = lane; e < m * m; e += nl) {
      const int i = k + 1 + e / m, j = k + 1 + e % m;
      A[i * n + j] -= A[i * n + k] * A[k * n + j];
    }
    ex.sync();
  }
  for (int c = lane; c < n; c += nl) {
    for (int i = 0; i < n; i++) {   // L y = P e_c
      double v = (perm[i] == c) ? 1.0 : 0.0;
      for (int j = 0; j < i; j++) v -= A[i * n + j] * Inv[j * n + c];
      Inv[i * n + c] = v;
    }
    for (int i = n - 1; i >= 0; i--) {   // U x = y
      double v = Inv[i * n + c];
      for (int j = i + 1; j < n; j++) v -= A[i * n + j] * Inv[j * n + c];
      Inv[i * n + c] = v / A[i * n + i];
    }
  }
  ex.sync();
}

// rows [idx, idx + d) of M (all columns < ncols) <- G * them; G is d x d row-major (Gt != 0: use G^T).  One column per lane.
template <class Ex>
IEKF_HD void left_block(const Ex& ex, double* dst, const double* src, int idx, int d, const double* G, bool Gt, int ncols) {
  for (int i = ex.lane(); i < ncols; i += ex.lanes()) {
    double o[3], r[3];
    for (int k = 0; k < d; k++) o[k] = src[(idx + k) * N + i];
    for (int a = 0; a < d; a++) {
      double v = (Gt ? G[0 * d + a] : G[a * d + 0]) * o[0];
      for (int k = 1; k < d; k++) v += (Gt ? G[k * d + a] : G[a * d + k]) * o[k];
      r[a] = v;
    }
    for (int a = 0; a < d; a++) dst[(idx + a) * N + i] = r[a];
  }
  ex.sync();
}
// columns [idx, idx + d) of M <- them * G (Gt: * G^T).  One row per lane.
template <class Ex>
IEKF_HD void right_block(const Ex& ex, double* M, int idx, int d, const double* G, bool Gt) {
  for (int i = ex.lane(); i < N; i += ex.lanes()) {
    double o[3], r[3];
    for (int k = 0; k < d; k++) o[k] = M[i * N + idx + k];
    for (int a = 0; a < d; a++) {
      double v = o[0] * (Gt ? G[a * d + 0] : G[0 * d + a]);
      for (int k = 1; k < d; k++) v += o[k] * (Gt ? G[a * d + k] : G[k * d + a]);
      r[a] = v;
    }
    for (int a = 0; a < d; a++) M[i * N + idx + a] = r[a];
  }
  ex.sync();
}

// One pass of the loop body esekfom.hpp:1540-1833 with the sums of the ObsModel call just made (78 HTH upper + 12 HTh + sum h^2 +
// count).  Returns through b.ctl; `next` receives the float pose and converge flag of the following call.
template <class Ex>
IEKF_HD void step(const Ex& ex, Block& b, const double* sums, Work& w, PoseF* next) {
  const int lane = ex.lane(), nl = ex.lanes();
  Ctl c = b.ctl;
  if (c.done) return;
  const Params& prm = b.prm;
  const int i = c.i;
  const int n_eff = (int)sums[91];
  State x = b.x;
  ex.sync();   // every lane holds the call's control block and state before lane 0 rewrites them
  if (c.iterations < kMaxCalls) {
    Trace& tr = b.tr[c.iterations];
    if (lane == 0) { tr.x = x; tr.converge = c.converge; tr.n_eff = n_eff; }
    for (int k = lane; k < 90; k += nl) tr.sums[k] = sums[k];
    for (int k = lane; k < N; k += nl) tr.dx[k] = 0.0;
  }
  c.iterations += 1;
  c.rematches += c.converge ? 1 : 0;
  c.n_eff_last = n_eff;
  c.sum_h2_last = sums[90];
  bool exit_now = false;
  if (n_eff >= 1) {   // dyn_share.valid
    c.valid_calls += 1;
    double dx[N], dx_new[N];
    state_boxminus(x, b.x_prop, dx);
    for (int k = 0; k < N; k++) dx_new[k] = dx[k];
    for (int e = lane; e < NN; e += nl) w.P[e] = b.P_prop[e];
    ex.sync();
    for (int s = 0; s < 2; s++) {   // SO3_state  :1563-1578
      const int idx = s ? kOffR : kRot;
      double A[9], r[3];
      A_matrix(dx + idx, A);   // res_temp_SO3 = A^T
      for (int a = 0; a < 3; a++) r[a] = (A[0 * 3 + a] * dx_new[idx] + A[1 * 3 + a] * dx_new[idx + 1]) + A[2 * 3 + a] * dx_new[idx + 2];
      for (int a = 0; a < 3; a++) dx_new[idx + a] = r[a];
      left_block(ex, w.P, w.P, idx, 3, A, true, N);
      right_block(ex, w.P, idx, 3, A, false);
    }
    {   // S2_state  :1582-1601
      double G[4], r[2];
      s2_NxMx(x.grav, b.x_prop.grav, dx + kGrav, G);
      for (int a = 0; a < 2; a++) r[a] = G[a * 2 + 0] * dx_new[kGrav] + G[a * 2 + 1] * dx_new[kGrav + 1];
      dx_new[kGrav] = r[0]; dx_new[kGrav + 1] = r[1];
      left_block(ex, w.P, w.P, kGrav, 2, G, false, N);
      right_block(ex, w.P, kGrav, 2, G, true);
    }
    // P_temp = (P_ / R).inverse(); P_temp.block<12, 12>(0, 0) += HTH; P_inv = P_temp.inverse()   :1685-1706
    for (int e = lane; e < NN; e += nl) w.T[e] = w.P[e] / prm.R;
    ex.sync();
    lu_inverse(ex, w.T, w.Pinv, N);
    for (int e = lane; e < NN; e += nl) {
      const int r = e / N, cc = e % N;
      double v = w.Pinv[e];
      if (r < 12 && cc < 12) {
        const int a = r < cc ? r : cc, bb = r < cc ? cc : r;
        v += sums[a * 12 - a * (a - 1) / 2 + (bb - a)];
      }
      w.T[e] = v;
    }
    ex.sync();
    lu_inverse(ex, w.T, w.Pinv, N);
    // K_h, K_x (:1708-1713) and dx_ (:1719): one row per lane
    for (int r = lane; r < N; r += nl) {
      double kh = 0.0;
      for (int k = 0; k < 12; k++) kh += w.Pinv[r * N + k] * sums[78 + k];
      for (int cc = 0; cc < N; cc++) {
        double v = 0.0;
        if (cc < 12)
          for (int k = 0; k < 12; k++) {
            const int a = k < cc ? k : cc, bb = k < cc ? cc : k;
            v += w.Pinv[r * N + k] * sums[a * 12 - a * (a - 1) / 2 + (bb - a)];
          }
        w.Kx[r * N + cc] = v;
      }
      double acc = 0.0;
      for (int cc = 0; cc < N; cc++) acc += (w.Kx[r * N + cc] - (r == cc ? 1.0 : 0.0)) * dx_new[cc];
      w.dx_[r] = kh + acc;
    }
    ex.sync();
    double dx_[N];
    for (int k = 0; k < N; k++) dx_[k] = w.dx_[k];
    if (c.iterations - 1 < kMaxCalls) for (int k = lane; k < N; k += nl) b.tr[c.iterations - 1].dx[k] = dx_[k];
    state_boxplus(x, dx_);   // :1721
    c.converge = 1;
    for (int k = 0; k < N; k++)
      if (fabs(dx_[k]) > prm.limit[k]) { c.converge = 0; break; }
    if (c.converge) c.t++;
    if (!c.t && i == prm.max_iter - 2) c.converge = 1;
    if (c.t > 1 || i == prm.max_iter - 1) {   // :1735-1830
      exit_now = true;
      for (int e = lane; e < NN; e += nl) w.L[e] = w.P[e];
      ex.sync();
      for (int s = 0; s < 2; s++) {
        const int idx = s ? kOffR : kRot;
        double A[9];
        A_matrix(dx_ + idx, A);
        left_block(ex, w.L, w.P, idx, 3, A, true, N);
        left_block(ex, w.Kx, w.Kx, idx, 3, A, true, 12);
        right_block(ex, w.L, idx, 3, A, false);
        right_block(ex, w.P, idx, 3, A, false);
      }
      {
        double G[4];
        s2_NxMx(x.grav, b.x_prop.grav, dx_ + kGrav, G);
        left_block(ex, w.L, w.P, kGrav, 2, G, false, N);
        left_block(ex, w.Kx, w.Kx, kGrav, 2, G, false, 12);
        right_block(ex, w.L, kGrav, 2, G, true);
        right_block(ex, w.P, kGrav, 2, G, true);
      }
      for (int e = lane; e < NN; e += nl) {   // P_ = L_ - K_x.block<n, 12>(0, 0) * P_.block<12, n>(0, 0)
        const int r = e / N, cc = e % N;
        double v = 0.0;
        for (int k = 0; k < 12; k++) v += w.Kx[r * N + k] * w.P[k * N + cc];
        w.T[e] = w.L[e] - v;
      }
      ex.sync();
      for (int e = lane; e < NN; e += nl) b.P[e] = w.T[e];
    } else {
      for (int e = lane; e < NN; e += nl) b.P[e] = w.P[e];
    }
  }
  c.i = i + 1;
  if (exit_now || c.i >= prm.max_iter) c.done = 1;
  if (lane == 0) {
    b.x = x;
    b.ctl = c;
    pose_of(x, next);
    next->rematch = c.converge;
  }
  ex.sync();
}

// x_ = x_propagated, P_ = P_propagated, dyn_share.converge = true, t = 0, i = -1   :1528-1539
IEKF_HD void begin(Block& b) {
  b.x = b.x_prop;
  for (int e = 0; e < NN; e++) b.P[e] = b.P_prop[e];
  Ctl c{};
  c.i = -1;
  c.converge = 1;
  b.ctl = c;
}

}  // namespace iekf
}  // namespace pcm
