// lio_predict.h -- arithmetic of jueying_lio's IMU forward propagation, host + device, double precision throughout.
//
// Restates, for state_ikfom (use-ikfom.hpp:14-15) and on the manifold pieces of lio_iekf.h:
//   get_f, df_dx, df_dw                        use-ikfom.hpp:35-72       (24-row "flatted" layout: rows 0-20 = DOF indices, grav rows 21-23)
//   esekf::predict(dt, Q, in)                  esekfom.hpp:269-374       (the dense, non-USE_sparse branch)
//   the forward loop of ImuProcess::UndistortPcl   imu_processing.hpp:167-243
//   ImuProcess::IMUInit and the init branch of ImuProcess::Process   imu_processing.hpp:113-163, 295-315   (host only)
// quirks included:
//   (a) the exponentials that build the diagonal blocks of F_x1 are scaled by scalar_type(1 / 2) == 0: the SO3 blocks stay the
//       identity, the S2 block is Nx(x_after) * Mx(x_before, 0)                                        esekfom.hpp:305,336
//   (b) S2_Mx is called with a zero delta: its -hat(vec) branch                                        esekfom.hpp:334,340
//   (c) A_matrix is the identity below a norm of 1e-11                                                 mtkmath.hpp:238
//   (d) Q_ is 12 x 12 with the caller's four diagonals (cov_gyr, cov_acc, cov_bias_gyr, cov_bias_acc) and zeros elsewhere
//                                                                                                      imu_processing.hpp:217-220
//   - acc_avr is scaled by G_m_s2 = 9.81 over |mean_acc| while the S2 length is 9.809                  imu_processing.hpp:207
// Pinned where the reference reads an undefined value:
//   - acc_s_last_ (never initialised by the constructor) is zero until the first propagation writes it
//   - `in` of the closing predict is zero when every pair of the frame was skipped
//
// Written for `lanes` cooperating lanes through the executor of lio_iekf.h (the device: one 64-lane wave; a host caller: one).
// State-sized pieces are computed by every lane alike in registers; P, F_x1, one 23 x 23 temporary and the 23 x 12 noise Jacobian
// live in the Work block (LDS on the device) and are spread over the lanes element-wise.  Every output element is summed by one
// lane in a fixed order, structural zeros included.
#pragma once

#include "lio_iekf.h"

namespace pcm {
namespace predict {

using iekf::N;
using iekf::NN;
using iekf::State;

constexpr int NW = 12;              // process_noise_ikfom::DOF: ng, na, nbg, nba
constexpr int kMaxSamples = 1024;   // IMU samples of one call
constexpr double kG = 9.81;         // common::G_m_s2
constexpr int kMaxIniCount = 20;    // MAX_INI_COUNT  imu_processing.hpp:19

struct Sample {   // = pcm_imu_sample
  double t, acc[3], gyr[3];
};
struct Pose {     // = pcm_imu_pose
  double offset_time, acc[3], gyr[3], vel[3], pos[3], rot[9];
};
struct Input {    // input_ikfom
  double acc[3], gyr[3];
};
struct ImuState {   // = pcm_lio_imu_state
  double mean_acc[3], mean_gyr[3], cov_acc[3], cov_gyr[3], cov_bias_gyr[3], cov_bias_acc[3];
  double cov_acc_scale[3], cov_gyr_scale[3];
  double lidar_T_wrt_imu[3], lidar_R_wrt_imu[4];
  double angvel_last[3], acc_s_last[3], last_lidar_end_time;
  Sample last_imu;
  int32_t init_iter_num, first_frame, need_init, reserved[5];
};
struct Frame {    // the block one call uploads; its n samples follow it
  Sample last_imu;
  double last_lidar_end_time, pcl_beg_time, pcl_end_time, mean_acc_norm;
  double q[NW];   // the diagonal of Q_
  State x;
  double P[NN];
  double angvel_last[3], acc_s_last[3];
  int32_t n, pad;
};
struct Result {   // the block one call downloads; its num_poses poses follow it
  State x;
  double P[NN];
  double angvel_last[3], acc_s_last[3];
  int32_t num_poses, pad;
};
struct Lin {      // the state-sized pieces of one predict
  double mRH[9], mR[9], Mx[6];   // blocks of df_dx / df_dw: -R hat(acc - ba), -R, S2_Mx(grav, 0)
  double A[2][9];                // A_matrix(-f dt) of rot, offset_R_L_I
  double E[2][9];                // their diagonal blocks of F_x1
  double G[4];                   // the S2 diagonal block of F_x1
  double S[6];                   // res_temp_S2
};
struct Work {     // scratch of a propagation (LDS on the device)
  double P[NN], F[NN], T[NN];
  double W[N * NW];              // dt * f_w_final
  Lin lin;
};

// ---- small dense products in Eigen's order of additions -------------------------------------------------------------------------
IEKF_HD void mul_23_33(const double* A, const double* B, double* C) {   // 2 x 3 * 3 x 3
  for (int r = 0; r < 2; r++)
    for (int c = 0; c < 3; c++) C[r * 3 + c] = (A[r * 3 + 0] * B[0 * 3 + c] + A[r * 3 + 1] * B[1 * 3 + c]) + A[r * 3 + 2] * B[2 * 3 + c];
}

// ---- get_f, df_dx, df_dw (use-ikfom.hpp:35-72) ----------------------------------------------------------------------------------
// f24: the flatted rows; only rows 0-2 (vel), 3-5 (gyro - bg) and 12-14 (rot * (acc - ba) + grav) are set by the reference
IEKF_HD void get_f(const State& s, const Input& in, double* f24) {
  for (int k = 0; k < 24; k++) f24[k] = 0.0;
  double am[3], a_inertial[3];
  for (int a = 0; a < 3; a++) am[a] = in.acc[a] - s.ba[a];
  iekf::quat_rot(s.rot, am, a_inertial);
  for (int a = 0; a < 3; a++) {
    f24[a] = s.vel[a];
    f24[a + 3] = in.gyr[a] - s.bg[a];
    f24[a + 12] = a_inertial[a] + s.grav[a];
  }
}
// the three non-constant blocks of df_dx (and the one of df_dw, which is mR again)
IEKF_HD void df_blocks(const State& s, const Input& in, Lin& L) {
  double R[9], H[9], am[3];
  const double zero2[2] = {0.0, 0.0};
  for (int a = 0; a < 3; a++) am[a] = in.acc[a] - s.ba[a];
  iekf::quat_to_rot(s.rot, R);
  iekf::hat(am, H);
  for (int k = 0; k < 9; k++) L.mR[k] = -R[k];
  iekf::mat33_mul(L.mR, H, L.mRH);
  iekf::s2_Mx(s.grav, zero2, L.Mx);
}
// f_x_(r, c): r a flatted row (0..23), c a DOF column (0..22)
IEKF_HD double fx(const Lin& L, int r, int c) {
  if (r < 3) return c == 12 + r ? 1.0 : 0.0;
  if (r < 6) return (c >= 15 && c < 18) ? (c == 12 + r ? -1.0 : -0.0) : 0.0;   // -Identity()
  if (r >= 12 && r < 15) {
    const int a = r - 12;
    if (c >= 3 && c < 6) return L.mRH[a * 3 + (c - 3)];
    if (c >= 18 && c < 21) return L.mR[a * 3 + (c - 18)];
    if (c >= 21) return L.Mx[a * 2 + (c - 21)];
  }
  return 0.0;
}
// f_w_(r, a): a a noise column (0..11)
IEKF_HD double fw(const Lin& L, int r, int a) {
  if (r >= 3 && r < 6) return a < 3 ? (a == r - 3 ? -1.0 : -0.0) : 0.0;
  if (r >= 12 && r < 15) return (a >= 3 && a < 6) ? L.mR[(r - 12) * 3 + (a - 3)] : 0.0;
  if (r >= 15 && r < 21) return a == r - 9 ? 1.0 : 0.0;
  return 0.0;
}
// f_x_final(r, c) / f_w_final(r, a), r a DOF row: vect_state rows copied, SO3 rows A * rows, S2 rows res_temp_S2 * rows  esekfom.hpp:280-362
IEKF_HD double fx_final(const Lin& L, int r, int c) {
  if (r >= 3 && r < 9) {
    const int s = r >= 6 ? 1 : 0, idx = s ? 6 : 3;
    const double* A = L.A[s] + (r - idx) * 3;
    return (A[0] * fx(L, idx, c) + A[1] * fx(L, idx + 1, c)) + A[2] * fx(L, idx + 2, c);
  }
  if (r >= 21) {
    const double* S = L.S + (r - 21) * 3;
    return (S[0] * fx(L, 21, c) + S[1] * fx(L, 22, c)) + S[2] * fx(L, 23, c);
  }
  return fx(L, r, c);
}
IEKF_HD double fw_final(const Lin& L, int r, int a) {
  if (r >= 3 && r < 9) {
    const int s = r >= 6 ? 1 : 0, idx = s ? 6 : 3;
    const double* A = L.A[s] + (r - idx) * 3;
    return (A[0] * fw(L, idx, a) + A[1] * fw(L, idx + 1, a)) + A[2] * fw(L, idx + 2, a);
  }
  if (r >= 21) {
    const double* S = L.S + (r - 21) * 3;
    return (S[0] * fw(L, 21, a) + S[1] * fw(L, 22, a)) + S[2] * fw(L, 23, a);
  }
  return fw(L, r, a);
}
// F_x1(r, c) before `+= f_x_final * dt`: the identity with its SO3 and S2 diagonal blocks overwritten  esekfom.hpp:279,314,349
IEKF_HD double fx1_base(const Lin& L, int r, int c) {
  if (r >= 3 && r < 9 && c >= 3 && c < 9 && (r >= 6) == (c >= 6)) {
    const int s = r >= 6 ? 1 : 0, idx = s ? 6 : 3;
    return L.E[s][(r - idx) * 3 + (c - idx)];
  }
  if (r >= 21 && c >= 21) return L.G[(r - 21) * 2 + (c - 21)];
  return r == c ? 1.0 : 0.0;
}

// The state-sized part of predict (esekfom.hpp:270-362): f, the blocks of df_dx / df_dw at x, x <- x.oplus(f, dt), and the pieces of
// f_x_final, f_w_final and F_x1 that depend on the state before and after.
IEKF_HD void linearize(State& x, const Input& in, double dt, Lin& L) {
  double f[24];
  get_f(x, in, f);
  df_blocks(x, in, L);
  double grav_before[3];
  for (int a = 0; a < 3; a++) grav_before[a] = x.grav[a];
  // x_.oplus(f_, dt): vect += dt * f; SO3: q * exp(f, dt / 2) (SOn.hpp:219-222); S2: R(exp(f, dt / 2)) * vec (S2.hpp:125-129)
  for (int a = 0; a < 3; a++) {
    x.pos[a] += dt * f[0 + a]; x.off_T[a] += dt * f[9 + a]; x.vel[a] += dt * f[12 + a];
    x.bg[a] += dt * f[15 + a]; x.ba[a] += dt * f[18 + a];
  }
  for (int s = 0; s < 2; s++) {
    double* q = s ? x.off_R : x.rot;
    double d[4], r[4];
    iekf::exp_quat(f + (s ? 6 : 3), dt / 2, d);
    iekf::quat_mul(q, d, r);
    for (int a = 0; a < 4; a++) q[a] = r[a];
  }
  {
    double d[4], Rm[9], r[3];
    iekf::exp_quat(f + 21, dt / 2, d);
    iekf::quat_to_rot(d, Rm);
    iekf::mat33_vec(Rm, x.grav, r);
    for (int a = 0; a < 3; a++) x.grav[a] = r[a];
  }
  for (int s = 0; s < 2; s++) {   // SO3_state  :298-323
    double seg[3], d[4];
    for (int a = 0; a < 3; a++) seg[a] = -1 * f[(s ? 6 : 3) + a] * dt;
    iekf::exp_quat(seg, (double)(1 / 2), d);   // integer division: scale 0, the identity rotation
    iekf::quat_to_rot(d, L.E[s]);
    iekf::A_matrix(seg, L.A[s]);
  }
  {   // S2_state  :328-362
    double seg[3], d[4], Rm[9], Nx[6], Mx[6], H[9], A[9], At[9], NR[6], NRH[6], mNx[6];
    const double zero2[2] = {0.0, 0.0};
    for (int a = 0; a < 3; a++) seg[a] = f[21 + a] * dt;
    iekf::exp_quat(seg, (double)(1 / 2), d);
    iekf::quat_to_rot(d, Rm);
    iekf::s2_Nx_yy(x.grav, Nx);
    iekf::s2_Mx(grav_before, zero2, Mx);
    mul_23_33(Nx, Rm, NR);
    for (int r = 0; r < 2; r++)
      for (int c = 0; c < 2; c++) L.G[r * 2 + c] = (NR[r * 3 + 0] * Mx[0 * 2 + c] + NR[r * 3 + 1] * Mx[1 * 2 + c]) + NR[r * 3 + 2] * Mx[2 * 2 + c];
    iekf::hat(grav_before, H);
    iekf::A_matrix(seg, A);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) At[r * 3 + c] = A[c * 3 + r];
    for (int k = 0; k < 6; k++) mNx[k] = -Nx[k];
    mul_23_33(mNx, Rm, NR);
    mul_23_33(NR, H, NRH);
    mul_23_33(NRH, At, L.S);
  }
}

// esekf::predict(dt, Q, in): x in registers (every lane alike), P in w.P.  q: the 12 diagonal entries of Q.
template <class Ex>
IEKF_HD void predict(const Ex& ex, State& x, Work& w, double dt, const double* q, const Input& in) {
  const int lane = ex.lane(), nl = ex.lanes();
  {
    Lin L;
    linearize(x, in, dt, L);
    if (lane == 0) w.lin = L;
  }
  ex.sync();
  const Lin& L = w.lin;
  for (int e = lane; e < NN; e += nl) {   // F_x1 = base; F_x1 += f_x_final * dt   :371
    const int r = e / N, c = e % N;
    w.F[e] = fx1_base(L, r, c) + fx_final(L, r, c) * dt;
  }
  for (int e = lane; e < N * NW; e += nl) w.W[e] = dt * fw_final(L, e / NW, e % NW);
  ex.sync();
  for (int e = lane; e < NN; e += nl) {   // T = F_x1 * P_
    const int r = e / N, c = e % N;
    double v = 0.0;
    for (int k = 0; k < N; k++) v += w.F[r * N + k] * w.P[k * N + c];
    w.T[e] = v;
  }
  ex.sync();
  for (int e = lane; e < NN; e += nl) {   // P_ = T * F_x1^T + (dt f_w_final) * Q * (dt f_w_final)^T   :372
    const int r = e / N, c = e % N;
    double v = 0.0, u = 0.0;
    for (int k = 0; k < N; k++) v += w.T[r * N + k] * w.F[c * N + k];
    for (int a = 0; a < NW; a++) u += (w.W[r * NW + a] * q[a]) * w.W[c * NW + a];
    w.P[e] = v + u;
  }
  ex.sync();
}

IEKF_HD void pose_of(double offset_time, const double* acc, const double* gyr, const State& x, Pose* p) {   // common::set_pose6d
  p->offset_time = offset_time;
  for (int a = 0; a < 3; a++) { p->acc[a] = acc[a]; p->gyr[a] = gyr[a]; p->vel[a] = x.vel[a]; p->pos[a] = x.pos[a]; }
  iekf::quat_to_rot(x.rot, p->rot);
}

// The forward loop of ImuProcess::UndistortPcl and the closing predict (imu_processing.hpp:167-243).  poses must hold fr.n + 1.
template <class Ex>
IEKF_HD void propagate(const Ex& ex, const Frame& fr, const Sample* smp, Result& out, Pose* poses, Work& w) {
  const int lane = ex.lane(), nl = ex.lanes();
  const int n = fr.n;
  State x = fr.x;
  double angvel_last[3], acc_s_last[3], q[NW];
  for (int a = 0; a < 3; a++) { angvel_last[a] = fr.angvel_last[a]; acc_s_last[a] = fr.acc_s_last[a]; }
  for (int a = 0; a < NW; a++) q[a] = fr.q[a];
  for (int e = lane; e < NN; e += nl) w.P[e] = fr.P[e];
  ex.sync();
  int np = 0;
  if (lane == 0) pose_of(0.0, acc_s_last, angvel_last, x, &poses[0]);
  np++;
  Input in;
  for (int a = 0; a < 3; a++) { in.acc[a] = 0.0; in.gyr[a] = 0.0; }
  const double last_end = fr.last_lidar_end_time;
  for (int i = 0; i < n; i++) {
    const Sample head = i ? smp[i - 1] : fr.last_imu;
    const Sample tail = smp[i];
    if (tail.t < last_end) continue;
    for (int a = 0; a < 3; a++) {
      in.gyr[a] = 0.5 * (head.gyr[a] + tail.gyr[a]);
      in.acc[a] = 0.5 * (head.acc[a] + tail.acc[a]);
    }
    for (int a = 0; a < 3; a++) in.acc[a] = in.acc[a] * kG / fr.mean_acc_norm;
    const double dt = head.t < last_end ? tail.t - last_end : tail.t - head.t;
    predict(ex, x, w, dt, q, in);
    double am[3], r[3];
    for (int a = 0; a < 3; a++) { angvel_last[a] = in.gyr[a] - x.bg[a]; am[a] = in.acc[a] - x.ba[a]; }
    iekf::quat_rot(x.rot, am, r);
    for (int a = 0; a < 3; a++) acc_s_last[a] = r[a] + x.grav[a];
    if (lane == 0) pose_of(tail.t - fr.pcl_beg_time, acc_s_last, angvel_last, x, &poses[np]);
    np++;
  }
  {
    const double imu_end_time = smp[n - 1].t;
    const double note = fr.pcl_end_time > imu_end_time ? 1.0 : -1.0;
    const double dt = note * (fr.pcl_end_time - imu_end_time);
    predict(ex, x, w, dt, q, in);
  }
  for (int e = lane; e < NN; e += nl) out.P[e] = w.P[e];
  if (lane == 0) {
    out.x = x;
    for (int a = 0; a < 3; a++) { out.angvel_last[a] = angvel_last[a]; out.acc_s_last[a] = acc_s_last[a]; }
    out.num_poses = np;
    out.pad = 0;
  }
  ex.sync();
}

// ---- host only: the constructor, Reset, IMUInit and the init branch of Process (imu_processing.hpp:71-98, 113-163, 295-315) -----
inline void default_imu_state(ImuState* s) {
  *s = ImuState{};
  for (int a = 0; a < 3; a++) {
    s->cov_acc[a] = 0.1; s->cov_gyr[a] = 0.1; s->cov_bias_gyr[a] = 0.0001; s->cov_bias_acc[a] = 0.0001;
    s->cov_acc_scale[a] = 0.1; s->cov_gyr_scale[a] = 0.1;   // mapping/acc_cov, mapping/gyr_cov  laser_mapping.cc:97-98
  }
  s->mean_acc[2] = -1.0;
  s->lidar_R_wrt_imu[3] = 1.0;
  s->init_iter_num = 1;
  s->first_frame = 1;
  s->need_init = 1;
}

// One init frame: IMUInit over the n samples, then the MAX_INI_COUNT switch.  x and P are the filter's (get_x / change_x, change_P).
inline void imu_init(ImuState* s, const Sample* imu, int n, State* x, double* P) {
  int Nn = s->init_iter_num;
  if (s->first_frame) {
    for (int a = 0; a < 3; a++) { s->mean_acc[a] = 0.0; s->mean_gyr[a] = 0.0; s->angvel_last[a] = 0.0; }   // Reset()
    s->mean_acc[2] = -1.0;
    s->need_init = 1;
    s->last_imu = Sample{};
    Nn = 1;
    s->first_frame = 0;
    for (int a = 0; a < 3; a++) { s->mean_acc[a] = imu[0].acc[a]; s->mean_gyr[a] = imu[0].gyr[a]; }
  }
  for (int i = 0; i < n; i++) {
    for (int a = 0; a < 3; a++) {
      const double cur_acc = imu[i].acc[a], cur_gyr = imu[i].gyr[a];
      s->mean_acc[a] += (cur_acc - s->mean_acc[a]) / Nn;
      s->mean_gyr[a] += (cur_gyr - s->mean_gyr[a]) / Nn;
      const double da = cur_acc - s->mean_acc[a], dg = cur_gyr - s->mean_gyr[a];
      s->cov_acc[a] = s->cov_acc[a] * (Nn - 1.0) / Nn + da * da * (Nn - 1.0) / (Nn * Nn);
      s->cov_gyr[a] = s->cov_gyr[a] * (Nn - 1.0) / Nn + dg * dg * (Nn - 1.0) / (Nn * Nn);
    }
    Nn++;
  }
  s->init_iter_num = Nn;
  const double* m = s->mean_acc;
  const double norm = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  {   // S2(-mean_acc / |mean_acc| * G_m_s2): the constructor normalises and scales to the S2 length (S2.hpp:120-123)
    double g[3];
    for (int a = 0; a < 3; a++) g[a] = -m[a] / norm * kG;
    const double z = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    if (z > 0.0) { const double sz = sqrt(z); for (int a = 0; a < 3; a++) g[a] /= sz; }
    for (int a = 0; a < 3; a++) x->grav[a] = g[a] * iekf::s2_length();
  }
  for (int a = 0; a < 3; a++) { x->bg[a] = s->mean_gyr[a]; x->off_T[a] = s->lidar_T_wrt_imu[a]; }
  for (int a = 0; a < 4; a++) x->off_R[a] = s->lidar_R_wrt_imu[a];
  for (int e = 0; e < NN; e++) P[e] = 0.0;
  for (int k = 0; k < N; k++) P[k * N + k] = 1.0;
  for (int k = 6; k < 12; k++) P[k * N + k] = 0.00001;
  for (int k = 15; k < 18; k++) P[k * N + k] = 0.0001;
  for (int k = 18; k < 21; k++) P[k * N + k] = 0.001;
  for (int k = 21; k < 23; k++) P[k * N + k] = 0.00001;
  s->last_imu = imu[n - 1];
  s->need_init = 1;
  if (s->init_iter_num > kMaxIniCount) {
    const double sc = pow(kG / norm, 2);
    for (int a = 0; a < 3; a++) s->cov_acc[a] *= sc;
    s->need_init = 0;
    for (int a = 0; a < 3; a++) { s->cov_acc[a] = s->cov_acc_scale[a]; s->cov_gyr[a] = s->cov_gyr_scale[a]; }
  }
}

// the host side of one propagation call: the block to upload from the caller's members ...
inline void fill_frame(const ImuState& s, const Sample* imu, int n, double pcl_beg_time, double pcl_end_time, const State& x, const double* P, Frame* fr, Sample* smp) {
  fr->last_imu = s.last_imu;
  fr->last_lidar_end_time = s.last_lidar_end_time;
  fr->pcl_beg_time = pcl_beg_time;
  fr->pcl_end_time = pcl_end_time;
  const double* m = s.mean_acc;
  fr->mean_acc_norm = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  for (int a = 0; a < 3; a++) { fr->q[a] = s.cov_gyr[a]; fr->q[3 + a] = s.cov_acc[a]; fr->q[6 + a] = s.cov_bias_gyr[a]; fr->q[9 + a] = s.cov_bias_acc[a]; }
  fr->x = x;
  for (int e = 0; e < NN; e++) fr->P[e] = P[e];
  for (int a = 0; a < 3; a++) { fr->angvel_last[a] = s.angvel_last[a]; fr->acc_s_last[a] = s.acc_s_last[a]; }
  fr->n = n;
  fr->pad = 0;
  for (int i = 0; i < n; i++) smp[i] = imu[i];
}
// ... and the members the reference leaves behind (imu_processing.hpp:225-226, 242-243)
inline void take_result(const Result& r, const Sample* imu, int n, double pcl_end_time, ImuState* s, State* x, double* P) {
  *x = r.x;
  for (int e = 0; e < NN; e++) P[e] = r.P[e];
  for (int a = 0; a < 3; a++) { s->angvel_last[a] = r.angvel_last[a]; s->acc_s_last[a] = r.acc_s_last[a]; }
  s->last_imu = imu[n - 1];
  s->last_lidar_end_time = pcl_end_time;
}
}  // namespace predict
}  // namespace pcm
