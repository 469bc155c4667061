// g++ view of pointcloud-slam_amd/csrc/lio_iekf.h for tests/test_lio_iekf.py: the very functions k_iekf_step runs, with one lane.
#include <stddef.h>
#include <string.h>

#include "lio_iekf.h"
#include "pcm_amd.h"

using namespace pcm::iekf;

static_assert(sizeof(State) == sizeof(pcm_lio_filter_state), "state layout");
static_assert(offsetof(State, grav) == offsetof(pcm_lio_filter_state, grav), "state layout");

extern "C" {

// op: 0 so3 boxplus (q4, d3 -> q4)   1 so3 boxminus (q4, o4 -> 3)   2 s2 boxplus (v3, d2 -> v3)   3 s2 boxminus (v3, o3 -> 2)
//     4 A_matrix (v3 -> 9)   5 S2_Bx (v3 -> 6)   6 S2_Nx_yy (v3 -> 6)   7 S2_Mx (v3, d2 -> 6)   8 cos_sinc_sqrt (x2 -> 2)
//     9 state boxplus (26, 23 -> 26)   10 state boxminus (26, 26 -> 23)
void iekf_hook_op(int op, const double* a, const double* b, double* out) {
  switch (op) {
    case 0: memcpy(out, a, 32); so3_boxplus(out, b); break;
    case 1: so3_boxminus(a, b, out); break;
    case 2: memcpy(out, a, 24); s2_boxplus(out, b); break;
    case 3: s2_boxminus(a, b, out); break;
    case 4: A_matrix(a, out); break;
    case 5: s2_Bx(a, out); break;
    case 6: s2_Nx_yy(a, out); break;
    case 7: s2_Mx(a, b, out); break;
    case 8: cos_sinc_sqrt(a[0], out, out + 1); break;
    case 9: { State s; memcpy(&s, a, sizeof(s)); state_boxplus(s, b); memcpy(out, &s, sizeof(s)); break; }
    case 10: { State s, o; memcpy(&s, a, sizeof(s)); memcpy(&o, b, sizeof(o)); state_boxminus(s, o, out); break; }
  }
}

void iekf_hook_inverse(const double* A, double* Inv) {
  double T[NN];
  memcpy(T, A, sizeof(T));
  lu_inverse(SerialExec{}, T, Inv, N);
}

// x, P in/out; drives step() over `ncalls` rows of 96 sums.  ctl8: i, t, converge, done, iterations, rematches, valid_calls, n_eff_last.
// Stops early when done.  trace_dx: [ncalls][23], trace_flags: [ncalls][2] (converge, n_eff), poses: [ncalls][30] floats + flag.
int iekf_hook_run(double* x26, double* P, double R, int max_iter, const double* limit, const double* sums, int ncalls, int* ctl8, double* trace_dx,
                  int* trace_flags, float* poses) {
  static Block b;
  static Work w;
  memset(&b, 0, sizeof(b));
  memcpy(&b.x_prop, x26, sizeof(State));
  memcpy(b.P_prop, P, sizeof(b.P_prop));
  b.prm.R = R; b.prm.max_iter = max_iter; b.prm.extrinsic = 0;
  for (int k = 0; k < N; k++) b.prm.limit[k] = limit[k];
  begin(b);
  int made = 0;
  for (int k = 0; k < ncalls && !b.ctl.done; k++) {
    PoseF next;
    memset(&next, 0, sizeof(next));
    step(SerialExec{}, b, sums + 96 * k, w, &next);
    if (poses) memcpy(poses + 32 * k, &next, sizeof(next));
    made++;
  }
  for (int k = 0; k < made && k < kMaxCalls; k++) {
    memcpy(trace_dx + N * k, b.tr[k].dx, sizeof(double) * N);
    trace_flags[2 * k] = b.tr[k].converge; trace_flags[2 * k + 1] = b.tr[k].n_eff;
  }
  memcpy(x26, &b.x, sizeof(State));
  memcpy(P, b.P, sizeof(b.P));
  ctl8[0] = b.ctl.i; ctl8[1] = b.ctl.t; ctl8[2] = b.ctl.converge; ctl8[3] = b.ctl.done; ctl8[4] = b.ctl.iterations; ctl8[5] = b.ctl.rematches;
  ctl8[6] = b.ctl.valid_calls; ctl8[7] = b.ctl.n_eff_last;
  return made;
}

void iekf_hook_pose(const double* x26, float* pose32) {
  State s; memcpy(&s, x26, sizeof(s));
  PoseF p; memset(&p, 0, sizeof(p));
  pose_of(s, &p);
  memcpy(pose32, &p, sizeof(p));
}

void iekf_hook_layout(long* o) {
  o[0] = sizeof(pcm_lio_filter_state); o[1] = sizeof(pcm_lio_update_params); o[2] = sizeof(pcm_lio_update_result);
  o[3] = offsetof(pcm_lio_update_params, limit); o[4] = offsetof(pcm_lio_update_params, reserved);
  o[5] = offsetof(pcm_lio_update_result, sum_h2_last); o[6] = offsetof(pcm_lio_update_result, reserved); o[7] = sizeof(PoseF);
  o[8] = kMaxCalls;
}

}  // extern "C"
