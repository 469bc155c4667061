// icp_hooks.cpp -- the host half of csrc/icp.h (and the SC pose algebra of csrc/loam_loop.h) behind a C interface, built with g++
// by tests/test_icp.py: the very functions the device loop and pcm_loam_sc_loop_verify evaluate.
#include <stddef.h>
#include <string.h>

#include "icp.h"
#include "loam_loop.h"
#include "pcm_amd.h"

using namespace pcm;

extern "C" {

// sums: the 17 values of a row -> R (9), t (3); returns S(2)
int icp_hook_umeyama(const double* sums, double* R, double* t) { return icp::umeyama_step(sums, R, t); }

// the row of m pairs (c, q as float xyz triples), added in index order
void icp_hook_sums(const float* c, const float* q, int m, double* sums) {
  for (int k = 0; k < icp::kSums; k++) sums[k] = 0.0;
  for (int i = 0; i < m; i++) {
    double v[icp::kSums];
    icp::pair_terms(c + 3 * i, q + 3 * i, icp::sq_dist(q + 3 * i, c + 3 * i), v);
    for (int k = 0; k < icp::kSums; k++) sums[k] += v[k];
  }
}

void icp_hook_transform(const double* F, const float* s, int n, float* out) {
  float m[12];
  icp::pose_to_float(F, m);
  for (int i = 0; i < n; i++) icp::transform_point(m, s[3 * i], s[3 * i + 1], s[3 * i + 2], out + 3 * i);
}

int icp_hook_keep(float d2, double max_correspondence_distance) { return icp::keep_pair(d2, icp::max_sq_of(max_correspondence_distance)) ? 1 : 0; }

static icp::Params params_of(const pcm_icp_params* p) {
  icp::Params P;
  P.max_iterations = p->max_iterations;
  P.max_sq = icp::max_sq_of(p->max_correspondence_distance);
  P.transformation_epsilon = p->transformation_epsilon;
  P.rot_thr = icp::rot_thr_of(p->rotation_epsilon, p->transformation_epsilon);
  P.euclidean_fitness_epsilon = p->euclidean_fitness_epsilon;
  P.mse_absolute = p->mse_absolute;
  return P;
}

int icp_hook_convergence(const pcm_icp_params* p, int k, const double* R, const double* t, double mse, double* prev_mse) {
  return icp::convergence(params_of(p), k, R, t, mse, prev_mse);
}

// a whole loop over given sum rows: F (16, in: the guess as doubles; out), out4 = iterations, converged, stop, done
void icp_hook_loop(const pcm_icp_params* p, const float* guess, const double* rows, int nrows, double* F, int* out4, double* mse) {
  icp::Loop L;
  icp::loop_begin(&L, guess);
  const icp::Params P = params_of(p);
  for (int k = 0; k < nrows && !L.done; k++) icp::loop_step(P, rows + (size_t)k * icp::kSums, &L);
  memcpy(F, L.F, sizeof(L.F));
  out4[0] = L.iterations; out4[1] = L.converged; out4[2] = L.stop; out4[3] = L.done;
  *mse = L.mse;
}

void icp_hook_sc_factor(const float* correction, double* from6, double* to6, double* B16, double* b6) { loam::loop::sc_loop_factor(correction, from6, to6, B16, b6); }

// sizeof and offsets of the new structs: params (8 numbers), info (7), sc params (12), sc result (19)
void icp_hook_layout(size_t* o) {
  size_t k = 0;
  o[k++] = sizeof(pcm_icp_params); o[k++] = offsetof(pcm_icp_params, max_iterations); o[k++] = offsetof(pcm_icp_params, max_correspondence_distance);
  o[k++] = offsetof(pcm_icp_params, transformation_epsilon); o[k++] = offsetof(pcm_icp_params, rotation_epsilon);
  o[k++] = offsetof(pcm_icp_params, euclidean_fitness_epsilon); o[k++] = offsetof(pcm_icp_params, mse_absolute); o[k++] = offsetof(pcm_icp_params, reserved);
  o[k++] = sizeof(pcm_icp_info); o[k++] = offsetof(pcm_icp_info, stop_reason); o[k++] = offsetof(pcm_icp_info, iterations); o[k++] = offsetof(pcm_icp_info, converged);
  o[k++] = offsetof(pcm_icp_info, num_pairs); o[k++] = offsetof(pcm_icp_info, mse); o[k++] = offsetof(pcm_icp_info, reserved);
  o[k++] = sizeof(pcm_loam_sc_loop_params); o[k++] = offsetof(pcm_loam_sc_loop_params, icp_max_correspondence_distance); o[k++] = offsetof(pcm_loam_sc_loop_params, reserved);
  o[k++] = sizeof(pcm_loam_sc_loop_result); o[k++] = offsetof(pcm_loam_sc_loop_result, fitness); o[k++] = offsetof(pcm_loam_sc_loop_result, correction);
  o[k++] = offsetof(pcm_loam_sc_loop_result, between); o[k++] = offsetof(pcm_loam_sc_loop_result, reserved);
}

}  // extern "C"
