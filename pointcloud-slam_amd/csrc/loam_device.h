// loam_device.h -- what the LOAM scan-to-map kernels (loam.hip) and their host side (loam_api.hip) share.
#pragma once

#include "loam_step.h"
#include "pcm_device.h"

struct pcm_ctx;

namespace pcm {
namespace loam {

// one context of a (batched) LOAM optimisation, as the kernels read it
struct LoamDesc {
  TargetView map[2];       // [0] corner map, [1] surf map; pts.w = the point's index in the caller's cloud (raw bits)
  const float4* feats;     // body-frame features: n_c corner features, then n_s surf features
  uint32_t n_c, n_s;
  LoamState* st;
  double* partials;        // [cdiv(n_c + n_s, kLanes)][kSums]
  float4* coeff_out;       // parity hook: (coeff.xyz, intensity) per feature, x = NaN when not selected; nullptr: off
  int32_t* nn_out;         // parity hook: [feature][5] caller indices of the neighbours with d2 <= 1 (-1 pads); nullptr: off
  double* sums_out;        // parity hook: the step kernel exports the summed row instead of stepping; nullptr: step
  float x0[6];             // initial pose (roll, pitch, yaw, x, y, z)
  int32_t pad[2];
};

__host__ __device__ inline uint32_t num_blocks(uint32_t n) { return (n + kLanes - 1) / kLanes; }

// loam.hip
void launch_tag_input_index(hipStream_t stream, float4* pts, const uint32_t* order, uint32_t n);
void launch_init(hipStream_t stream, const LoamDesc* d_descs, int n);
// one iteration of every context still running: the correspondence pass, then the step kernel
void launch_round(hipStream_t stream, const LoamDesc* d_descs, int n, uint32_t max_blocks, const StepParams& p);

// loam_api.hip: the front end (loam_features.hip) writes the context's source features in place: room for n features, then
// the counts once they are on the device (the same state pcm_loam_set_source leaves)
int loam_source_reserve(pcm_ctx* c, size_t n, float4** feats);
void loam_source_commit(pcm_ctx* c, uint32_t n_c, uint32_t n_s);

}  // namespace loam
}  // namespace pcm
