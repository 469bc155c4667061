// host_util.h -- host-side plumbing shared by the operators behind the C ABI: the argument check and the loader of strided
// xyz(w) records and a few one-line helpers.  The HIP error checks and the grow-only device and pinned buffers are dev_buf.h's
// (through pcm_host.h).  Host code only; device helpers live in pcm_device.h / loam_device.h.
#pragma once

#include "pcm_host.h"

namespace pcm {

inline bool finite_f(float v) { return v == v && v <= 3.402823466e38f && v >= -3.402823466e38f; }
// the key-frame store's check of poses and leaves: it has always stopped short of FLT_MAX
inline bool finite_f_3e38(float v) { return v == v && v <= 3.0e38f && v >= -3.0e38f; }
inline bool finite_d(double v) { return v == v && v <= 1.7976931348623157e308 && v >= -1.7976931348623157e308; }

// n records of `stride` bytes that begin with three floats, in host or device memory.  check_memory = false: the caller reads
// every value other than PCM_MEM_DEVICE as host memory (pcm_set_*, pcm_loam_set_*) and `memory` is not looked at.
inline int check_point_records(pcm_ctx* c, const void* pts, size_t n, size_t stride, int memory, size_t max_n, bool check_memory = true) {
  if (!pts && n) { c->err = "null point buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  if (stride < 3 * sizeof(float) || (stride % sizeof(float)) != 0) { c->err = "stride must be a multiple of 4 and >= 12 bytes"; return PCM_ERR_INVALID_ARGUMENT; }
  if (check_memory && pcm::check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  if (n > max_n) { c->err = "cloud too large"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

// voxel_hash.hip: n strided records -> float4 rows (x, y, z, w) on the context's stream; w is the record's fourth float when it
// has one (stride >= 16) and want_w, else 0.  Host records: one 2-D copy, after a clear of the rows when w is not copied.
int load_xyzw_rows(pcm_ctx* c, const void* pts, size_t n, size_t stride, int memory, bool want_w, float4* dst);

}  // namespace pcm
