// host_util.h -- host-side plumbing shared by the operators behind the C ABI: the HIP error check of functions that report
// through a context, grow-only device and pinned buffers, the argument check and the loader of strided xyz(w) records, and a
// few one-line helpers.  Host code only; device helpers live in pcm_device.h / loam_device.h.
#pragma once

#include "pcm_host.h"

// a failed HIP call: its text and the runtime's message into the context's error string, PCM_ERR_HIP to the caller
#define PCM_HIPCK(ctx, x)                                                            \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      (ctx)->err = std::string(#x) + ": " + hipGetErrorString(e_);                   \
      return PCM_ERR_HIP;                                                            \
    }                                                                                \
  } while (0)

namespace pcm {

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool finite_f(float v) { return v == v && v <= 3.402823466e38f && v >= -3.402823466e38f; }
// the key-frame store's check of poses and leaves: it has always stopped short of FLT_MAX
inline bool finite_f_3e38(float v) { return v == v && v <= 3.0e38f && v >= -3.0e38f; }
inline bool finite_d(double v) { return v == v && v <= 1.7976931348623157e308 && v >= -1.7976931348623157e308; }

inline int hip_failure(std::string* err, const char* call, const char* what, hipError_t e) {
  *err = std::string(call) + "(" + what + "): " + hipGetErrorString(e);
  return PCM_ERR_HIP;
}

// Room for `need` elements in the grow-only array (*p, *cap).  On growth the array is replaced by one of new_cap elements (the
// caller's growth formula; at least one element is allocated, so the pointer is never null afterwards) and the old contents are
// dropped: the stream is synchronised first (queued kernels may still read the old array), and after a failed hipMalloc the
// pair is (null, 0), so nothing freed stays reachable.  zero: a new array is cleared.  what: the array's name in an error text.
template <typename T>
int dev_reserve(T** p, size_t* cap, size_t need, size_t new_cap, hipStream_t stream, std::string* err, bool zero = false, const char* what = "device buffer") {
  if (*p && need <= *cap) return PCM_OK;
  if (*p) { (void)hipStreamSynchronize(stream); hipFree(*p); }
  *p = nullptr; *cap = 0;
  const size_t bytes = sizeof(T) * (new_cap ? new_cap : 1);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(p), bytes);
  if (e != hipSuccess) { *p = nullptr; return hip_failure(err, "hipMalloc", what, e); }
  if (zero && (e = hipMemset(*p, 0, bytes)) != hipSuccess) return hip_failure(err, "hipMemset", what, e);
  *cap = new_cap;
  return PCM_OK;
}

// The same, but the first `keep` elements move to the new array (device to device).  The new array is allocated first; the old
// one stays valid and owned until the copy has completed (hipStreamSynchronize), and when anything fails the new one is freed and
// the pair is unchanged.
template <typename T>
int dev_reserve_keep(T** p, size_t* cap, size_t need, size_t new_cap, size_t keep, hipStream_t stream, std::string* err, const char* what = "device buffer") {
  if (*p && need <= *cap) return PCM_OK;
  T* q = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&q), sizeof(T) * (new_cap ? new_cap : 1));
  if (e != hipSuccess) return hip_failure(err, "hipMalloc", what, e);
  if (*p) {
    e = keep ? hipMemcpyAsync(q, *p, sizeof(T) * keep, hipMemcpyDeviceToDevice, stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(stream);   // without a copy too: queued kernels may still read the old array
    if (e != hipSuccess) { hipFree(q); return hip_failure(err, "growth", what, e); }
    hipFree(*p);
  }
  *p = q; *cap = new_cap;
  return PCM_OK;
}

// an owned grow-only device array; freed with its owner.  what: its name in the error text of a failed growth.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;   // elements (the new_cap of the last growth)
  const char* what;
  explicit DevBuf(const char* w = "device buffer") : what(w) {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  // the caller has made sure that nothing queued reads the array
  void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
  // takes over an allocation of n elements the caller made (a growth that is more than a copy); same condition as release()
  void adopt(T* q, size_t n) { release(); p = q; cap = n; }
  int reserve(pcm_ctx* c, size_t need, size_t new_cap, bool zero = false) { return dev_reserve(&p, &cap, need, new_cap, c->stream, &c->err, zero, what); }
  int reserve_keep(pcm_ctx* c, size_t need, size_t new_cap, size_t keep) { return dev_reserve_keep(&p, &cap, need, new_cap, keep, c->stream, &c->err, what); }
};

// an owned grow-only block of pinned host memory (staging of uploads and read-backs); growth drops the contents
template <typename T>
struct PinnedBuf {
  T* p = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
  operator T*() const { return p; }
  void release() { if (p) hipHostFree(p); p = nullptr; cap = 0; }
  int reserve(pcm_ctx* c, size_t need, size_t new_cap) {
    if (p && need <= cap) return PCM_OK;
    if (p) { (void)hipStreamSynchronize(c->stream); hipHostFree(p); }   // a queued copy may still use the old block
    p = nullptr; cap = 0;
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(T) * (new_cap ? new_cap : 1));
    if (e != hipSuccess) { p = nullptr; return hip_failure(&c->err, "hipHostMalloc", "pinned buffer", e); }
    cap = new_cap;
    return PCM_OK;
  }
};

// n records of `stride` bytes that begin with three floats, in host or device memory.  check_memory = false: the caller reads
// every value other than PCM_MEM_DEVICE as host memory (pcm_set_*, pcm_loam_set_*) and `memory` is not looked at.
inline int check_point_records(pcm_ctx* c, const void* pts, size_t n, size_t stride, int memory, size_t max_n, bool check_memory = true) {
  if (!pts && n) { c->err = "null point buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  if (stride < 3 * sizeof(float) || (stride % sizeof(float)) != 0) { c->err = "stride must be a multiple of 4 and >= 12 bytes"; return PCM_ERR_INVALID_ARGUMENT; }
  if (check_memory && memory != PCM_MEM_HOST && memory != PCM_MEM_DEVICE) { c->err = "memory must be PCM_MEM_HOST or PCM_MEM_DEVICE"; return PCM_ERR_INVALID_ARGUMENT; }
  if (n > max_n) { c->err = "cloud too large"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

// voxel_hash.hip: n strided records -> float4 rows (x, y, z, w) on the context's stream; w is the record's fourth float when it
// has one (stride >= 16) and want_w, else 0.  Host records: one 2-D copy, after a clear of the rows when w is not copied.
int load_xyzw_rows(pcm_ctx* c, const void* pts, size_t n, size_t stride, int memory, bool want_w, float4* dst);

}  // namespace pcm
