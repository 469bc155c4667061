// dev_buf.h -- the project's one way to hold device and pinned host memory: the HIP error checks, grow-only owned buffers
// (the 256-byte round-up is arena_carver.h's).  Knows nothing of the context (pcm_host.h holds these buffers as members and adds the pcm_ctx forms).
// Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>

#include "../../include/pcm_amd.h"
#include "arena_carver.h"

// a failed HIP call: its text and the runtime's message into *errptr, PCM_ERR_HIP to the caller
#define PCM_HIPCK_ERR(errptr, x)                                                     \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      *(errptr) = std::string(#x) + ": " + hipGetErrorString(e_);                    \
      return PCM_ERR_HIP;                                                            \
    }                                                                                \
  } while (0)
// the same into the context's error string
#define PCM_HIPCK(ctx, x) PCM_HIPCK_ERR(&(ctx)->err, x)

struct pcm_ctx;

namespace pcm {

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
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(what, o.what); }
  int reserve(hipStream_t stream, std::string* err, size_t need, size_t new_cap, bool zero = false) { return dev_reserve(&p, &cap, need, new_cap, stream, err, zero, what); }
  int reserve_keep(hipStream_t stream, std::string* err, size_t need, size_t new_cap, size_t keep) { return dev_reserve_keep(&p, &cap, need, new_cap, keep, stream, err, what); }
  // on the context's stream, into its error string (pcm_host.h)
  int reserve(pcm_ctx* c, size_t need, size_t new_cap, bool zero = false);
  int reserve_keep(pcm_ctx* c, size_t need, size_t new_cap, size_t keep);
};

// an owned grow-only block of pinned host memory (staging of uploads and read-backs, status bytes the device stores); growth
// drops the contents.  flags: hipHostMalloc's (the owner of a hipHostMallocMapped block asks hipHostGetDevicePointer for its device view).
template <typename T>
struct PinnedBuf {
  T* p = nullptr;
  size_t cap = 0;
  const char* what;
  explicit PinnedBuf(const char* w = "pinned buffer") : what(w) {}
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
  operator T*() const { return p; }
  void release() { if (p) hipHostFree(p); p = nullptr; cap = 0; }
  void swap(PinnedBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(what, o.what); }
  int reserve(hipStream_t stream, std::string* err, size_t need, size_t new_cap, unsigned flags = hipHostMallocDefault) {
    if (p && need <= cap) return PCM_OK;
    if (p) { (void)hipStreamSynchronize(stream); hipHostFree(p); }   // a queued copy may still use the old block
    p = nullptr; cap = 0;
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(T) * (new_cap ? new_cap : 1), flags);
    if (e != hipSuccess) { p = nullptr; return hip_failure(err, "hipHostMalloc", what, e); }
    cap = new_cap;
    return PCM_OK;
  }
  int reserve(pcm_ctx* c, size_t need, size_t new_cap, unsigned flags = hipHostMallocDefault);
};

}  // namespace pcm
