// dev_scratch.h -- the scratch of one device build: everything a build takes for its own duration comes from one DevScratch and
// goes back when it leaves scope, on every path.  Knows nothing of the context.  Host code only, but for the rocPRIM wrappers at the
// bottom, which a .hip file gets.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "dev_buf.h"

namespace pcm {

// Blocks are carved from the caller's arena (grow-only, owned elsewhere: a sliding map's update then makes no allocation call at
// all) while they fit, and come from the stream-ordered pool otherwise.  All of them live until release().
class DevScratch {
 public:
  explicit DevScratch(hipStream_t stream, char* arena = nullptr, size_t arena_bytes = 0) : stream_(stream), base_(arena), cap_(arena ? arena_bytes : 0) {}
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  ~DevScratch() { release(); }

  // n elements of T: a 256-byte-aligned carve of the arena, or a pool block (of at least one byte).  Failure: *p == nullptr,
  // PCM_ERR_HIP, and *err names `what`.
  template <class T>
  int take(T** p, size_t n, std::string* err, const char* what) {
    *p = nullptr;
    const size_t bytes = sizeof(T) * n, b = up256(bytes);
    if (base_ && b >= bytes && used_ + b <= cap_) { *p = reinterpret_cast<T*>(base_ + used_); used_ += b; return PCM_OK; }
    void* q = nullptr;
    const hipError_t e = hipMallocAsync(&q, bytes ? bytes : 1, stream_);
    if (e != hipSuccess) return hip_failure(err, "hipMallocAsync", what, e);
    pooled_.push_back(q);
    *p = static_cast<T*>(q);
    return PCM_OK;
  }

  // The temporary storage of a rocPRIM call: a block of at least `bytes`, the one handed out before unless that is too small.
  // One block serves every sort and scan of a build because all of a build's work is ordered on the one stream: a call has read
  // and written its temporary for the last time before the next call on the stream starts.
  int temp(void** p, size_t bytes, std::string* err) {
    if (!tmp_ || bytes > tmp_bytes_) {
      char* q = nullptr;
      if (const int rc = take(&q, bytes, err, "rocPRIM temporary"); rc != PCM_OK) { *p = nullptr; return rc; }
      tmp_ = q; tmp_bytes_ = bytes;
    }
    *p = tmp_;
    return PCM_OK;
  }

  // everything handed out goes back: the pool blocks behind the work queued on the stream, the arena to its owner's next build
  void release() {
    for (void* q : pooled_) (void)hipFreeAsync(q, stream_);
    pooled_.clear();
    used_ = 0;
    tmp_ = nullptr; tmp_bytes_ = 0;
    scan_n = scan_bytes = 0;
  }

  hipStream_t stream() const { return stream_; }
  size_t arena_used() const { return used_; }
  size_t scan_n = 0, scan_bytes = 0;   // scratch_exclusive_scan: the temporary's size that rocPRIM asked for a scan of scan_n elements

 private:
  hipStream_t stream_;
  char* base_;
  size_t cap_, used_ = 0;
  std::vector<void*> pooled_;
  void* tmp_ = nullptr;
  size_t tmp_bytes_ = 0;
};

}  // namespace pcm

#ifdef __HIPCC__
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace pcm {

// rocPRIM's calling sequence -- ask for the temporary's size, get it, run -- on the scratch's stream with the scratch's temporary.
// call(tmp, bytes) is the rocPRIM call; known_bytes != 0: a size that an earlier query of the same call gave for at least as much
// input, so this one is not made (a query is host work, but not free: it asks the runtime for the stream's device and its properties).
template <class F>
int scratch_run(DevScratch& sc, std::string* err, const char* what, F call, size_t* bytes_out = nullptr, size_t known_bytes = 0) {
  size_t bytes = known_bytes;
  void* tmp = nullptr;
  hipError_t e = bytes ? hipSuccess : call(nullptr, bytes);
  if (e != hipSuccess) return hip_failure(err, what, "size query", e);
  if (const int rc = sc.temp(&tmp, bytes, err); rc != PCM_OK) return rc;
  if ((e = call(tmp, bytes)) != hipSuccess) return hip_failure(err, what, "run", e);
  if (bytes_out) *bytes_out = bytes;
  return PCM_OK;
}
template <class KI, class KO, class VI, class VO>
int scratch_sort_pairs(DevScratch& sc, std::string* err, KI keys_in, KO keys_out, VI vals_in, VO vals_out, size_t n, unsigned begin_bit, unsigned end_bit) {
  return scratch_run(sc, err, "rocprim::radix_sort_pairs", [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, sc.stream()); });
}
template <class KI, class KO>
int scratch_sort_keys(DevScratch& sc, std::string* err, KI keys_in, KO keys_out, size_t n, unsigned begin_bit, unsigned end_bit) {
  return scratch_run(sc, err, "rocprim::radix_sort_keys", [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, keys_in, keys_out, n, begin_bit, end_bit, sc.stream()); });
}
// out[i] = in[0] + ... + in[i - 1] over uint32_t.  The size asked for the largest scan of this scratch so far serves every scan of
// no more elements (a build's scans repeat over the same arrays, or over their front after an eviction): one query, not one each.
template <class I, class O>
int scratch_exclusive_scan(DevScratch& sc, std::string* err, I in, O out, size_t n) {
  static_assert(sizeof(*in) == sizeof(uint32_t) && sizeof(*out) == sizeof(uint32_t), "one element type: the remembered size belongs to it");
  size_t bytes = 0;
  const int rc = scratch_run(sc, err, "rocprim::exclusive_scan", [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, in, out, 0u, n, rocprim::plus<uint32_t>(), sc.stream()); },
                             &bytes, n <= sc.scan_n ? sc.scan_bytes : 0);
  if (rc == PCM_OK && n > sc.scan_n) { sc.scan_n = n; sc.scan_bytes = bytes; }
  return rc;
}

}  // namespace pcm
#endif
