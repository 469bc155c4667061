// arena_carver.h -- how the pre-processing operators and the entry points in front of them lay device memory out: blocks at
// 256-byte steps from one base, carved by a layout function.  A layout run over a null base is the size query, the same layout run
// over the real base is the carve, so the two cannot disagree.  No allocation, no growth, no overflow policing: the caller makes
// room for used() bytes (take_pre_arena, a DevBuf) between the two runs.  Host code, no HIP header (tests/arena_carver_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <initializer_list>

#include "../../include/pcm_amd.h"

namespace pcm {

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

class ArenaCarver {
 public:
  explicit ArenaCarver(void* base = nullptr) : base_(static_cast<char*>(base)) {}
  // the next block: n elements of T (null over a null base); n = 0 is the current position and takes nothing
  template <class T> T* take(size_t n) {
    char* p = base_ ? base_ + used_ : nullptr;
    used_ += up256(sizeof(T) * n);
    return reinterpret_cast<T*>(p);
  }
  // one block shared by alternatives that are never alive together (the operators of a frame, one after the other): the largest
  void* take_largest(std::initializer_list<size_t> bytes) { return take<char>(std::max(bytes)); }
  size_t used() const { return used_; }

 private:
  char* base_;
  size_t used_ = 0;
};

// The carver of an entry point whose buffers may be the caller's host memory: a host buffer gets a block of the arena and a copy,
// a device buffer is used where it is.  Copy queues on the entry point's stream: int h2d(dst, src, bytes), int d2h(dst, src, bytes),
// PCM_OK or the error (StreamCopy in pcm_host.h).  Over a null base nothing is copied; the first error stays in rc.
template <class Copy>
struct Stage : ArenaCarver {
  Copy copy;
  int rc = PCM_OK;
  Stage(void* base, Copy cp) : ArenaCarver(base), copy(cp) {}
  // host memory -> the block dst
  template <class T> T* upload(T* dst, const void* src, size_t bytes) {
    if (dst && bytes && rc == PCM_OK) rc = copy.h2d(dst, src, bytes);
    return dst;
  }
  // where the operator reads `bytes` of the caller's `user`: a staged copy of host memory, or `user` itself
  const void* in(int memory, const void* user, size_t bytes) { return memory == PCM_MEM_HOST ? upload(take<char>(bytes), user, bytes) : user; }
  // where the operator writes up to `bytes` for the caller's `user`; stage_back returns what it wrote
  void* out(int memory, void* user, size_t bytes) { return memory == PCM_MEM_HOST ? take<char>(bytes) : user; }
};
// after the operator: `bytes` from the block Stage::in or Stage::out gave back to the caller's host memory (nothing for device memory)
template <class Copy> int stage_back(Copy copy, int memory, void* user, const void* dev, size_t bytes) {
  return memory == PCM_MEM_HOST && bytes ? copy.d2h(user, dev, bytes) : PCM_OK;
}

}  // namespace pcm
