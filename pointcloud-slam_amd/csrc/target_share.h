// target_share.h -- how registration contexts hold a built target: a counted reference to one holder object.  A context that
// never shares is the only holder of its own; pcm_share_target makes a second context hold the same one.  The rules, which the
// callers in pcm_api.hip and lio_api.hip keep and tests/target_share_check.cpp walks through:
//   * a holder with more than one reference is immutable: whoever would change it asks mutable_by_me() first and refuses;
//   * attach / detach change one reference only: the other holders never notice;
//   * the last reference to go runs the release hook (device current, stream synchronised: the DevBuf rule of dev_buf.h) and
//     then deletes the holder, exactly once.
// The count is atomic: contexts that share a target may be driven, and destroyed, from different threads.
// Host code only, no HIP.
#pragma once

#include <atomic>
#include <new>
#include <utility>

namespace pcm {

template <class T>
class SharedTarget {
  struct Box {
    T value;
    std::atomic<int> holders{1};
  };
  Box* b_ = nullptr;

 public:
  SharedTarget() = default;
  SharedTarget(const SharedTarget&) = delete;
  SharedTarget& operator=(const SharedTarget&) = delete;
  // a reference that was not detached by its owner: the holder goes without a hook (nothing of it may be in use on a device)
  ~SharedTarget() { detach([] {}); }

  // a new, empty holder with this reference as its only one; false: out of host memory.  The reference must be empty.
  bool create() {
    b_ = new (std::nothrow) Box();
    return b_ != nullptr;
  }
  bool empty() const { return b_ == nullptr; }
  T* get() const { return b_ ? &b_->value : nullptr; }
  T* operator->() const { return &b_->value; }
  T& operator*() const { return b_->value; }
  // references to this holder (1 = not shared); 0 for an empty reference
  int holders() const { return b_ ? b_->holders.load(std::memory_order_acquire) : 0; }
  bool shared() const { return holders() > 1; }
  // a call that would change the target goes ahead only when this is true
  bool mutable_by_me() const { return holders() == 1; }
  bool same_as(const SharedTarget& o) const { return b_ == o.b_; }

  // Gives up this reference.  The last one calls before_free() and deletes the holder; returns whether it did.
  template <class Hook>
  bool detach(Hook&& before_free) {
    Box* b = b_;
    b_ = nullptr;
    if (!b || b->holders.fetch_sub(1, std::memory_order_acq_rel) != 1) return false;
    before_free();
    delete b;
    return true;
  }
  // Gives up this reference (as detach) and takes one to src's holder.  src must hold one, and not the same as this.
  template <class Hook>
  void attach(const SharedTarget& src, Hook&& before_free) {
    src.b_->holders.fetch_add(1, std::memory_order_acq_rel);
    Box* taken = src.b_;
    detach(std::forward<Hook>(before_free));
    b_ = taken;
  }
  // Gives up this reference (as detach) and becomes the only holder of a new, empty target.  false: out of host memory, and the
  // old reference is kept.
  template <class Hook>
  bool renew(Hook&& before_free) {
    Box* fresh = new (std::nothrow) Box();
    if (!fresh) return false;
    detach(std::forward<Hook>(before_free));
    b_ = fresh;
    return true;
  }
};

}  // namespace pcm
