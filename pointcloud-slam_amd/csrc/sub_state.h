// sub_state.h -- the one way a context holds a lazily created piece of state whose type only one translation unit knows (the batch
// workspaces, the LOAM state and its stores, the occupancy map): a type-erased owning pointer.  The object is made on first use
// and deleted with its owner; whatever it has to undo beyond its members belongs in its destructor.  Host code only, no HIP.
#pragma once

#include <new>

namespace pcm {

struct SubState {
  void* p = nullptr;
  void (*del)(void*) = nullptr;
  SubState() = default;
  SubState(const SubState&) = delete;
  SubState& operator=(const SubState&) = delete;
  ~SubState() { if (p) del(p); }
  // the object, or null before its creation.  T is the type it was created with.
  template <class T> T* get() const { return static_cast<T*>(p); }
  // null: out of host memory
  template <class T> T* get_or_create() {
    if (!p) {
      p = new (std::nothrow) T();
      del = [](void* q) { delete static_cast<T*>(q); };
    }
    return static_cast<T*>(p);
  }
};

}  // namespace pcm
