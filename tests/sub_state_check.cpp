// csrc/sub_state.h on its own: a host program (no HIP) that prints "ok" when the holder keeps its promises.
#include <cstdio>
#include <string>
#include <type_traits>

#include "sub_state.h"

using pcm::SubState;

static std::string g_log;   // one letter per destructor, in the order they ran
static int g_fail = 0;

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); g_fail++; } \
  } while (0)

template <char Tag> struct Probe {
  int value = 7;
  ~Probe() { g_log += Tag; }
};

struct Three {   // members die in reverse declaration order: c, b, a
  SubState a, b, c;
};

int main() {
  static_assert(!std::is_copy_constructible<SubState>::value && !std::is_copy_assignable<SubState>::value, "the holder owns its object");
  {   // an empty holder: nothing to return, nothing to destroy
    SubState s;
    CHECK(s.get<Probe<'x'>>() == nullptr);
  }
  CHECK(g_log.empty());
  {   // created once, the same object ever after, destroyed once with the holder
    SubState s;
    CHECK(s.get<Probe<'x'>>() == nullptr);
    Probe<'x'>* p = s.get_or_create<Probe<'x'>>();
    CHECK(p != nullptr && p->value == 7);
    p->value = 8;
    CHECK(s.get_or_create<Probe<'x'>>() == p && s.get<Probe<'x'>>() == p && p->value == 8);
    CHECK(g_log.empty());
  }
  CHECK(g_log == "x");
  g_log.clear();
  {   // inside a struct: reverse declaration order, and a member never created stays silent
    Three t;
    t.a.get_or_create<Probe<'a'>>();
    t.c.get_or_create<Probe<'c'>>();
    CHECK(t.b.get<Probe<'b'>>() == nullptr);
  }
  CHECK(g_log == "ca");
  g_log.clear();
  {
    Three t;
    t.b.get_or_create<Probe<'b'>>();
    t.a.get_or_create<Probe<'a'>>();
    t.c.get_or_create<Probe<'c'>>();
  }
  CHECK(g_log == "cba");
  if (g_fail) return 1;
  std::printf("ok\n");
  return 0;
}
