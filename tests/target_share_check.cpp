// target_share_check.cpp -- the attach / detach / last-release rules of csrc/target_share.h, walked through on the host: plain
// g++, no GPU, own main, so that it is also built with -fsanitize=address,undefined (tests/test_shared_target_capi.py).  A
// "context" here is the reference plus the calls pcm_api.hip and lio_api.hip make on it; the payload counts its constructions and destructions,
// and the release hook counts its runs, so a double release, a leak or a use after the release shows as a wrong count or as a
// sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pointcloud-slam_amd/csrc/target_share.h"

namespace {

int g_alive = 0, g_made = 0, g_freed = 0, g_hooks = 0, g_hook_saw_alive = 0;

struct Payload {
  std::vector<int> points;   // heap memory: a use after the release is an ASan report
  int version = 0;
  Payload() { g_alive++; g_made++; }
  ~Payload() { g_alive--; g_freed++; }
};

struct Ctx {
  pcm::SharedTarget<Payload> tg;
  Ctx() { if (!tg.create()) abort(); }
  static auto hook() { return [] { g_hooks++; g_hook_saw_alive += g_alive > 0 ? 1 : 0; }; }
  // pcm_set_target: a holder of a shared target goes on with one of its own; a sole holder rewrites its own
  void set_target(int n) {
    if (tg.shared() && !tg.renew(hook())) abort();
    tg->points.assign((size_t)n, n);
    tg->version++;
  }
  // pcm_target_insert and its kin: refused while shared, nothing touched
  bool insert(int v) {
    if (!tg.mutable_by_me()) return false;
    tg->points.push_back(v);
    tg->version++;
    return true;
  }
  void share_from(Ctx& src) { tg.attach(src.tg, hook()); }
  void destroy() { tg.detach(hook()); }
};

int g_failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } \
  } while (0)

void reset() { g_made = g_freed = g_hooks = g_hook_saw_alive = 0; }

// A owns, B shares; A goes first: B keeps a working target, which goes with B
void owner_first() {
  reset();
  Ctx* a = new Ctx(); Ctx* b = new Ctx();
  a->set_target(100);
  EXPECT(a->tg.holders() == 1 && b->tg.holders() == 1);
  b->share_from(*a);                       // B's own empty target goes: hook 1
  EXPECT(g_hooks == 1 && g_freed == 1);
  EXPECT(a->tg.holders() == 2 && b->tg.holders() == 2 && a->tg.same_as(b->tg));
  a->destroy(); delete a;
  EXPECT(g_hooks == 1 && g_freed == 1);    // not the last holder: nothing released
  EXPECT(b->tg.holders() == 1 && b->tg->points.size() == 100 && b->tg->points[99] == 100);
  EXPECT(b->insert(7));                    // sole holder again: mutable
  b->destroy(); delete b;
  EXPECT(g_hooks == 2 && g_freed == 2 && g_made == 2 && g_alive == 0);
  EXPECT(g_hook_saw_alive == g_hooks);     // the hook runs before the payload goes
}

// the sharer goes first
void sharer_first() {
  reset();
  Ctx* a = new Ctx(); Ctx* b = new Ctx();
  a->set_target(50);
  b->share_from(*a);
  b->destroy(); delete b;
  EXPECT(g_hooks == 1 && g_freed == 1);
  EXPECT(a->tg.holders() == 1 && a->tg->points.size() == 50);
  a->destroy(); delete a;
  EXPECT(g_hooks == 2 && g_freed == 2 && g_alive == 0);
}

// a sharer sets a target of its own: that sharer only
void detach_by_set_target() {
  reset();
  Ctx a, b, c;
  a.set_target(10);
  b.share_from(a); c.share_from(a);
  EXPECT(a.tg.holders() == 3 && g_hooks == 2);
  b.set_target(20);
  EXPECT(g_hooks == 2);                    // B was not the last holder of the shared target
  EXPECT(a.tg.holders() == 2 && c.tg.holders() == 2 && b.tg.holders() == 1);
  EXPECT(!b.tg.same_as(a.tg) && b.tg->points.size() == 20 && a.tg->points.size() == 10 && c.tg->points.size() == 10);
  EXPECT(a.tg->version == 1);              // untouched
  a.set_target(30);                        // the original owner detaches the same way
  EXPECT(c.tg.holders() == 1 && c.tg->points.size() == 10 && a.tg->points.size() == 30);
  a.destroy(); b.destroy(); c.destroy();
  EXPECT(g_hooks == 5 && g_made == 5 && g_freed == 5 && g_alive == 0);
  a.destroy();                             // an empty reference: nothing happens
  EXPECT(g_hooks == 5 && a.tg.holders() == 0 && a.tg.empty());
}

// C shares from B, which shares from A: one target, three holders, released once by whoever is last
void chain() {
  reset();
  Ctx* a = new Ctx(); Ctx* b = new Ctx(); Ctx* c = new Ctx();
  a->set_target(5);
  b->share_from(*a);
  c->share_from(*b);
  EXPECT(a->tg.holders() == 3 && c->tg.same_as(a->tg) && g_hooks == 2);
  c->share_from(*b);                       // again: the count stays (pcm_share_target returns early; attach itself is neutral too)
  EXPECT(a->tg.holders() == 3 && g_hooks == 2);
  a->destroy(); delete a;
  b->destroy(); delete b;
  EXPECT(g_hooks == 2 && c->tg.holders() == 1 && c->tg->points.size() == 5);
  c->destroy(); delete c;
  EXPECT(g_hooks == 3 && g_made == 3 && g_freed == 3 && g_alive == 0);
}

// a mutation of a shared target is refused and leaves both holders as they were; after the other detaches it goes through
void refused_mutation() {
  reset();
  Ctx a, b;
  a.set_target(8);
  b.share_from(a);
  EXPECT(!a.insert(1) && !b.insert(1));
  EXPECT(a.tg->version == 1 && a.tg->points.size() == 8 && a.tg.holders() == 2);
  b.destroy();
  EXPECT(a.insert(1) && a.tg->points.size() == 9 && a.tg->version == 2);
  a.destroy();
  EXPECT(g_hooks == 2 && g_freed == 2 && g_alive == 0);
}

// a reference that nobody detached goes with its owner, without a hook
void destructor_releases() {
  reset();
  { Ctx a, b; a.set_target(3); b.share_from(a); }
  EXPECT(g_hooks == 1 && g_made == 2 && g_freed == 2 && g_alive == 0);
}

}  // namespace

int main() {
  owner_first();
  sharer_first();
  detach_by_set_target();
  chain();
  refused_mutation();
  destructor_releases();
  if (g_failures) { printf("%d check(s) failed\n", g_failures); return 1; }
  printf("target_share_check ok\n");
  return 0;
}
