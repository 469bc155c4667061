// tile_share_check.cpp -- the rules of a tile store several LOAM contexts hold (csrc/loam_dynmap.h, TileHolder over
// csrc/target_share.h), walked through on the host: plain g++, no GPU, own main, so that it is also built with
// -fsanitize=address,undefined (tests/test_loam_tile_share.py).  A "context" here is the holder plus the calls loam_dynmap.hip makes
// on it; the payload counts its constructions and destructions and the release hook counts its runs, so a double release, a leak
// or a use after the release shows as a wrong count or as a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pointcloud-slam_amd/csrc/loam_dynmap.h"

namespace {

int g_alive = 0, g_made = 0, g_freed = 0, g_hooks = 0, g_hook_saw_alive = 0;

struct Store {
  std::vector<int> tiles;   // heap memory: a use after the release is an ASan report
  int version = 0;
  Store() { g_alive++; g_made++; }
  ~Store() { g_alive--; g_freed++; }
};

struct Ctx {
  pcm::loam::TileHolder<Store> h;
  Ctx() { if (!h.ready()) abort(); }
  static auto hook() { return [] { g_hooks++; g_hook_saw_alive += g_alive > 0 ? 1 : 0; }; }
  // pcm_loam_tile_add / pcm_loam_tiles_build: refused while shared, nothing touched
  bool add_tile(int v) {
    if (!h.writable()) return false;
    h.ts->tiles.push_back(v);
    h.ts->version++;
    return true;
  }
  // pcm_loam_dynmap_load: a selection over the store's tiles
  void load() {
    h.s.sel[0].assign(h.ts->tiles.size(), 0);
    h.s.loaded = true;
    h.s.sel_gen++;
    for (int k = 0; k < 6; k++) h.s.last_load[k] = 1.f;
    h.s.last_valid = true;
  }
  bool never_loaded() const {
    bool never = !h.s.loaded && !h.s.last_valid && h.s.sel[0].empty() && h.s.sel[1].empty();
    for (int k = 0; k < 6; k++) never = never && h.s.last_load[k] == pcm::loam::kNeverLoaded;
    return never;
  }
  void share_from(Ctx& src) { h.share_from(src.h, hook()); }
  bool clear() { return h.clear_or_detach(hook(), [](Store& s) { s.tiles.clear(); s.version++; }); }
  void destroy() { h.let_go(hook()); }
};

int g_failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } \
  } while (0)

void reset() { g_made = g_freed = g_hooks = g_hook_saw_alive = 0; }

// A owns, B shares; A goes first: B keeps a working store, which goes with B
void owner_first() {
  reset();
  Ctx* a = new Ctx(); Ctx* b = new Ctx();
  for (int i = 0; i < 100; i++) EXPECT(a->add_tile(i));
  EXPECT(a->h.holders() == 1 && b->h.holders() == 1);
  b->load();
  const uint64_t gen = b->h.s.sel_gen;
  b->share_from(*a);                       // B's own empty store goes: hook 1
  EXPECT(g_hooks == 1 && g_freed == 1);
  EXPECT(a->h.holders() == 2 && b->h.holders() == 2 && a->h.ts.same_as(b->h.ts));
  EXPECT(b->never_loaded() && b->h.s.sel_gen > gen);   // the selection starts over, the generation moved on
  a->load();
  a->destroy(); delete a;
  EXPECT(g_hooks == 1 && g_freed == 1);    // not the last holder: nothing released
  EXPECT(b->h.holders() == 1 && b->h.ts->tiles.size() == 100 && b->h.ts->tiles[99] == 99);
  EXPECT(b->add_tile(7));                  // sole holder again: writable
  b->destroy(); delete b;
  EXPECT(g_hooks == 2 && g_freed == 2 && g_made == 2 && g_alive == 0);
  EXPECT(g_hook_saw_alive == g_hooks);     // the hook runs before the store goes
}

// the sharer goes first; the owner's selection is not touched by any of it
void sharer_first() {
  reset();
  Ctx* a = new Ctx(); Ctx* b = new Ctx();
  for (int i = 0; i < 50; i++) a->add_tile(i);
  a->load();
  const uint64_t gen = a->h.s.sel_gen;
  b->share_from(*a);
  b->load();
  b->destroy(); delete b;
  EXPECT(g_hooks == 1 && g_freed == 1);
  EXPECT(a->h.holders() == 1 && a->h.ts->tiles.size() == 50);
  EXPECT(a->h.s.loaded && a->h.s.sel_gen == gen && a->h.s.sel[0].size() == 50 && a->h.s.last_valid);
  a->destroy(); delete a;
  EXPECT(g_hooks == 2 && g_freed == 2 && g_alive == 0);
}

// pcm_loam_tile_clear on a sharer: that sharer only, with an empty store of its own; on the sole holder: its store is emptied
void detach_by_clear() {
  reset();
  Ctx a, b, c;
  for (int i = 0; i < 10; i++) a.add_tile(i);
  b.share_from(a); c.share_from(a);
  EXPECT(a.h.holders() == 3 && g_hooks == 2);
  b.load();
  EXPECT(b.clear());
  EXPECT(g_hooks == 2);                    // B was not the last holder of the shared store
  EXPECT(a.h.holders() == 2 && c.h.holders() == 2 && b.h.holders() == 1);
  EXPECT(!b.h.ts.same_as(a.h.ts) && b.h.ts->tiles.empty() && b.never_loaded());
  EXPECT(a.h.ts->tiles.size() == 10 && c.h.ts->tiles.size() == 10 && a.h.ts->version == 10);   // untouched
  EXPECT(b.add_tile(1) && b.h.ts->tiles.size() == 1);
  EXPECT(a.clear());                       // the original owner detaches the same way
  EXPECT(c.h.holders() == 1 && c.h.ts->tiles.size() == 10 && a.h.ts->tiles.empty());
  const Store* kept = c.h.ts.get();
  c.load();
  EXPECT(c.clear());                       // the sole holder: the same store, emptied in place
  EXPECT(c.h.ts.get() == kept && c.h.ts->tiles.empty() && c.h.ts->version == 11 && c.never_loaded() && g_hooks == 2);
  a.destroy(); b.destroy(); c.destroy();
  EXPECT(g_hooks == 5 && g_made == 5 && g_freed == 5 && g_alive == 0);
  a.destroy();                             // an empty reference: nothing happens
  EXPECT(g_hooks == 5 && a.h.holders() == 0);
}

// C shares from B, which shares from A: one store, three holders, released once by whoever is last
void chain() {
  reset();
  Ctx* a = new Ctx(); Ctx* b = new Ctx(); Ctx* c = new Ctx();
  for (int i = 0; i < 5; i++) a->add_tile(i);
  b->share_from(*a);
  c->share_from(*b);
  EXPECT(a->h.holders() == 3 && c->h.ts.same_as(a->h.ts) && g_hooks == 2);
  c->load();
  c->share_from(*b);                       // again: the count stays, the selection starts over all the same
  EXPECT(a->h.holders() == 3 && g_hooks == 2 && c->never_loaded());
  a->destroy(); delete a;
  b->destroy(); delete b;
  EXPECT(g_hooks == 2 && c->h.holders() == 1 && c->h.ts->tiles.size() == 5);
  c->destroy(); delete c;
  EXPECT(g_hooks == 3 && g_made == 3 && g_freed == 3 && g_alive == 0);
}

// a mutation of a shared store is refused on every holder and leaves it as it was; after the other detaches it goes through
void refused_mutation() {
  reset();
  Ctx a, b;
  for (int i = 0; i < 8; i++) a.add_tile(i);
  b.share_from(a);
  EXPECT(!a.add_tile(1) && !b.add_tile(1));
  EXPECT(a.h.ts->version == 8 && a.h.ts->tiles.size() == 8 && a.h.holders() == 2);
  b.destroy();
  EXPECT(a.add_tile(1) && a.h.ts->tiles.size() == 9 && a.h.ts->version == 9);
  a.destroy();
  EXPECT(g_hooks == 2 && g_freed == 2 && g_alive == 0);
}

// sharing an empty store is allowed
void empty_store() {
  reset();
  Ctx a, b;
  b.add_tile(3);
  b.share_from(a);
  EXPECT(b.h.holders() == 2 && b.h.ts->tiles.empty());
  a.destroy(); b.destroy();
  EXPECT(g_hooks == 2 && g_made == 2 && g_freed == 2 && g_alive == 0);
}

// a reference that nobody let go of goes with its owner, without a hook
void destructor_releases() {
  reset();
  { Ctx a, b; a.add_tile(3); b.share_from(a); }
  EXPECT(g_hooks == 1 && g_made == 2 && g_freed == 2 && g_alive == 0);
}

}  // namespace

int main() {
  owner_first();
  sharer_first();
  detach_by_clear();
  chain();
  refused_mutation();
  empty_store();
  destructor_releases();
  if (g_failures) { printf("%d check(s) failed\n", g_failures); return 1; }
  printf("tile_share_check ok\n");
  return 0;
}
