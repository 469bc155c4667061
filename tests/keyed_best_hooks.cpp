// Host hooks of tests/test_keyed_best_host.py: the keyed 5-best list of k_linearize_lists (csrc/keyed_best.h, the very functions the
// kernel runs) and a plain restatement of best_offer_d2 (csrc/linearize_common.h) over one candidate sequence.
#include <cstdint>

#include "keyed_best.h"

extern "C" {

// candidates d2[0 .. n) offered in order, n <= 128.  Returns 1 iff the keyed list is unambiguous; pos / m as keyed_decode leaves them.
int kb_keyed(const float* d2, int n, float max_r2f, uint32_t* pos, int* m) {
  pcm::KeyedBest b;
  pcm::keyed_init(b);
  for (int k = 0; k < n; k++) pcm::keyed_offer(b, pcm::keyed_pack(d2[k], (uint32_t)k));
  uint32_t p[pcm::kKeyedBest];
  int mm = 0;
  const bool ok = pcm::keyed_decode(b, max_r2f, p, mm);
  for (int j = 0; j < pcm::kKeyedBest; j++) pos[j] = p[j];
  *m = mm;
  return ok ? 1 : 0;
}

// the six keys themselves (sortedness and the pad keys are checked on them)
void kb_keys(const float* d2, int n, uint32_t* keys) {
  pcm::KeyedBest b;
  pcm::keyed_init(b);
  for (int k = 0; k < n; k++) pcm::keyed_offer(b, pcm::keyed_pack(d2[k], (uint32_t)k));
  for (int j = 0; j < pcm::kKeyedDepth; j++) keys[j] = b.k[j];
}

// best_offer_d2 restated: ascending list of five, a candidate enters iff d2 < min(d[4], max_r2f) (strict: an equal distance stays
// behind the entries already there = visit order; NaN and +inf never enter), m = finite entries.  Free slots keep id 0xffffffff.
void kb_plain(const float* d2, int n, float max_r2f, uint32_t* id, int* m) {
  const float inf = __builtin_inff();
  float d[5];
  for (int j = 0; j < 5; j++) { d[j] = inf; id[j] = 0xffffffffu; }
  for (int k = 0; k < n; k++) {
    const float v = d2[k];
    const float thr = d[4] < max_r2f ? d[4] : max_r2f;
    if (!(v < thr)) continue;
    int at = 4;
    while (at > 0 && v < d[at - 1]) at--;
    for (int j = 4; j > at; j--) { d[j] = d[j - 1]; id[j] = id[j - 1]; }
    d[at] = v; id[at] = (uint32_t)k;
  }
  int c = 0;
  for (int j = 0; j < 5; j++) c += d[j] < inf ? 1 : 0;
  *m = c;
}

}  // extern "C"
