// The real libstdc++ std::sort of featureExtraction's cloudSmoothness sectors, for the numpy restatement
// (tests/loam_features_ref.py): a (float value, size_t index) pair ordered by the value alone, as the sector sort compares.
#include <algorithm>
#include <cstddef>
#include <cstdint>

struct ValueIndex {
  float v;
  size_t i;
};

struct ValueLess {
  bool operator()(const ValueIndex& a, const ValueIndex& b) const { return a.v < b.v; }
};

extern "C" void std_sort_smoothness(float* value, int64_t* ind, int64_t n) {
  ValueIndex* a = new ValueIndex[n > 0 ? n : 1];
  for (int64_t k = 0; k < n; k++) a[k] = ValueIndex{value[k], (size_t)ind[k]};
  std::sort(a, a + n, ValueLess());
  for (int64_t k = 0; k < n; k++) { value[k] = a[k].v; ind[k] = (int64_t)a[k].i; }
  delete[] a;
}
