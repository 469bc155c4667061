"""csrc/intro_sort.h (the device restatement of libstdc++ std::sort) against the real std::sort, permutation for permutation."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pointcloud-slam_amd", "csrc")

CHECK = r'''
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
static long g_heap = 0;
#define PCM_INTRO_COUNT_HEAP_SORT (++g_heap)
#include "intro_sort.h"
struct ValueIndex { float v; size_t i; };
struct ValueLess { bool operator()(const ValueIndex& a, const ValueIndex& b) const { return a.v < b.v; } };
int main() {
  long cases = 0, bad = 0;
  int n;
  while (std::fread(&n, 4, 1, stdin) == 1) {
    std::vector<float> v(n);
    if (n && std::fread(v.data(), 4, n, stdin) != (size_t)n) return 2;
    std::vector<ValueIndex> a(n);
    std::vector<pcm::DistId> b(n);
    for (int i = 0; i < n; i++) { a[i] = ValueIndex{v[i], (size_t)i}; b[i] = pcm::DistId{v[i], (uint32_t)i}; }
    std::sort(a.begin(), a.end(), ValueLess());
    pcm::intro_sort_libstdcxx(b.data(), n);
    for (int i = 0; i < n; i++) if (a[i].i != b[i].id) { bad++; break; }
    cases++;
  }
  std::printf("%ld %ld %ld\n", cases, bad, g_heap);
  return 0;
}
'''


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("intro_sort")
    src = d / "check.cpp"
    src.write_text(CHECK)
    exe = d / "check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", str(exe), str(src)])
    return exe


def _run(exe, arrays):
    buf = b"".join(np.int32(len(a)).tobytes() + np.asarray(a, np.float32).tobytes() for a in arrays)
    out = subprocess.run([str(exe)], input=buf, capture_output=True, check=True).stdout.split()
    return int(out[0]), int(out[1]), int(out[2])


def test_random_sizes_and_ties(checker):
    rng = np.random.default_rng(1)
    arrays = []
    for n in list(range(0, 64)) + list(rng.integers(64, 3001, 150)):
        k = int(rng.integers(1, 9))
        vals = rng.uniform(0, 1, k).astype(np.float32)
        arrays.append(vals[rng.integers(0, k, n)])
        arrays.append(rng.uniform(0, 1, n).astype(np.float32))
    arrays.append(np.zeros(3000, np.float32))
    cases, bad, _ = _run(checker, arrays)
    assert cases == len(arrays) and bad == 0


def test_sorted_reversed_organ_pipe(checker):
    arrays = []
    for n in (17, 100, 1000, 3000):
        a = np.arange(n, dtype=np.float32)
        arrays += [a, a[::-1].copy(), np.concatenate([a[: n // 2], a[: n - n // 2][::-1]]), np.floor(a / 7)]
    cases, bad, _ = _run(checker, arrays)
    assert cases == len(arrays) and bad == 0


def _median_of_three_killer(n):
    """Musser's sequence for the median-of-three pivot: quadratic for plain quicksort, so introsort falls back to heap sort."""
    k = n // 2
    a = np.zeros(n, np.float32)
    for i in range(1, k + 1):
        if i % 2 == 1:
            a[i - 1] = i
            a[i] = k + i
        a[k + i - 1] = 2 * i
    return a


def test_heap_fallback(checker):
    arrays = [_median_of_three_killer(n) for n in (256, 1024, 2048, 3000)]
    # search a few random permutations of the killer too: at least one case must take the heap path
    cases, bad, heap = _run(checker, arrays)
    assert cases == len(arrays) and bad == 0
    assert heap > 0, "no case reached the depth limit"
