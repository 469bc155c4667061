// intro_sort.h -- std::sort as libstdc++ implements it, usable in device code.
//
// featureExtraction::extractFeatures sorts every sector of cloudSmoothness with std::sort(..., by_value())
// (jueying_slam/src/featureExtraction.cpp:164; by_value :11-14 compares `left.value < right.value` only).
// std::sort is unstable, and which of several tied curvatures the corner / surf loops meet first decides the selection, so the
// order of ties is part of the result.  It is a property of the standard library the reference is built with, restated here from
// the container's own <bits/stl_algo.h> and <bits/stl_heap.h> (GCC 11.4; unchanged since GCC 4.x):
//   __sort                      stl_algo.h:1949-1958   depth limit 2 * lg(n), then the final insertion sort
//   __introsort_loop            stl_algo.h:1925-1941   while the range is longer than _S_threshold = 16 (:1855)
//   __unguarded_partition_pivot stl_algo.h:1900-1907   median of (first + 1, mid, last - 1) moved to first (__move_median_to_first :79-98)
//   __unguarded_partition       stl_algo.h:1878-1895
//   __partial_sort(first, last, last)  stl_algo.h:1912-1919 = __heap_select (:1642-1650, a plain __make_heap here) + __sort_heap
//                               (stl_heap.h:418-425; __pop_heap :253-265, __adjust_heap :223-247, __push_heap :134-146)
//   __final_insertion_sort      stl_algo.h:1861-1872   __insertion_sort (:1819-1838) of the first 16, __unguarded_insertion_sort
//                               (:1843-1848, __unguarded_linear_insert :1799-1813) of the rest
// The recursion of __introsort_loop (right part first, then the loop continues on the left part) becomes an explicit stack: the
// parts are disjoint, so the order in which they are finished does not change the result.  The heap and insertion helpers are
// those of nth_select.h (same libstdc++ functions, same comparison on DistId::d).  Checked on the host against the real
// std::sort, permutation for permutation (tests/test_intro_sort.py compiles this header with g++).
#pragma once

#include "nth_select.h"

namespace pcm {

// __sort_heap after __make_heap: std::__partial_sort(a, a + n, a + n)
PCM_NTH_FN void intro_heap_sort(DistId* a, int n) {
  nth_heap_select(a, n, n);
  for (int last = n - 1; last > 0; last--) {   // __pop_heap(first, last, last)
    const DistId v = a[last];
    a[last] = a[0];
    nth_adjust_heap(a, 0, last, v);
  }
}

// std::sort(a, a + n) with comparison a.d < b.d
PCM_NTH_FN void intro_sort_libstdcxx(DistId* a, int n) {
  if (n <= 1) return;
  int lg = 0;
  for (int m = n; m > 1; m >>= 1) lg++;   // std::__lg(n)
  struct Range { int first, last, depth; };
  Range stack[64];
  int top = 0;
  stack[top++] = Range{0, n, 2 * lg};
  while (top > 0) {
    Range r = stack[--top];
    while (r.last - r.first > 16) {
      if (r.depth == 0) {
#if defined(PCM_INTRO_COUNT_HEAP_SORT)
        PCM_INTRO_COUNT_HEAP_SORT;   // host test hook: the depth limit was reached
#endif
        intro_heap_sort(a + r.first, r.last - r.first);
        break;
      }
      --r.depth;
      const int first = r.first, last = r.last, mid = first + (last - first) / 2;
      {   // __move_median_to_first(first, first + 1, mid, last - 1)
        const int ia = first + 1, ib = mid, ic = last - 1;
        if (nth_less(a[ia], a[ib])) {
          if (nth_less(a[ib], a[ic])) nth_swap(a, first, ib);
          else if (nth_less(a[ia], a[ic])) nth_swap(a, first, ic);
          else nth_swap(a, first, ia);
        } else if (nth_less(a[ia], a[ic])) nth_swap(a, first, ia);
        else if (nth_less(a[ib], a[ic])) nth_swap(a, first, ic);
        else nth_swap(a, first, ib);
      }
      int lo = first + 1, hi = last;   // __unguarded_partition(first + 1, last, pivot = first)
      for (;;) {
        while (nth_less(a[lo], a[first])) ++lo;
        --hi;
        while (nth_less(a[first], a[hi])) --hi;
        if (!(lo < hi)) break;
        nth_swap(a, lo, hi);
        ++lo;
      }
      stack[top++] = Range{first, lo, r.depth};   // the left part, after the right one (__introsort_loop(cut, last); last = cut)
      r.first = lo;
    }
  }
  // __final_insertion_sort
  if (n > 16) {
    nth_insertion_sort(a, 0, 16);
    for (int i = 16; i < n; i++) {   // __unguarded_linear_insert
      const DistId v = a[i];
      int lastp = i, next = i - 1;
      while (nth_less(v, a[next])) {
        a[lastp] = a[next];
        lastp = next;
        --next;
      }
      a[lastp] = v;
    }
  } else {
    nth_insertion_sort(a, 0, n);
  }
}

}  // namespace pcm
