// keyed_best.h -- the running 5-best list of k_linearize_lists (neighbour_lists.hip) as six sorted 32-bit keys, usable from host
// and device code (tests/test_keyed_best_host.py runs this header against a restatement of best_offer_d2 with g++).
//
// best_offer_d2 (linearize_common.h) keeps five distances AND five indices; every insert moves the indices with compares and
// selects, the dearest instructions of the walk.  Here the index rides inside the sort key.  A squared distance is non-negative,
// so the unsigned order of its bit pattern is the order of the distances; the low kKeyIdBits bits of the pattern are replaced by
// the candidate's position in its run:
//
//     key = (float_as_uint(d2) & ~0x7F) | (k - s)          (runs of at most 128 entries)
//
// and the list is the SIX smallest keys, kept by a branch-free network of one unsigned min and five unsigned med3 per candidate.
// The keys of a run are distinct (distinct positions), so their order is total.  A pad entry (d2 = +inf) has the key
// 0x7F800000 | position and sorts behind every finite distance; a NaN distance sorts there or further back.
//
// Exactness.  Let t(K) = K & ~0x7F be the truncated distance of a key and R = float_as_uint(max_r2f) & ~0x7F.  A list is
// UNAMBIGUOUS iff
//   (1) no entry K[j], j <= 4, has t(K[j]) == R, and
//   (2) for every j <= 4 with t(K[j]) < R, t(K[j]) != t(K[j + 1])          (K[5] is the sixth key: it is kept for this test only).
// Then the keyed list equals what best_offer_d2 leaves after the same candidates, whatever their order:
//   * Truncation is monotone, so distinct truncated distances order like the exact ones: the in-range entries of K[0..4] are in
//     strictly ascending exact distance.
//   * A candidate outside the key top-5 has a key >= K[5], hence a truncated distance >= t(K[5]) > t(K[4]) >= ... (by (2), as far
//     as the entries are in range): its exact distance exceeds that of every kept in-range entry.  No tie exists, so no tie rule
//     (visit order) is needed.
//   * t(K) < R gives d2 < uint_as_float(R) <= max_r2f: in range.  t(K) > R gives bits(d2) >= R + 128 > bits(max_r2f): out of
//     range (or NaN, which best_offer_d2 never inserts either).  t(K) == R, the only undecided case, is excluded by (1); the keys
//     are sorted, so the in-range entries are a prefix and every later candidate is out of range as well.
//   So the set, its ascending order and the count m = min(5, #in range) are best_offer_d2's.
// An ambiguous list (true ties of lattice clouds and duplicate points, distances within 128 ulp of each other or of the range
// limit, max_r2f = +inf with fewer than five candidates) decides nothing: the caller repeats the walk with best_offer_d2.  So does
// a run longer than kKeyedMaxRun, whose positions do not fit the key, and a max_r2f that is negative or NaN.
#pragma once

#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef PCM_HD
#if defined(__HIPCC__)
#define PCM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PCM_HD inline
#endif
#endif

namespace pcm {

constexpr int kKeyIdBits = 7;
constexpr uint32_t kKeyIdMask = (1u << kKeyIdBits) - 1u;
constexpr uint32_t kKeyedMaxRun = 1u << kKeyIdBits;   // positions 0 .. 127
constexpr int kKeyedDepth = 6;                        // the five best and the key behind them
constexpr int kKeyedBest = 5;

struct KeyedBest {
  uint32_t k[kKeyedDepth];   // ascending
};

PCM_HD uint32_t keyed_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, sizeof u);
  return u;
}
PCM_HD uint32_t keyed_umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
PCM_HD uint32_t keyed_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
// integer median of three (v_med3_u32): the keys may be denormal, infinite or NaN bit patterns, a float median would quiet them
PCM_HD uint32_t keyed_umed3(uint32_t a, uint32_t b, uint32_t c) { return keyed_umin(keyed_umax(a, b), keyed_umax(keyed_umin(a, b), c)); }

PCM_HD void keyed_init(KeyedBest& b) {
  for (int j = 0; j < kKeyedDepth; j++) b.k[j] = 0xffffffffu;
}

// d2 >= 0 (or NaN); pos = k - s < kKeyedMaxRun
PCM_HD uint32_t keyed_pack(float d2, uint32_t pos) { return (keyed_bits(d2) & ~kKeyIdMask) | pos; }

// sorted insert: new K[j] = median(key, K[j - 1], K[j]) of the old values, new K[0] = min(key, K[0])
PCM_HD void keyed_offer(KeyedBest& b, uint32_t key) {
  b.k[5] = keyed_umed3(key, b.k[4], b.k[5]);
  b.k[4] = keyed_umed3(key, b.k[3], b.k[4]);
  b.k[3] = keyed_umed3(key, b.k[2], b.k[3]);
  b.k[2] = keyed_umed3(key, b.k[1], b.k[2]);
  b.k[1] = keyed_umed3(key, b.k[0], b.k[1]);
  b.k[0] = keyed_umin(key, b.k[0]);
}

// pos[j] = position of the j-th best in its run, m = in-range entries among the five best.  Returns true iff the list is
// unambiguous (see above); pos and m mean nothing otherwise.
PCM_HD bool keyed_decode(const KeyedBest& b, float max_r2f, uint32_t (&pos)[kKeyedBest], int& m) {
  const uint32_t rb = keyed_bits(max_r2f), R = rb & ~kKeyIdMask;
  bool ambiguous = rb > 0x7f800000u;   // negative or NaN: best_offer_d2's `d2 < thr` decides
  int n = 0;
  for (int j = 0; j < kKeyedBest; j++) {
    const uint32_t t = b.k[j] & ~kKeyIdMask, tn = b.k[j + 1] & ~kKeyIdMask;
    const bool in = t < R;
    ambiguous = ambiguous || t == R || (in && t == tn);
    n += in ? 1 : 0;
    pos[j] = b.k[j] & kKeyIdMask;
  }
  m = n;
  return !ambiguous;
}

}  // namespace pcm
