// Harness of tests/test_gpu_fast_divsqrt.py: the window sequences of plane_fit.h (fsqrt_fast, fdiv_recip + fdiv_fast) against the
// full correctly rounded sequences (sqrtf, __fdiv_rn) and against the double-precision result rounded to float (double rounding
// is innocuous for sqrt and / at 53 >= 2 * 24 + 2 bits), plus raw outputs for host-side IEEE comparisons.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "plane_fit.h"

using namespace pcm;

// every float with bits in [b0, b0 + n): count inputs inside the window and mismatches there
__global__ void k_sqrt_all(uint32_t b0, uint32_t n, unsigned long long* cnt) {
#if defined(__HIP_DEVICE_COMPILE__)   // the window sequences exist in the device pass only
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float x = __uint_as_float(b0 + t);
  if (!fsqrt_in_window(x)) return;
  const float f = fsqrt_fast(x);
  const float r = (float)sqrt((double)x);
  const bool bad = __float_as_uint(f) != __float_as_uint(r) || __float_as_uint(f) != __float_as_uint(sqrtf(x));
  atomicAdd(&cnt[0], 1ull);
  if (bad) atomicAdd(&cnt[1], 1ull);
#endif
}

// denominator b = (1 + s * 2^-23) * 2^eb for every significand s, numerators a_j = a significand from a hash * 2^ea_j
__device__ inline uint32_t mix(uint32_t v) { v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16; return v; }
__global__ void k_div_all(int eb, const int* ea, int nea, int per, uint32_t seed, unsigned long long* cnt) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= (1u << 23)) return;
  const uint32_t sb = (mix(s ^ seed) & 1u) << 31;
  const float b = __uint_as_float(sb | ((uint32_t)(eb + 127) << 23) | s);
  const float y = fdiv_recip(b);
  unsigned long long in = 0, bad = 0;
  for (int e = 0; e < nea; e++) {
    for (int j = 0; j < per; j++) {
      const uint32_t h = mix(s * 977u + (uint32_t)j * 131071u + (uint32_t)e * 7919u + seed);
      const float a = __uint_as_float((h & 0x807fffffu) | ((uint32_t)(ea[e] + 127) << 23));
      if (!(fdiv_in_window(a) && fdiv_in_window(b))) continue;
      const float q = fdiv_fast(a, b, y);
      const float r = (float)((double)a / (double)b);
      in++;
      if (__float_as_uint(q) != __float_as_uint(r) || __float_as_uint(q) != __float_as_uint(__fdiv_rn(a, b))) bad++;
    }
  }
  atomicAdd(&cnt[0], in);
  atomicAdd(&cnt[1], bad);
#endif
}

// raw outputs for the host: window flags and fast results of given inputs
__global__ void k_eval(const float* a, const float* b, int n, float* q, float* sq, int* win) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  q[i] = fdiv_fast(a[i], b[i], fdiv_recip(b[i]));
  sq[i] = fsqrt_fast(a[i]);
  win[i] = (fdiv_in_window(a[i]) ? 1 : 0) | (fdiv_in_window(b[i]) ? 2 : 0) | (fsqrt_in_window(a[i]) ? 4 : 0);
#endif
}

#define CK(x) do { if ((x) != hipSuccess) return -1; } while (0)

extern "C" int check_sqrt_range(uint32_t b0, uint64_t n, unsigned long long* out2) {
  unsigned long long* d = nullptr;
  CK(hipMalloc(&d, 16));
  CK(hipMemset(d, 0, 16));
  const uint32_t chunk = 1u << 28;
  for (uint64_t o = 0; o < n; o += chunk) {
    const uint32_t m = (uint32_t)((n - o) < chunk ? (n - o) : chunk);
    k_sqrt_all<<<(m + 255) / 256, 256>>>(b0 + (uint32_t)o, m, d);
    CK(hipGetLastError());
  }
  CK(hipMemcpy(out2, d, 16, hipMemcpyDeviceToHost));
  CK(hipFree(d));
  return 0;
}

extern "C" int check_div(int eb, const int* ea, int nea, int per, uint32_t seed, unsigned long long* out2) {
  unsigned long long* d = nullptr;
  int* dea = nullptr;
  CK(hipMalloc(&d, 16));
  CK(hipMalloc(&dea, sizeof(int) * nea));
  CK(hipMemset(d, 0, 16));
  CK(hipMemcpy(dea, ea, sizeof(int) * nea, hipMemcpyHostToDevice));
  k_div_all<<<(1u << 23) / 256, 256>>>(eb, dea, nea, per, seed, d);
  CK(hipGetLastError());
  CK(hipMemcpy(out2, d, 16, hipMemcpyDeviceToHost));
  CK(hipFree(d));
  CK(hipFree(dea));
  return 0;
}

extern "C" int eval(const float* a, const float* b, int n, float* q, float* sq, int* win) {
  float *da, *db, *dq, *ds;
  int* dw;
  CK(hipMalloc(&da, 4 * (size_t)n)); CK(hipMalloc(&db, 4 * (size_t)n)); CK(hipMalloc(&dq, 4 * (size_t)n)); CK(hipMalloc(&ds, 4 * (size_t)n));
  CK(hipMalloc(&dw, 4 * (size_t)n));
  CK(hipMemcpy(da, a, 4 * (size_t)n, hipMemcpyHostToDevice));
  CK(hipMemcpy(db, b, 4 * (size_t)n, hipMemcpyHostToDevice));
  k_eval<<<(n + 255) / 256, 256>>>(da, db, n, dq, ds, dw);
  CK(hipGetLastError());
  CK(hipMemcpy(q, dq, 4 * (size_t)n, hipMemcpyDeviceToHost));
  CK(hipMemcpy(sq, ds, 4 * (size_t)n, hipMemcpyDeviceToHost));
  CK(hipMemcpy(win, dw, 4 * (size_t)n, hipMemcpyDeviceToHost));
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(dq); (void)hipFree(ds); (void)hipFree(dw);
  return 0;
}
