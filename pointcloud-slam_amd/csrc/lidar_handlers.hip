// lidar_handlers.hip -- jueying_lio's PointCloud2 handlers on the device (include/pcm_amd.h, pcm_lidar_filter; DESIGN.md section
// 16), gfx950.  The arithmetic of a point is lidar_handlers.h's (shared with the host and tested there); this file is the parallel
// form around it.
//
// Yaw path (Velodyne / RoboSense clouds without times): the reference carries time_last[ring] serially through the cloud.  Each
// point is a function of time_last of the form x > b ? hi : lo, such functions compose exactly into one of the same form
// (lh_compose), and a ring's first point is a constant, which also cuts the chain between two rings.  So:
//   k_lh_yaw          one lane per point: yaw (double atan2), the sort key (ring) and value (input index), the bad-ring count;
//   rocPRIM           one stable 8-bit radix pass over (ring, index): input order is kept inside a ring;
//   k_lh_heads        the first point of every ring -> first_idx[ring] (one writer per ring);
//   k_lh_block_totals the composition of each workgroup's 256 functions (wave scan by shuffles, then the 4 wave totals);
//   k_lh_tops         one workgroup walks the workgroup totals 256 at a time and leaves time_last as it enters every workgroup;
//   k_lh_times        the workgroup scan again, applied to that value: the curvature, stored at the point's input position.
// All four handlers then share k_lh_flags -> rocPRIM exclusive scan -> k_lh_write, as the Livox message filter does.  No atomic
// decides a position and no sum is reordered: two runs give the same bytes.  Every lane of a wave runs every shuffle; a lane
// past the end carries the constant function, which sits behind every real point.
#include "host_util.h"
#include "lidar_handlers.h"
#include "pre_layouts.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cstdio>

namespace pcm {

namespace {

using namespace lidar;

constexpr uint32_t kLhBlock = 256;

__global__ void __launch_bounds__(kLhBlock) k_lh_yaw(const LhView V, double* __restrict__ yaw, uint8_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t* __restrict__ bad) {
  const uint32_t i = blockIdx.x * kLhBlock + threadIdx.x;
  bool is_bad = false;
  if (i < V.n) {
    const char* rec = V.base + (size_t)i * V.stride;
    yaw[i] = lh_yaw(lh_load_f32(rec + V.xoff), lh_load_f32(rec + V.xoff + 4));
    const uint32_t ring = lh_ring(V, rec);
    is_bad = ring >= (uint32_t)V.num_scans;
    key[i] = (uint8_t)(ring < 255u ? ring : 255u);   // every table has 256 slots; a bad ring fails the call later
    val[i] = i;
  }
  const unsigned long long m = __ballot(is_bad);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(bad, (uint32_t)__popcll(m));   // an integer count: the same in every order
}

__global__ void __launch_bounds__(kLhBlock) k_lh_heads(const uint8_t* __restrict__ key_s, const uint32_t* __restrict__ val_s, uint32_t n, uint32_t* __restrict__ first_idx) {
  const uint32_t j = blockIdx.x * kLhBlock + threadIdx.x;
  if (j >= n) return;
  const uint8_t r = key_s[j];
  if (j == 0 || key_s[j - 1] != r) first_idx[r] = val_s[j];
}

// the function of the point at sorted position j
__device__ inline LhFn lh_fn_at(uint32_t j, uint32_t n, const uint8_t* __restrict__ key_s, const uint32_t* __restrict__ val_s, const double* __restrict__ yaw,
                                const uint32_t* __restrict__ first_idx) {
  if (j >= n) return lh_fn_first();
  const uint32_t i = val_s[j], fi = first_idx[key_s[j]];
  if (fi == i) return lh_fn_first();
  return lh_fn_point(lh_b(yaw[i], yaw[fi]));
}

__device__ inline LhFn lh_shfl_up(const LhFn& f, int off) { return LhFn{__shfl_up(f.b, off, 64), __shfl_up(f.lo, off, 64), __shfl_up(f.hi, off, 64)}; }

// inclusive scan of one function per lane over the workgroup's kLhBlock lanes, in lane order; *total: all of them composed, in
// every lane.  sh: kLhBlock / 64 entries, free again on return.
__device__ inline LhFn lh_block_scan(LhFn f, LhFn* sh, LhFn* total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const LhFn c = lh_compose(lh_shfl_up(f, off), f);   // every lane shuffles; the lanes without a partner keep theirs
    if (lane >= (uint32_t)off) f = c;
  }
  if (lane == 63u) sh[wv] = f;
  __syncthreads();
  LhFn acc = sh[0], inc = f;
#pragma unroll
  for (uint32_t w = 1; w < kLhBlock / 64; w++) {
    if (w == wv) inc = lh_compose(acc, f);   // wave-uniform
    acc = lh_compose(acc, sh[w]);
  }
  __syncthreads();
  *total = acc;
  return inc;
}

__global__ void __launch_bounds__(kLhBlock) k_lh_block_totals(uint32_t n, const uint8_t* __restrict__ key_s, const uint32_t* __restrict__ val_s, const double* __restrict__ yaw,
                                                              const uint32_t* __restrict__ first_idx, LhFn* __restrict__ tot) {
  __shared__ LhFn sh[kLhBlock / 64];
  LhFn total;
  (void)lh_block_scan(lh_fn_at(blockIdx.x * kLhBlock + threadIdx.x, n, key_s, val_s, yaw, first_idx), sh, &total);
  if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// one workgroup: after[k] = time_last behind workgroup k's points.  The chain starts at a ring's first point, a constant, so the
// value it starts from (0) is never seen.
__global__ void __launch_bounds__(kLhBlock) k_lh_tops(const LhFn* __restrict__ tot, uint32_t nb, float* __restrict__ after) {
  __shared__ LhFn sh[kLhBlock / 64];
  float carry = 0.f;
  for (uint32_t base = 0; base < nb; base += kLhBlock) {
    const uint32_t k = base + threadIdx.x;
    LhFn total;
    const LhFn inc = lh_block_scan(k < nb ? tot[k] : lh_fn_first(), sh, &total);
    if (k < nb) after[k] = lh_apply(inc, carry);
    carry = lh_apply(total, carry);
  }
}

__global__ void __launch_bounds__(kLhBlock) k_lh_times(uint32_t n, const uint8_t* __restrict__ key_s, const uint32_t* __restrict__ val_s, const double* __restrict__ yaw,
                                                       const uint32_t* __restrict__ first_idx, const float* __restrict__ after, float* __restrict__ curv) {
  __shared__ LhFn sh[kLhBlock / 64];
  const uint32_t j = blockIdx.x * kLhBlock + threadIdx.x;
  LhFn total;
  const LhFn inc = lh_block_scan(lh_fn_at(j, n, key_s, val_s, yaw, first_idx), sh, &total);
  const float before = blockIdx.x ? after[blockIdx.x - 1] : 0.f;
  if (j < n) curv[val_s[j]] = lh_apply(inc, before);
}

__global__ void __launch_bounds__(kLhBlock) k_lh_flags(const LhView V, int given, const uint32_t* __restrict__ first_idx, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * kLhBlock + threadIdx.x;
  if (i >= V.n) return;
  const char* rec = V.base + (size_t)i * V.stride;
  bool keep = lh_keep(V, i, lh_load_f32(rec + V.xoff), lh_load_f32(rec + V.xoff + 4), lh_load_f32(rec + V.xoff + 8));
  if (!given) {   // the ring's first point leaves through the reference's `continue`
    const uint32_t ring = lh_ring(V, rec);
    keep = keep && ring < (uint32_t)V.num_scans && first_idx[ring < 255u ? ring : 255u] != i;
  }
  flag[i] = keep ? 1u : 0u;
}

__global__ void __launch_bounds__(kLhBlock) k_lh_write(const LhView V, int given, const float* __restrict__ curv, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                       uint32_t capacity, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * kLhBlock + threadIdx.x;
  if (i >= V.n || !flag[i]) return;
  const uint32_t p = pos[i];
  if (p >= capacity) return;
  const char* rec = V.base + (size_t)i * V.stride;
  float w[12];
  lh_record(lh_load_f32(rec + V.xoff), lh_load_f32(rec + V.xoff + 4), lh_load_f32(rec + V.xoff + 8), lh_load_f32(rec + V.ioff),
            given ? lh_curvature_given(V, rec, lh_time(V, V.base)) : curv[i], w);
  float4* o = out + 3 * (size_t)p;
  o[0] = make_float4(w[0], w[1], w[2], w[3]);
  o[1] = make_float4(w[4], w[5], w[6], w[7]);
  o[2] = make_float4(w[8], w[9], w[10], w[11]);
}

__global__ void __launch_bounds__(kLhBlock) k_lh_time_keys(const float* __restrict__ rec48, uint32_t m, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t j = blockIdx.x * kLhBlock + threadIdx.x;
  if (j >= m) return;
  key[j] = lh_time_key(rec48[12 * (size_t)j + 9]);
  val[j] = j;
}

__global__ void __launch_bounds__(kLhBlock) k_lh_gather(const float4* __restrict__ in, const uint32_t* __restrict__ val_s, uint32_t m, float4* __restrict__ out) {
  const uint32_t j = blockIdx.x * kLhBlock + threadIdx.x;
  if (j >= m) return;
  const float4* s = in + 3 * (size_t)val_s[j];
  float4* o = out + 3 * (size_t)j;
  o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
}

// rocPRIM's temporaries for one handler call of n points
void lh_tmp_bytes(size_t n, size_t* scan_bytes, size_t* sort_bytes) {
  uint32_t* v = nullptr; uint8_t* k = nullptr;
  *scan_bytes = 0; *sort_bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, *scan_bytes, v, v, 0u, n ? n : 1, rocprim::plus<uint32_t>(), nullptr);
  (void)rocprim::radix_sort_pairs(nullptr, *sort_bytes, k, k, v, v, n ? n : 1, 0, 8, nullptr);
}

#define CHECK_CTX(c)                                                   \
  do {                                                                 \
    if (!(c)) return PCM_ERR_INVALID_ARGUMENT;                         \
    if ((c)->device < 0) return PCM_ERR_HIP;                           \
  } while (0)

}  // namespace

size_t lidar_filter_scratch_bytes(size_t n) {
  size_t scan_bytes, sort_bytes;
  lh_tmp_bytes(n, &scan_bytes, &sort_bytes);
  ArenaCarver a;
  (void)lidar_filter_layout(a, n, kLhBlock, scan_bytes, sort_bytes);
  return a.used();
}

// d_pts: n >= 1 records on the device (the descriptor has passed lh_check_desc); d_out: room for `capacity` records, 16-byte
// aligned.  given_hint: what lh_given_time says when the caller could read the cloud on the host, -1 to read the last point's
// time back here.  *n_out counts every kept point; no record past the capacity is written.  One synchronisation at the end.
int lidar_filter_device(hipStream_t stream, const void* d_pts, size_t n, const pcm_lidar_desc& D, int given_hint, void* d_out, size_t capacity, size_t* n_out, int* given_out,
                        void* scratch, std::string* err) {
  *n_out = 0;
  LhView V = lh_view(D, d_pts, n);
  int given = given_hint;
  if (given < 0) {
    given = 1;
    if (lh_uses_yaw_path(D.type)) {   // the last record's time field (at most 8 bytes), read as the header reads it
      alignas(8) char last[8] = {0};
      const size_t tsize = D.time_kind == PCM_LIDAR_TIME_DOUBLE ? 8 : 4;
      PCM_HIPCK_ERR(err, hipMemcpyAsync(last, V.base + (n - 1) * (size_t)V.stride + V.toff, tsize, hipMemcpyDeviceToHost, stream));
      PCM_HIPCK_ERR(err, hipStreamSynchronize(stream));
      LhView H = V;
      H.base = last; H.n = 1; H.toff = 0;
      given = lh_given_time(H) ? 1 : 0;
    }
  }
  *given_out = given;
  size_t scan_bytes, sort_bytes;
  lh_tmp_bytes(n, &scan_bytes, &sort_bytes);
  ArenaCarver a(scratch);
  const LhScratch S = lidar_filter_layout(a, n, kLhBlock, scan_bytes, sort_bytes);
  const unsigned nb = (unsigned)((n + kLhBlock - 1) / kLhBlock);
  PCM_HIPCK_ERR(err, hipMemsetAsync(S.small, 0, 256, stream));
  if (!given) {
    PCM_HIPCK_ERR(err, hipMemsetAsync(S.first_idx, 0xff, 4 * PCM_LIDAR_MAX_SCANS, stream));
    k_lh_yaw<<<nb, kLhBlock, 0, stream>>>(V, S.yaw, S.key, S.val, S.small);
    PCM_HIPCK_ERR(err, hipGetLastError());
    PCM_HIPCK_ERR(err, rocprim::radix_sort_pairs(S.sort_tmp, sort_bytes, S.key, S.key_s, S.val, S.val_s, n, 0, 8, stream));
    k_lh_heads<<<nb, kLhBlock, 0, stream>>>(S.key_s, S.val_s, (uint32_t)n, S.first_idx);
    k_lh_block_totals<<<nb, kLhBlock, 0, stream>>>((uint32_t)n, S.key_s, S.val_s, S.yaw, S.first_idx, S.tot);
    k_lh_tops<<<1, kLhBlock, 0, stream>>>(S.tot, nb, S.after);
    k_lh_times<<<nb, kLhBlock, 0, stream>>>((uint32_t)n, S.key_s, S.val_s, S.yaw, S.first_idx, S.after, S.curv);
    PCM_HIPCK_ERR(err, hipGetLastError());
  }
  k_lh_flags<<<nb, kLhBlock, 0, stream>>>(V, given, S.first_idx, S.flag);
  PCM_HIPCK_ERR(err, hipGetLastError());
  PCM_HIPCK_ERR(err, rocprim::exclusive_scan(S.scan_tmp, scan_bytes, S.flag, S.pos, 0u, n, rocprim::plus<uint32_t>(), stream));
  k_lh_write<<<nb, kLhBlock, 0, stream>>>(V, given, S.curv, S.flag, S.pos, (uint32_t)(capacity < n ? capacity : n), static_cast<float4*>(d_out));
  PCM_HIPCK_ERR(err, hipGetLastError());
  uint32_t tails[3] = {0, 0, 0};
  PCM_HIPCK_ERR(err, hipMemcpyAsync(&tails[0], S.flag + (n - 1), 4, hipMemcpyDeviceToHost, stream));
  PCM_HIPCK_ERR(err, hipMemcpyAsync(&tails[1], S.pos + (n - 1), 4, hipMemcpyDeviceToHost, stream));
  PCM_HIPCK_ERR(err, hipMemcpyAsync(&tails[2], S.small, 4, hipMemcpyDeviceToHost, stream));
  PCM_HIPCK_ERR(err, hipStreamSynchronize(stream));
  if (tails[2]) {
    char msg[160];
    std::snprintf(msg, sizeof(msg), "%u of the %zu points have a ring >= num_scans (%d)", tails[2], n, D.num_scans);
    *err = msg;
    return PCM_ERR_INVALID_ARGUMENT;
  }
  *n_out = (size_t)tails[0] + tails[1];
  return PCM_OK;
}

// rocPRIM's temporary for the time sort of m records
static size_t lh_time_sort_tmp_bytes(size_t m) {
  size_t t = 0;
  uint32_t* v = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, t, v, v, v, v, m ? m : 1, 0, 32, nullptr);
  return t;
}

size_t lidar_time_sort_scratch_bytes(size_t m) {
  ArenaCarver a;
  (void)lidar_time_sort_layout(a, m, lh_time_sort_tmp_bytes(m));
  return a.used();
}

// d_in: m 48-byte records; d_out: the same records in (curvature, input index) order (lh_time_key; the radix sort is stable)
int lidar_time_sort_device(hipStream_t stream, const void* d_in, size_t m, void* d_out, void* scratch, std::string* err) {
  if (m == 0) return PCM_OK;
  size_t t = lh_time_sort_tmp_bytes(m);
  ArenaCarver a(scratch);
  const TimeSortScratch S = lidar_time_sort_layout(a, m, t);
  uint32_t *key = S.key, *key_s = S.key_s, *val = S.val, *val_s = S.val_s;
  const unsigned nb = (unsigned)((m + kLhBlock - 1) / kLhBlock);
  k_lh_time_keys<<<nb, kLhBlock, 0, stream>>>(static_cast<const float*>(d_in), (uint32_t)m, key, val);
  PCM_HIPCK_ERR(err, hipGetLastError());
  PCM_HIPCK_ERR(err, rocprim::radix_sort_pairs(S.tmp, t, key, key_s, val, val_s, m, 0, 32, stream));
  k_lh_gather<<<nb, kLhBlock, 0, stream>>>(static_cast<const float4*>(d_in), val_s, (uint32_t)m, static_cast<float4*>(d_out));
  PCM_HIPCK_ERR(err, hipGetLastError());
  return PCM_OK;
}

// the argument rules pcm_lidar_filter and pcm_lio_frame_begin_cloud share
int lidar_check_cloud(pcm_ctx* c, const void* points, size_t n, int memory, const pcm_lidar_desc* desc) {
  if (const char* why = lh_check_desc(desc)) { c->err = why; return PCM_ERR_INVALID_ARGUMENT; }
  if (!points && n) { c->err = "null point buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  if (check_memory(c, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  if (n > kLhMaxPoints) { c->err = "cloud too large"; return PCM_ERR_INVALID_ARGUMENT; }
  if (((uintptr_t)points % 4) != 0) { c->err = "the point buffer must be 4-byte aligned"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

int lidar_given_on_host(const void* points, size_t n, const pcm_lidar_desc& D) { return lh_given_time(lh_view(D, points, n)) ? 1 : 0; }

}  // namespace pcm

using namespace pcm;

extern "C" {

int pcm_lidar_default_desc(int type, pcm_lidar_desc* desc) {
  if (!desc) return PCM_ERR_INVALID_ARGUMENT;
  lidar::lh_default_desc(type, desc);
  return lidar::lh_check_desc(desc) ? PCM_ERR_INVALID_ARGUMENT : PCM_OK;
}

int pcm_lidar_filter(pcm_ctx* c, const void* points, size_t n, int memory, const pcm_lidar_desc* desc, void* out, size_t capacity_points, int out_memory, size_t* n_out,
                     int* given_offset_time) {
  CHECK_CTX(c);
  if (!n_out) { c->err = "null n_out"; return PCM_ERR_INVALID_ARGUMENT; }
  *n_out = 0;
  int rc = lidar_check_cloud(c, points, n, memory, desc);
  if (rc != PCM_OK) return rc;
  if (!out && capacity_points) { c->err = "null output buffer"; return PCM_ERR_INVALID_ARGUMENT; }
  if (check_memory(c, out_memory, "out_memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  if (out_memory == PCM_MEM_DEVICE && ((uintptr_t)out % 16) != 0) { c->err = "a device output buffer must be 16-byte aligned"; return PCM_ERR_INVALID_ARGUMENT; }
  if (given_offset_time) *given_offset_time = 1;
  if (n == 0) return PCM_OK;
  PCM_HIPCK(c, hipSetDevice(c->device));
  const size_t cap = capacity_points < n ? capacity_points : n;
  const size_t scratch_bytes = lidar_filter_scratch_bytes(n);
  FilterArena F;
  rc = carve_pre_arena(c, "pcm_lidar_filter", [&](ArenaStage& a) { F = filter_layout(a, memory, points, n * desc->stride_bytes, out_memory, out, 48 * (cap ? cap : 1), scratch_bytes); });
  if (rc != PCM_OK) return rc;
  const int hint = memory == PCM_MEM_HOST ? lidar_given_on_host(points, n, *desc) : -1;
  size_t m = 0;
  int given = 1;
  rc = lidar_filter_device(c->stream, F.src, n, *desc, hint, F.dst, cap, &m, &given, F.scratch, &c->err);
  if (given_offset_time) *given_offset_time = given;
  if (rc != PCM_OK) return rc;
  *n_out = m;
  if (m > capacity_points) { c->err = "output buffer too small"; return PCM_ERR_INVALID_ARGUMENT; }
  if (out_memory == PCM_MEM_HOST && m) {
    if ((rc = stage_back(c, out_memory, out, F.dst, 48 * m)) != PCM_OK) return rc;
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  }
  return PCM_OK;
}

}  // extern "C"
