// scan_fuse.hip -- the ring-tagged scan of the LOAM front end made on the device from the sensors' buffers (include/pcm_amd.h,
// pcm_scan_fuse / pcm_scan_fused), gfx950.  The arithmetic of a point is scan_fuse.h's (shared with the host
// and tested there); this file is the order-preserving compaction around it:
//   k_scan_count   one lane per input point over the concatenated segments: the drop test, the kept count of every workgroup
//                  (wave ballots + popcount) and the per-segment NaN / depth-filter counters out of the same ballots;
//   rocPRIM        exclusive scan over the workgroup counts;
//   k_scan_write   the drop test again, position = workgroup offset + waves before + lanes before (no atomic decides a
//                  position: two runs give the same bytes), the record of a kept point -- the camera points' double transform,
//                  sqrt and asin only here -- as two 16-byte stores.
// Nothing per point is kept between the passes: the second pass re-reads x y z (the input is read twice, 12 of its 32 bytes the
// first time) instead of writing and reading a flag and a position per point.  The segment table (at most 8 entries) travels
// in the kernel arguments; a lane finds its segment by a fixed-trip walk over the 8 start indices.
#include "host_util.h"
#include "pre_layouts.h"
#include "scan_fuse.h"

#include <rocprim/device/device_scan.hpp>

#include <vector>

namespace pcm {

namespace {

using namespace scan;

struct ScanArgs {
  SegView seg[PCM_SCAN_MAX_SEGMENTS];   // unused entries: start = total, n = 0
  FuseRule R;
  uint32_t total;
  uint32_t capacity;                    // records the output holds
};

constexpr int kCtrNan = 0, kCtrFiltered = PCM_SCAN_MAX_SEGMENTS, kCtrClamped = 2 * PCM_SCAN_MAX_SEGMENTS, kCtrCount = 2 * PCM_SCAN_MAX_SEGMENTS + 1;

__device__ inline void load_xyz(const char* rec, uint32_t vec16, float* p) {
  if (vec16) {
    const float4 v = *reinterpret_cast<const float4*>(rec);
    p[0] = v.x; p[1] = v.y; p[2] = v.z;
  } else {
    const float* f = reinterpret_cast<const float*>(rec);
    p[0] = f[0]; p[1] = f[1]; p[2] = f[2];
  }
}

__global__ void __launch_bounds__(256) k_scan_count(const ScanArgs A, uint32_t* __restrict__ block_kept, uint32_t* __restrict__ counters) {
  __shared__ uint32_t s_cnt[kCtrCount];   // [kCtrClamped] holds the kept count here
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  if (threadIdx.x < kCtrCount) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  int cls = -1, seg = 0;
  if (i < A.total) {
    const char* base = A.seg[0].base;
    uint32_t start = 0u, stride = A.seg[0].stride, vec16 = A.seg[0].vec16;
    int kind = A.seg[0].kind;
#pragma unroll
    for (int s = 1; s < PCM_SCAN_MAX_SEGMENTS; s++) {
      if (i >= A.seg[s].start) { seg = s; base = A.seg[s].base; start = A.seg[s].start; stride = A.seg[s].stride; vec16 = A.seg[s].vec16; kind = A.seg[s].kind; }
    }
    float p[3];
    load_xyz(base + (size_t)(i - start) * stride, vec16, p);
    cls = scan_drop_class(kind, p[0], p[1], p[2], A.R.depth_filter);
  }
  const unsigned long long kept = __ballot(cls == kKeep);
  if (lane == 0u && kept) atomicAdd(&s_cnt[kCtrClamped], (uint32_t)__popcll(kept));
#pragma unroll
  for (int s = 0; s < PCM_SCAN_MAX_SEGMENTS; s++) {
    const unsigned long long bn = __ballot(cls == kNan && seg == s), bf = __ballot(cls == kDepthFiltered && seg == s);
    if (lane == 0u && bn) atomicAdd(&s_cnt[kCtrNan + s], (uint32_t)__popcll(bn));
    if (lane == 0u && bf) atomicAdd(&s_cnt[kCtrFiltered + s], (uint32_t)__popcll(bf));
  }
  __syncthreads();
  if (threadIdx.x == 0) block_kept[blockIdx.x] = s_cnt[kCtrClamped];
  if (threadIdx.x < 2 * PCM_SCAN_MAX_SEGMENTS && s_cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], s_cnt[threadIdx.x]);
}

__global__ void __launch_bounds__(256) k_scan_write(const ScanArgs A, const uint32_t* __restrict__ block_off, uint4* __restrict__ out, uint32_t* __restrict__ counters) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  bool keep = false, clamped = false;
  SegView S = A.seg[0];
  float p[3] = {0.f, 0.f, 0.f};
  const char* rec = nullptr;
  if (i < A.total) {
#pragma unroll
    for (int s = 1; s < PCM_SCAN_MAX_SEGMENTS; s++) {
      if (i >= A.seg[s].start) S = A.seg[s];
    }
    rec = S.base + (size_t)(i - S.start) * S.stride;
    load_xyz(rec, S.vec16, p);
    keep = scan_drop_class(S.kind, p[0], p[1], p[2], A.R.depth_filter) == kKeep;
  }
  const unsigned long long kept = __ballot(keep);
  if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(kept);
  __syncthreads();
  uint32_t pos = block_off[blockIdx.x] + (uint32_t)__popcll(kept & ((1ull << lane) - 1ull));
  for (uint32_t w = 0; w < wave; w++) pos += s_wave[w];
  if (keep && pos < A.capacity) {
    uint32_t w[8];
    scan_point_record(S, A.R, rec, i - S.start, p[0], p[1], p[2], w, &clamped);
    out[2 * (size_t)pos] = make_uint4(w[0], w[1], w[2], w[3]);
    out[2 * (size_t)pos + 1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
  const unsigned long long bc = __ballot(clamped);
  if (lane == 0u && bc) atomicAdd(&counters[kCtrClamped], (uint32_t)__popcll(bc));
}

#define CHECK_CTX(c)                                                   \
  do {                                                                 \
    if (!(c)) return PCM_ERR_INVALID_ARGUMENT;                         \
    if ((c)->device < 0) return PCM_ERR_HIP;                           \
  } while (0)

}  // namespace

}  // namespace pcm

using namespace pcm;

extern "C" {

void pcm_scan_default_fuse_params(pcm_scan_fuse_params* params) {
  if (params) scan::scan_default_params(params);
}

int pcm_scan_fuse(pcm_ctx* c, const pcm_scan_segment* segs, int n_segs, const pcm_scan_fuse_params* params, void* out, size_t capacity_points, int out_memory,
                  pcm_scan_fuse_result* res) {
  CHECK_CTX(c);
  if (!res) { c->err = "null result"; return PCM_ERR_INVALID_ARGUMENT; }
  std::memset(res, 0, sizeof(*res));
  res->status = PCM_ERR_INVALID_ARGUMENT;
  pcm_scan_fuse_params P;
  if (params) P = *params; else scan::scan_default_params(&P);
  if (const char* why = scan::scan_check_args(segs, n_segs, &P)) { c->err = why; return PCM_ERR_INVALID_ARGUMENT; }
  if (out && check_memory(c, out_memory, "out_memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  if (out && out_memory == PCM_MEM_DEVICE && ((uintptr_t)out % 16) != 0) { c->err = "a device output buffer must be 16-byte aligned"; return PCM_ERR_INVALID_ARGUMENT; }
  size_t total = 0;
  for (int s = 0; s < n_segs; s++) {
    int rc = check_point_records(c, segs[s].points, segs[s].n, segs[s].stride_bytes, segs[s].memory, scan::kScanMaxPoints);
    if (rc != PCM_OK) return rc;
    total += segs[s].n;
  }
  PCM_HIPCK(c, hipSetDevice(c->device));
  const bool own_out = !out || out_memory == PCM_MEM_HOST;   // the records are written to the context's buffer
  if (own_out) c->scan_n = 0;   // the context's buffer is about to be rewritten
  const size_t nb = (total + 255) / 256;
  size_t scan_tmp_bytes = 0;
  {
    uint32_t* v = nullptr;
    (void)rocprim::exclusive_scan(nullptr, scan_tmp_bytes, v, v, 0u, nb ? nb : 1, rocprim::plus<uint32_t>(), c->stream);
  }
  const void* seg_base[PCM_SCAN_MAX_SEGMENTS] = {nullptr};
  ArenaCarver tmp_size;
  ArenaStage in_size = arena_stage(c, nullptr);
  (void)scan_scratch_layout(tmp_size, kCtrCount, segs, n_segs, P, nb, scan_tmp_bytes);
  scan_input_layout(in_size, segs, n_segs, seg_base);
  const size_t tmp_need = tmp_size.used(), in_bytes = in_size.used();
  int rc = c->scan_tmp.reserve(c, tmp_need, tmp_need + tmp_need / 4);
  if (rc != PCM_OK) return rc;
  if (in_bytes && (rc = c->scan_in.reserve(c, in_bytes, in_bytes + in_bytes / 4)) != PCM_OK) return rc;
  if (own_out && total && (rc = c->scan_out.reserve(c, 32 * total, 32 * total + 8 * total)) != PCM_OK) return rc;
  ArenaCarver tmp_carver(c->scan_tmp.p);
  const ScanScratch T = scan_scratch_layout(tmp_carver, kCtrCount, segs, n_segs, P, nb, scan_tmp_bytes);
  ArenaStage in_stage = arena_stage(c, c->scan_in.p);   // every host segment staged, one upload each
  scan_input_layout(in_stage, segs, n_segs, seg_base);
  if (in_stage.rc != PCM_OK) return in_stage.rc;

  // tables: cast to uint16 as the reference's assignment to `ring` does, one upload
  std::vector<uint16_t> h_tab((size_t)(reinterpret_cast<uint16_t*>(T.kept) - T.pitch_tab), 0);
  ScanArgs A;
  std::memset(&A, 0, sizeof(A));
  if (P.pitch_ring_table)
    for (int k = 0; k < P.pitch_ring_table_len; k++) h_tab[k] = (uint16_t)P.pitch_ring_table[k];
  A.R = scan::scan_rule(P, T.pitch_tab);
  uint32_t start = 0;
  for (int s = 0; s < PCM_SCAN_MAX_SEGMENTS; s++) {
    if (s >= n_segs) { A.seg[s].start = (uint32_t)total; A.seg[s].stride = 16; A.seg[s].divisor = 1; continue; }
    const pcm_scan_segment& g = segs[s];
    if (g.kind == PCM_SCAN_LIDAR_XYZI)
      for (int k = 0; k < g.ring_table_len; k++) h_tab[(size_t)(T.seg_tab[s] - T.pitch_tab) + k] = (uint16_t)g.ring_table[k];
    A.seg[s] = scan::scan_view(g, static_cast<const char*>(seg_base[s]), T.seg_tab[s], start);
    start += (uint32_t)g.n;
  }
  A.total = (uint32_t)total;
  A.capacity = (uint32_t)(out ? (capacity_points < total ? capacity_points : total) : total);

  uint32_t h_ctr[kCtrCount] = {0};
  uint32_t *d_ctr = T.ctr, *d_kept = T.kept, *d_off = T.off;
  if (total) {
    PCM_HIPCK(c, hipMemsetAsync(d_ctr, 0, 4 * kCtrCount, c->stream));
    if (!h_tab.empty()) PCM_HIPCK(c, hipMemcpyAsync(T.pitch_tab, h_tab.data(), 2 * h_tab.size(), hipMemcpyHostToDevice, c->stream));
    uint4* d_out = reinterpret_cast<uint4*>(own_out ? c->scan_out.p : static_cast<char*>(out));
    k_scan_count<<<(unsigned)nb, 256, 0, c->stream>>>(A, d_kept, d_ctr);
    PCM_HIPCK(c, hipGetLastError());
    PCM_HIPCK(c, rocprim::exclusive_scan(T.tmp, scan_tmp_bytes, d_kept, d_off, 0u, nb, rocprim::plus<uint32_t>(), c->stream));
    k_scan_write<<<(unsigned)nb, 256, 0, c->stream>>>(A, d_off, d_out, d_ctr);
    PCM_HIPCK(c, hipGetLastError());
    PCM_HIPCK(c, hipMemcpyAsync(h_ctr, d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, c->stream));
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the one synchronisation: n_out (h_tab and the host inputs are free again, too)
  }
  scan::scan_fill_result(segs, n_segs, h_ctr + kCtrNan, h_ctr + kCtrFiltered, h_ctr[kCtrClamped], res);
  if (out && res->n_out > capacity_points) { c->err = "output buffer too small"; return PCM_ERR_INVALID_ARGUMENT; }
  if (out && out_memory == PCM_MEM_HOST && res->n_out) {
    PCM_HIPCK(c, hipMemcpyAsync(out, c->scan_out.p, 32 * (size_t)res->n_out, hipMemcpyDeviceToHost, c->stream));
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  }
  if (!out) c->scan_n = res->n_out;
  res->status = PCM_OK;
  return PCM_OK;
}

int pcm_scan_fused(pcm_ctx* c, const void** device_points, size_t* n) {
  CHECK_CTX(c);
  if (!device_points || !n) { c->err = "null output"; return PCM_ERR_INVALID_ARGUMENT; }
  *device_points = c->scan_n ? c->scan_out.p : nullptr;
  *n = c->scan_n;
  return PCM_OK;
}

}  // extern "C"
