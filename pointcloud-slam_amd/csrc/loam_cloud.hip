// loam_cloud.hip -- jueying_slam's cachePointCloud on the device: the driver's organised cloud becomes the ring-tagged,
// time-stamped records the LOAM front end reads, in a buffer of the context (include/pcm_amd.h, pcm_loam_cloud_prepare /
// pcm_loam_cloud_cached / pcm_loam_frame_begin_cloud[_batch]), gfx950.  The making of a record -- the
// field copies, the ring and time rules, the zero padding -- is loam_cloud.h's (shared with the host and tested there); this file is
// the order-preserving NaN removal around it, for the B clouds of B contexts in one round of launches (grid.y = cloud):
//   k_lc_count     non-dense clouds: one lane per input record, the finite test, the kept count of every workgroup (wave ballots +
//                  popcount; the workgroups of all clouds share one array);
//   rocPRIM        one exclusive scan over the workgroup counts of the batch, one element more than counts: the total;
//   k_lc_write     the finite test again, position = workgroup offset - the cloud's first offset + waves before + lanes before (no
//                  atomic decides a position: two runs give the same bytes), the record as 16-byte stores; a dense cloud's
//                  position is its index.  Lane 0 of a non-dense cloud's first workgroup leaves the cloud's kept count.
// A batch of dense clouds runs k_lc_write alone and reads nothing back; otherwise the kept counts are the one read-back between
// the upload and the features.  The records are read where they lie at any even point_step (loam_cloud.h: a word that is not
// 4-byte aligned is read as two halves); a host cloud is staged in one upload of its raw bytes.
#include "host_util.h"
#include "loam_cloud.h"
#include "loam_device.h"
#include "pre_layouts.h"

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

using namespace pcm;

namespace {

constexpr uint32_t kLcBlock = 256;

struct LcFrame {
  loam::CloudView V;
  uint4* out;           // records (16-byte aligned)
  uint32_t capacity;    // records `out` holds
  uint32_t blk0, nblk;  // a non-dense cloud's workgroups in the batch's count / offset arrays (nblk = 0: dense or empty)
};

__global__ void __launch_bounds__(kLcBlock) k_lc_count(const LcFrame* __restrict__ fr, uint32_t* __restrict__ block_kept) {
  __shared__ uint32_t s_wave[kLcBlock / 64];
  const LcFrame& F = fr[blockIdx.y];
  if (blockIdx.x >= F.nblk) return;   // the same in every lane of the workgroup
  const uint32_t i = blockIdx.x * kLcBlock + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const bool keep = i < F.V.n && loam::cloud_finite(F.V, F.V.base + (size_t)i * F.V.step);
  const unsigned long long kept = __ballot(keep);
  if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(kept);
  __syncthreads();
  if (threadIdx.x == 0) block_kept[F.blk0 + blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

__global__ void __launch_bounds__(kLcBlock) k_lc_write(const LcFrame* __restrict__ fr, const uint32_t* __restrict__ block_off, uint32_t* __restrict__ info) {
  __shared__ uint32_t s_wave[kLcBlock / 64];
  const LcFrame& F = fr[blockIdx.y];
  if ((size_t)blockIdx.x * kLcBlock >= F.V.n) return;   // the same in every lane of the workgroup
  const uint32_t i = blockIdx.x * kLcBlock + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const char* rec = F.V.base + (size_t)i * F.V.step;
  uint32_t pos = i;
  bool keep = i < F.V.n;
  if (F.nblk) {   // a non-dense cloud
    keep = keep && loam::cloud_finite(F.V, rec);
    const unsigned long long kept = __ballot(keep);
    if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(kept);
    __syncthreads();
    const uint32_t first = block_off[F.blk0];
    pos = block_off[F.blk0 + blockIdx.x] - first + (uint32_t)__popcll(kept & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; w++) pos += s_wave[w];
    if (blockIdx.x == 0 && threadIdx.x == 0) info[blockIdx.y] = block_off[F.blk0 + F.nblk] - first;
  }
  if (!keep || pos >= F.capacity) return;
  uint32_t w[12];
  loam::cloud_record(F.V, rec, i, w);
  if (F.V.kind == PCM_LOAM_CLOUD_MAPPING) {
    uint4* o = F.out + 3 * (size_t)pos;
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    o[2] = make_uint4(w[8], w[9], w[10], w[11]);
  } else {
    uint4* o = F.out + 2 * (size_t)pos;
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
}

// what a context keeps of cachePointCloud: the staged raw clouds and the scratch of a call it leads, and its own prepared cloud
struct CloudState {
  DevBuf<char> in{"loam cloud staging"}, tmp{"loam cloud scratch"};
  DevBuf<uint4> out{"loam cloud records"};
  DevBuf<LcFrame> d_fr{"loam cloud frames"};
  PinnedBuf<LcFrame> h_fr{"loam cloud frames (host)"};
  size_t n = 0;          // records of the last call with out = NULL that `out` still holds
  uint32_t stride = 0;   // their size
};

CloudState* cloud_of(pcm_ctx* c) { return c->loam_cloud.get_or_create<CloudState>(); }

int check_ctx_cloud(pcm_ctx* c) {
  const int rc = loam::loam_check_ctx(c, PCM_ERR_UNSUPPORTED, "pcm_loam_cloud_* / pcm_loam_frame_begin_cloud* need a context created with PCM_MODEL_LOAM");
  if (rc != PCM_OK) return rc;
  if (!cloud_of(c)) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  return PCM_OK;
}

// cachePointCloud of B clouds of B contexts on the first context's stream.  user_out (B == 1 only): the caller's buffer of
// `capacity` records, else every cloud goes to its context's buffer.  Every argument is checked before any device work.
int prepare_frames(pcm_ctx* const* ctxs, int B, const void* const* data, const pcm_loam_cloud_desc* descs, int memory, void* user_out, size_t capacity, int out_memory,
                   pcm_loam_cloud_result* results) {
  if (!ctxs || B <= 0 || !ctxs[0]) return PCM_ERR_INVALID_ARGUMENT;
  pcm_ctx* c0 = ctxs[0];
  int rc = check_ctx_cloud(c0);
  if (rc != PCM_OK) return rc;
  if (!data || !descs || !results) { c0->err = "null argument"; return PCM_ERR_INVALID_ARGUMENT; }
  if (check_memory(c0, memory, "memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < B; i++) {
    std::memset(&results[i], 0, sizeof(results[i]));
    results[i].status = PCM_ERR_INVALID_ARGUMENT;
  }
  std::vector<size_t> bytes((size_t)B);
  for (int i = 0; i < B; i++) {
    if ((rc = check_ctx_cloud(ctxs[i])) != PCM_OK) { if (ctxs[i] && ctxs[i] != c0) c0->err = ctxs[i]->err; return rc; }
    if (ctxs[i]->device != c0->device) { c0->err = "all contexts of a batch must live on one device"; return PCM_ERR_INVALID_ARGUMENT; }
    for (int j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) { c0->err = "a context appears twice in the batch"; return PCM_ERR_INVALID_ARGUMENT; }
    if (const char* why = loam::cloud_check_desc(&descs[i])) { c0->err = why; return PCM_ERR_INVALID_ARGUMENT; }
    if (descs[i].record_kind != descs[0].record_kind) { c0->err = "all clouds of a batch must have one record_kind"; return PCM_ERR_INVALID_ARGUMENT; }
    const size_t n = (size_t)descs[i].height * descs[i].width;
    if (!data[i] && n) { c0->err = "null cloud buffer"; return PCM_ERR_INVALID_ARGUMENT; }
    if ((reinterpret_cast<uintptr_t>(data[i]) % 4) != 0) { c0->err = "the cloud buffer must be 4-byte aligned"; return PCM_ERR_INVALID_ARGUMENT; }
    bytes[(size_t)i] = n * descs[i].point_step;
  }
  if (user_out) {
    if (B != 1) return PCM_ERR_INVALID_ARGUMENT;
    if (check_memory(c0, out_memory, "out_memory") != PCM_OK) return PCM_ERR_INVALID_ARGUMENT;
    if (out_memory == PCM_MEM_DEVICE && (reinterpret_cast<uintptr_t>(user_out) % 16) != 0) { c0->err = "a device output buffer must be 16-byte aligned"; return PCM_ERR_INVALID_ARGUMENT; }
  }
  PCM_HIPCK(c0, hipSetDevice(c0->device));
  const bool own_out = !user_out || out_memory == PCM_MEM_HOST;   // the records are written to the context's buffer
  const uint32_t rec_bytes = loam::cloud_record_bytes(descs[0].record_kind), rec_vecs = rec_bytes / 16;
  // the workgroups of the non-dense clouds, one after the other
  CloudState* S0 = cloud_of(c0);
  if ((rc = S0->h_fr.reserve(c0, (size_t)B, (size_t)B)) != PCM_OK) return rc;
  PCM_HIPCK(c0, hipStreamSynchronize(c0->stream));   // the pinned frame records of an earlier call are free again
  LcFrame* h_fr = S0->h_fr.p;
  size_t nb = 0;
  uint32_t max_scan = 0, max_all = 0;
  for (int i = 0; i < B; i++) {
    LcFrame& F = h_fr[i];
    std::memset(&F, 0, sizeof(F));
    const size_t n = (size_t)descs[i].height * descs[i].width;
    const uint32_t blocks = (uint32_t)((n + kLcBlock - 1) / kLcBlock);
    F.blk0 = (uint32_t)nb;
    F.nblk = descs[i].is_dense ? 0u : blocks;
    nb += F.nblk;
    max_scan = std::max(max_scan, F.nblk);
    max_all = std::max(max_all, blocks);
  }
  size_t scan_tmp_bytes = 0;
  if (nb) {
    uint32_t* v = nullptr;
    (void)rocprim::exclusive_scan(nullptr, scan_tmp_bytes, v, v, 0u, nb + 1, rocprim::plus<uint32_t>(), c0->stream);
  }
  ArenaCarver tmp_size;
  (void)loam_cloud_scratch_layout(tmp_size, nb, (size_t)B, scan_tmp_bytes);
  std::vector<const void*> base((size_t)B, nullptr);
  ArenaStage in_size = arena_stage(c0, nullptr);
  loam_cloud_input_layout(in_size, B, memory, data, bytes.data(), base.data());
  const size_t tmp_need = tmp_size.used(), in_need = in_size.used();
  if ((rc = S0->tmp.reserve(c0, tmp_need, tmp_need + tmp_need / 4)) != PCM_OK) return rc;
  if (in_need && (rc = S0->in.reserve(c0, in_need, in_need + in_need / 4)) != PCM_OK) return rc;
  if ((rc = S0->d_fr.reserve(c0, (size_t)B, (size_t)B)) != PCM_OK) return rc;
  for (int i = 0; i < B && own_out; i++) {
    CloudState* S = cloud_of(ctxs[i]);
    S->n = 0;   // the context's buffer is about to be rewritten
    const size_t vecs = (size_t)rec_vecs * descs[i].height * descs[i].width;
    if (vecs && (rc = S->out.reserve(ctxs[i], vecs, vecs + vecs / 4)) != PCM_OK) { if (ctxs[i] != c0) c0->err = ctxs[i]->err; return rc; }
  }
  ArenaCarver tmp_carver(S0->tmp.p);
  const LoamCloudScratch T = loam_cloud_scratch_layout(tmp_carver, nb, (size_t)B, scan_tmp_bytes);
  ArenaStage in_stage = arena_stage(c0, S0->in.p);   // every host cloud staged: one upload of its raw bytes
  loam_cloud_input_layout(in_stage, B, memory, data, bytes.data(), base.data());
  if (in_stage.rc != PCM_OK) return in_stage.rc;
  for (int i = 0; i < B; i++) {
    LcFrame& F = h_fr[i];
    F.V = loam::cloud_view(descs[i], base[(size_t)i]);
    F.out = own_out ? cloud_of(ctxs[i])->out.p : static_cast<uint4*>(user_out);
    F.capacity = own_out ? F.V.n : (uint32_t)std::min<size_t>(capacity, F.V.n);
  }
  hipStream_t st = c0->stream;
  std::vector<uint32_t> h_info((size_t)B, 0u);
  if (max_all) {
    PCM_HIPCK(c0, hipMemcpyAsync(S0->d_fr.p, h_fr, sizeof(LcFrame) * (size_t)B, hipMemcpyHostToDevice, st));
    if (nb) {
      PCM_HIPCK(c0, hipMemsetAsync(T.kept + nb, 0, 4, st));   // the element behind the counts: its offset is the total
      k_lc_count<<<dim3(max_scan, (unsigned)B), kLcBlock, 0, st>>>(S0->d_fr.p, T.kept);
      PCM_HIPCK(c0, hipGetLastError());
      PCM_HIPCK(c0, rocprim::exclusive_scan(T.tmp, scan_tmp_bytes, T.kept, T.off, 0u, nb + 1, rocprim::plus<uint32_t>(), st));
    }
    k_lc_write<<<dim3(max_all, (unsigned)B), kLcBlock, 0, st>>>(S0->d_fr.p, T.off, T.info);
    PCM_HIPCK(c0, hipGetLastError());
    if (nb) {
      PCM_HIPCK(c0, hipMemcpyAsync(h_info.data(), T.info, 4 * (size_t)B, hipMemcpyDeviceToHost, st));
      PCM_HIPCK(c0, hipStreamSynchronize(st));   // the one synchronisation: the kept counts
    } else if (memory == PCM_MEM_HOST) {
      PCM_HIPCK(c0, hipStreamSynchronize(st));   // dense clouds: nothing to read back, but the caller's host bytes are free on return
    }
  }
  for (int i = 0; i < B; i++) {
    const LcFrame& F = h_fr[i];
    pcm_loam_cloud_result& r = results[i];
    r.n_in = F.V.n;
    r.n_out = F.nblk ? h_info[(size_t)i] : F.V.n;
    r.n_nonfinite = r.n_in - r.n_out;
    loam::cloud_fill_flags(descs[i], &r);
  }
  if (user_out && results[0].n_out > capacity) { c0->err = "output buffer too small (the counts are in the result)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (user_out && out_memory == PCM_MEM_HOST && results[0].n_out) {
    PCM_HIPCK(c0, hipMemcpyAsync(user_out, S0->out.p, (size_t)rec_bytes * results[0].n_out, hipMemcpyDeviceToHost, st));
    PCM_HIPCK(c0, hipStreamSynchronize(st));
  }
  for (int i = 0; i < B; i++) {
    if (!user_out) {
      CloudState* S = cloud_of(ctxs[i]);
      S->n = (size_t)results[i].n_out;
      S->stride = rec_bytes;
    }
    results[i].status = PCM_OK;
  }
  return PCM_OK;
}

// the prepared clouds of the contexts through the batched front end, where they lie
int begin_frames(pcm_ctx* const* ctxs, int B, const void* const* data, const pcm_loam_cloud_desc* descs, int memory, const pcm_loam_feature_params* params,
                 pcm_loam_features_result* results, const pcm_loam_deskew* const* deskews, pcm_loam_cloud_result* cloud_results) {
  if (!ctxs || B <= 0 || !ctxs[0]) return PCM_ERR_INVALID_ARGUMENT;
  if (!results || !cloud_results) { ctxs[0]->err = "null result"; return PCM_ERR_INVALID_ARGUMENT; }
  int rc = prepare_frames(ctxs, B, data, descs, memory, nullptr, 0, PCM_MEM_DEVICE, cloud_results);
  if (rc != PCM_OK) return rc;
  const int kind = descs[0].record_kind;
  std::vector<const void*> pts((size_t)B);
  std::vector<size_t> ns((size_t)B);
  std::vector<pcm_loam_deskew> dk((size_t)B);
  std::vector<const pcm_loam_deskew*> dkp((size_t)B, nullptr);
  for (int i = 0; i < B; i++) {
    const CloudState* S = cloud_of(ctxs[i]);
    ns[(size_t)i] = S->n;
    pts[(size_t)i] = S->n ? S->out.p : nullptr;
    if (deskews && deskews[i] && cloud_results[i].time_available) {
      dk[(size_t)i] = *deskews[i];
      dk[(size_t)i].time_offset_bytes = loam::cloud_record_time_offset(kind);
      dk[(size_t)i].time_kind = loam::cloud_record_time_kind(kind);
      dkp[(size_t)i] = &dk[(size_t)i];
    }
  }
  return pcm_loam_frame_begin_batch_deskew(ctxs, B, pts.data(), ns.data(), loam::cloud_record_bytes(kind), 16, loam::cloud_record_ring_offset(kind), PCM_MEM_DEVICE, params,
                                           results, dkp.data());
}

}  // namespace

extern "C" {

int pcm_loam_cloud_default_desc(int lidar_type, int record_kind, pcm_loam_cloud_desc* desc) {
  if (!desc) return PCM_ERR_INVALID_ARGUMENT;
  loam::cloud_default_desc(lidar_type, record_kind, desc);
  return loam::cloud_check_desc(desc) ? PCM_ERR_INVALID_ARGUMENT : PCM_OK;
}

int pcm_loam_cloud_prepare(pcm_ctx* c, const void* data, const pcm_loam_cloud_desc* desc, int memory, void* out, size_t capacity_points, int out_memory,
                           pcm_loam_cloud_result* result) {
  if (!c) return PCM_ERR_INVALID_ARGUMENT;
  pcm_ctx* arr[1] = {c};
  const void* d[1] = {data};
  return prepare_frames(arr, 1, d, desc, memory, out, capacity_points, out_memory, result);
}

int pcm_loam_cloud_cached(pcm_ctx* c, const void** device_records, size_t* n, size_t* stride_bytes) {
  const int rc = check_ctx_cloud(c);
  if (rc != PCM_OK) return rc;
  if (!device_records || !n) { c->err = "null output"; return PCM_ERR_INVALID_ARGUMENT; }
  const CloudState* S = cloud_of(c);
  *device_records = S->n ? S->out.p : nullptr;
  *n = S->n;
  if (stride_bytes) *stride_bytes = S->stride;
  return PCM_OK;
}

int pcm_loam_frame_begin_cloud(pcm_ctx* c, const void* data, const pcm_loam_cloud_desc* desc, int memory, const pcm_loam_feature_params* feature_params,
                               pcm_loam_features_result* features_result, const pcm_loam_deskew* deskew, pcm_loam_cloud_result* cloud_result) {
  if (!c) return PCM_ERR_INVALID_ARGUMENT;
  pcm_ctx* arr[1] = {c};
  const void* d[1] = {data};
  const pcm_loam_deskew* dks[1] = {deskew};
  return begin_frames(arr, 1, d, desc, memory, feature_params, features_result, dks, cloud_result);
}

int pcm_loam_frame_begin_cloud_batch(pcm_ctx* const* ctxs, int n, const void* const* data, const pcm_loam_cloud_desc* descs, int memory,
                                     const pcm_loam_feature_params* feature_params, pcm_loam_features_result* results, const pcm_loam_deskew* const* deskews,
                                     pcm_loam_cloud_result* cloud_results) {
  return begin_frames(ctxs, n, data, descs, memory, feature_params, results, deskews, cloud_results);
}

}  // extern "C"
