// approx_voxel.hip -- pcl::ApproximateVoxelGrid on the device (the rules: approx_voxel.h), gfx950.
//   keys      one lane per point: voxel, history entry h, validity                          -> keys (kNoEntry: dropped), vals = index
//   sort      rocPRIM radix sort over the 10 key bits: a stable partition by entry
//   heads     sorted order: a run begins where the entry or the voxel differs from the predecessor (the predecessor's voxel comes
//             through a shuffle, lane 0 of a wave loads it); the marks go to input order, the entries in use are flagged
//   scans     runs in front (sorted order), marks in front (input order); 512 entries ranked by one workgroup with ballots
//   means     one wave per run, grid-stride, through the VoxelGrid's cell_mean; the slot is approx_voxel.h's run_slot
// No float atomic and no position decided by an atomic: two calls on one input give the same bytes.  One wait, by the caller's
// entry point, for {runs, valid points}; when the runs exceed the capacity the means kernel writes nothing.
#include "approx_voxel.h"

#include "pcm_device.h"
#include "pcm_host.h"
#include "voxel_grid.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace pcm {

namespace {

// records of 3..16 floats, x y z first: what vg::cell_mean reads its elements through
struct Records {
  static constexpr int kFields = 16;
  const char* base; size_t stride; int nfields;
  __device__ int fields() const { return nfields; }
  __device__ const float* fetch(uint32_t g, uint32_t) const { return reinterpret_cast<const float*>(base + (size_t)g * stride); }
  __device__ av::Key key(uint32_t g, float inv) const {
    const float* p = fetch(g, 0u);
    return av::key_of(p[0], p[1], p[2], inv);
  }
};

// also the zeros of the call: the totals and the entries in use
__global__ void __launch_bounds__(256) k_av_keys(Records R, uint32_t N, float inv, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ in_use,
                                                 uint32_t* __restrict__ small) {
  if (blockIdx.x == 0) {
    for (uint32_t h = threadIdx.x; h < av::kEntries; h += 256u) in_use[h] = 0u;
    if (threadIdx.x < av::Work::kSmallWords) small[threadIdx.x] = 0u;
  }
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const av::Key k = R.key(i, inv);
  keys[i] = k.valid ? k.h : av::kNoEntry;
  vals[i] = i;
}

__global__ void __launch_bounds__(256) k_av_heads(Records R, uint32_t N, float inv, const uint32_t* __restrict__ keys_s, const uint32_t* __restrict__ vals_s,
                                                  uint32_t* __restrict__ head, uint32_t* __restrict__ mark, uint32_t* __restrict__ in_use) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t h = j < N ? keys_s[j] : av::kNoEntry;
  const uint32_t g = j < N ? vals_s[j] : 0u;
  const bool valid = h != av::kNoEntry;
  av::Key me{0, 0, 0, av::kNoEntry, false};
  if (valid) me = R.key(g, inv);
  // the predecessor in sorted order: the lane below, or a load for the first lane of the wave
  uint32_t hp = (uint32_t)__shfl_up((int)h, 1, 64);
  int32_t px = __shfl_up(me.ix, 1, 64), py = __shfl_up(me.iy, 1, 64), pz = __shfl_up(me.iz, 1, 64);
  if (lane == 0u && valid && j > 0u) {
    hp = keys_s[j - 1];                 // valid: the dropped points sort behind every entry
    const av::Key p = R.key(vals_s[j - 1], inv);
    px = p.ix; py = p.iy; pz = p.iz;
  }
  if (j >= N) return;
  const bool first = valid && (j == 0u || hp != h);                                                  // of its entry
  const bool hd = valid && (first || px != me.ix || py != me.iy || pz != me.iz);
  head[j] = hd ? 1u : 0u;
  mark[g] = (hd && !first) ? 1u : 0u;   // every input index is some vals_s[j]: the array is written whole
  if (first) in_use[h] = 1u;
}

// the first sorted element of every run; the last valid element gives the totals
__global__ void __launch_bounds__(256) k_av_pos(const uint32_t* __restrict__ keys_s, const uint32_t* __restrict__ head, const uint32_t* __restrict__ run, uint32_t N,
                                                uint32_t* __restrict__ pos, uint32_t* __restrict__ small) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= N || keys_s[j] == av::kNoEntry) return;
  if (head[j]) pos[run[j]] = j;
  if (j + 1 == N || keys_s[j + 1] == av::kNoEntry) { small[0] = run[j] + head[j]; small[1] = j + 1; }
}

// entries in use in front of every entry, by ballots; the marks of the call.  One workgroup of 512 lanes.
__global__ void __launch_bounds__(512) k_av_entries(const uint32_t* __restrict__ in_use, const uint32_t* __restrict__ mark, const uint32_t* __restrict__ before, uint32_t N,
                                                    uint32_t* __restrict__ rank, uint32_t* __restrict__ small) {
  __shared__ uint32_t wave_total[8];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(in_use[threadIdx.x] != 0u);
  if (lane == 0u) wave_total[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t base = 0u, all = 0u;
  for (uint32_t v = 0; v < 8u; v++) { base += v < w ? wave_total[v] : 0u; all += wave_total[v]; }
  rank[threadIdx.x] = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (threadIdx.x == 0u) { small[2] = before[N - 1] + mark[N - 1]; small[3] = all; }
}

// one wave per run (grid-stride); nothing is written when the runs exceed the capacity
__global__ void __launch_bounds__(256) k_av_means(Records R, float* __restrict__ out, uint32_t capacity, const uint32_t* __restrict__ keys_s, const uint32_t* __restrict__ vals_s,
                                                  const uint32_t* __restrict__ pos, const uint32_t* __restrict__ before, const uint32_t* __restrict__ rank,
                                                  const uint32_t* __restrict__ small) {
  const uint32_t nruns = small[0], nvalid = small[1], nmarks = small[2];
  if (nruns > capacity) return;
  const uint32_t lane = threadIdx.x & 63u;
  const int nfields = R.nfields;
  for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < nruns; r += gridDim.x * 4u) {
    const uint32_t b = pos[r], e = r + 1 < nruns ? pos[r + 1] : nvalid;
    const uint32_t h = keys_s[b];
    const bool next_in_entry = r + 1 < nruns && keys_s[e] == h;
    const uint32_t slot = av::run_slot(next_in_entry, next_in_entry ? before[vals_s[e]] : 0u, nmarks, rank[h]);
    float mean[Records::kFields];
    vg::cell_mean(R, 0u, vals_s, b, e, lane, mean);
    if (lane == 0u && slot < nruns) {   // slots are a permutation of [0, runs): the test only keeps a broken table inside the buffer
      float* o = out + (size_t)slot * nfields;
#pragma unroll
      for (int f = 0; f < Records::kFields; f++)
        if (f < nfields) o[f] = mean[f];
    }
  }
}

av::Work work_layout(char* base, size_t n, size_t* bytes) {
  size_t sort_tmp = 0, scan_tmp = 0;
  uint32_t* v = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, v, v, v, v, n, 0, av::kKeyBits, nullptr);
  (void)rocprim::exclusive_scan(nullptr, scan_tmp, v, v, 0u, n, rocprim::plus<uint32_t>(), nullptr);
  ArenaCarver a(base);
  const av::Work W = av::work_carve(a, n, sort_tmp, scan_tmp);
  *bytes = a.used();
  return W;
}

}  // namespace

// scratch bytes approx_voxel_downsample_device needs for n points
size_t approx_voxel_scratch_bytes(size_t n) {
  size_t bytes = 0;
  (void)work_layout(nullptr, n, &bytes);
  return bytes;
}

// d_in: n >= 1 records of `stride` bytes (stride / 4 floats, x y z first); d_out: room for `capacity` records.  Queues the whole
// filter and the copy of {runs, valid points} to totals[0..2) (host memory, read after the caller's wait); when the runs exceed
// the capacity nothing is written to d_out.  `scratch`: approx_voxel_scratch_bytes(n) bytes of device memory owned by the caller.
int approx_voxel_downsample_device(hipStream_t stream, const void* d_in, size_t n, size_t stride, float leaf, float* d_out, size_t capacity, uint32_t* totals, void* scratch,
                                   std::string* err) {
  const uint32_t N = (uint32_t)n;
  size_t bytes = 0;
  const av::Work W = work_layout(static_cast<char*>(scratch), n, &bytes);
  const Records R{static_cast<const char*>(d_in), stride, (int)(stride / 4)};
  const float inv = 1.0f / leaf;
  const unsigned nb = (N + 255u) / 256u;
  k_av_keys<<<nb, 256, 0, stream>>>(R, N, inv, W.keys, W.vals, W.in_use, W.small);
  PCM_HIPCK_ERR(err, hipGetLastError());
  size_t tb = W.sort_tmp_bytes;
  PCM_HIPCK_ERR(err, rocprim::radix_sort_pairs(W.sort_tmp, tb, W.keys, W.keys_s, W.vals, W.vals_s, n, 0, av::kKeyBits, stream));
  k_av_heads<<<nb, 256, 0, stream>>>(R, N, inv, W.keys_s, W.vals_s, W.head, W.mark, W.in_use);
  PCM_HIPCK_ERR(err, hipGetLastError());
  tb = W.scan_tmp_bytes;
  PCM_HIPCK_ERR(err, rocprim::exclusive_scan(W.scan_tmp, tb, W.head, W.run, 0u, n, rocprim::plus<uint32_t>(), stream));
  tb = W.scan_tmp_bytes;
  PCM_HIPCK_ERR(err, rocprim::exclusive_scan(W.scan_tmp, tb, W.mark, W.before, 0u, n, rocprim::plus<uint32_t>(), stream));
  k_av_pos<<<nb, 256, 0, stream>>>(W.keys_s, W.head, W.run, N, W.pos, W.small);
  k_av_entries<<<1, 512, 0, stream>>>(W.in_use, W.mark, W.before, N, W.rank, W.small);
  PCM_HIPCK_ERR(err, hipGetLastError());
  const uint32_t cap = (uint32_t)std::min<size_t>(capacity, 0xffffffffull);
  k_av_means<<<std::min<unsigned>(1024u, (N + 3u) / 4u), 256, 0, stream>>>(R, d_out, cap, W.keys_s, W.vals_s, W.pos, W.before, W.rank, W.small);
  PCM_HIPCK_ERR(err, hipGetLastError());
  PCM_HIPCK_ERR(err, hipMemcpyAsync(totals, W.small, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  return PCM_OK;
}

}  // namespace pcm
