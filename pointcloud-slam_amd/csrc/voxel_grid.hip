// voxel_grid.hip -- what the two VoxelGrid pipelines of voxel_grid.h do not need a caller's element type for: the workspace, the
// clears, and the middle of a pass (radix sort, cell heads, cell starts, totals).  gfx950.
#include "voxel_grid.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace pcm {
namespace vg {

namespace {

int bit_len(uint64_t x) { int b = 0; while (x) { b++; x >>= 1; } return b; }

__global__ void k_clear(unsigned int* __restrict__ mm, uint32_t* __restrict__ small, uint32_t nbox, uint32_t nsmall) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < nbox)
    for (int a = 0; a < 3; a++) { mm[6 * s + a] = 0xffffffffu; mm[6 * s + 3 + a] = 0u; }
  if (s < nsmall) small[s] = 0u;
}

// n_part partial boxes -> mm, and k_clear's zeros; one workgroup.  Min and max are exact in any order: wave_minmax's box, bit for bit.
__global__ void __launch_bounds__(256) k_fold_boxes(const unsigned int* __restrict__ part, uint32_t n_part, unsigned int* __restrict__ mm, uint32_t* __restrict__ small) {
  unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (uint32_t i = threadIdx.x; i < n_part; i += 256u)
    for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], part[6 * i + a]); hi[a] = max(hi[a], part[6 * i + 3 + a]); }
  fold_block_box(lo, hi, mm);
  if (threadIdx.x < Work::kSmallWords) small[threadIdx.x] = 0u;
}

// 1 where a cell begins in the sorted 32-bit keys, evaluated by the scan itself
struct Head32 {
  const uint32_t* keys;
  __host__ __device__ uint32_t operator()(uint32_t i) const {
    const uint32_t k = keys[i];
    return (k != kInvalid32 && (i == 0 || keys[i - 1] != k)) ? 1u : 0u;
  }
};

// cell c starts at sorted element pos[c]; the last valid element gives the totals (invalid keys sort behind every valid one)
__global__ void k_pos32(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ slot, uint32_t N, uint32_t* __restrict__ pos, uint32_t* __restrict__ small) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const uint32_t k = keys[i];
  if (k == kInvalid32) return;
  const uint32_t head = (i == 0 || keys[i - 1] != k) ? 1u : 0u;
  if (head) pos[slot[i]] = i;
  if (i + 1 == N || keys[i + 1] == kInvalid32) { small[0] = slot[i] + head; small[1] = i + 1; }
}

__global__ void k_heads64(const uint64_t* __restrict__ keys, uint32_t n, uint32_t nseg, uint32_t* __restrict__ head, uint32_t* __restrict__ scnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = keys[i];
  const bool h = (k >> 32) < nseg && (i == 0 || keys[i - 1] != k);
  head[i] = h ? 1u : 0u;
  if (h) atomicAdd(&scnt[k >> 32], 1u);
}

// cell c starts at sorted element pos[c]; the first cell of every segment -> sfirst[segment]
__global__ void k_pos64(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head, const uint32_t* __restrict__ slot, uint32_t n, uint32_t* __restrict__ pos,
                        uint32_t* __restrict__ sfirst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !head[i]) return;
  pos[slot[i]] = i;
  const uint32_t s = (uint32_t)(keys[i] >> 32);
  if (i == 0 || (uint32_t)(keys[i - 1] >> 32) != s) sfirst[s] = slot[i];
}

// the last valid element: valid count and cell count
__global__ void k_count64(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head, const uint32_t* __restrict__ slot, uint32_t n, uint32_t nseg,
                          uint32_t* __restrict__ small) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (keys[i] >> 32) >= nseg) return;
  if (i + 1 == n || (keys[i + 1] >> 32) >= nseg) { small[0] = slot[i] + head[i]; small[1] = i + 1; }
}

}  // namespace

Work work_layout(char* base, size_t N, size_t key_bytes, size_t nseg, size_t* bytes) {
  size_t sort_tmp = 0, scan_tmp = 0;
  uint32_t* v = nullptr;
  if (nseg) {
    uint64_t* k = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, k, k, v, v, N, 0, 64, nullptr);
    (void)rocprim::exclusive_scan(nullptr, scan_tmp, v, v, 0u, N, rocprim::plus<uint32_t>(), nullptr);
  } else {
    (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, v, v, v, v, N, 0, 32, nullptr);
    auto heads = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u), Head32{v});
    (void)rocprim::exclusive_scan(nullptr, scan_tmp, heads, v, 0u, N, rocprim::plus<uint32_t>(), nullptr);
  }
  ArenaCarver a(base);
  const Work W = work_carve(a, N, key_bytes, nseg, sort_tmp, scan_tmp);
  *bytes = a.used();
  return W;
}

void clear(hipStream_t st, const Work& W) {
  const uint32_t nbox = W.nseg ? W.nseg : 1u, nsmall = Work::kSmallWords + 2 * W.nseg;
  k_clear<<<(std::max(nbox, nsmall) + 255) / 256, 256, 0, st>>>(W.mm, W.small, nbox, nsmall);
}

void fold_boxes(hipStream_t st, const unsigned int* part, uint32_t n_part, const Work& W) { k_fold_boxes<<<1, 256, 0, st>>>(part, n_part, W.mm, W.small); }

int sort_cells32(std::string* err, hipStream_t st, const Work& W, uint32_t N) {
  uint32_t* keys = static_cast<uint32_t*>(W.keys);
  uint32_t* keys_s = static_cast<uint32_t*>(W.keys_s);
  size_t tb = W.tmp_bytes, tb2 = W.tmp2_bytes;
  PCM_HIPCK_ERR(err, rocprim::radix_sort_pairs(W.tmp, tb, keys, keys_s, W.vals, W.vals_s, (size_t)N, 0, 32, st));
  auto heads = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u), Head32{keys_s});
  PCM_HIPCK_ERR(err, rocprim::exclusive_scan(W.tmp2, tb2, heads, W.slot, 0u, (size_t)N, rocprim::plus<uint32_t>(), st));
  k_pos32<<<(N + 255) / 256, 256, 0, st>>>(keys_s, W.slot, N, W.vals, W.small);   // vals is free after the sort: it takes the cell starts
  PCM_HIPCK_ERR(err, hipGetLastError());
  return PCM_OK;
}

int sort_cells64(std::string* err, hipStream_t st, const Work& W, uint32_t N) {
  uint64_t* keys = static_cast<uint64_t*>(W.keys);
  uint64_t* keys_s = static_cast<uint64_t*>(W.keys_s);
  size_t tb = W.tmp_bytes, tb2 = W.tmp2_bytes;
  PCM_HIPCK_ERR(err, rocprim::radix_sort_pairs(W.tmp, tb, keys, keys_s, W.vals, W.vals_s, (size_t)N, 0, 32 + bit_len(W.nseg), st));
  const unsigned nb = (N + 255) / 256;
  k_heads64<<<nb, 256, 0, st>>>(keys_s, N, W.nseg, W.head, W.scnt());
  PCM_HIPCK_ERR(err, hipGetLastError());
  PCM_HIPCK_ERR(err, rocprim::exclusive_scan(W.tmp2, tb2, W.head, W.slot, 0u, (size_t)N, rocprim::plus<uint32_t>(), st));
  k_pos64<<<nb, 256, 0, st>>>(keys_s, W.head, W.slot, N, W.vals, W.sfirst());
  k_count64<<<nb, 256, 0, st>>>(keys_s, W.head, W.slot, N, W.nseg, W.small);
  PCM_HIPCK_ERR(err, hipGetLastError());
  return PCM_OK;
}

}  // namespace vg
}  // namespace pcm
