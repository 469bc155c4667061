// loam_sc.hip -- Scan Context store and loop detection of jueying_slam on the device (include/pcm_amd.h, pcm_loam_sc_* and
// pcm_loam_loop_detect_distance): makeAndSaveScancontextAndKeys (Scancontext.cpp:151-250), detectLoopClosureID (:253-344) with
// distanceBtnScanContext (:116-148), and detectLoopClosureDistance (mapOptmization.cpp:843-880).  Arithmetic: loam_sc.h.
//
// Store: four growing device arrays, one row per descriptor: the descriptor as float (num_ring x num_sector, column-major), the
// ring key as float (what the reference's kd-tree holds), the sector key and the column norms as double.
// Descriptor of a cloud: k_sc_bins (one lane per point, ordered-int atomicMax into a workgroup's LDS table, one global atomicMax
// per touched bin, or straight into the global table when it is too large for LDS; an integer maximum does not depend on the schedule) and k_sc_finish (one workgroup: descriptor, keys, norms).
// Detection: k_sc_ringkeys (one lane per entry of the search set: nanoflann's squared distance as a (d2, index) sort key),
// k_sc_select (one workgroup, the num_candidates smallest keys in ascending order), k_sc_distance (one workgroup per candidate,
// one lane per column; the column sums of a shift are added by one lane in column order, as loam_sc.h's host composition does)
// and k_sc_fold (minimum by (distance, candidate position); NaN never wins).  The result record is read back once at the end.
// No float atomics anywhere, so two runs over the same store give the same bits.
#include "host_util.h"
#include "loam_device.h"
#include "loam_sc.h"
#include "voxel_grid.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace pcm;
using namespace pcm::loam;

namespace {

constexpr double kScLarge = 10000000;   // the reference's initial minimum
constexpr int kShiftChunk = 8;          // shifts evaluated side by side in k_sc_distance
constexpr uint32_t kScLdsWords = 8192;  // largest bin table k_sc_bins keeps in LDS (32 KB; 20 x 60 is 1 200 words)

__global__ void k_sc_table_init(uint32_t* __restrict__ table, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) table[i] = f2ord(kScNoPoint);
}

// One lane per point (grid-stride): the workgroup's maxima in a table of num_ring * num_sector words of dynamic LDS, flushed with
// one global atomic per touched bin.  use_lds = 0 (tables above kScLdsWords, no LDS asked for): every lane goes to the global
// table directly, so no launch depends on more than 32 KB of dynamic LDS.
__global__ void __launch_bounds__(256) k_sc_bins(const float4* __restrict__ pts, uint32_t n, ScShape sh, uint32_t* __restrict__ table, int use_lds) {
  extern __shared__ uint32_t sc_lds[];
  const uint32_t nb = (uint32_t)(sh.num_ring * sh.num_sector);
  const uint32_t empty = f2ord(kScNoPoint);
  if (!use_lds) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += gridDim.x * blockDim.x) {
      const float4 p = pts[g];
      int ring, sector;
      float zp;
      if (sc_point_bin(p.x, p.y, p.z, sh, &ring, &sector, &zp)) atomicMax(&table[(uint32_t)sector * (uint32_t)sh.num_ring + (uint32_t)ring], f2ord(zp));
    }
    return;
  }
  for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) sc_lds[i] = empty;
  __syncthreads();
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += gridDim.x * blockDim.x) {
    const float4 p = pts[g];
    int ring, sector;
    float zp;
    if (sc_point_bin(p.x, p.y, p.z, sh, &ring, &sector, &zp)) atomicMax(&sc_lds[(uint32_t)sector * (uint32_t)sh.num_ring + (uint32_t)ring], f2ord(zp));
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x)
    if (sc_lds[i] != empty) atomicMax(&table[i], sc_lds[i]);
}

// one workgroup: the bin table (or a ready descriptor in doubles) -> float descriptor, ring key, sector key, column norms
__global__ void __launch_bounds__(256) k_sc_finish(const uint32_t* __restrict__ table, const double* __restrict__ ready, int R, int S, float* desc, float* __restrict__ rkey,
                                                   double* __restrict__ skey, double* __restrict__ norm) {
  const int nb = R * S;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) desc[i] = table ? sc_bin_value(vg::ord2f(table[i])) : (float)ready[i];
  __threadfence_block();
  __syncthreads();
  for (int r = threadIdx.x; r < R; r += blockDim.x) rkey[r] = sc_ring_key(desc, R, S, r);
  for (int s = threadIdx.x; s < S; s += blockDim.x) {
    double nrm;
    skey[s] = sc_sector_key(desc, R, s, &nrm);
    norm[s] = nrm;
  }
}

// (d2, index) of every entry of the search set against the query's ring key; d2 >= 0, so its bits order as an unsigned integer
__global__ void __launch_bounds__(256) k_sc_ringkeys(const float* __restrict__ rkeys, int R, uint32_t q, uint32_t n, uint64_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float d2 = sc_ring_d2(rkeys + (size_t)q * R, rkeys + (size_t)i * R, R);
  keys[i] = ((uint64_t)__float_as_uint(d2) << 32) | i;
}

// one workgroup: the k smallest keys in ascending order (round t takes the smallest key above that of round t - 1; the keys are
// distinct): k passes over the keys.  Measured: 11 us for the reference's 3 candidates at 10 000 keys; at
// 64 candidates and 100 000 keys the passes make up most of a 1.0 ms call, where a sort of the keys has not been tried.
__global__ void __launch_bounds__(1024) k_sc_select(const uint64_t* __restrict__ keys, uint32_t n, uint32_t k, int32_t* __restrict__ cand, pcm_loam_sc_result* __restrict__ res) {
  __shared__ uint64_t red[16];
  __shared__ uint64_t prev_s;
  uint64_t prev = 0;
  for (uint32_t t = 0; t < k; t++) {
    uint64_t best = ~0ull;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      const uint64_t key = keys[i];
      if ((t == 0 || key > prev) && key < best) best = key;
    }
    best = vg::wave_min_u64(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t b = red[0];
      for (uint32_t w = 1; w < blockDim.x / 64; w++) b = red[w] < b ? red[w] : b;
      prev_s = b;
      cand[t] = (int32_t)(uint32_t)b;
      res->cand_index[t] = (int32_t)(uint32_t)b;
      res->cand_d2[t] = __uint_as_float((uint32_t)(b >> 32));
    }
    __syncthreads();
    prev = prev_s;
  }
}

// distanceBtnScanContext(query, candidate): one workgroup per candidate, lane j = column j.  Dynamic LDS: 12 S doubles and 8 S flags.
__global__ void __launch_bounds__(384) k_sc_distance(const float* __restrict__ descs, const double* __restrict__ skeys, const double* __restrict__ norms, int R, int S,
                                                     uint32_t q, const int32_t* __restrict__ cand, uint32_t first, int radius, double* __restrict__ out_dist,
                                                     int32_t* __restrict__ out_shift) {
  extern __shared__ double sc_ldsd[];
  double* v1 = sc_ldsd;
  double* v2 = v1 + S;
  double* n1 = v2 + S;
  double* n2 = n1 + S;
  double* sims = n2 + S;                                             // [kShiftChunk][S]
  unsigned char* ok = reinterpret_cast<unsigned char*>(sims + kShiftChunk * S);   // [kShiftChunk][S]
  __shared__ int arg_s, best_shift_s;
  __shared__ double best_s, chunk_dist[kShiftChunk];
  const uint32_t ci = cand ? (uint32_t)cand[blockIdx.x] : first + blockIdx.x;
  const int j = threadIdx.x;
  const float* d1 = descs + (size_t)q * R * S;
  const float* d2 = descs + (size_t)ci * R * S;
  if (j < S) {
    v1[j] = skeys[(size_t)q * S + j]; v2[j] = skeys[(size_t)ci * S + j];
    n1[j] = norms[(size_t)q * S + j]; n2[j] = norms[(size_t)ci * S + j];
  }
  __syncthreads();
  // fastAlignUsingVkey: lane j takes shift j, one lane takes the first strict minimum
  if (j < S) sims[j] = sc_shift_norm(v1, v2, S, j);
  __syncthreads();
  if (j == 0) {
    int arg = 0;
    double best = kScLarge;
    for (int sh = 0; sh < S; sh++) if (sims[sh] < best) { arg = sh; best = sims[sh]; }
    arg_s = arg;
    best_s = kScLarge;
    best_shift_s = 0;
  }
  __syncthreads();
  const int arg = arg_s;
  for (int base = 0; base < S; base += kShiftChunk) {
    bool any = false;
    for (int t = 0; t < kShiftChunk && base + t < S; t++) any = any || sc_in_window(base + t, arg, radius, S);
    if (!any) continue;   // the same in every lane
    if (j < S)
      for (int t = 0; t < kShiftChunk && base + t < S; t++) {
        const int sh = base + t;
        if (!sc_in_window(sh, arg, radius, S)) continue;
        const int c = sc_src_col(j, sh, S);
        double sim = 0.0;
        const bool use = sc_col_sim(d1 + (size_t)j * R, d2 + (size_t)c * R, R, n1[j], n2[c], &sim);
        sims[t * S + j] = sim;
        ok[t * S + j] = use ? 1 : 0;
      }
    __syncthreads();
    if (j < kShiftChunk && base + j < S && sc_in_window(base + j, arg, radius, S)) {
      int eff = 0;
      double sum = 0.0;
      for (int col = 0; col < S; col++)
        if (ok[j * S + col]) { sum = sum + sims[j * S + col]; eff = eff + 1; }
      chunk_dist[j] = 1.0 - sum / (double)eff;
    }
    __syncthreads();
    if (j == 0)
      for (int t = 0; t < kShiftChunk && base + t < S; t++)
        if (sc_in_window(base + t, arg, radius, S) && chunk_dist[t] < best_s) { best_s = chunk_dist[t]; best_shift_s = base + t; }
    __syncthreads();
  }
  if (j == 0) { out_dist[blockIdx.x] = best_s; out_shift[blockIdx.x] = best_shift_s; }
}

// one workgroup: the candidates folded in candidate order with strict < (= minimum by (distance, position)); a NaN or a distance
// >= 10000000 never wins.  Lanes < 64 also copy the first candidates' figures into the result record.
__global__ void __launch_bounds__(1024) k_sc_fold(const double* __restrict__ dist, const int32_t* __restrict__ shift, const int32_t* __restrict__ cand, uint32_t n,
                                                  const uint64_t* __restrict__ keys, double threshold, pcm_loam_sc_result* __restrict__ res) {
  __shared__ double rd[16];
  __shared__ int rp[16];
  double bd = kScLarge;
  int bp = 0x7fffffff;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double d = dist[i];
    if (d < bd) { bd = d; bp = (int)i; }   // ascending positions per lane: the first of equal distances stays
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const double od = __shfl_xor(bd, off, 64);
    const int op = __shfl_xor(bp, off, 64);
    if (od < bd || (od == bd && op < bp)) { bd = od; bp = op; }
  }
  if ((threadIdx.x & 63) == 0) { rd[threadIdx.x >> 6] = bd; rp[threadIdx.x >> 6] = bp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < blockDim.x / 64; w++)
      if (rd[w] < bd || (rd[w] == bd && rp[w] < bp)) { bd = rd[w]; bp = rp[w]; }
    int nn_idx = 0, nn_align = 0;
    if (bp != 0x7fffffff) { nn_idx = cand ? cand[bp] : bp; nn_align = shift[bp]; }
    res->min_dist = bd;
    res->nn_idx = nn_idx;
    res->nn_align = nn_align;
    res->loop_id = bd < threshold ? nn_idx : -1;
  }
  if (threadIdx.x < kScMaxCandidates && threadIdx.x < n) {
    const uint32_t t = threadIdx.x;
    res->cand_dist[t] = dist[t];
    res->cand_shift[t] = shift[t];
    if (!cand) { res->cand_index[t] = (int32_t)t; res->cand_d2[t] = __uint_as_float((uint32_t)(keys[t] >> 32)); }
  }
}

struct ScStore {
  int R = 0, S = 0;
  size_t count = 0, cap = 0;        // descriptors
  DevBuf<float> desc{"scan-context store"};    // [cap][R * S]
  DevBuf<float> rkey{"scan-context store"};    // [cap][R]
  DevBuf<double> skey{"scan-context store"};   // [cap][S]
  DevBuf<double> norm{"scan-context store"};   // [cap][S]
  DevBuf<uint32_t> table;           // [R * S] ordered-int maxima of the descriptor being built
  DevBuf<double> ready;             // [R * S] staging of pcm_loam_sc_put
  DevBuf<float4> pts;               // staged input cloud, then room for its VoxelGrid cells
  DevBuf<char> vg;                  // VoxelGrid scratch
  DevBuf<uint64_t> keys;            // [set] ring-key sort keys
  DevBuf<double> dist;              // [set] candidate distances
  DevBuf<int32_t> shift;            // [set]
  DevBuf<int32_t> cand;             // [kScMaxCandidates]
  DevBuf<pcm_loam_sc_result> d_res;
  PinnedBuf<pcm_loam_sc_result> h_res;
  // the reference's stale tree
  uint64_t counter = 0;
  size_t tree_size = 0;
  bool have_tree = false;
};

// create = false (queries): *out stays null when the context has no store yet, and none is made
int check_ctx_sc(pcm_ctx* c, ScStore** out, bool create = true) {
  return loam_check_store(c, "pcm_loam_sc_* / pcm_loam_loop_detect_distance need a context created with PCM_MODEL_LOAM", LoamStore::sc, out, create,
                          "the context's LOAM state could not be allocated (out of host memory)", "the Scan Context store could not be allocated (out of host memory)");
}

int check_scparams(pcm_ctx* c, const ScStore* S, const pcm_loam_sc_params& p) {
  if (p.num_ring < 1 || p.num_ring > kScMaxRing) { c->err = "num_ring must be in [1, 64]"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.num_sector < 1 || p.num_sector > kScMaxSector) { c->err = "num_sector must be in [1, 360]"; return PCM_ERR_INVALID_ARGUMENT; }
  if (S->count > 0 && (p.num_ring != S->R || p.num_sector != S->S)) {
    c->err = "num_ring / num_sector differ from those of the stored descriptors (pcm_loam_sc_clear starts a new store)"; return PCM_ERR_INVALID_ARGUMENT;
  }
  if (!(p.max_radius > 0.0) || !finite_d(p.max_radius)) { c->err = "max_radius must be a positive number"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!finite_d(p.lidar_height)) { c->err = "lidar_height must be finite"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.num_exclude_recent < 0) { c->err = "num_exclude_recent must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.num_candidates < 0 || p.num_candidates > kScMaxCandidates) { c->err = "num_candidates must be in [0, 64] (0: every entry of the search set)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.search_ratio >= 0.0) || !(p.search_ratio <= 1.0)) { c->err = "search_ratio must be in [0, 1]"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.dist_threshold == p.dist_threshold)) { c->err = "dist_threshold must be a number"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.tree_making_period < 1) { c->err = "tree_making_period must be >= 1"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.leaf >= 0.f) || !finite_f(p.leaf)) { c->err = "leaf must be >= 0 (0: no down-sampling)"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

// the shape of an empty store, its fixed-size buffers, and room for one more descriptor
int ensure_store(pcm_ctx* c, ScStore* S, int R, int Sec) {
  if (S->count == 0 && (S->R != R || S->S != Sec)) {
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));
    S->desc.release(); S->rkey.release(); S->skey.release(); S->norm.release(); S->table.release(); S->ready.release();
    S->cap = 0;
    S->R = R; S->S = Sec;
  }
  const size_t nb = (size_t)S->R * S->S, nr = (size_t)S->R, ns = (size_t)S->S;
  int rc;
  if ((rc = S->table.reserve(c, nb, nb)) != PCM_OK || (rc = S->ready.reserve(c, nb, nb)) != PCM_OK || (rc = S->cand.reserve(c, kScMaxCandidates, kScMaxCandidates)) != PCM_OK ||
      (rc = S->d_res.reserve(c, 1, 1)) != PCM_OK || (rc = S->h_res.reserve(c, 1, 1)) != PCM_OK)
    return rc;
  if (S->count + 1 > S->cap) {   // the stored rows move to the larger arrays
    const size_t cap = S->cap + S->cap / 2 + 256, n = S->count;
    if ((rc = S->desc.reserve_keep(c, cap * nb, cap * nb, n * nb)) != PCM_OK || (rc = S->rkey.reserve_keep(c, cap * nr, cap * nr, n * nr)) != PCM_OK ||
        (rc = S->skey.reserve_keep(c, cap * ns, cap * ns, n * ns)) != PCM_OK || (rc = S->norm.reserve_keep(c, cap * ns, cap * ns, n * ns)) != PCM_OK)
      return rc;
    S->cap = cap;
  }
  return PCM_OK;
}

int ensure_set(pcm_ctx* c, ScStore* S, size_t n) {
  const size_t cap = n + n / 2 + 256;
  int rc;
  if ((rc = S->keys.reserve(c, n, cap)) != PCM_OK || (rc = S->dist.reserve(c, n, cap)) != PCM_OK) return rc;
  return S->shift.reserve(c, n, cap);
}

// table (or S->ready) -> row S->count of the store; the caller bumps the count
void launch_finish(pcm_ctx* c, ScStore* S, bool from_table) {
  const size_t i = S->count, nb = (size_t)S->R * S->S;
  k_sc_finish<<<1, 256, 0, c->stream>>>(from_table ? S->table : nullptr, from_table ? nullptr : S->ready, S->R, S->S, S->desc + i * nb, S->rkey + i * S->R,
                                         S->skey + i * S->S, S->norm + i * S->S);
}

void launch_distance(pcm_ctx* c, ScStore* S, uint32_t q, const int32_t* cand, uint32_t first, uint32_t n, double search_ratio) {
  const unsigned block = (unsigned)((S->S + 63) / 64 * 64);
  const size_t lds = sizeof(double) * (4 + kShiftChunk) * S->S + (size_t)kShiftChunk * S->S;
  k_sc_distance<<<n, block, lds, c->stream>>>(S->desc, S->skey, S->norm, S->R, S->S, q, cand, first, sc_search_radius(search_ratio, S->S), S->dist, S->shift);
}

// the descriptor of `cloud` (n_cloud points on the device; may be empty) becomes row S->count of the store; waits, so the caller may
// reuse its buffers on return
int add_descriptor(pcm_ctx* c, ScStore* S, const pcm_loam_sc_params& p, const float4* cloud, uint32_t n_cloud, size_t n_in, pcm_loam_sc_add_result* result) {
  hipStream_t st = c->stream;
  const uint32_t nb = (uint32_t)(S->R * S->S);
  k_sc_table_init<<<(nb + 255) / 256, 256, 0, st>>>(S->table, nb);
  if (n_cloud > 0) {
    const ScShape sh{S->R, S->S, p.lidar_height, p.max_radius};
    const unsigned grid = std::min<unsigned>(1024u, (n_cloud + 255) / 256);
    const int use_lds = nb <= kScLdsWords ? 1 : 0;
    k_sc_bins<<<grid, 256, use_lds ? sizeof(uint32_t) * nb : 0, st>>>(cloud, n_cloud, sh, S->table, use_lds);
  }
  launch_finish(c, S, true);
  PCM_HIPCK(c, hipGetLastError());
  PCM_HIPCK(c, hipStreamSynchronize(st));
  S->count++;
  if (result) {
    result->index = (int32_t)(S->count - 1);
    result->num_points_in = (int32_t)n_in;
    result->num_points = (int32_t)n_cloud;
    result->status = PCM_OK;
  }
  return PCM_OK;
}

}  // namespace

extern "C" {

void pcm_loam_default_sc_params(pcm_loam_sc_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->lidar_height = 0.3;        // Scancontext.h:80 LIDAR_HEIGHT
  p->max_radius = 80.0;         // :84 PC_MAX_RADIUS
  p->search_ratio = 0.1;        // :93 SEARCH_RATIO
  p->dist_threshold = 0.3;      // :95 SC_DIST_THRES
  p->num_ring = 20;             // :82 PC_NUM_RING
  p->num_sector = 60;           // :83 PC_NUM_SECTOR
  p->num_exclude_recent = 30;   // :89 NUM_EXCLUDE_RECENT
  p->num_candidates = 3;        // :90 NUM_CANDIDATES_FROM_TREE
  p->tree_making_period = 10;   // :99 TREE_MAKING_PERIOD_
  p->leaf = 0.5f;               // mapOptmization.cpp:239 kSCFilterSize
}

int pcm_loam_sc_add(pcm_ctx* c, const pcm_loam_sc_params* params, int input, int key, const void* points, size_t n, size_t stride, int memory,
                    pcm_loam_sc_add_result* result) {
  ScStore* S = nullptr;
  int rc = check_ctx_sc(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_sc_params p;
  if (params) p = *params; else pcm_loam_default_sc_params(&p);
  if ((rc = check_scparams(c, S, p)) != PCM_OK) return rc;
  if (result) std::memset(result, 0, sizeof(*result));
  const float4* cloud = nullptr;
  uint32_t n_cloud = 0;
  size_t n_in = 0;
  if (input == PCM_LOAM_SC_KEYFRAME_NEAR) {
    c->err = "PCM_LOAM_SC_KEYFRAME_NEAR needs search_num and leaf, which this entry point has no room for: call pcm_loam_sc_add_near";
    return PCM_ERR_UNSUPPORTED;
  }
  if (input == PCM_LOAM_SC_KEYFRAME_SURF) {
    if (!loam_keyframe_cloud(c, key, 1, &cloud, &n_cloud)) { c->err = "pcm_loam_sc_add: key outside [0, K)"; return PCM_ERR_INVALID_ARGUMENT; }
    n_in = n_cloud;
  } else if (input == PCM_LOAM_SC_POINTS) {
    if ((rc = check_point_records(c, points, n, stride, memory, 0x3fffffffull)) != PCM_OK) return rc;
    n_in = n;
  } else {
    c->err = "input must be PCM_LOAM_SC_POINTS, PCM_LOAM_SC_KEYFRAME_SURF or PCM_LOAM_SC_KEYFRAME_NEAR";
    return PCM_ERR_INVALID_ARGUMENT;
  }
  PCM_HIPCK(c, hipSetDevice(c->device));
  if ((rc = ensure_store(c, S, p.num_ring, p.num_sector)) != PCM_OK) return rc;
  hipStream_t st = c->stream;
  if (input == PCM_LOAM_SC_POINTS && n > 0) {
    const bool vg = p.leaf > 0.f;
    const size_t need = vg ? 2 * n : n;   // the staged cloud, then its cells
    if ((rc = S->pts.reserve(c, need, need + need / 4 + 1024)) != PCM_OK) return rc;
    if ((rc = load_xyzw_rows(c, points, n, stride, memory, true, S->pts)) != PCM_OK) return rc;
    cloud = S->pts;
    n_cloud = (uint32_t)n;
    if (vg) {
      // downSizeFilterSC: the VoxelGrid of pcm_voxel_downsample (one implementation, so the cells are the same bits)
      const size_t sb = voxel_downsample_scratch_bytes(n);
      if ((rc = S->vg.reserve(c, sb, sb + sb / 4)) != PCM_OK) return rc;
      size_t m = 0;
      float4* cells = S->pts + n;
      if ((rc = voxel_downsample_device(st, S->pts, n, sizeof(float4), p.leaf, reinterpret_cast<float*>(cells), &m, S->vg.p, &c->err)) != PCM_OK) return rc;
      cloud = cells;
      n_cloud = (uint32_t)m;
    }
  }
  return add_descriptor(c, S, p, cloud, n_cloud, n_in, result);
}

int pcm_loam_sc_add_near(pcm_ctx* c, const pcm_loam_sc_params* params, int key, int search_num, int wrt_key, float leaf, pcm_loam_sc_add_result* result) {
  ScStore* S = nullptr;
  int rc = check_ctx_sc(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_sc_params p;
  if (params) p = *params; else pcm_loam_default_sc_params(&p);
  if ((rc = check_scparams(c, S, p)) != PCM_OK) return rc;
  if (result) std::memset(result, 0, sizeof(*result));
  // pcm_loam_submap_near's cloud, queued in the near workspace of the key-frame store and read where it lies
  NearCloud near{};
  if ((rc = loam_near_queue(c, 0, key, search_num, wrt_key, leaf, &near)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipSetDevice(c->device));
  uint32_t n_cloud = 0;
  if (near.pts) {
    PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the count of the cells
    loam_near_waited(c);
    if (near.h_small[2]) { c->err = "leaf size too small for the extent of the cloud (index overflow)"; return PCM_ERR_OUT_OF_RANGE; }
    n_cloud = near.h_small[0];
    if (n_cloud > near.n_in) { c->err = "pcm_loam_sc_add_near: inconsistent counts"; return PCM_ERR_INTERNAL; }
  }
  if ((rc = ensure_store(c, S, p.num_ring, p.num_sector)) != PCM_OK) return rc;
  return add_descriptor(c, S, p, near.pts, n_cloud, near.n_in, result);
}

int pcm_loam_sc_put(pcm_ctx* c, const double* desc, int num_ring, int num_sector) {
  ScStore* S = nullptr;
  int rc = check_ctx_sc(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_sc_params p;
  pcm_loam_default_sc_params(&p);
  p.num_ring = num_ring; p.num_sector = num_sector;
  if ((rc = check_scparams(c, S, p)) != PCM_OK) return rc;
  if (!desc) { c->err = "null descriptor"; return PCM_ERR_INVALID_ARGUMENT; }
  const size_t nb = (size_t)num_ring * num_sector;
  for (size_t i = 0; i < nb; i++)
    if (!finite_d(desc[i]) || (double)(float)desc[i] != desc[i]) { c->err = "pcm_loam_sc_put: every entry must be representable as a float"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  if ((rc = ensure_store(c, S, num_ring, num_sector)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipMemcpyAsync(S->ready, desc, sizeof(double) * nb, hipMemcpyHostToDevice, c->stream));
  launch_finish(c, S, false);
  PCM_HIPCK(c, hipGetLastError());
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  S->count++;
  return PCM_OK;
}

int pcm_loam_sc_get(pcm_ctx* c, int index, double* desc, float* ring_key, double* sector_key) {
  ScStore* S = nullptr;
  int rc = check_ctx_sc(c, &S);
  if (rc != PCM_OK) return rc;
  if (index < 0 || (size_t)index >= S->count) { c->err = "pcm_loam_sc_get: index outside [0, count)"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  const size_t nb = (size_t)S->R * S->S, i = (size_t)index;
  std::vector<float> h(desc ? nb : 0);
  if (desc) PCM_HIPCK(c, hipMemcpyAsync(h.data(), S->desc + i * nb, sizeof(float) * nb, hipMemcpyDeviceToHost, c->stream));
  if (ring_key) PCM_HIPCK(c, hipMemcpyAsync(ring_key, S->rkey + i * S->R, sizeof(float) * S->R, hipMemcpyDeviceToHost, c->stream));
  if (sector_key) PCM_HIPCK(c, hipMemcpyAsync(sector_key, S->skey + i * S->S, sizeof(double) * S->S, hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  if (desc) for (size_t k = 0; k < nb; k++) desc[k] = (double)h[k];
  return PCM_OK;
}

int pcm_loam_sc_count(pcm_ctx* c) {
  ScStore* S = nullptr;
  int rc = check_ctx_sc(c, &S, false);
  if (rc != PCM_OK) return rc;
  return S ? (int)S->count : 0;
}

int pcm_loam_sc_shape(pcm_ctx* c, int* num_ring, int* num_sector) {
  ScStore* S = nullptr;
  int rc = check_ctx_sc(c, &S, false);
  if (rc != PCM_OK) return rc;
  if (num_ring) *num_ring = S && S->count ? S->R : 0;
  if (num_sector) *num_sector = S && S->count ? S->S : 0;
  return PCM_OK;
}

int pcm_loam_sc_clear(pcm_ctx* c) {
  ScStore* S = nullptr;
  int rc = check_ctx_sc(c, &S, false);
  if (rc != PCM_OK) return rc;
  if (!S) return PCM_OK;
  S->count = 0;   // the arrays keep their memory
  S->counter = 0;
  S->tree_size = 0;
  S->have_tree = false;
  return PCM_OK;
}

int pcm_loam_sc_detect(pcm_ctx* c, const pcm_loam_sc_params* params, pcm_loam_sc_result* result) {
  ScStore* S = nullptr;
  int rc = check_ctx_sc(c, &S);
  if (rc != PCM_OK) return rc;
  if (!result) { c->err = "null result"; return PCM_ERR_INVALID_ARGUMENT; }
  pcm_loam_sc_params p;
  if (params) p = *params; else pcm_loam_default_sc_params(&p);
  if (S->count > 0) { p.num_ring = S->R; p.num_sector = S->S; }   // the shape is the store's; num_ring / num_sector are not read here
  if ((rc = check_scparams(c, S, p)) != PCM_OK) return rc;
  std::memset(result, 0, sizeof(*result));
  result->loop_id = -1;
  result->num_descriptors = (int32_t)S->count;
  result->tree_size = (int32_t)S->tree_size;
  if (S->count < (size_t)p.num_exclude_recent + 1) return PCM_OK;   // Scancontext.cpp:263-267: the counter does not advance
  int rebuilt = 0;
  if (S->counter % (uint64_t)p.tree_making_period == 0 || !S->have_tree) {   // :270-281
    S->tree_size = S->count - (size_t)p.num_exclude_recent;
    S->have_tree = true;
    rebuilt = 1;
  }
  S->counter++;
  const uint32_t T = (uint32_t)S->tree_size, q = (uint32_t)(S->count - 1);
  const uint32_t n_eval = p.num_candidates == 0 ? T : std::min<uint32_t>((uint32_t)p.num_candidates, T);
  PCM_HIPCK(c, hipSetDevice(c->device));
  if ((rc = ensure_set(c, S, T)) != PCM_OK) return rc;
  hipStream_t st = c->stream;
  PCM_HIPCK(c, hipMemsetAsync(S->d_res, 0, sizeof(pcm_loam_sc_result), st));
  k_sc_ringkeys<<<(T + 255) / 256, 256, 0, st>>>(S->rkey, S->R, q, T, S->keys);
  const int32_t* cand = nullptr;
  if (p.num_candidates > 0) {
    k_sc_select<<<1, 1024, 0, st>>>(S->keys, T, n_eval, S->cand, S->d_res);
    cand = S->cand;
  }
  launch_distance(c, S, q, cand, 0u, n_eval, p.search_ratio);
  k_sc_fold<<<1, 1024, 0, st>>>(S->dist, S->shift, cand, n_eval, S->keys, p.dist_threshold, S->d_res);
  PCM_HIPCK(c, hipGetLastError());
  PCM_HIPCK(c, hipMemcpyAsync(S->h_res, S->d_res, sizeof(pcm_loam_sc_result), hipMemcpyDeviceToHost, st));
  PCM_HIPCK(c, hipStreamSynchronize(st));
  *result = *S->h_res;
  result->yaw_diff_rad = sc_yaw(result->nn_align, S->S);
  result->num_descriptors = (int32_t)S->count;
  result->tree_size = (int32_t)T;
  result->tree_rebuilt = rebuilt;
  result->num_evaluated = (int32_t)n_eval;
  result->status = PCM_OK;
  return PCM_OK;
}

int pcm_loam_sc_distance(pcm_ctx* c, const pcm_loam_sc_params* params, int i, int j, double* dist, int32_t* shift) {
  ScStore* S = nullptr;
  int rc = check_ctx_sc(c, &S);
  if (rc != PCM_OK) return rc;
  pcm_loam_sc_params p;
  if (params) p = *params; else pcm_loam_default_sc_params(&p);
  if (S->count > 0) { p.num_ring = S->R; p.num_sector = S->S; }   // as pcm_loam_sc_detect
  if ((rc = check_scparams(c, S, p)) != PCM_OK) return rc;
  if (i < 0 || j < 0 || (size_t)i >= S->count || (size_t)j >= S->count) { c->err = "pcm_loam_sc_distance: index outside [0, count)"; return PCM_ERR_INVALID_ARGUMENT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  if ((rc = ensure_set(c, S, 1)) != PCM_OK) return rc;
  launch_distance(c, S, (uint32_t)i, nullptr, (uint32_t)j, 1u, p.search_ratio);
  PCM_HIPCK(c, hipGetLastError());
  double d = 0.0;
  int32_t s = 0;
  PCM_HIPCK(c, hipMemcpyAsync(&d, S->dist, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipMemcpyAsync(&s, S->shift, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  if (dist) *dist = d;
  if (shift) *shift = s;
  return PCM_OK;
}

int pcm_loam_loop_detect_distance(pcm_ctx* c, float radius, double time_diff_s, double time_cur, int32_t* key_cur, int32_t* key_pre) {
  ScStore* S = nullptr;   // not read: the key poses live in the key-frame store
  int rc = check_ctx_sc(c, &S, false);
  if (rc != PCM_OK) return rc;
  if (!(radius > 0.f) || !finite_f(radius)) { c->err = "radius must be a positive number"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(time_diff_s == time_diff_s) || !(time_cur == time_cur)) { c->err = "the times must be numbers"; return PCM_ERR_INVALID_ARGUMENT; }
  const KeyPose* kp = nullptr;
  const int K = loam_keyposes(c, &kp);
  if (key_cur) *key_cur = K - 1;
  if (key_pre) *key_pre = -1;
  const int pre = select_loop_distance(kp, K, radius, time_diff_s, time_cur);
  if (pre < 0 || pre == K - 1) return 0;
  if (key_pre) *key_pre = pre;
  return 1;
}

}  // extern "C"
