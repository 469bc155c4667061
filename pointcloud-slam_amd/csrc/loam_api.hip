// loam_api.hip -- C ABI of the LOAM scan-to-map optimisation (include/pcm_amd.h, pcm_loam_*): maps, features, the queued
// iteration loop and the parity hooks.  Kernels: loam.hip; arithmetic: loam_step.h.
//
// Host side of jueying_slam's scan2MapOptimization (mapOptmization.cpp:1560-1586): the reference builds two FLANN kd-trees
// (:1569-1570) and runs every iteration on the host; here the two maps become brick-hashed grids (build_target_map) built
// once per map (the tag rule keeps them across frames) and all iterations are queued without a host round trip.
#include "host_util.h"
#include "loam_device.h"

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

using namespace pcm;
using namespace pcm::loam;

namespace {

struct LoamCtx {
  DevBuf<float4> map_pts[2];   // corner / surf map, caller order
  size_t map_n[2] = {0, 0};
  TargetMap map[2];
  float built_cell = 0.f;      // cell of the grids in map[] (0: not built)
  uint64_t tgt_tag = 0, src_tag = 0;
  bool have_tgt = false, have_src = false;
  DevBuf<float4> feats;        // corner features, then surf features (body frame)
  DevBuf<float> src_int;       // pcm_loam_set_source with records of >= 16 bytes: their fourth float (a key frame keeps it)
  bool src_has_int = false;    // src_int is current
  bool src_from_fe = false;    // the source came from the front end (its intensity lives in loam_features.hip's output)
  uint64_t src_fe_gen = 0;     // generation of that output when the source was committed
  TargetOwner tgt_owner = TargetOwner::caller;   // who wrote the target clouds (loam_target_commit)
  SubState store[4];           // by LoamStore
  uint32_t n_c = 0, n_s = 0;
  DevBuf<double> partials;
  DevBuf<LoamState> st;
  PinnedBuf<LoamState> h_st;   // read-back
  DevBuf<LoamDesc> d_desc;     // descriptors of the batches this context leads
  PinnedBuf<LoamDesc> h_desc;  // staging of the same
};

LoamCtx* loam_of(pcm_ctx* c) { return c->loam.get_or_create<LoamCtx>(); }

int check_ctx(pcm_ctx* c) {
  const int rc = loam_check_ctx(c, PCM_ERR_UNSUPPORTED, "pcm_loam_* needs a context created with PCM_MODEL_LOAM");
  if (rc != PCM_OK) return rc;
  if (!loam_of(c)) { c->err = "out of host memory"; return PCM_ERR_INTERNAL; }
  return PCM_OK;
}

int check_params(pcm_ctx* c, const pcm_loam_params& p) {
  if (!(p.search_cell >= 1.0f) || !(p.search_cell <= 64.0f)) { c->err = "search_cell must be in [1, 64] m (the walk covers distance 1 in at most 4 cells per axis)"; return PCM_ERR_INVALID_ARGUMENT; }
  if (p.iter_num < 0 || p.iter_num > 1000) { c->err = "iter_num must be in [0, 1000]"; return PCM_ERR_INVALID_ARGUMENT; }
  if (!(p.rot_conv_deg >= 0.0) || !(p.trans_conv_cm >= 0.0) || !(p.degeneracy_threshold >= 0.0)) { c->err = "thresholds must be >= 0"; return PCM_ERR_INVALID_ARGUMENT; }
  return PCM_OK;
}

int check_cloud(pcm_ctx* c, const void* pts, size_t n, size_t stride) { return check_point_records(c, pts, n, stride, PCM_MEM_HOST, 0x3fffffffull, false); }

// records of >= 16 bytes -> features (x, y, z, w = index: k_load_points' layout) and their fourth float, one float per record.
// base may be `out` itself (rows staged in place): every lane reads its own row before it writes it.
__global__ void k_load_feats(const char* base, size_t stride, uint32_t n, float4* out, float* __restrict__ inten) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = reinterpret_cast<const float*>(base + (size_t)i * stride);
  const float x = p[0], y = p[1], z = p[2], w = p[3];
  inten[i] = w;
  out[i] = make_float4(x, y, z, __uint_as_float(i));
}

// load_points_to_device for records that carry a fourth float: the same single transfer (16 instead of 12 bytes per row) and one
// kernel, which also keeps the fourth float
int load_feats_xyzw(pcm_ctx* c, const void* pts, size_t n, size_t stride, int memory, float4* out, float* inten) {
  if (n == 0) return PCM_OK;
  const char* base = static_cast<const char*>(pts);
  size_t st = stride;
  if (memory != PCM_MEM_DEVICE) {
    PCM_HIPCK(c, hipMemcpy2DAsync(out, sizeof(float4), pts, stride, sizeof(float4), n, hipMemcpyHostToDevice, c->stream));
    base = reinterpret_cast<const char*>(out);
    st = sizeof(float4);
  }
  k_load_feats<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(base, st, (uint32_t)n, out, inten);
  PCM_HIPCK(c, hipGetLastError());
  return PCM_OK;
}

int load_cloud(pcm_ctx* c, LoamCtx* L, int m, const void* pts, size_t n, size_t stride, int memory) {
  int rc = L->map_pts[m].reserve(c, n, n);
  if (rc != PCM_OK) return rc;
  L->map_n[m] = n;
  return load_points_to_device(c->stream, pts, n, stride, memory, 0u, L->map_pts[m], &c->err);
}

// the search grids of both maps at `cell`; the map points' w then carries the caller index
int ensure_maps(pcm_ctx* c, LoamCtx* L, float cell, int* built) {
  *built = 0;
  // built_cell is reset by every real pcm_loam_set_target: it alone says whether both grids (an empty map has none) are current
  if (L->built_cell == cell) return PCM_OK;
  L->built_cell = 0.f;
  for (int m = 0; m < 2; m++) {
    uint32_t n = (uint32_t)L->map_n[m];
    if (n == 0) { L->map[m].release(); continue; }
    MapBuildOptions opt; opt.keep_order = true;
    int rc = build_target_map(c->stream, L->map_pts[m], &n, cell, COORD_FLOOR_MUL, &L->map[m], &c->err, opt);
    if (rc != PCM_OK) return rc;
    launch_tag_input_index(c->stream, L->map[m].pts, L->map[m].order, n);
    PCM_HIPCK(c, hipGetLastError());
  }
  // the grids are read by launches on other streams too (a batch runs on the stream of its first context): they are
  // complete, index tags included, before this returns
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  L->built_cell = cell;
  *built = 1;
  return PCM_OK;
}

// an empty map has no grid; a built one has no Gauss voxels (ensure_maps never asks for them, so m.gvox is null)
TargetView view_of_loam_map(const TargetMap& m) { return m.valid ? view_of(m) : TargetView{}; }

int ensure_state(pcm_ctx* c, LoamCtx* L) {
  const size_t need = (size_t)num_blocks(L->n_c + L->n_s) * kSums;
  int rc;
  if ((rc = L->partials.reserve(c, need, need)) != PCM_OK || (rc = L->st.reserve(c, 1, 1)) != PCM_OK) return rc;
  return L->h_st.reserve(c, 1, 1);
}

int ensure_descs(pcm_ctx* c, LoamCtx* L, int n) {
  int rc = L->d_desc.reserve(c, (size_t)n, (size_t)n);
  if (rc != PCM_OK) return rc;
  return L->h_desc.reserve(c, (size_t)n, (size_t)n);
}

LoamDesc make_desc(const LoamCtx* L, const float* x6) {
  LoamDesc d;
  std::memset(&d, 0, sizeof(d));
  d.map[0] = view_of_loam_map(L->map[0]);
  d.map[1] = view_of_loam_map(L->map[1]);
  d.feats = L->feats;
  d.n_c = L->n_c; d.n_s = L->n_s;
  d.st = L->st;
  d.partials = L->partials;
  for (int k = 0; k < 6; k++) d.x0[k] = x6[k];
  return d;
}

StepParams step_params(const pcm_loam_params& p) {
  StepParams s;
  s.iter_num = p.iter_num; s.pad = 0;
  s.rot_conv_deg = p.rot_conv_deg; s.trans_conv_cm = p.trans_conv_cm; s.degeneracy = p.degeneracy_threshold;
  return s;
}

void unchanged_result(const float* x6, int status, pcm_loam_result* r) {
  std::memset(r, 0, sizeof(*r));
  for (int k = 0; k < 6; k++) r->x[k] = x6[k];
  r->corner_fitness = DBL_MAX;
  r->surf_fitness = DBL_MAX;
  r->status = status;
}

// context i of a batch: ready to run (PCM_OK), too few features (result written), or an error
int prepare_one(pcm_ctx* c, const pcm_loam_params& p, const float* x6, pcm_loam_result* r, bool* run) {
  *run = false;
  int rc = check_ctx(c);
  if (rc != PCM_OK) return rc;
  LoamCtx* L = loam_of(c);
  if (!L->have_tgt || !L->have_src) { c->err = "pcm_loam_align before pcm_loam_set_target / pcm_loam_set_source"; return PCM_ERR_NO_INPUT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  // scan2MapOptimization :1563: laserCloudCornerLastDSNum > edgeFeatureMinValidNum && laserCloudSurfLastDSNum > surfFeatureMinValidNum
  if (!((int64_t)L->n_c > (int64_t)p.edge_min_valid && (int64_t)L->n_s > (int64_t)p.surf_min_valid)) {
    unchanged_result(x6, PCM_ERR_TOO_FEW_FEATURES, r);
    c->err = "not enough features";
    return PCM_OK;
  }
  int built = 0;
  rc = ensure_maps(c, L, p.search_cell, &built);
  if (rc != PCM_OK) return rc;
  rc = ensure_state(c, L);
  if (rc != PCM_OK) return rc;
  r->maps_built = built;
  *run = true;
  return PCM_OK;
}

int align_batch(pcm_ctx* const* ctxs, int n, const pcm_loam_params* params, const float* x6_in, pcm_loam_result* results) {
  if (!ctxs || n <= 0 || !x6_in || !results) return PCM_ERR_INVALID_ARGUMENT;
  pcm_loam_params p;
  if (params) p = *params; else pcm_loam_default_params(&p);
  pcm_ctx* c0 = ctxs[0];
  int rc = check_ctx(c0);
  if (rc != PCM_OK) return rc;
  rc = check_params(c0, p);
  if (rc != PCM_OK) return rc;
  for (int i = 0; i < n; i++) {
    rc = check_ctx(ctxs[i]);
    if (rc != PCM_OK) return rc;
    if (ctxs[i]->device != c0->device) { c0->err = "all contexts of a batch must live on one device"; return PCM_ERR_INVALID_ARGUMENT; }
    for (int j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) { c0->err = "a context appears twice in the batch"; return PCM_ERR_INVALID_ARGUMENT; }
  }
  std::vector<int> live;
  live.reserve((size_t)n);
  for (int i = 0; i < n; i++) {
    std::memset(&results[i], 0, sizeof(pcm_loam_result));
    bool run = false;
    rc = prepare_one(ctxs[i], p, x6_in + 6 * i, &results[i], &run);
    if (rc != PCM_OK) {
      if (ctxs[i] != c0) c0->err = ctxs[i]->err;
      return rc;
    }
    if (run) live.push_back(i);
  }
  int worst = PCM_OK;
  for (int i = 0; i < n; i++) if (results[i].status != PCM_OK && worst == PCM_OK) worst = results[i].status;
  if (live.empty()) return worst;
  LoamCtx* L0 = loam_of(c0);
  const int m = (int)live.size();
  rc = ensure_descs(c0, L0, m);
  if (rc != PCM_OK) return rc;
  hipStream_t st = c0->stream;
  PCM_HIPCK(c0, hipSetDevice(c0->device));
  PCM_HIPCK(c0, hipStreamSynchronize(st));   // the pinned staging of an earlier batch is free again
  uint32_t max_blocks = 1;
  for (int k = 0; k < m; k++) {
    const int i = live[(size_t)k];
    const LoamCtx* L = loam_of(ctxs[i]);
    L0->h_desc[k] = make_desc(L, x6_in + 6 * i);
    max_blocks = std::max(max_blocks, num_blocks(L->n_c + L->n_s));
  }
  PCM_HIPCK(c0, hipMemcpyAsync(L0->d_desc, L0->h_desc, sizeof(LoamDesc) * (size_t)m, hipMemcpyHostToDevice, st));
  launch_init(st, L0->d_desc, m);
  PCM_HIPCK(c0, hipGetLastError());
  const StepParams sp = step_params(p);
  for (int it = 0; it < p.iter_num; it++) launch_round(st, L0->d_desc, m, max_blocks, sp);
  PCM_HIPCK(c0, hipGetLastError());
  for (int k = 0; k < m; k++) {
    const LoamCtx* L = loam_of(ctxs[live[(size_t)k]]);
    PCM_HIPCK(c0, hipMemcpyAsync(L->h_st, L->st, sizeof(LoamState), hipMemcpyDeviceToHost, st));
  }
  PCM_HIPCK(c0, hipStreamSynchronize(st));
  for (int k = 0; k < m; k++) {
    const int i = live[(size_t)k];
    const LoamState& s = *loam_of(ctxs[i])->h_st;
    pcm_loam_result& r = results[i];
    for (int j = 0; j < 6; j++) r.x[j] = s.x[j];
    r.iterations = s.iter;
    r.converged = s.converged;
    r.degenerate = s.degenerate;
    r.status = PCM_OK;
    for (int j = 0; j < 6; j++) r.eigenvalues[j] = s.eig[j];
    r.num_corner = s.n_corner;
    r.num_surf = s.n_surf;
    r.corner_fitness = s.fit[0];
    r.surf_fitness = s.fit[1];
  }
  return worst;
}

// one correspondence pass at x6 with the parity outputs switched on (temporary device buffers)
int probe(pcm_ctx* c, const float* x6, float* corner_out, float* surf_out, double* AtA, double* AtB, int32_t* counts, int32_t* corner_nn, int32_t* surf_nn) {
  int rc = check_ctx(c);
  if (rc != PCM_OK) return rc;
  if (!x6) return PCM_ERR_INVALID_ARGUMENT;
  LoamCtx* L = loam_of(c);
  if (!L->have_tgt || !L->have_src) { c->err = "parity hook before pcm_loam_set_target / pcm_loam_set_source"; return PCM_ERR_NO_INPUT; }
  if (L->n_c + L->n_s == 0) { c->err = "no features"; return PCM_ERR_NO_INPUT; }
  PCM_HIPCK(c, hipSetDevice(c->device));
  pcm_loam_params p;
  pcm_loam_default_params(&p);
  int built = 0;
  rc = ensure_maps(c, L, L->built_cell > 0.f ? L->built_cell : p.search_cell, &built);
  if (rc != PCM_OK) return rc;
  rc = ensure_state(c, L);
  if (rc != PCM_OK) return rc;
  rc = ensure_descs(c, L, 1);
  if (rc != PCM_OK) return rc;
  const size_t nf = (size_t)L->n_c + L->n_s;
  DevBuf<char> buf;
  const size_t b_coeff = sizeof(float4) * nf, b_nn = sizeof(int32_t) * 5 * nf, b_sums = sizeof(double) * kSums;
  if ((rc = buf.reserve(c, b_coeff + b_nn + b_sums, b_coeff + b_nn + b_sums)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  LoamDesc d = make_desc(L, x6);
  d.coeff_out = reinterpret_cast<float4*>(buf.p);
  d.nn_out = reinterpret_cast<int32_t*>(buf.p + b_coeff);
  d.sums_out = reinterpret_cast<double*>(buf.p + b_coeff + b_nn);
  L->h_desc[0] = d;
  std::vector<float4> co(nf);
  std::vector<int32_t> nn(5 * nf);
  double sums[kSums];
  hipError_t e = hipMemcpyAsync(L->d_desc, L->h_desc, sizeof(LoamDesc), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    launch_init(c->stream, L->d_desc, 1);
    StepParams sp = step_params(p);
    sp.iter_num = 1;
    launch_round(c->stream, L->d_desc, 1, num_blocks((uint32_t)nf), sp);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(co.data(), d.coeff_out, b_coeff, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(nn.data(), d.nn_out, b_nn, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(sums, d.sums_out, b_sums, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(c->stream);
  buf.release();
  if (e != hipSuccess) { c->err = std::string("LOAM parity pass: ") + hipGetErrorString(e); return PCM_ERR_HIP; }
  if (corner_out) std::memcpy(corner_out, co.data(), sizeof(float4) * L->n_c);
  if (surf_out) std::memcpy(surf_out, co.data() + L->n_c, sizeof(float4) * L->n_s);
  if (corner_nn) std::memcpy(corner_nn, nn.data(), sizeof(int32_t) * 5 * L->n_c);
  if (surf_nn) std::memcpy(surf_nn, nn.data() + 5 * (size_t)L->n_c, sizeof(int32_t) * 5 * L->n_s);
  if (AtA) {
    int t = kSumAtA;
    for (int i = 0; i < 6; i++)
      for (int j = i; j < 6; j++) { AtA[i * 6 + j] = sums[t]; AtA[j * 6 + i] = sums[t]; t++; }
  }
  if (AtB) for (int i = 0; i < 6; i++) AtB[i] = sums[kSumAtB + i];
  if (counts) {
    counts[0] = (int32_t)sums[kSumCorner];
    counts[1] = (int32_t)sums[kSumSurf];
    counts[2] = (int32_t)sums[kSumFitCN];
    counts[3] = (int32_t)sums[kSumFitSN];
  }
  return PCM_OK;
}

}  // namespace

namespace pcm {
namespace loam {
int loam_source_reserve(pcm_ctx* c, size_t n, float4** feats) {
  int rc = check_ctx(c);
  if (rc != PCM_OK) return rc;
  LoamCtx* L = loam_of(c);
  L->have_src = false;
  if ((rc = L->feats.reserve(c, n, n)) != PCM_OK) return rc;
  *feats = L->feats;
  return PCM_OK;
}

void loam_source_commit(pcm_ctx* c, uint32_t n_c, uint32_t n_s) {
  LoamCtx* L = loam_of(c);
  L->n_c = n_c;
  L->n_s = n_s;
  L->src_tag = 0;
  L->src_from_fe = true;
  L->src_fe_gen = 0;
  const float4* out = nullptr;
  uint32_t fc = 0, fs = 0;
  (void)loam_features_last_out(c, &out, &fc, &fs, &L->src_fe_gen);
  L->src_has_int = false;
  L->have_src = true;
}

int loam_target_reserve(pcm_ctx* c, size_t n_corner, size_t n_surf, float4** corner, float4** surf) {
  int rc = check_ctx(c);
  if (rc != PCM_OK) return rc;
  LoamCtx* L = loam_of(c);
  L->have_tgt = false;
  L->tgt_owner = TargetOwner::caller;
  L->built_cell = 0.f;
  L->map[0].valid = L->map[1].valid = false;
  L->map_n[0] = L->map_n[1] = 0;
  if ((rc = L->map_pts[0].reserve(c, n_corner, n_corner)) != PCM_OK) return rc;
  if ((rc = L->map_pts[1].reserve(c, n_surf, n_surf)) != PCM_OK) return rc;
  *corner = L->map_pts[0];
  *surf = L->map_pts[1];
  return PCM_OK;
}

void loam_target_commit(pcm_ctx* c, uint32_t n_corner, uint32_t n_surf, TargetOwner owner) {
  LoamCtx* L = loam_of(c);
  L->map_n[0] = n_corner;
  L->map_n[1] = n_surf;
  L->tgt_tag = 0;
  L->have_tgt = true;
  L->tgt_owner = owner;
}

bool loam_target_view(pcm_ctx* c, TargetOwner owner, const float4** corner, uint32_t* n_corner, const float4** surf, uint32_t* n_surf) {
  LoamCtx* L = loam_of(c);
  if (!L || !L->have_tgt || L->tgt_owner != owner) return false;
  *corner = L->map_pts[0]; *n_corner = (uint32_t)L->map_n[0];
  *surf = L->map_pts[1]; *n_surf = (uint32_t)L->map_n[1];
  return true;
}

int loam_source_view(pcm_ctx* c, const float4** feats, uint32_t* n_c, uint32_t* n_s, const float4** xyzi, const float** inten) {
  LoamCtx* L = loam_of(c);
  if (!L || !L->have_src) return 1;
  *feats = L->feats; *n_c = L->n_c; *n_s = L->n_s; *xyzi = nullptr; *inten = nullptr;
  if (L->src_from_fe) {
    // the front end's output must still be the frame that became the source: pcm_loam_extract_features, a failed frame or
    // a batch led by another context rewrites it without touching the source
    uint32_t fc = 0, fs = 0;
    uint64_t gen = 0;
    if (!loam_features_last_out(c, xyzi, &fc, &fs, &gen) || gen != L->src_fe_gen || fc != L->n_c || fs != L->n_s) return 2;
  } else if (L->src_has_int) {
    *inten = L->src_int;
  }
  return 0;
}

SubState* loam_store_holder(pcm_ctx* c, LoamStore which) {
  LoamCtx* L = loam_of(c);
  return L ? &L->store[(int)which] : nullptr;
}
}  // namespace loam
}  // namespace pcm

extern "C" {

void pcm_loam_default_params(pcm_loam_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->iter_num = 30;               // utility.h:253
  p->edge_min_valid = 10;         // utility.h:267
  p->surf_min_valid = 100;        // utility.h:268
  p->rot_conv_deg = 0.01;         // mapOptmization.cpp:1551
  p->trans_conv_cm = 0.05;
  p->degeneracy_threshold = 100.0;   // :1524
  p->search_cell = 1.0f;
}

int pcm_loam_set_target(pcm_ctx* c, const void* corner, size_t n_c, const void* surf, size_t n_s, size_t stride, int memory, uint64_t tag) {
  int rc = check_ctx(c);
  if (rc != PCM_OK) return rc;
  LoamCtx* L = loam_of(c);
  if (tag != 0 && tag == L->tgt_tag && L->have_tgt && L->map_n[0] == n_c && L->map_n[1] == n_s) return PCM_OK;
  if ((rc = check_cloud(c, corner, n_c, stride)) != PCM_OK || (rc = check_cloud(c, surf, n_s, stride)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipSetDevice(c->device));
  L->have_tgt = false;
  L->tgt_owner = TargetOwner::caller;
  L->built_cell = 0.f;
  L->map[0].valid = L->map[1].valid = false;
  if ((rc = load_cloud(c, L, 0, corner, n_c, stride, memory)) != PCM_OK) return rc;
  if ((rc = load_cloud(c, L, 1, surf, n_s, stride, memory)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));   // the caller may reuse its buffers on return
  L->tgt_tag = tag;
  L->have_tgt = true;
  return PCM_OK;
}

int pcm_loam_set_source(pcm_ctx* c, const void* corner, size_t n_c, const void* surf, size_t n_s, size_t stride, int memory, uint64_t tag) {
  int rc = check_ctx(c);
  if (rc != PCM_OK) return rc;
  LoamCtx* L = loam_of(c);
  if (tag != 0 && tag == L->src_tag && L->have_src && L->n_c == n_c && L->n_s == n_s) return PCM_OK;
  if ((rc = check_cloud(c, corner, n_c, stride)) != PCM_OK || (rc = check_cloud(c, surf, n_s, stride)) != PCM_OK) return rc;
  PCM_HIPCK(c, hipSetDevice(c->device));
  L->have_src = false;
  if ((rc = L->feats.reserve(c, n_c + n_s, n_c + n_s)) != PCM_OK) return rc;
  L->src_from_fe = false;
  L->src_has_int = false;
  if (stride >= 4 * sizeof(float)) {   // the records carry a fourth float (PointXYZI's intensity): a key frame keeps it
    if ((rc = L->src_int.reserve(c, n_c + n_s, n_c + n_s)) != PCM_OK) return rc;
    if ((rc = load_feats_xyzw(c, corner, n_c, stride, memory, L->feats, L->src_int)) != PCM_OK) return rc;
    if ((rc = load_feats_xyzw(c, surf, n_s, stride, memory, L->feats + n_c, L->src_int + n_c)) != PCM_OK) return rc;
    L->src_has_int = true;
  } else {
    if ((rc = load_points_to_device(c->stream, corner, n_c, stride, memory, 0u, L->feats, &c->err)) != PCM_OK) return rc;
    if ((rc = load_points_to_device(c->stream, surf, n_s, stride, memory, 0u, L->feats + n_c, &c->err)) != PCM_OK) return rc;
  }
  PCM_HIPCK(c, hipStreamSynchronize(c->stream));
  L->n_c = (uint32_t)n_c;
  L->n_s = (uint32_t)n_s;
  L->src_tag = tag;
  L->have_src = true;
  return PCM_OK;
}

int pcm_loam_align(pcm_ctx* c, const pcm_loam_params* params, const float x6_in[6], pcm_loam_result* result) {
  pcm_ctx* arr[1] = {c};
  return align_batch(arr, 1, params, x6_in, result);
}

int pcm_loam_align_batch(pcm_ctx* const* ctxs, int n, const pcm_loam_params* params, const float* x6_in, pcm_loam_result* results) {
  return align_batch(ctxs, n, params, x6_in, results);
}

int pcm_loam_coefficients(pcm_ctx* c, const float x6[6], float* corner_out, float* surf_out, double AtA[36], double AtB[6], int32_t counts[4]) {
  return probe(c, x6, corner_out, surf_out, AtA, AtB, counts, nullptr, nullptr);
}

int pcm_loam_neighbours(pcm_ctx* c, const float x6[6], int32_t* corner_nn, int32_t* surf_nn) {
  return probe(c, x6, nullptr, nullptr, nullptr, nullptr, nullptr, corner_nn, surf_nn);
}

}  // extern "C"
