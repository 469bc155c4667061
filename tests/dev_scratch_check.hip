// dev_scratch_check.hip -- csrc/dev_scratch.h on its own: a stand-alone program (the header, the HIP runtime and rocPRIM, nothing
// else of the project).
//   dev_scratch_check nodevice   on a machine without a HIP device: a take fails with a null pointer and a named error; release
//                                and the destructor are harmless afterwards
//   dev_scratch_check device     on a GPU: arena carves, the pool behind a full arena, the shared rocPRIM temporary, release,
//                                and the three wrappers against the host (a few KB, one process)
// Exit status 0 and a last line "ok" when every check held; otherwise the failed checks are printed.
#include "dev_scratch.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace pcm;

static int g_failed = 0;
#define CHECK(x)                                                                  \
  do {                                                                            \
    if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); g_failed++; }  \
  } while (0)

static bool names(const std::string& err, const char* what) { return err.find(what) != std::string::npos; }

static int nodevice() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) { std::printf("a HIP device is present: nothing to check in this mode\n"); return 2; }
  std::string err;
  {
    DevScratch sc(nullptr);
    float dummy = 0.f;
    float* p = &dummy;
    CHECK(sc.take(&p, 64, &err, "alpha") == PCM_ERR_HIP);
    CHECK(p == nullptr && names(err, "alpha"));
    void* t = &dummy;
    err.clear();
    CHECK(sc.temp(&t, 100, &err) == PCM_ERR_HIP);
    CHECK(t == nullptr && names(err, "rocPRIM temporary"));
    sc.release();
    sc.release();   // a second release is harmless
    CHECK(sc.arena_used() == 0);
    // an arena is host arithmetic only: carves come out of it without a device, the take that does not fit fails as above
    alignas(256) static char arena[1024];
    DevScratch sa(nullptr, arena, sizeof(arena));
    char *a = nullptr, *b = nullptr;
    CHECK(sa.take(&a, 100, &err, "first") == PCM_OK && a == arena && sa.arena_used() == 256);
    CHECK(sa.take(&b, 700, &err, "second") == PCM_OK && b == arena + 256 && sa.arena_used() == 1024);
    err.clear();
    CHECK(sa.take(&a, 1, &err, "third") == PCM_ERR_HIP && a == nullptr && names(err, "third") && sa.arena_used() == 1024);
    sa.release();
    CHECK(sa.arena_used() == 0);
  }   // the destructors of released scratches are harmless
  return g_failed ? 1 : 0;
}

static bool inside(const void* p, size_t bytes, const char* base, size_t cap) {
  const char* q = static_cast<const char*>(p);
  return q >= base && q + bytes <= base + cap;
}

static int device() {
  if (hipSetDevice(0) != hipSuccess) { std::printf("no HIP device\n"); return 2; }
  hipStream_t st = nullptr;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { std::printf("hipStreamCreate failed\n"); return 2; }
  std::string err;
  {
    constexpr size_t kArena = 2048;
    DevBuf<char> arena("arena");
    CHECK(arena.reserve(st, &err, kArena, kArena) == PCM_OK);
    DevScratch sc(st, arena, kArena);
    uint32_t *a = nullptr, *b = nullptr, *c = nullptr;
    uint64_t* big = nullptr;
    CHECK(sc.take(&a, 10, &err, "a") == PCM_OK && sc.take(&b, 65, &err, "b") == PCM_OK && sc.take(&c, 0, &err, "c") == PCM_OK);
    CHECK(a && b && c && ((uintptr_t)a % 256) == 0 && ((uintptr_t)b % 256) == 0 && ((uintptr_t)c % 256) == 0);
    CHECK(inside(a, 40, arena, kArena) && inside(b, 260, arena, kArena) && inside(c, 0, arena, kArena));
    CHECK((char*)b >= (char*)a + 40 && (char*)c >= (char*)b + 260);   // disjoint
    CHECK(sc.arena_used() == 256 + 512);
    CHECK(sc.take(&big, 1000, &err, "big") == PCM_OK && big != nullptr && !inside(big, 8000, arena, kArena));   // does not fit: from the pool
    CHECK(sc.arena_used() == 256 + 512);
    CHECK(hipMemsetAsync(big, 0, 8000, st) == hipSuccess && hipMemsetAsync(a, 0, 40, st) == hipSuccess);   // both are device memory

    void *t1 = nullptr, *t2 = nullptr, *t3 = nullptr, *t4 = nullptr;
    CHECK(sc.temp(&t1, 300, &err) == PCM_OK && t1 != nullptr);
    CHECK(sc.temp(&t2, 300, &err) == PCM_OK && t2 == t1);    // an equal request: the same block
    CHECK(sc.temp(&t3, 1, &err) == PCM_OK && t3 == t1);      // a smaller one too
    CHECK(sc.temp(&t4, 5000, &err) == PCM_OK && t4 != nullptr && t4 != t1);   // a larger one: a new block
    CHECK(sc.temp(&t2, 300, &err) == PCM_OK && t2 == t4);    // which serves the smaller requests from now on

    sc.release();
    CHECK(sc.arena_used() == 0);
    CHECK(sc.take(&a, 10, &err, "a") == PCM_OK && (char*)a == arena.p);   // the arena is handed out from its start again
    CHECK(sc.temp(&t1, 8, &err) == PCM_OK && inside(t1, 8, arena, kArena));   // the temporary of the last round is forgotten
    sc.release();

    // the wrappers against the host, from the pool alone
    constexpr uint32_t N = 1000;
    DevScratch sp(st);
    uint32_t *k_in = nullptr, *k_out = nullptr, *v_in = nullptr, *v_out = nullptr, *s_out = nullptr;
    CHECK(sp.take(&k_in, N, &err, "keys") == PCM_OK && sp.take(&k_out, N, &err, "keys out") == PCM_OK && sp.take(&v_in, N, &err, "values") == PCM_OK &&
          sp.take(&v_out, N, &err, "values out") == PCM_OK && sp.take(&s_out, N, &err, "scan out") == PCM_OK);
    std::vector<uint32_t> hk(N), hv(N), got_k(N), got_v(N), got_s(N);
    for (uint32_t i = 0; i < N; i++) { hk[i] = (i * 2654435761u) >> 20; hv[i] = i; }
    CHECK(hipMemcpyAsync(k_in, hk.data(), 4 * N, hipMemcpyHostToDevice, st) == hipSuccess && hipMemcpyAsync(v_in, hv.data(), 4 * N, hipMemcpyHostToDevice, st) == hipSuccess);
    CHECK(scratch_sort_pairs(sp, &err, k_in, k_out, v_in, v_out, N, 0, 32) == PCM_OK);
    CHECK(scratch_exclusive_scan(sp, &err, k_out, s_out, N) == PCM_OK);
    CHECK(hipMemcpyAsync(got_k.data(), k_out, 4 * N, hipMemcpyDeviceToHost, st) == hipSuccess && hipMemcpyAsync(got_v.data(), v_out, 4 * N, hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipMemcpyAsync(got_s.data(), s_out, 4 * N, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess);
    std::vector<uint32_t> order(N);
    for (uint32_t i = 0; i < N; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return hk[x] < hk[y]; });
    bool pairs = true, scan = true, keys = true;
    uint32_t run = 0;
    for (uint32_t i = 0; i < N; i++) { pairs &= got_k[i] == hk[order[i]] && got_v[i] == order[i]; scan &= got_s[i] == run; run += got_k[i]; }
    CHECK(pairs);   // sorted, and stable
    CHECK(scan);
    // a scan of fewer elements runs with the size the larger one asked for (no second query), and is right
    const size_t asked = sp.scan_bytes;
    CHECK(sp.scan_n == N && asked > 0);
    CHECK(scratch_exclusive_scan(sp, &err, v_out, s_out, N / 2) == PCM_OK && sp.scan_n == N && sp.scan_bytes == asked);
    CHECK(hipMemcpyAsync(got_s.data(), s_out, 4 * (N / 2), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess);
    bool half = true;
    run = 0;
    for (uint32_t i = 0; i < N / 2; i++) { half &= got_s[i] == run; run += got_v[i]; }
    CHECK(half);
    CHECK(scratch_sort_keys(sp, &err, k_in, k_out, N, 0, 32) == PCM_OK);
    CHECK(hipMemcpyAsync(got_v.data(), k_out, 4 * N, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess);
    for (uint32_t i = 0; i < N; i++) keys &= got_v[i] == got_k[i];
    CHECK(keys);
  }   // the scratches give back what is left, then the arena's owner frees it
  CHECK(err.empty());
  CHECK(hipStreamSynchronize(st) == hipSuccess);
  CHECK(hipStreamDestroy(st) == hipSuccess);
  return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
  const bool dev = argc == 2 && std::strcmp(argv[1], "device") == 0;
  if (!dev && !(argc == 2 && std::strcmp(argv[1], "nodevice") == 0)) { std::printf("usage: dev_scratch_check nodevice|device\n"); return 2; }
  const int rc = dev ? device() : nodevice();
  if (rc == 0) std::printf("ok\n");
  return rc;
}
