// dev_buf_check.hip -- csrc/dev_buf.h on its own: a stand-alone program (host code + the HIP runtime, nothing else of the project).
//   dev_buf_check nodevice   on a machine without a HIP device: every growth fails and leaves the buffers as the header promises
//   dev_buf_check device     on a GPU: growth, zero fill, kept contents, swap, the mapped pinned block (a few KB, one process)
// Exit status 0 and a last line "ok" when every check held; otherwise the failed checks are printed.
#include "dev_buf.h"

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
  hipStream_t st = nullptr;
  std::string err;
  {
    DevBuf<float> a("alpha");
    CHECK(a.reserve(st, &err, 64, 64) == PCM_ERR_HIP);
    CHECK(a.p == nullptr && a.cap == 0 && names(err, "alpha"));
    err.clear();
    CHECK(a.reserve(st, &err, 64, 80, true) == PCM_ERR_HIP);
    CHECK(a.p == nullptr && a.cap == 0 && names(err, "alpha"));
    err.clear();
    CHECK(a.reserve_keep(st, &err, 64, 80, 0) == PCM_ERR_HIP);
    CHECK(a.p == nullptr && a.cap == 0 && names(err, "alpha"));   // the pair is unchanged
    // reserve_keep on a pair that looks owned: a failure must not touch it (nothing is dereferenced or freed on this path)
    float dummy[4];
    a.p = dummy; a.cap = 4;
    err.clear();
    CHECK(a.reserve_keep(st, &err, 8, 8, 4) == PCM_ERR_HIP);
    CHECK(a.p == dummy && a.cap == 4 && names(err, "alpha"));
    CHECK(a.reserve_keep(st, &err, 4, 8, 4) == PCM_OK && a.p == dummy && a.cap == 4);   // below capacity: no call at all
    a.p = nullptr; a.cap = 0;
    a.release();
    a.release();   // a second release is harmless
    CHECK(a.p == nullptr && a.cap == 0);

    PinnedBuf<int> h("eta");
    err.clear();
    CHECK(h.reserve(st, &err, 16, 16) == PCM_ERR_HIP);
    CHECK(h.p == nullptr && h.cap == 0 && names(err, "eta"));
    err.clear();
    CHECK(h.reserve(st, &err, 16, 16, hipHostMallocMapped) == PCM_ERR_HIP);
    CHECK(h.p == nullptr && h.cap == 0 && names(err, "eta"));
    h.release();
    h.release();

    DevBuf<float> b("beta");
    a.swap(b);
    CHECK(a.p == nullptr && b.p == nullptr && a.cap == 0 && b.cap == 0);
    CHECK(std::strcmp(a.what, "beta") == 0 && std::strcmp(b.what, "alpha") == 0);
    PinnedBuf<int> k("kappa");
    h.swap(k);
    CHECK(h.p == nullptr && k.p == nullptr && std::strcmp(h.what, "kappa") == 0 && std::strcmp(k.what, "eta") == 0);
  }   // the destructors of empty buffers are harmless
  return g_failed ? 1 : 0;
}

static int device() {
  if (hipSetDevice(0) != hipSuccess) { std::printf("no HIP device\n"); return 2; }
  hipStream_t st = nullptr;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { std::printf("hipStreamCreate failed\n"); return 2; }
  std::string err;
  {
    DevBuf<uint32_t> a("alpha");
    CHECK(a.reserve(st, &err, 64, 100) == PCM_OK && a.p != nullptr && a.cap == 100);
    uint32_t* first = a.p;
    CHECK(a.reserve(st, &err, 100, 4000) == PCM_OK && a.p == first && a.cap == 100);   // below capacity: the same array
    CHECK(a.reserve(st, &err, 101, 256, true) == PCM_OK && a.cap == 256);               // growth, cleared
    std::vector<uint32_t> h(256, 0xffffffffu);
    CHECK(hipMemcpy(h.data(), a.p, sizeof(uint32_t) * 256, hipMemcpyDeviceToHost) == hipSuccess);
    bool zeros = true;
    for (uint32_t v : h) zeros &= v == 0u;
    CHECK(zeros);

    for (uint32_t i = 0; i < 64; i++) h[i] = i;
    CHECK(hipMemcpyAsync(a.p, h.data(), sizeof(uint32_t) * 64, hipMemcpyHostToDevice, st) == hipSuccess);
    CHECK(a.reserve_keep(st, &err, 200, 256, 64) == PCM_OK && a.cap == 256);            // below capacity
    CHECK(a.reserve_keep(st, &err, 300, 512, 64) == PCM_OK && a.cap == 512);            // grows, the first 64 stay
    std::vector<uint32_t> back(64, 0xffffffffu);
    CHECK(hipMemcpy(back.data(), a.p, sizeof(uint32_t) * 64, hipMemcpyDeviceToHost) == hipSuccess);
    bool kept = true;
    for (uint32_t i = 0; i < 64; i++) kept &= back[i] == i;
    CHECK(kept);

    DevBuf<uint32_t> b("beta");
    CHECK(b.reserve(st, &err, 8, 8) == PCM_OK);
    uint32_t *pa = a.p, *pb = b.p;
    a.swap(b);
    CHECK(a.p == pb && a.cap == 8 && std::strcmp(a.what, "beta") == 0);
    CHECK(b.p == pa && b.cap == 512 && std::strcmp(b.what, "alpha") == 0);
    b.release();
    b.release();
    CHECK(b.p == nullptr && b.cap == 0);

    PinnedBuf<unsigned char> f("flags");
    CHECK(f.reserve(st, &err, 1000, 1024, hipHostMallocMapped) == PCM_OK && f.p != nullptr && f.cap == 1024);
    void* dview = nullptr;
    CHECK(hipHostGetDevicePointer(&dview, f.p, 0) == hipSuccess && dview != nullptr);
    unsigned char* hp = f.p;
    CHECK(f.reserve(st, &err, 1024, 4096, hipHostMallocMapped) == PCM_OK && f.p == hp && f.cap == 1024);
    PinnedBuf<unsigned char> g("staging");
    CHECK(g.reserve(st, &err, 16, 16) == PCM_OK);
    f.swap(g);
    CHECK(g.p == hp && g.cap == 1024 && std::strcmp(g.what, "flags") == 0 && f.cap == 16 && std::strcmp(f.what, "staging") == 0);
  }   // the owners free what is left
  CHECK(err.empty());
  CHECK(hipStreamDestroy(st) == hipSuccess);
  return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
  const bool dev = argc == 2 && std::strcmp(argv[1], "device") == 0;
  if (!dev && !(argc == 2 && std::strcmp(argv[1], "nodevice") == 0)) { std::printf("usage: dev_buf_check nodevice|device\n"); return 2; }
  const int rc = dev ? device() : nodevice();
  if (rc == 0) std::printf("ok\n");
  return rc;
}
