"""pcm_share_target / pcm_target_share_count without a GPU: the symbols are exported and bound, a context without a device answers
with the library's readable error as every other entry point does, the C++ adapter's shareTargetWith meets a compiler (against
the stand-in PCL / Eigen headers of tests/stubs, as tests/test_adapter_compiles.py does), and the holder logic of
csrc/target_share.h -- attach, detach, last release -- runs its sequences in a stand-alone program built with
-fsanitize=address,undefined (tests/target_share_check.cpp; nothing sanitized is loaded into Python)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloud-slam_amd", "csrc")
NEW = ("pcm_share_target", "pcm_target_share_count")


def test_symbols_are_exported_and_bound(pcm):
    pcm.build_library()
    L = pcm.load_library()
    version_script = open(os.path.join(CSRC, "exports.map")).read()
    assert "global: pcm_*;" in version_script          # the pattern that lets every pcm_* entry point out
    dynsyms = subprocess.check_output(["nm", "-D", "--defined-only", pcm.capi.library_path()]).decode()
    hdr = open(os.path.join(ROOT, "include", "pcm_amd.h")).read()
    for name in NEW:
        assert name in pcm.capi.SYMBOLS
        assert (" T " + name + "\n") in dynsyms, name
        assert ("int " + name + "(") in hdr
        assert getattr(L, name).argtypes is not None   # a prototype, not ctypes' default
    assert L.pcm_share_target.argtypes == [C.c_void_p, C.c_void_p] and L.pcm_target_share_count.argtypes == [C.c_void_p]
    assert L.pcm_abi_version() == 3                    # added entry points: the ABI version stays


def test_no_device_fails_with_the_readable_error(pcm):
    """A context of a device that does not exist is kept so that the caller can read why; both calls refuse it."""
    L = pcm.load_library()
    a, b = L.pcm_create(9999, None), L.pcm_create(9999, None)
    assert a and b
    try:
        for rc in (L.pcm_share_target(a, b), L.pcm_share_target(b, a), L.pcm_target_share_count(a)):
            assert rc == -3                            # PCM_ERR_HIP, as pcm_align and the rest answer on such a context
        assert L.pcm_share_target(None, a) == -1 and L.pcm_target_share_count(None) == -1
        assert b"no CPU fallback" in L.pcm_last_error(a) and b"no CPU fallback" in L.pcm_last_error(b)
    finally:
        L.pcm_destroy(a)
        L.pcm_destroy(b)


ADAPTER_SRC = r'''
#define PCM_AMD_PCLOMP_ALIASES
#include <pcm_amd/registration.hpp>
#include <memory>
#include <vector>
using P = pcl::PointXYZ;
using Cloud = pcl::PointCloud<P>;

// one map, N registration objects: the first holds the map, the others share it
template <typename Reg> static int one_map(const Cloud::ConstPtr& map, const Cloud::ConstPtr& other_map, const Cloud::ConstPtr& scan) {
  std::vector<std::unique_ptr<Reg>> regs;
  for (int i = 0; i < 3; i++) regs.emplace_back(new Reg());
  regs[0]->setInputTarget(map);
  for (int i = 1; i < 3; i++) regs[i]->shareTargetWith(*regs[0]);
  int n = regs[0]->targetShareCount();
  for (auto& r : regs) {
    r->setInputTarget(map);            // the shared cloud: the reference's no-op
    r->setInputSource(scan);
    Cloud aligned;
    r->align(aligned, Eigen::Matrix4f::Identity());
  }
  regs[2]->setInputTarget(other_map);  // a target of its own again
  regs[0].reset();                     // the first holder goes, the map stays with regs[1]
  return n + regs[1]->targetShareCount() + regs[2]->targetShareCount();
}

int main() {
  auto map = std::make_shared<Cloud>(); auto other = std::make_shared<Cloud>(); auto scan = std::make_shared<Cloud>();
  int s = 0;
  s += one_map<pcm_amd::P2PlaneRegistration<P, P>>(map, other, scan);
  s += one_map<pcm_amd::GicpRegistration<P, P>>(map, other, scan);
  s += one_map<pcm_amd::VgicpRegistration<P, P>>(map, other, scan);
  s += one_map<pcm_amd::VgicpCudaRegistration<P, P>>(map, other, scan);
  s += one_map<pcm_amd::NdtRegistration<P, P>>(map, other, scan);
  s += one_map<pcm_amd::PclNdtRegistration<P, P>>(map, other, scan);
  s += one_map<pclomp::NormalDistributionsTransform<P, P>>(map, other, scan);
  return s > 0 ? 0 : 1;
}
'''


def test_adapter_share_target_compiles_and_links(tmp_path):
    inc = ["-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include")]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-fsyntax-only", "-x", "c++", "-"] + inc, input=ADAPTER_SRC.encode(), check=True)
    lib = os.path.join(ROOT, "pointcloud-slam_amd", "libpcm_amd.so")
    assert os.path.exists(lib)   # built by the test above / build(): the adapter's pcm_share_target call resolves against it
    subprocess.run(["g++", "-std=c++17", "-x", "c++", "-", "-o", str(tmp_path / "pcm_adapter_share_link_check")] + inc +
                   ["-L", os.path.dirname(lib), "-lpcm_amd", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--unresolved-symbols=ignore-in-shared-libs"],
                   input=ADAPTER_SRC.encode(), check=True)


def test_holder_sequences_under_the_sanitizers(tmp_path):
    """share then destroy the owner first / the sharer first, detach by set_target, a chain A -> B -> C, a refused mutation:
    the counts, and the release hook exactly once per target (tests/target_share_check.cpp)."""
    exe = str(tmp_path / "target_share_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "target_share_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"target_share_check ok" in out.stdout, out.stdout.decode()
