"""csrc/dev_scratch.h on its own: tests/dev_scratch_check.hip is a stand-alone program (the header, the HIP runtime and rocPRIM,
nothing else of the project).  Without a device a take fails with a null pointer and a named error, and release and the destructor
are harmless afterwards; on a GPU the arena carves (aligned, disjoint, inside), the pool behind a full arena, the shared rocPRIM
temporary, release and the three wrappers are checked (a few KB, one process, its own time limit)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pointcloud-slam_amd", "csrc")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("devscratch") / "dev_scratch_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result", "-Wno-unused-value", "-I" + CSRC, os.path.join(HERE, "dev_scratch_check.hip"), "-o", out])
    return out


def _run(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)


def test_take_fails_cleanly_without_a_device(request):
    import torch
    if torch.cuda.is_available():   # asked before anything is compiled for this test
        pytest.skip("a GPU is present")
    _run(request.getfixturevalue("check"), "nodevice")


@pytest.mark.gpu
def test_scratch_on_the_device(check):
    _run(check, "device")
