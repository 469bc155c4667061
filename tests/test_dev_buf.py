"""csrc/dev_buf.h on its own: tests/dev_buf_check.hip is a stand-alone program (host code and the HIP runtime, nothing else of the
project).  Without a device every growth fails and must leave the buffers as the header promises; on a GPU the growth, zero fill,
kept contents, swap and the mapped pinned block are checked (a few KB, one process, its own time limit)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pointcloud-slam_amd", "csrc")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("devbuf") / "dev_buf_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result", "-Wno-unused-value", "-I" + CSRC, os.path.join(HERE, "dev_buf_check.hip"), "-o", out])
    return out


def _run(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)


def test_growth_fails_cleanly_without_a_device(check):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _run(check, "nodevice")


@pytest.mark.gpu
def test_buffers_on_the_device(check):
    _run(check, "device")
