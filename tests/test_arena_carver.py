"""csrc/arena_carver.h and the layout functions on it (csrc/pre_layouts.h, vg::work_carve) on their own: tests/arena_carver_check.cpp
is a stand-alone host program (g++, no HIP).  It checks the carver's properties over a host buffer, pins every offset and total of
every layout to the closed-form expressions the entry points and *_scratch_bytes functions used before the carver, and carves each
layout from a heap block of exactly used() bytes, writing a pattern of its own into every block and reading all of them back.
Built plain and with -fsanitize=address,undefined, where a block that ends past used() is a heap overflow."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pointcloud-slam_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True])
def test_arena_carver_and_layouts(tmp_path, sanitize):
    out = str(tmp_path / "arena_carver_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", CSRC] + flags + [os.path.join(HERE, "arena_carver_check.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), (r.returncode, r.stdout, r.stderr)
