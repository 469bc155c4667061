"""csrc/sub_state.h on its own: tests/sub_state_check.cpp is a stand-alone host program (g++, no HIP, nothing else of the project).
An empty holder returns null and destroys nothing; get_or_create makes the object once and returns it ever after; the owned
type's destructor runs exactly once, when the holder dies; holders inside a struct die in reverse declaration order."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pointcloud-slam_amd", "csrc")


def test_sub_state_holder(tmp_path):
    out = str(tmp_path / "sub_state_check")
    subprocess.check_call([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, os.path.join(HERE, "sub_state_check.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)
