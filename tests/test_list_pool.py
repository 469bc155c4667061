"""csrc/list_pool.h on its own (the pool of the following candidate lists, PCM_FLAG_FOLLOWING_LISTS): tests/list_pool_check.cpp is
a stand-alone host program (g++, no HIP) that drives the per-run decision, the counters and the rebuild policy with random
sequences of growth, shrinkage, eviction and new lists against a brute-force model of the pool -- no two live runs overlap, starts
are whole trips, bump pointer + tail stay inside the capacity, the counters add up, a rebuild is asked for exactly at the three
thresholds.  Built plain and with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("sanitize", [False, True])
def test_list_pool_against_a_model(tmp_path, sanitize):
    out = str(tmp_path / "list_pool_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(HERE, "list_pool_check.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), (r.returncode, r.stdout, r.stderr)
