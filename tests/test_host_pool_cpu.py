"""CPU check of the host worker pool (shadow_amd/csrc/host_pool.h, shared by the H2D codec, the
late-loss thread and the key-widen thread): tests/cpp/host_pool_check.cpp issues thousands of
back-to-back run() calls on pools of 1, 2 and 8, runs two callers against one pool, and destroys
pools that never ran or just ran.  Built plain and under ThreadSanitizer."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.parametrize("sanitize", [[], ["-O1", "-fsanitize=thread"]], ids=["plain", "tsan"])
@pytest.mark.parametrize("cxx", ["g++", CLANG])
def test_host_pool(tmp_path, cxx, sanitize):
    if shutil.which(cxx) is None and not os.path.exists(cxx):
        pytest.skip(f"{cxx} not available")
    exe = tmp_path / "host_pool_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-pthread"] + sanitize +
                   ["-o", str(exe), os.path.join(HERE, "cpp", "host_pool_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
