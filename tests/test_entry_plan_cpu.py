"""CPU check of the host entry's plan (shadow_amd/csrc/entry_plan.h): tests/cpp/entry_plan_check.cpp
runs the library's own rank_rows, slice_tables, offered_form and make_entry_plan; it checks the tiling,
make_plan's [p0, p1), the slice tables (64-bit arithmetic at E = 3e9), the eight offered forms and the
flags itself, and its rank_rows results are compared here with shadow_amd.dist.source_split, the split
the Python side uses.  Built plain and under AddressSanitizer + UndefinedBehaviorSanitizer."""
import json
import os
import shutil
import subprocess

import pytest

from shadow_amd.dist import source_split

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.parametrize("sanitize", [[], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("cxx", ["g++", CLANG])
def test_entry_plan(tmp_path, cxx, sanitize):
    if shutil.which(cxx) is None and not os.path.exists(cxx):
        pytest.skip(f"{cxx} not available")
    exe = tmp_path / "entry_plan_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall"] + sanitize +
                   ["-o", str(exe), os.path.join(HERE, "cpp", "entry_plan_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    # the tiling, make_plan, slice_tables, offered_form and the flags are checked inside the program
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["failed_checks"] == 0
    cases = out["rank_rows"]
    want = {(G, r, n) for G in range(1, 9) for r in range(G) for n in {0, 1, 7, G - 1, G, 10000}}
    assert {(c["G"], c["r"], c["n"]) for c in cases} == want
    assert len(cases) == len(want)
    for c in cases:
        assert (c["lo"], c["hi"]) == source_split(c["n"], c["G"])[c["r"]], c
