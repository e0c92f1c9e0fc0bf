"""CPU check of the distribution plan (shadow_amd/csrc/plan.h): tests/cpp/plan_check.cpp runs the
library's own make_plan, tri_tile_h, xcd_tile_order and scan_group_cut; its make_plan results are
compared here with shadow_amd.dist.split_rows / source_split, which tests/test_dist_cpu.py uses as
the library's split.  Built plain and under AddressSanitizer + UndefinedBehaviorSanitizer."""
import json
import os
import shutil
import subprocess

import pytest

from shadow_amd.dist import source_split, split_rows

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.parametrize("sanitize", [[], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("cxx", ["g++", CLANG])
def test_plan(tmp_path, cxx, sanitize):
    if shutil.which(cxx) is None and not os.path.exists(cxx):
        pytest.skip(f"{cxx} not available")
    exe = tmp_path / "plan_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall"] + sanitize +
                   ["-o", str(exe), os.path.join(HERE, "cpp", "plan_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    # tri_tile_h, xcd_tile_order and scan_group_cut are checked inside the program
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["failed_checks"] == 0
    cases = out["make_plan"]
    want = {(G, g, V, T, n) for G in range(1, 9) for g in range(G) for V in (1, 63, 64, 65, 1000, 10000)
            for T in (64, 128) for n in {0, 1, 7, V}}
    assert {(c["G"], c["g"], c["V"], c["T"], c["n"]) for c in cases} == want
    assert len(cases) == len(want)
    for c in cases:
        G, g = c["G"], c["g"]
        nb = (c["V"] + c["T"] - 1) // c["T"]
        assert c["nb"] == nb, c
        rows = split_rows(nb, G)
        assert c["blk_lo"] == [a for a, _ in rows] + [nb], c
        assert (c["rb0"], c["rb1"]) == rows[g], c
        assert (c["p0"], c["p1"]) == source_split(c["n"], G)[g], c
        assert c["slice_ok"] and c["owner_ok"], c
