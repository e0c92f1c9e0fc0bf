"""CPU check of the send batch's decision rule (shadow_amd/csrc/send_rule.h, included by
k_ev_prep<true>): tests/cpp/send_rule_check.cpp feeds it the drop boundary at loss 0.25, loss 0 and
1, payload 0, the bootstrap boundary, a loss whose f32 reliability rounds to 1 (the f32-then-widen
order of worker.rs:563-568) and both table forms of the latency fetch.  The GPU side of the same
header: tests/test_send_packets_gpu.py."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_send_rule_cases(tmp_path):
    exe = tmp_path / "send_rule_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                    os.path.join(HERE, "cpp", "send_rule_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "ok"
