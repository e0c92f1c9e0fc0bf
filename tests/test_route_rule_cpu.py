"""CPU check of the route rule (shadow_amd/csrc/route_rule.h, included by the walk kernels of
routes.hip.h): tests/cpp/route_rule_check.cpp feeds it the source label (0, +0) against a nonzero
diagonal, a loss whose fold differs from the raw edge loss (fold(0, p) != p), an undirected edge in
either orientation, an ignored self-loop, two bit-equal candidates (the lower edge index wins), the
key-form table fetch and the latency compare at D near 2^64.  Built with -ffp-contract=off, as the
library.  Also: the numpy restatement (tests/routes_ref.py) on a reference table, and the binding.
The GPU side: tests/test_routes_gpu.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import routes_ref
from shadow_amd import _native as N
from shadow_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_route_rule_cases(tmp_path):
    exe = tmp_path / "route_rule_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", str(exe),
                    os.path.join(HERE, "cpp", "route_rule_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "ok"


def test_reference_walk_explains_every_pair_of_a_reference_table():
    """The premise: on the reference-equivalent table (oracle mode 0) every ordered pair has an exact
    predecessor, the traced edges re-fold to the table bits, and the tie graph really has ties."""
    e = synth.random_graph(40, 0.2, 14, lat_hi=3, p_zero=1.0, parallel=0.3)
    lat, loss = oracle.compute_shortest_paths(e.as_tuple(), np.arange(40, dtype=np.uint32), mode=0)
    pairs = routes_ref.all_pairs(40)
    off, he, hv, info = routes_ref.trace(e, lat, loss, pairs)
    assert info["unexplained"] == []
    assert routes_ref.certify(e, lat, loss, pairs, off, he, hv) == []
    assert info["steps"] == 3551 and info["multi_steps"] == 1087


def test_route_binding():
    assert N.SRG_ERR_ROUTE == 13
    assert ctypes.sizeof(N.RouteResult) == 8 * 3 + 4 + 4 + 8
    L = N.lib()
    assert L.srg_trace_routes_device.argtypes[11]._type_ is N.RouteResult
    assert L.srg_link_loads_device.argtypes[6]._type_ is N.RouteResult
    import shadow_amd
    assert shadow_amd.RouteResult is N.RouteResult
