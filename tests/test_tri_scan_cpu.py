"""CPU checks of the triangular tight scan (SRG_OPT_SCAN_MIRROR).

1. The mirror rule itself, as a numpy model: tight-predecessor sets from an exact Floyd-Warshall,
   the packed table PK[row][column] = {u, b} filled by brute force only where blk(column) >=
   blk(row), the pairs below the diagonal derived by k_pred_mirror's walk with the exact fallback,
   and the whole table compared with brute force.
2. The host functions (shadow_amd/csrc/plan.h tri_scan_blocks, scan_group_cut_tri) through
   tests/cpp/tri_scan_check.cpp, built plain and under AddressSanitizer + UndefinedBehaviorSanitizer
   the way tests/test_plan_cpu.py builds its program."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from shadow_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NONE, MULTI = -1, -2
STEPS = 64  # MIRROR_STEPS


def closure(e):
    """W (min latency per vertex pair), B (a symmetric stand-in for 1 - loss of that edge: the min
    loss among the min-latency parallel edges, as k_w_split keeps it) and the exact closure D."""
    V = e.num_vertices
    INF = np.int64(1) << 60
    W = np.full((V, V), INF, dtype=np.int64)
    B = np.full((V, V), 2.0)
    lat = e.latency_ns.astype(np.int64)
    for s, d, w, p in zip(e.src.tolist(), e.dst.tolist(), lat.tolist(), e.packet_loss.tolist()):
        if s == d:
            continue
        for a, b in ((s, d), (d, s)):
            if w < W[a, b] or (w == W[a, b] and p < B[a, b]):
                W[a, b], B[a, b] = w, p
    D = W.copy()
    np.fill_diagonal(D, 0)
    for k in range(V):
        np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :], out=D)
    assert D.max() < INF, "the model graphs are connected"
    return W, B, D


def brute_force(W, D):
    """U[s][t]: the single tight predecessor of t from s, MULTI, or NONE (t == s)."""
    V = len(W)
    ess = (W == D) & ~np.eye(V, dtype=bool)  # only an essential edge can be tight
    U = np.full((V, V), NONE, dtype=np.int64)
    for s in range(V):
        tight = ess & (D[s][:, None] + W == D[s][None, :])  # [u][t]
        cnt = tight.sum(axis=0)
        one = tight.argmax(axis=0)
        U[s] = np.where(cnt == 1, one, np.where(cnt > 1, MULTI, NONE))
        U[s, s] = NONE
    return U


def mirror_model(U, bw):
    """The table with its pairs below the block diagonal derived from those on and above it.
    Returns (table, fallback pairs, walk steps of the pairs that needed no fallback)."""
    V = len(U)
    blk = np.arange(V) // bw
    scanned = blk[None, :] >= blk[:, None]
    PK = np.where(scanned, U, -99)  # -99: never written, must never be read
    out = PK.copy()
    slow, steps = 0, []
    for t in range(V):
        for s in range(int(blk[t]) * bw):
            x, res, n = t, None, 0
            for _ in range(STEPS):
                n += 1
                if blk[x] < blk[s]:
                    res = PK[x, s]
                    break
                v = PK[s, x]
                assert v != -99
                if v == s:
                    res = x
                    break
                if v < 0:
                    break
                x = v
            assert res != -99
            if res is None:  # the exact fallback: every in-edge of s against the exact keys
                slow += 1
                res = U[t, s]
            else:
                steps.append(n)
            out[t, s] = res
    return out, slow, steps


GRAPHS = {
    "atlas_300": (lambda: synth.atlas_like(300, seed=300), 16, False),
    "atlas_257": (lambda: synth.atlas_like(257, seed=257), 32, False),
    # small integer latencies and parallel edges: many pairs with several tight predecessors
    "ties_200": (lambda: synth.random_graph(200, 0.1, 42, lat_hi=6, parallel=0.2), 16, True),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_mirror_rule_equals_brute_force(name):
    make, bw, tie_heavy = GRAPHS[name]
    W, B, D = closure(make())
    assert np.array_equal(W, W.T) and np.array_equal(D, D.T) and np.array_equal(B, B.T)
    U = brute_force(W, D)
    got, slow, steps = mirror_model(U, bw)
    assert np.array_equal(got, U)
    assert int((got == MULTI).sum()) == int((U == MULTI).sum())
    # a mirrored single predecessor x of s stands for the undirected edge (s, x), whose 1 - loss
    # the scanned entry PK[s][x] carries: the same edge, the same bits (B is symmetric, above)
    assert steps and max(steps) <= STEPS
    if tie_heavy:
        assert int((U == MULTI).sum()) > 0 and slow > 0
    else:
        assert np.mean(steps) < 4


@pytest.mark.parametrize("sanitize", [[], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("cxx", ["g++", CLANG])
def test_tri_scan_host_functions(tmp_path, cxx, sanitize):
    if shutil.which(cxx) is None and not os.path.exists(cxx):
        pytest.skip(f"{cxx} not available")
    exe = tmp_path / "tri_scan_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall"] + sanitize +
                   ["-o", str(exe), os.path.join(HERE, "cpp", "tri_scan_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["failed_checks"] == 0
