"""CPU checks behind the route trees (shadow_amd/csrc/route_trees.hip.h):
  * tests/cpp/route_tree_check.cpp runs route_tree_rule.h (the header the kernels include) on a chain
    of 9 (3 moving rounds, not 8), a star, a fixpoint that is not a child of the source, and the
    saturating push at 2^64 - 1;
  * the premise of the essential filter on oracle tables: keeping only the arcs with
    lat(e) == D[u][t] leaves every row's predecessors unchanged and no edge lies below its entry;
  * the numpy restatement (tests/route_trees_ref.py) against the pairwise one (tests/routes_ref.py);
  * the binding.
The GPU side: tests/test_route_trees_gpu.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import route_trees_ref as T
import routes_ref as R
import structured
from shadow_amd import _native as N
from shadow_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))

GRAPHS = {
    "rand14_ties": lambda: synth.random_graph(40, 0.2, 14, lat_hi=3, p_zero=1.0, parallel=0.3),
    "rand12_directed": lambda: synth.random_graph(40, 0.2, 12, directed=True, lat_hi=6, parallel=0.2),
    "atlas48": lambda: synth.atlas_like(48, seed=5),
    "atlas300": lambda: synth.atlas_like(300, seed=300),
    "chain200": lambda: structured.chain(200),
    "bip10_140": lambda: structured.bipartite(10, 140),
    "grid12x9": lambda: structured.grid(12, 9),
}
_cache = {}


def case(name):
    if name not in _cache:
        e = GRAPHS[name]()
        lat, loss = oracle.compute_shortest_paths(e.as_tuple(), np.arange(e.num_vertices, dtype=np.uint32), mode=0)
        _cache[name] = (e, lat, loss)
    return _cache[name]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_route_tree_rule_cases(tmp_path):
    exe = tmp_path / "route_tree_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", str(exe),
                    os.path.join(HERE, "cpp", "route_tree_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "ok"


@pytest.mark.parametrize("name", list(GRAPHS))
def test_essential_filter_keeps_every_predecessor(name):
    e, lat, loss = case(name)
    full = R.arcs(e)
    ess, below = T.essential_arcs(e, lat)
    assert below == 0, "an edge below its table entry on a shortest-path table"
    assert 0 < len(ess[0]) <= len(full[0])
    for s in range(e.num_vertices):
        a = R.predecessors(e, lat, loss, s, full)
        b = R.predecessors(e, lat, loss, s, ess)
        off = np.arange(e.num_vertices) != s
        assert np.array_equal(a[0][off], b[0][off]) and np.array_equal(a[1][off], b[1][off]), s
        assert (a[0][off] != R.NONE).all(), "every off-diagonal entry has a predecessor"


@pytest.mark.parametrize("name", ["rand14_ties", "rand12_directed", "atlas48", "chain200", "grid12x9"])
def test_reference_trees_equal_the_reference_trace(name):
    """Hops, last and first hops of the tree equal the pairwise walk's, pair by pair."""
    e, lat, loss = case(name)
    V = e.num_vertices
    pe, pv, hops, first, bad = T.trees(e, lat, loss)
    assert bad == []
    pairs = R.all_pairs(V)
    off, he, hv, info = R.trace(e, lat, loss, pairs)
    assert info["unexplained"] == []
    lens = np.diff(off.astype(np.int64)).reshape(V, V)
    offd = ~np.eye(V, dtype=bool)
    assert np.array_equal(hops[offd], lens[offd]) and int(hops.max()) == info["max_hops"]
    last = he[(off[1:].astype(np.int64) - 1)].reshape(V, V)
    frst = he[off[:-1].astype(np.int64).clip(max=len(he) - 1)].reshape(V, V)
    assert np.array_equal(pe[offd], last[offd]) and np.array_equal(first[offd], frst[offd])
    d = np.arange(V)
    assert (pe[d, d] == T.NONE32).all() and (pv[d, d] == T.NONE32).all() and (first[d, d] == T.NONE32).all()
    assert (hops[d, d] == 0).all()


@pytest.mark.parametrize("name,nnz", [("rand14_ties", 1600), ("atlas48", 400), ("atlas300", 300), ("chain200", 300),
                                      ("bip10_140", 300), ("grid12x9", 300), ("rand12_directed", 300)])
def test_reference_tree_loads_equal_the_pairwise_loads(name, nnz):
    e, lat, loss = case(name)
    V = e.num_vertices
    rng = np.random.default_rng(V + nnz)
    counts = np.zeros((V, V), np.uint64)
    if nnz >= V * V:
        counts[:] = rng.integers(1, 1000, (V, V), dtype=np.uint64)
    else:
        counts.reshape(-1)[rng.choice(V * V, nnz, replace=False)] = rng.integers(1, 1000, nnz, dtype=np.uint64)
    want, volume = R.link_loads(e, lat, loss, counts)
    got, info = T.link_loads(e, lat, loss, counts)
    assert np.array_equal(got, want)
    assert int(got.astype(object).sum()) == volume and info["num_pairs"] == int((counts != 0).sum())


def test_route_trees_binding():
    assert N.SRG_OPT_ROUTE_TREE_ROWS == 44 and N.SRG_ROUTE_NONE == 0xFFFFFFFF
    assert "srg_route_trees_device" in N.EXPORTS and "srg_link_loads_trees_device" in N.EXPORTS
    L = N.lib()
    a = L.srg_route_trees_device.argtypes
    assert len(a) == 13 and a[4] is ctypes.c_uint32 and a[10]._type_ is N.RouteResult
    b = L.srg_link_loads_trees_device.argtypes
    assert len(b) == 9 and b[6]._type_ is N.RouteResult
    assert L.srg_route_trees_device.restype is ctypes.c_int and L.srg_link_loads_trees_device.restype is ctypes.c_int
    from shadow_amd import routes
    for name in ("route_trees_device", "route_trees", "link_loads_trees_device", "link_loads_trees", "ROUTE_NONE"):
        assert name in routes.__all__ and hasattr(routes, name)
