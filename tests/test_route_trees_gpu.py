"""Route trees and tree link loads (srg_route_trees_device, srg_link_loads_trees_device;
route_trees.hip.h, route_tree_rule.h).  Every comparison is exact: against the numpy restatement
(tests/route_trees_ref.py, which filters nothing), against the library's own pairwise calls
(trace_routes of all pairs, link_loads) and against tests/routes_ref.py.  Tables come from
Router.compute_shortest_paths over all vertices."""
import numpy as np
import pytest

import route_trees_ref as T
import routes_ref as R
import structured
from shadow_amd import _native as N
from shadow_amd import events as ev
from shadow_amd import generate_routing_info, routes, synth
from shadow_amd.device import DeviceGraph
from shadow_amd.graph import Edges, NetGraphError

pytestmark = pytest.mark.gpu

U64_MAX = 2**64 - 1
NONE = T.NONE32
SENT = 0x7ABCDEF0

# the ten graphs of test_routes_gpu.py
GRAPHS = {
    "rand11": lambda: synth.random_graph(40, 0.15, 11, lat_hi=6, parallel=0.2),
    "rand12_directed": lambda: synth.random_graph(40, 0.2, 12, directed=True, lat_hi=6, parallel=0.2),
    "rand13_lossy": lambda: synth.random_graph(40, 0.3, 13, lat_hi=1000, loss_hi=1.0, p_zero=0.0),
    "rand14_ties": lambda: synth.random_graph(40, 0.2, 14, lat_hi=3, p_zero=1.0, parallel=0.3),
    "rand15": lambda: synth.random_graph(40, 0.2, 15, lat_hi=3, p_zero=0.8, parallel=0.3),
    "atlas48": lambda: synth.atlas_like(48, seed=5),
    "chain200": lambda: structured.chain(200),            # 199 hops: 8 doubling rounds, 199 push levels
    "bip10_140": lambda: structured.bipartite(10, 140),   # a list of 140: three 64-chunks, the last partial
    "grid12x9": lambda: structured.grid(12, 9),           # V = 108
    "chain_chords80": lambda: structured.chain_chords(80, 3, 12),
}
_cache = {}


def case(router, name):
    """(edges, latency, loss, DevicePathTable, reference trees), computed once per graph, never changed."""
    if name not in _cache:
        e = GRAPHS[name]()
        t = router.compute_shortest_paths(e, np.arange(e.num_vertices, dtype=np.uint32))
        lat, loss = t.latency_ns.copy(), t.packet_loss.copy()
        ref = T.trees(e, lat, loss)
        assert ref[4] == [], "the reference must explain every entry of a correct table"
        _cache[name] = (e, lat, loss, ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss), ref[:4])
    return _cache[name]


def reversed_edges(e):
    return Edges(e.num_vertices, e.src[::-1], e.dst[::-1], e.latency_ns[::-1], e.packet_loss[::-1], e.directed)


def raw_trees(router, e, table, sources, ns=None, want=(1, 1, 1, 1), pe_null=False):
    """The raw call with sentinel-prefilled outputs: (rc, result, message, [pe, pv, hops, first]); an
    output not wanted is passed as NULL and returned as None."""
    import torch
    dev = "cuda:0"
    dg = e if isinstance(e, DeviceGraph) else DeviceGraph(e, dev)
    n = table.n
    src_t = None if sources is None else ev._i32(np.asarray(sources, dtype=np.uint32), dev)
    ns = (n if sources is None else len(sources)) if ns is None else ns
    outs = [torch.full((max(ns * n, 1),), SENT, dtype=torch.int32, device=dev) if w else None for w in want]
    if pe_null:
        outs[0] = None
    rc, res, msg = routes.route_trees_device(router, dg, table, src_t, ns, *outs, check=False)
    torch.cuda.synchronize()
    host = [None if o is None else o.cpu().numpy().view(np.uint32)[:ns * n].reshape(ns, n) for o in outs]
    return rc, res, msg, host


def assert_trees(got, ref, rows=None):
    for g, r, what in zip(got, ref, ("pred_edge", "pred_vertex", "hops", "first_edge")):
        if g is not None:
            assert np.array_equal(g, r if rows is None else r[rows]), what


# ---- 1. all sources of each graph -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_all_sources_equal_reference_and_trace(router, name):
    e, lat, loss, table, ref = case(router, name)
    V = e.num_vertices
    pe, pv, hops, first, res = routes.route_trees(router, e, table)
    assert_trees((pe, pv, hops, first), ref)
    d = np.arange(V)
    assert (pe[d, d] == NONE).all() and (pv[d, d] == NONE).all() and (first[d, d] == NONE).all()
    assert (hops[d, d] == 0).all()
    # the library's own trace of every off-diagonal pair: last hop, length, first hop
    offd = ~np.eye(V, dtype=bool)
    pairs = R.all_pairs(V)[offd.reshape(-1)]
    off, he, hv, tres = routes.trace_routes(router, e, table, pairs)
    off = off.astype(np.int64)
    assert np.array_equal(hops[offd], np.diff(off))
    assert np.array_equal(pe[offd], he[off[1:] - 1]) and np.array_equal(first[offd], he[off[:-1]])
    two = np.diff(off) >= 2
    assert np.array_equal(pv[offd][two], hv[off[1:] - 2][two]) and (pv[offd][~two] == pairs[~two, 0]).all()
    assert res["num_pairs"] == V * (V - 1) == tres["num_pairs"]
    assert res["total_hops"] == tres["total_hops"] == int(hops.sum()) and res["max_hops"] == tres["max_hops"]
    assert res["bad_pair"] == U64_MAX


def test_chain_needs_eight_rounds_and_counts_199_hops(router):
    e, _, _, table, _ = case(router, "chain200")
    pe, pv, hops, first, res = routes.route_trees(router, e, table, [0, 199, 100])
    assert res["max_hops"] == 199 and np.array_equal(hops[0], np.arange(200)) and np.array_equal(hops[1], np.arange(199, -1, -1))
    assert (first[0, 1:] == 200).all() and (first[1, :199] == 200 + 198).all()  # the self-loops come first
    assert (first[2, :100] == 200 + 99).all() and (first[2, 101:] == 200 + 100).all()
    assert np.array_equal(pv[0, 1:], np.arange(199)) and np.array_equal(pe[0, 1:], 200 + np.arange(199))


# ---- 2. tie rule ----------------------------------------------------------------------------------
def test_tie_rule_follows_the_edge_index(router):
    e, lat, loss, table, ref = case(router, "rand14_ties")
    rev = reversed_edges(e)
    xref = T.trees(rev, lat, loss)
    assert xref[4] == []
    got = routes.route_trees(router, rev, table)
    assert_trees(got[:4], xref[:4])
    # the choice really moved with the indices: some predecessor is another physical edge now
    offd = ~np.eye(e.num_vertices, dtype=bool)
    assert not np.array_equal(got[0][offd], (e.num_edges - 1 - ref[0][offd].astype(np.int64)).astype(np.uint32))


# ---- 3. both table forms ---------------------------------------------------------------------------
def test_key_table_gives_the_same_trees(router):
    g = synth.random_graph(40, 0.2, 21, lat_hi=50)
    e = Edges(40, g.src, g.dst, g.latency_ns * np.uint64(1000), g.packet_loss)
    ri = generate_routing_info(e, list(range(40)), True, router)
    kt = ri.key_tables()
    assert kt is not None and ri.stats["table_keys"] == 1
    key, diag, unit, loss = kt
    lat, loss64, _ = ri.tables()
    t_key = ev.DevicePathTable.from_arrays(key=key, diag=diag, unit=unit, packet_loss=loss)
    t_u64 = ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss64)
    a = routes.route_trees(router, e, t_key)
    b = routes.route_trees(router, e, t_u64)
    r = T.trees(e, np.asarray(lat), np.asarray(loss64))
    assert r[4] == []
    assert_trees(a[:4], r[:4])
    assert_trees(b[:4], r[:4])


# ---- 4. directed ----------------------------------------------------------------------------------
def test_directed_trees_differ_by_direction(router):
    e, lat, loss, table, ref = case(router, "rand12_directed")
    pe, pv, hops, first, _ = routes.route_trees(router, e, table)
    assert_trees((pe, pv, hops, first), ref)
    ok = pe != NONE
    assert (e.dst[pe[ok]] == np.nonzero(ok)[1]).all() and (e.src[pe[ok]] == pv[ok]).all(), "edges point at their target"
    assert not np.array_equal(hops, hops.T)


# ---- 5. sources -----------------------------------------------------------------------------------
def test_sources_subset_permuted_with_a_duplicate(router):
    e, _, _, table, ref = case(router, "grid12x9")
    src = [107, 3, 64, 3, 0, 65]
    rc, res, msg, got = raw_trees(router, e, table, src)
    assert rc == N.SRG_OK, msg
    assert_trees(got, ref, rows=src)
    assert res["num_pairs"] == 6 * 107 and res["total_hops"] == int(ref[2][src].sum())


def test_null_sources_with_fewer_rows(router):
    e, _, _, table, ref = case(router, "atlas48")
    rc, res, msg, got = raw_trees(router, e, table, None, ns=5)
    assert rc == N.SRG_OK, msg
    assert_trees(got, ref, rows=np.arange(5))
    assert res["num_pairs"] == 5 * 47 and res["max_hops"] == int(ref[2][:5].max())


# ---- 6. optional outputs ----------------------------------------------------------------------------
@pytest.mark.parametrize("missing", [1, 2, 3])
def test_each_optional_output_as_null(router, missing):
    e, _, _, table, ref = case(router, "chain_chords80")
    want = [1, 1, 1, 1]
    want[missing] = 0
    rc, res, msg, got = raw_trees(router, e, table, None, want=want)
    assert rc == N.SRG_OK, msg
    assert got[missing] is None
    assert_trees(got, ref)
    assert res["total_hops"] == int(ref[2].sum())


# ---- 7. batches -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 7])
def test_forced_batches_give_the_same_trees(router, rows):
    e, _, _, table, ref = case(router, "rand15")
    base = raw_trees(router, e, table, None)
    router.set_option(N.SRG_OPT_ROUTE_TREE_ROWS, rows)
    try:
        assert router.get_option(N.SRG_OPT_ROUTE_TREE_ROWS) == rows
        rc, res, msg, got = raw_trees(router, e, table, None)          # 40 sources: the last batch is partial
        rc2, res2, _, got2 = raw_trees(router, e, table, None, want=(1, 0, 1, 1))  # the workspace pred_vertex
    finally:
        router.set_option(N.SRG_OPT_ROUTE_TREE_ROWS, 0)
    assert rc == N.SRG_OK and rc2 == N.SRG_OK, msg
    assert_trees(got, ref)
    assert_trees(got2, ref)
    for k in ("num_pairs", "total_hops", "max_hops", "bad_pair"):
        assert res[k] == base[1][k] == res2[k]


# ---- 8. refusals --------------------------------------------------------------------------------------
def damaged(lat, loss, s, t, what):
    lat, loss = lat.copy(), loss.copy()
    if what == "latency":
        lat[s, t] += 1
    else:
        loss.view(np.uint32)[s, t] ^= 1
    return ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss)


def no_edge_between(e, s, t):
    m = ((e.src == s) & (e.dst == t)) | ((e.src == t) & (e.dst == s))
    return not m.any()


@pytest.mark.parametrize("what", ["latency", "loss_bit"])
def test_damaged_entry_is_refused(router, what):
    e, lat, loss, _, ref = case(router, "rand13_lossy")
    V = e.num_vertices
    # a pair of row 5 that no single edge joins (so no edge falls below the raised entry) and that is
    # nobody's predecessor in row 5 (so only its own entry goes unexplained)
    t = next(t for t in range(V) if t != 5 and no_edge_between(e, 5, t) and not (ref[1][5] == t).any())
    bad = damaged(lat, loss, 5, t, what)
    rc, res, msg, _ = raw_trees(router, e, bad, [3, 5, 20])
    assert rc == N.SRG_ERR_ROUTE and res["bad_pair"] == 1 * V + t, msg
    assert "from node index 5 to %d " % t in msg
    with pytest.raises(routes.RouteError) as ei:
        routes.route_trees(router, e, bad)
    assert ei.value.code == N.SRG_ERR_ROUTE and ei.value.bad_pair == 5 * V + t


def test_direct_path_table_is_refused(router):
    e = synth.complete_random(30, seed=33)
    t = router.get_direct_paths(e, np.arange(30, dtype=np.uint32))
    table = ev.DevicePathTable.from_arrays(latency_ns=t.latency_ns, packet_loss=t.packet_loss)
    rc, res, msg, _ = raw_trees(router, e, table, None)
    assert rc == N.SRG_ERR_ROUTE and res["bad_pair"] < 900, msg


def test_edge_below_its_entry_is_refused(router):
    e, lat, loss, table, ref = case(router, "rand11")
    V = e.num_vertices
    # the first edge between two vertices whose entry is at least 2 (a lowered latency stays >= 1)
    k = next(k for k in range(V, e.num_edges) if e.src[k] != e.dst[k] and lat[e.src[k], e.dst[k]] >= 2)
    u, t = int(e.src[k]), int(e.dst[k])
    assert lat[u, t] == lat[t, u], "an undirected table is symmetric"
    low = e.latency_ns.copy()
    low[k] = lat[u, t] - 1
    g = Edges(V, e.src, e.dst, low, e.packet_loss, e.directed)
    rc, res, msg, _ = raw_trees(router, g, table, [0])
    assert rc == N.SRG_ERR_ROUTE and res["bad_pair"] == min(u * V + t, t * V + u), msg
    a, b = divmod(res["bad_pair"], V)
    assert "from node index %d to %d " % (a, b) in msg and "shorter than the table entry" in msg


def test_argument_refusals(router):
    e, lat, loss, table, _ = case(router, "rand11")
    V = e.num_vertices
    small = ev.DevicePathTable.from_arrays(latency_ns=lat[:V - 1, :V - 1].copy(), packet_loss=loss[:V - 1, :V - 1].copy())
    rc, _, msg, _ = raw_trees(router, e, small, [0])
    assert rc == N.SRG_ERR_ARG and "num_vertices" in msg
    rc, _, msg, _ = raw_trees(router, e, table, [0, V])
    assert rc == N.SRG_ERR_ARG and "out of range" in msg
    rc, _, msg, _ = raw_trees(router, e, table, None, ns=V + 1)
    assert rc == N.SRG_ERR_ARG and "out of range" in msg
    rc, _, msg, _ = raw_trees(router, e, table, [0], pe_null=True)
    assert rc == N.SRG_ERR_ARG and "null" in msg
    zl = e.latency_ns.copy()
    zl[V + 3] = 0
    rc, _, msg, _ = raw_trees(router, Edges(V, e.src, e.dst, zl, e.packet_loss, e.directed), table, [0])
    assert rc == N.SRG_ERR_ARG and "latency 0" in msg
    far = e.dst.copy()
    far[V + 3] = V
    rc, _, msg, _ = raw_trees(router, Edges(V, e.src, far, e.latency_ns, e.packet_loss, e.directed), table, [0])
    assert rc == N.SRG_ERR_ARG and "endpoint" in msg
    no_loss = ev.DevicePathTable.from_arrays(latency_ns=lat)
    rc, _, msg, _ = raw_trees(router, e, no_loss, [0])
    assert rc == N.SRG_ERR_ARG and "packet_loss" in msg


def test_no_sources_is_ok_and_touches_nothing(router):
    e, _, _, table, _ = case(router, "rand11")
    rc, res, msg, got = raw_trees(router, e, table, [], ns=0)
    assert rc == N.SRG_OK and res["num_pairs"] == 0 and res["total_hops"] == 0, msg
    rc, res, msg, got = raw_trees(router, e, table, None, ns=0, pe_null=True)
    assert rc == N.SRG_OK, msg


# ---- 9. tree loads --------------------------------------------------------------------------------------
def sparse_counts(V, seed, nnz, diag=5):
    rng = np.random.default_rng(seed)
    c = np.zeros((V, V), np.uint64)
    idx = rng.choice(V * V, nnz, replace=False)
    c.reshape(-1)[idx] = rng.integers(1, 1000, nnz, dtype=np.uint64)
    d = rng.choice(V, diag, replace=False)
    c[d, d] = rng.integers(1, 1000, diag, dtype=np.uint64)
    return c


def both_loads(router, e, table, counts, loads=None):
    """(tree loads, tree result, pairwise loads, pairwise result), the timing left out of the results."""
    a, ra = routes.link_loads_trees(router, e, table, counts, loads)
    b, rb = routes.link_loads(router, e, table, counts, loads)
    ra.pop("ms_total"), rb.pop("ms_total")
    return a, ra, b, rb


@pytest.mark.parametrize("name,nnz", [("atlas48", 400), ("chain200", 300), ("rand14_ties", 1600)])
def test_tree_loads_equal_reference_and_pairwise_and_accumulate(router, name, nnz):
    e, lat, loss, table, _ = case(router, name)
    V = e.num_vertices
    if nnz == V * V:
        counts = np.random.default_rng(9).integers(1, 1000, (V, V), dtype=np.uint64)  # every entry nonzero
    else:
        counts = sparse_counts(V, 100 + V, nnz)
    want, volume = R.link_loads(e, lat, loss, counts)
    got, res, pw, pres = both_loads(router, e, table, counts)
    assert np.array_equal(got, want) and np.array_equal(got, pw)
    assert res == pres and res["num_pairs"] == int((counts != 0).sum()) and res["bad_pair"] == U64_MAX
    tref, tinfo = T.link_loads(e, lat, loss, counts)
    assert np.array_equal(got, tref) and res["total_hops"] == tinfo["total_hops"] and res["max_hops"] == tinfo["max_hops"]
    assert int(got.astype(object).sum()) == volume, "conservation: sum(loads) == sum(count * hops)"
    # a second call accumulates onto nonzero loads
    counts2 = sparse_counts(V, 200 + V, min(nnz, 300) // 2)
    want2, _ = R.link_loads(e, lat, loss, counts2, loads=want)
    got2, _ = routes.link_loads_trees(router, e, table, counts2, loads=got)
    assert np.array_equal(got2, want2) and not np.array_equal(got2, got)
    # all-zero counts: nothing moves
    got3, res3 = routes.link_loads_trees(router, e, table, np.zeros((V, V), np.uint64), loads=got2)
    assert np.array_equal(got3, got2) and res3["num_pairs"] == 0


def test_tree_loads_saturate(router):
    e, lat, loss, table, _ = case(router, "chain200")
    V = e.num_vertices
    counts = np.zeros((V, V), np.uint64)
    counts[0, 2], counts[1, 3] = U64_MAX - 1, 5  # routes 0-1-2 and 1-2-3 share the edge 1 - 2
    got, res, pw, pres = both_loads(router, e, table, counts)
    e01, e12, e23 = V + 0, V + 1, V + 2
    assert int(got[e12]) == U64_MAX and int(got[e01]) == U64_MAX - 1 and int(got[e23]) == 5
    assert int((got != 0).sum()) == 3 and np.array_equal(got, pw) and res == pres
    # a subtree sum that saturates on its way up: 0 -> 3 and 0 -> 2 meet on the edges 1 - 2 and 0 - 1
    counts = np.zeros((V, V), np.uint64)
    counts[0, 3], counts[0, 2] = U64_MAX - 1, 7
    got, res, pw, pres = both_loads(router, e, table, counts)
    assert int(got[e23]) == U64_MAX - 1 and int(got[e12]) == U64_MAX and int(got[e01]) == U64_MAX
    assert np.array_equal(got, pw) and res == pres


def test_tree_loads_diagonal_without_self_loop_is_no_edge(router):
    import torch
    e, _, _, table, _ = case(router, "rand11")
    V = e.num_vertices
    keep = np.arange(e.num_edges) != 7  # vertex 7's self-loop removed from the device graph only
    cut = Edges(V, e.src[keep], e.dst[keep], e.latency_ns[keep], e.packet_loss[keep], e.directed)
    counts = np.zeros((V, V), np.uint64)
    counts[7, 7], counts[2, 9] = 3, 4
    pre = np.arange(cut.num_edges, dtype=np.uint64) + 11
    msgs = []
    for fn in (routes.link_loads_trees_device, routes.link_loads_device):
        loads_t = ev._i64(pre, "cuda:0")
        with pytest.raises(NetGraphError) as ei:
            fn(router, DeviceGraph(cut, "cuda:0"), table, ev._i64(counts, "cuda:0"), loads_t)
        assert ei.value.code == N.SRG_ERR_NO_EDGE
        torch.cuda.synchronize()
        assert np.array_equal(loads_t.cpu().numpy().view(np.uint64), pre)
        msgs.append(ei.value.message)
    assert msgs[0] == msgs[1] and "No edge connecting node 7 to 7" in msgs[0]


def test_tree_loads_failing_call_leaves_the_loads(router):
    import torch
    e, lat, loss, _, _ = case(router, "rand13_lossy")
    V = e.num_vertices
    bad = damaged(lat, loss, 5, 17, "latency")
    counts = np.zeros((V, V), np.uint64)
    counts[3, 9], counts[5, 17], counts[20, 2] = 4, 6, 8
    pre = np.arange(e.num_edges, dtype=np.uint64) + 11
    out = []
    for fn in (routes.link_loads_trees_device, routes.link_loads_device):
        loads_t = ev._i64(pre, "cuda:0")
        with pytest.raises(routes.RouteError) as ei:
            fn(router, DeviceGraph(e, "cuda:0"), bad, ev._i64(counts, "cuda:0"), loads_t)
        assert ei.value.code == N.SRG_ERR_ROUTE and ei.value.bad_pair == 5 * V + 17
        torch.cuda.synchronize()
        assert np.array_equal(loads_t.cpu().numpy().view(np.uint64), pre), "bit for bit"
        out.append(ei.value.message)
    assert out[0] == out[1]


@pytest.mark.parametrize("kind", ["far_leaf", "child_leaf"])
def test_damaged_leaf_with_a_zero_count_does_not_fail(router, kind):
    """far_leaf: no edge joins s and t, the essential lists stand.  child_leaf: t hangs on s by an edge
    that the raised entry puts below it, so the call falls back to the full in-edge lists."""
    e, lat, loss, _, ref = case(router, "rand13_lossy")
    V = e.num_vertices
    leaves = ((s, t) for s in range(5, V) for t in range(V) if t != s and not (ref[1][s] == t).any())
    if kind == "far_leaf":
        s, t = next((s, t) for s, t in leaves if no_edge_between(e, s, t))
    else:
        s, t = next((s, t) for s, t in leaves if ref[1][s][t] == s)
        assert e.latency_ns[ref[0][s][t]] == lat[s, t]
    counts = sparse_counts(V, 77, 500)
    counts[s, t] = 0
    for what in ("latency", "loss_bit"):
        bad = damaged(lat, loss, s, t, what)
        got, res, pw, pres = both_loads(router, e, bad, counts)
        assert np.array_equal(got, pw) and res == pres and res["bad_pair"] == U64_MAX
    assert np.array_equal(got, R.link_loads(e, lat, loss, counts)[0])


@pytest.mark.parametrize("rows", [1, 7])
def test_tree_loads_forced_batches(router, rows):
    e, lat, loss, table, _ = case(router, "atlas48")
    V = e.num_vertices
    counts = sparse_counts(V, 100 + V, 400)
    base, bres = routes.link_loads_trees(router, e, table, counts)
    router.set_option(N.SRG_OPT_ROUTE_TREE_ROWS, rows)
    try:
        got, res = routes.link_loads_trees(router, e, table, counts)
    finally:
        router.set_option(N.SRG_OPT_ROUTE_TREE_ROWS, 0)
    assert np.array_equal(got, base) and np.array_equal(got, R.link_loads(e, lat, loss, counts)[0])
    for k in ("num_pairs", "total_hops", "max_hops", "bad_pair"):
        assert res[k] == bres[k]


def test_send_packets_counts_feed_tree_loads(router):
    import torch
    e, lat, loss, table, _ = case(router, "atlas48")
    V = e.num_vertices
    batch, round_end, _ = ev.synthetic_round(20_000, 64, V, loss=0.1)
    counts = torch.zeros((V, V), dtype=torch.int64, device="cuda:0")
    *_, res = ev.send_packets(router, batch, table, 64, round_end, 0, counts)
    assert res["num_sent"] > 10_000
    dg = DeviceGraph(e, "cuda:0")
    loads = torch.zeros(e.num_edges, dtype=torch.int64, device="cuda:0")
    lres = routes.link_loads_trees_device(router, dg, table, counts, loads)
    host_counts = counts.cpu().numpy().view(np.uint64)
    assert int(host_counts.sum()) == res["num_sent"] and lres["num_pairs"] == int((host_counts != 0).sum())
    want, volume = R.link_loads(e, lat, loss, host_counts)
    got = loads.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want) and int(got.sum()) == volume


# ---- 10. one workspace for both call families -----------------------------------------------------------
def loads_from_trees(ref, num_edges, counts):
    """Every off-diagonal count added along its route of the reference trees (pred_edge, pred_vertex)."""
    pe, pv = ref[0], ref[1]
    out = np.zeros(num_edges, np.uint64)
    for s, t in zip(*np.nonzero(counts)):
        c = counts[s, t]
        while t != s:
            out[pe[s, t]] += c
            t = pv[s, t]
    return out


def test_route_and_tree_calls_share_one_workspace(router):
    """The pairwise calls and the tree calls build their in-edge lists in the same buffers of the
    context.  Calls of both families on one router, over graphs of different size and direction, the
    essential lists and the full ones in turn: each result is that of the cached reference.  Step 3
    raises one table entry above the edge that carries it (the edge then lies below its entry), which
    makes the loads call drop the essential lists and build the full ones, and makes a trees call
    fail as test_edge_below_its_entry_is_refused expects."""
    big, _, _, big_table, big_ref = case(router, "bip10_140")
    # 1. essential lists of 150 vertices
    assert_trees(routes.route_trees(router, big, big_table)[:4], big_ref)
    # 2. full lists of a smaller, directed graph: every pair's route against the trees
    e, _, _, table, ref = case(router, "rand12_directed")
    V = e.num_vertices
    offd = ~np.eye(V, dtype=bool)
    pairs = R.all_pairs(V)[offd.reshape(-1)]
    off, he, hv, _ = routes.trace_routes(router, e, table, pairs)
    off = off.astype(np.int64)
    assert np.array_equal(ref[2][offd], np.diff(off))
    assert np.array_equal(ref[0][offd], he[off[1:] - 1]) and np.array_equal(ref[3][offd], he[off[:-1]])
    # 3. an edge below its entry: the essential lists are built, refused, and the full lists rebuilt
    e, lat, loss, _, ref = case(router, "rand11")
    V = e.num_vertices
    s, t = next((s, t) for s in range(V) for t in range(V)
                if t != s and ref[1][s][t] == s and not (ref[1][s] == t).any() and e.latency_ns[ref[0][s][t]] == lat[s, t])
    bad = damaged(lat, loss, s, t, "latency")
    counts = sparse_counts(V, 78, 500, diag=0)
    np.fill_diagonal(counts, 0)
    counts[s, t] = 0
    got, res = routes.link_loads_trees(router, e, bad, counts)
    assert np.array_equal(got, loads_from_trees(ref, e.num_edges, counts)) and res["bad_pair"] == U64_MAX
    rc, res, msg, _ = raw_trees(router, e, bad, [0])
    assert rc == N.SRG_ERR_ROUTE and res["bad_pair"] == s * V + t, msg
    assert "from node index %d to %d " % (s, t) in msg and "shorter than the table entry" in msg
    # 4. the pairwise loads, full lists of the large graph again
    counts = sparse_counts(big.num_vertices, 79, 300, diag=0)
    np.fill_diagonal(counts, 0)
    got, res = routes.link_loads(router, big, big_table, counts)
    assert np.array_equal(got, loads_from_trees(big_ref, big.num_edges, counts))
    assert res["num_pairs"] == int((counts != 0).sum())
    # 5. and its essential lists again
    assert_trees(routes.route_trees(router, big, big_table)[:4], big_ref)


# ---- 11. the other kernel paths --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain200", "bip10_140", "rand14_ties"])
def test_global_scratch_paths_and_wave_per_target(router, monkeypatch, name):
    """SRG_ROUTE_TREE_LDS_MAX_V=0 sends a small graph down the global-scratch doubling and push of a
    large one (V > 4096 / 8192), in several batches so that the scratch rows are indexed;
    SRG_ROUTE_TREE_GROUP=64 selects the wave-per-target predecessor kernel.  Same results."""
    e, lat, loss, table, ref = case(router, name)
    V = e.num_vertices
    counts = sparse_counts(V, 300 + V, 300)
    want, _ = R.link_loads(e, lat, loss, counts)
    base, bres = routes.link_loads_trees(router, e, table, counts)
    assert np.array_equal(base, want)
    for env, rows in ((("SRG_ROUTE_TREE_LDS_MAX_V", "0"), 0), (("SRG_ROUTE_TREE_LDS_MAX_V", "0"), 7),
                      (("SRG_ROUTE_TREE_GROUP", "64"), 0)):
        monkeypatch.setenv(*env)
        router.set_option(N.SRG_OPT_ROUTE_TREE_ROWS, rows)
        try:
            got = routes.route_trees(router, e, table)
            loads, res = routes.link_loads_trees(router, e, table, counts)
        finally:
            router.set_option(N.SRG_OPT_ROUTE_TREE_ROWS, 0)
            monkeypatch.delenv(env[0])
        assert_trees(got[:4], ref)
        assert got[4]["total_hops"] == int(ref[2].sum()) and got[4]["max_hops"] == int(ref[2].max())
        assert np.array_equal(loads, want)
        for k in ("num_pairs", "total_hops", "max_hops", "bad_pair"):
            assert res[k] == bres[k]
