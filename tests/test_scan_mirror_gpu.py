"""GPU: the triangular tight scan with mirrored pairs (SRG_OPT_SCAN_MIRROR) against
the full scan and the oracle, bit for bit on latency and loss; multi_pred_pairs unchanged; the
worklist-overflow rerun; and the builds that must not mirror."""
import ctypes
import threading

import numpy as np
import pytest

import oracle
from shadow_amd import LocalGroup, Router, synth
from shadow_amd import _native as N
from shadow_amd.graph import Edges
from helpers import bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    r = Router(0)
    r.set_option(N.SRG_OPT_SPARSE_THRESHOLD, 1.0)  # the essential-entry scan on every graph here
    yield r
    r.close()


def host(rt, e, nodes, mirror, **opts):
    """Host entry -> (table, SRG_OPT_SCAN_MIRRORED of the build)."""
    rt.set_option(N.SRG_OPT_SCAN_MIRROR, mirror)
    for k, v in opts.items():
        rt.set_option(getattr(N, "SRG_OPT_" + k), v)
    try:
        t = rt.compute_shortest_paths(e, nodes)
        return t, int(rt.get_option(N.SRG_OPT_SCAN_MIRRORED))
    finally:
        rt.set_option(N.SRG_OPT_SCAN_MIRROR, 1)
        for k in opts:
            rt.set_option(getattr(N, "SRG_OPT_" + k), 0)


def device(rt, e, mirror):
    """Device entry, every vertex in order -> (latency, loss, stats, mirrored)."""
    import torch
    from shadow_amd.device import DeviceGraph, compute_shortest_paths_device
    V = e.num_vertices
    dg = DeviceGraph(e)
    nodes = torch.arange(V, dtype=torch.int32, device="cuda:0")
    ol = torch.empty((V, V), dtype=torch.int64, device="cuda:0")
    os_ = torch.empty((V, V), dtype=torch.float32, device="cuda:0")
    rt.set_option(N.SRG_OPT_SCAN_MIRROR, mirror)
    try:
        st = compute_shortest_paths_device(rt, dg, nodes, ol, os_)
        mirrored = int(rt.get_option(N.SRG_OPT_SCAN_MIRRORED))
    finally:
        rt.set_option(N.SRG_OPT_SCAN_MIRROR, 1)
    torch.cuda.synchronize()
    return ol.cpu().numpy().view(np.uint64), os_.cpu().numpy(), st, mirrored


def same(t, lat, loss):
    return np.array_equal(t.latency_ns, lat) and bits_equal(t.packet_loss, loss)


def cut_tri(q, ng, nb):
    """The library's own scan_group_cut_tri (plan.h), as run_dense calls it."""
    f = N.lib().srg_internal_scan_group_cut_tri
    f.restype = ctypes.c_uint32
    f.argtypes = [ctypes.c_uint32] * 3
    return int(f(q, ng, nb))


@pytest.mark.parametrize("V", [100, 129, 300, 384])
def test_mirror_equals_full_scan_and_oracle(rt, V):
    """One source block (nothing to mirror), the second block of one row, three blocks partial and
    exact; both entries."""
    e = synth.atlas_like(V, seed=1000 + V)
    nodes = list(range(V))
    lat, loss = oracle.compute_shortest_paths(e.as_tuple(), nodes)
    t1, m1 = host(rt, e, nodes, 1)
    t0, m0 = host(rt, e, nodes, 0)
    assert (m1, m0) == (1, 0)
    assert t1.stats["scan_kind"] == N.SRG_SCAN_SPARSE
    assert same(t1, lat, loss) and same(t0, lat, loss)
    assert t1.stats["multi_pred_pairs"] == t0.stats["multi_pred_pairs"]
    assert t1.stats["loss_rounds"] == t0.stats["loss_rounds"]
    dl1, ds1, st1, dm1 = device(rt, e, 1)
    dl0, ds0, st0, dm0 = device(rt, e, 0)
    assert (dm1, dm0) == (1, 0)
    assert np.array_equal(dl1, lat) and bits_equal(ds1, loss)
    assert np.array_equal(dl0, lat) and bits_equal(ds0, loss)
    assert st1["multi_pred_pairs"] == st0["multi_pred_pairs"] == t0.stats["multi_pred_pairs"]


@pytest.mark.parametrize("V", [2049, 2501])
def test_host_entry_scan_groups(rt, V):
    """Host entry in scan groups.  2049 vertices = 17 source blocks is the smallest size at which
    scan_group_cut_tri yields three non-empty groups (8 / 8 / 1 blocks; in three groups as in the
    mirrored build's default four, whose third is empty there); its 50 MB table is below the size
    from which the host entry ships rows group by group, so 2501 vertices (20 blocks: 8 / 8 / 4) is
    the case whose groups are launched one by one."""
    nb = (V + 127) // 128

    def groups(ng, blocks):
        c = [cut_tri(q, ng, blocks) for q in range(ng + 1)]
        assert c[0] == 0 and c[-1] == blocks and c == sorted(c)
        return [(a, z) for a, z in zip(c, c[1:]) if z > a]

    for ng in (3, 4):
        assert groups(ng, nb) == [(0, 8), (8, 16), (16, nb)]
        for smaller in range(1, 17):
            assert len(groups(ng, smaller)) < 3
    e = synth.atlas_like(V, seed=V)
    nodes = list(range(V))
    rows = sorted({0, 127, 128, 1023, 1024, 1025, 2047, 2048, V - 1})
    lat, loss = oracle.compute_shortest_paths(e.as_tuple(), nodes, rows=rows, mode=2)
    t1, m1 = host(rt, e, nodes, 1)
    assert m1 == 1
    if V == 2501:  # every row left while later groups scanned
        assert t1.stats["d2h_overlapped_bytes"] == V * V * (8 if t1.stats["d2h_key_rows"] else 12)
    assert np.array_equal(t1.latency_ns[rows], lat) and bits_equal(t1.packet_loss[rows], loss)
    t0, m0 = host(rt, e, nodes, 0)
    assert m0 == 0
    assert same(t1, t0.latency_ns, t0.packet_loss)
    assert t1.stats["multi_pred_pairs"] == t0.stats["multi_pred_pairs"]


def tie_graph():
    # small integer latencies and parallel edges: thousands of pairs with several tight predecessors
    return synth.random_graph(300, 0.1, 4242, lat_hi=6, parallel=0.2)


BIG = 1 << 30  # SRG_OPT_SCAN_MIRROR_CAP: as many pairs as the packed rows leave room for


def test_ties(rt):
    """Thousands of pairs decided by k_mirror_slow (a worklist with room for them), both entries."""
    e = tie_graph()
    nodes = list(range(300))
    lat, loss = oracle.compute_shortest_paths(e.as_tuple(), nodes)
    t0, m0 = host(rt, e, nodes, 0)
    t1, m1 = host(rt, e, nodes, 1, SCAN_MIRROR_CAP=BIG)
    assert (m1, m0) == (1, 0)
    assert same(t1, lat, loss) and same(t0, lat, loss)
    assert t0.stats["multi_pred_pairs"] > 1000
    assert t1.stats["multi_pred_pairs"] == t0.stats["multi_pred_pairs"]
    rt.set_option(N.SRG_OPT_SCAN_MIRROR_CAP, BIG)
    try:
        dl1, ds1, st1, dm1 = device(rt, e, 1)
    finally:
        rt.set_option(N.SRG_OPT_SCAN_MIRROR_CAP, 0)
    assert dm1 == 1 and np.array_equal(dl1, lat) and bits_equal(ds1, loss)
    assert st1["multi_pred_pairs"] == t0.stats["multi_pred_pairs"]
    # the default worklist (1 / 1024 of the pairs, at least 256) is far too small for this graph:
    # full scan after the mirrored pass, same table
    t2, m2 = host(rt, e, nodes, 1)
    assert m2 == 2 and same(t2, lat, loss)
    assert t2.stats["multi_pred_pairs"] == t0.stats["multi_pred_pairs"]


def test_ties_worklist_overflow_reruns(rt):
    """A worklist of 4 pairs overflows on the tie graph: the build scans again in full (reported
    as 2) and is still exact, multi_pred_pairs included."""
    e = tie_graph()
    nodes = list(range(300))
    lat, loss = oracle.compute_shortest_paths(e.as_tuple(), nodes)
    t0, _ = host(rt, e, nodes, 0)
    t2, m2 = host(rt, e, nodes, 1, SCAN_MIRROR_CAP=4)
    assert m2 == 2
    assert same(t2, lat, loss)
    assert t2.stats["multi_pred_pairs"] == t0.stats["multi_pred_pairs"]
    assert t2.stats["loss_rounds"] == t0.stats["loss_rounds"]


def test_overflow_rerun_reships_grouped_rows(rt):
    """The rerun on a table large enough for the host entry to ship loss rows group by group: the
    mirrored pass's rows have left (or are leaving) when the overflow is seen; every row is folded
    and shipped again, and the table equals the full scan's and the oracle's rows."""
    V = 2501
    e = synth.random_graph(V, 0.02, 4244, lat_hi=6, parallel=0.1)
    nodes = list(range(V))
    rows = [0, 1, 1024, 2047, 2048, V - 1]
    lat, loss = oracle.compute_shortest_paths(e.as_tuple(), nodes, rows=rows, mode=2)
    dense = dict(ALGORITHM=N.SRG_ALGO_DENSE)  # (a graph this thin would take the Bellman-Ford path)
    t0, m0 = host(rt, e, nodes, 0, **dense)
    t2, m2 = host(rt, e, nodes, 1, SCAN_MIRROR_CAP=4, **dense)
    assert t0.stats["path_kind"] == t2.stats["path_kind"] == N.SRG_PATH_DENSE_U32
    assert (m0, m2) == (0, 2)
    assert t2.stats["d2h_overlapped_bytes"] >= V * V * 8  # rows left while kernels ran
    assert np.array_equal(t0.latency_ns[rows], lat) and bits_equal(t0.packet_loss[rows], loss)
    assert same(t2, t0.latency_ns, t0.packet_loss)
    assert t2.stats["multi_pred_pairs"] == t0.stats["multi_pred_pairs"] > 0
    # the default worklist overflows as well; the interleaved rerun reports this pass's loss_rounds
    t1, m1 = host(rt, e, nodes, 1, **dense)
    assert m1 == 2 and same(t1, t0.latency_ns, t0.packet_loss)
    assert t1.stats["multi_pred_pairs"] == t0.stats["multi_pred_pairs"]
    assert t1.stats["loss_rounds"] == t2.stats["loss_rounds"] == t0.stats["loss_rounds"]


def test_not_mirrored_directed(rt):
    e = synth.random_graph(300, 0.1, 4243, directed=True, lat_hi=50)
    nodes = list(range(300))
    lat, loss = oracle.compute_shortest_paths(e.as_tuple(), nodes)
    t, m = host(rt, e, nodes, 1)
    assert m == 0 and t.stats["scan_kind"] == N.SRG_SCAN_SPARSE and same(t, lat, loss)


@pytest.mark.parametrize("kind", ["subset", "permuted"])
def test_not_mirrored_node_lists(rt, kind):
    V = 300
    e = synth.atlas_like(V, seed=1300)
    rng = np.random.default_rng(7)
    nodes = sorted(rng.choice(V, size=200, replace=False).tolist()) if kind == "subset" else rng.permutation(V).tolist()
    lat, loss = oracle.compute_shortest_paths(e.as_tuple(), nodes)
    t, m = host(rt, e, nodes, 1)
    assert m == 0 and t.stats["scan_kind"] == N.SRG_SCAN_SPARSE and same(t, lat, loss)


def test_not_mirrored_two_ranks():
    V, G = 300, 2
    e = synth.atlas_like(V, seed=1300)
    nodes = list(range(V))
    lat, loss = oracle.compute_shortest_paths(e.as_tuple(), nodes)
    group = LocalGroup(G)
    routers = [Router(0) for _ in range(G)]
    for r, x in enumerate(routers):
        x.init_comm_local(group, r)
        x.set_option(N.SRG_OPT_SPARSE_THRESHOLD, 1.0)
    out, errs = [None] * G, [None] * G

    def work(r):
        try:
            out[r] = routers[r].compute_shortest_paths(e, nodes)
        except Exception as ex:  # noqa: BLE001
            errs[r] = ex

    th = [threading.Thread(target=work, args=(r,)) for r in range(G)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    try:
        assert errs == [None] * G
        for r in range(G):
            assert int(routers[r].get_option(N.SRG_OPT_SCAN_MIRRORED)) == 0
            assert out[r].stats["scan_kind"] == N.SRG_SCAN_SPARSE and same(out[r], lat, loss)
    finally:
        for x in routers:
            x.close()
        group.close()


def test_not_mirrored_u64_keys(rt, monkeypatch):
    """Nanosecond keys (SRG_LATENCY_UNIT=1) past u32: the scan runs on the keys' low words."""
    monkeypatch.setenv("SRG_LATENCY_UNIT", "1")
    g = synth.random_graph(300, 0.08, 37, lat_lo=1, lat_hi=6, parallel=0.1)
    lat_ns = g.latency_ns.astype(np.uint64) * np.uint64(2 ** 32) + np.uint64(1)
    e = Edges(g.num_vertices, g.src, g.dst, lat_ns, g.packet_loss, directed=False)
    nodes = list(range(300))
    lat, loss = oracle.compute_shortest_paths(e.as_tuple(), nodes)
    t, m = host(rt, e, nodes, 1)
    assert t.stats["path_kind"] == N.SRG_PATH_DENSE_U64 and t.stats["scan_kind"] == N.SRG_SCAN_SPARSE
    assert m == 0 and same(t, lat, loss)


def test_switch_is_an_option(rt):
    assert rt.get_option(N.SRG_OPT_SCAN_MIRROR) == 1
    rt.set_option(N.SRG_OPT_SCAN_MIRROR, 0)
    assert rt.get_option(N.SRG_OPT_SCAN_MIRROR) == 0
    rt.set_option(N.SRG_OPT_SCAN_MIRROR, 1)
    from shadow_amd import NetGraphError
    with pytest.raises(NetGraphError):
        rt.set_option(N.SRG_OPT_SCAN_MIRRORED, 1)  # read-only
