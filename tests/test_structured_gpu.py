"""GPU: the structured graphs (tests/structured.py; their shapes are asserted in
test_structured_cpu.py) through every loss pass and scan of the dense build and through the sparse
algorithm, whole tables bit for bit against the oracle.  What each case reaches is proved by the
build's own report: SRG_OPT_LOSS_KIND (which loss pass ran), SRG_OPT_SCAN_MIRRORED, stats."""
import contextlib

import numpy as np
import pytest

import oracle
import structured as S
from shadow_amd import Router, synth
from shadow_amd import _native as N
from shadow_amd.graph import Edges
from helpers import bits_equal

pytestmark = pytest.mark.gpu

BIG = 1 << 30  # SRG_OPT_SCAN_MIRROR_CAP: as many pairs as the packed rows leave room for
SPARSE_KINDS = (N.SRG_PATH_SPARSE_U32, N.SRG_PATH_SPARSE_U64)


@pytest.fixture(scope="module")
def rt():
    r = Router(0)
    yield r
    r.close()


@contextlib.contextmanager
def options(rt, **opts):
    """Set SRG_OPT_<name> for the block, then put the previous values back."""
    old = {k: rt.get_option(getattr(N, "SRG_OPT_" + k)) for k in opts}
    for k, v in opts.items():
        rt.set_option(getattr(N, "SRG_OPT_" + k), v)
    try:
        yield
    finally:
        for k, v in old.items():
            rt.set_option(getattr(N, "SRG_OPT_" + k), v)


def host(rt, e, nodes=None):
    """Host entry -> (latency, loss, stats, loss kind, mirrored)."""
    nodes = list(range(e.num_vertices)) if nodes is None else nodes
    t = rt.compute_shortest_paths(e, nodes)
    return (t.latency_ns, t.packet_loss, t.stats, int(rt.get_option(N.SRG_OPT_LOSS_KIND)),
            int(rt.get_option(N.SRG_OPT_SCAN_MIRRORED)))


def device(rt, e, nodes=None):
    """Device entry -> the same tuple."""
    import torch
    from shadow_amd.device import DeviceGraph, compute_shortest_paths_device
    nodes = list(range(e.num_vertices)) if nodes is None else nodes
    n = len(nodes)
    nt = torch.tensor(nodes, dtype=torch.int32, device="cuda:0")
    ol = torch.empty((n, n), dtype=torch.int64, device="cuda:0")
    os_ = torch.empty((n, n), dtype=torch.float32, device="cuda:0")
    st = compute_shortest_paths_device(rt, DeviceGraph(e), nt, ol, os_)
    kind, mirrored = int(rt.get_option(N.SRG_OPT_LOSS_KIND)), int(rt.get_option(N.SRG_OPT_SCAN_MIRRORED))
    torch.cuda.synchronize()
    return ol.cpu().numpy().view(np.uint64), os_.cpu().numpy(), st, kind, mirrored


def exact(got, want):
    """assert_parity's semantics: latency equal, loss bit-equal, whole table."""
    assert np.array_equal(got[0], want[0]), "latency_ns must be bit-exact"
    bad = np.argwhere(np.asarray(got[1]).view(np.uint32) != np.asarray(want[1]).view(np.uint32))
    assert len(bad) == 0, f"packet_loss differs at {len(bad)} pairs, first {bad[:4].tolist()}"


_ref, _multi = {}, {}


def ref(name):
    """The oracle's whole table of a named graph (computed once, never changed)."""
    if name not in _ref:
        e = S.graph(name)
        _ref[name] = oracle.compute_shortest_paths(e.as_tuple(), list(range(e.num_vertices)))
    return _ref[name]


def multi_pairs(name):
    if name not in _multi:
        _multi[name] = S.Shape(S.graph(name), depth=False).multi_pairs()
    return _multi[name]


ALL_SMALL = list(S.SMALL) + list(S.COMPOSITES)

# ---- 1. every structured graph, every configuration --------------------------------------------

CONFIGS = {
    # name: (options, expected loss kind, mirrored values allowed, entries)
    "sparse_scan": (dict(SPARSE_THRESHOLD=1.0, SCAN_MIRROR=0), N.SRG_LOSS_ROWS_LDS, (0,), (host,)),
    "mirror_big_cap": (dict(SPARSE_THRESHOLD=1.0, SCAN_MIRROR=1, SCAN_MIRROR_CAP=BIG), N.SRG_LOSS_ROWS_LDS, (1,),
                       (host, device)),
    "mirror_default_cap": (dict(SPARSE_THRESHOLD=1.0, SCAN_MIRROR=1, SCAN_MIRROR_CAP=0), N.SRG_LOSS_ROWS_LDS, (1, 2),
                           (host, device)),
    "dense_scan": (dict(SPARSE_THRESHOLD=0.0), N.SRG_LOSS_DENSE_SCAN, (0,), (host,)),
}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ALL_SMALL)
def test_dense_algorithm_configurations(rt, name, config):
    opts, kind, mirrored_ok, entries = CONFIGS[config]
    e = S.graph(name)
    with options(rt, ALGORITHM=N.SRG_ALGO_DENSE, **opts):
        for entry in entries:
            lat, loss, st, k, m = entry(rt, e)
            assert st["path_kind"] == N.SRG_PATH_DENSE_U32
            assert st["scan_kind"] == (N.SRG_SCAN_DENSE if config == "dense_scan" else N.SRG_SCAN_SPARSE)
            assert k == kind and m in mirrored_ok, (entry.__name__, k, m)
            exact((lat, loss), ref(name))
            # the same count whichever scan found the pairs
            assert st["multi_pred_pairs"] == multi_pairs(name), entry.__name__


@pytest.mark.parametrize("name", ALL_SMALL)
def test_sparse_algorithm(rt, name):
    e = S.graph(name)
    with options(rt, ALGORITHM=N.SRG_ALGO_SPARSE):
        lat, loss, st, k, m = host(rt, e)
    assert st["path_kind"] in SPARSE_KINDS and k == N.SRG_LOSS_NONE and m == 0
    exact((lat, loss), ref(name))


# ---- 2. the mirrored walk's step limit -----------------------------------------------------------

def test_mirror_step_limit(rt):
    """A chain in index order: the mirrored walk from t back to s takes t - s steps, so the pairs
    below the diagonal have walks of every length; t - s = MIRROR_STEPS is the longest the walk
    decides, MIRROR_STEPS + 1 the shortest that gives up and goes to the exact-key worklist."""
    steps = N.loss_limits()[2]
    V = max(400, 2 * steps + 130)
    e = S.chain(V, seed=21)
    want = oracle.compute_shortest_paths(e.as_tuple(), list(range(V)))
    # (t, s) with s in a lower 128-block than t, by name
    named = [(s + d, s) for s in (127, 128 + 100, 255) for d in (steps - 1, steps, steps + 1)]
    assert all(s // 128 < t // 128 and t < V for t, s in named)
    for cap, allowed in ((BIG, (1,)), (0, (1, 2))):
        with options(rt, ALGORITHM=N.SRG_ALGO_DENSE, SPARSE_THRESHOLD=1.0, SCAN_MIRROR=1, SCAN_MIRROR_CAP=cap):
            for entry in (host, device):
                lat, loss, st, k, m = entry(rt, e)
                assert m in allowed and k == N.SRG_LOSS_ROWS_LDS, (cap, entry.__name__, m, k)
                for t, s in named:
                    assert lat[t, s] == want[0][t, s] == t - s, (t, s)
                    assert loss[t, s].view(np.uint32) == want[1][t, s].view(np.uint32), (t, s, cap, entry.__name__)
                exact((lat, loss), want)
                assert st["multi_pred_pairs"] == 0


# ---- 3. the loss rows' multi-target list ---------------------------------------------------------

@pytest.mark.parametrize("name", list(S.LISTS))
def test_list_regimes_are_exact_and_repeatable(rt, name):
    """The list's slots are handed out by atomicAdd in arrival order: three runs of each entry must
    give the same bytes, and the oracle's."""
    e = S.graph(name)
    for mirror, entry in ((0, host), (1, host), (1, device)):
        with options(rt, ALGORITHM=N.SRG_ALGO_DENSE, SPARSE_THRESHOLD=1.0, SCAN_MIRROR=mirror, SCAN_MIRROR_CAP=BIG):
            runs = [entry(rt, e) for _ in range(3)]
        for lat, loss, st, k, m in runs:
            assert k == N.SRG_LOSS_ROWS_LDS and m == mirror
            assert st["multi_pred_pairs"] == multi_pairs(name)
            exact((lat, loss), ref(name))
        assert all(r[1].tobytes() == runs[0][1].tobytes() for r in runs[1:])


# ---- 4. depth: the two Jacobi folds --------------------------------------------------------------

@pytest.mark.parametrize("fold", ["dense_scan", "global_entries"])
@pytest.mark.parametrize("name", ["chain384", "chain_chords300", "grid17"])
def test_jacobi_rounds_reach_the_depth(rt, monkeypatch, name, fold):
    """A Jacobi round moves every value one hop, so the fold cannot have finished before the round
    that first reaches the row's farthest target (its fewest-hop depth in the tight DAG; the longest
    tight path is no bound, a cheaper path with fewer hops settles a target earlier), and it must
    stop within the V + 2 rounds the host loop allows."""
    e = S.graph(name)
    V = e.num_vertices
    depth = max(S.Shape(e, rows=[0, V // 2, V - 1]).depth_min)
    assert depth >= 32
    if fold == "global_entries":
        monkeypatch.setenv("SRG_LOSS_ROWS_MAX_V", "64")
    thr = 0.0 if fold == "dense_scan" else 1.0
    with options(rt, ALGORITHM=N.SRG_ALGO_DENSE, SPARSE_THRESHOLD=thr):
        lat, loss, st, k, m = host(rt, e)
    assert k == (N.SRG_LOSS_DENSE_SCAN if fold == "dense_scan" else N.SRG_LOSS_GLOBAL_ENTRIES)
    exact((lat, loss), ref(name))
    assert depth <= st["loss_rounds"] <= V + 2, st["loss_rounds"]


# ---- 5. the global-memory fold, forced at small V ------------------------------------------------

def forced(rt, e, want, nodes=None, kind=N.SRG_LOSS_GLOBAL_ENTRIES, path=N.SRG_PATH_DENSE_U32, mirrored=0):
    """Both entries with the mirror switched on: the global fold must switch it off by itself."""
    with options(rt, ALGORITHM=N.SRG_ALGO_DENSE, SPARSE_THRESHOLD=1.0, SCAN_MIRROR=1, SCAN_MIRROR_CAP=BIG):
        for entry in (host, device):
            lat, loss, st, k, m = entry(rt, e, nodes)
            assert (k, m) == (kind, mirrored), (entry.__name__, k, m)
            assert st["path_kind"] == path and st["scan_kind"] == N.SRG_SCAN_SPARSE
            exact((lat, loss), want)
    return st


@pytest.mark.parametrize("name", ALL_SMALL + list(S.LISTS))
def test_forced_global_fold_structured(rt, monkeypatch, name):
    """SRG_LOSS_ROWS_MAX_V=64: every graph above 64 vertices folds in global memory (and is not
    mirrored); the three below keep the LDS fold, the switch being 'V <= n'."""
    monkeypatch.setenv("SRG_LOSS_ROWS_MAX_V", "64")
    e = S.graph(name)
    small = e.num_vertices <= 64
    st = forced(rt, e, ref(name), kind=N.SRG_LOSS_ROWS_LDS if small else N.SRG_LOSS_GLOBAL_ENTRIES,
                mirrored=1 if small else 0)
    assert st["multi_pred_pairs"] == multi_pairs(name)


def test_forced_limit_is_v_le_n_and_only_lowers(rt, monkeypatch):
    e = S.graph("bip20_40")  # 60 vertices
    for n, kind in (("59", N.SRG_LOSS_GLOBAL_ENTRIES), ("60", N.SRG_LOSS_ROWS_LDS), ("0", N.SRG_LOSS_GLOBAL_ENTRIES),
                    (str(10 ** 9), N.SRG_LOSS_ROWS_LDS), ("", N.SRG_LOSS_ROWS_LDS), ("x", N.SRG_LOSS_ROWS_LDS)):
        monkeypatch.setenv("SRG_LOSS_ROWS_MAX_V", n)
        with options(rt, ALGORITHM=N.SRG_ALGO_DENSE, SPARSE_THRESHOLD=1.0):
            lat, loss, st, k, m = host(rt, e)
        assert k == kind, (n, k)
        exact((lat, loss), ref("bip20_40"))


RANDOM = {
    "ties": lambda: synth.random_graph(300, 0.1, 4242, lat_hi=6, parallel=0.2),
    "atlas": lambda: synth.atlas_like(300, seed=1300),
    "directed": lambda: synth.random_graph(300, 0.1, 4243, directed=True, lat_hi=50),
}


@pytest.mark.parametrize("name", list(RANDOM))
def test_forced_global_fold_random(rt, monkeypatch, name):
    monkeypatch.setenv("SRG_LOSS_ROWS_MAX_V", "64")
    e = RANDOM[name]()
    want = oracle.compute_shortest_paths(e.as_tuple(), list(range(300)))
    forced(rt, e, want)


def test_forced_global_fold_node_subset(rt, monkeypatch):
    """77 of 391 vertices in scrambled order: rows and columns are gathered through the node list."""
    monkeypatch.setenv("SRG_LOSS_ROWS_MAX_V", "64")
    e = S.graph("composite")
    V = e.num_vertices
    nodes = np.random.default_rng(77).permutation(V)[:77].tolist()
    full = ref("composite")
    want = (full[0][np.ix_(nodes, nodes)], full[1][np.ix_(nodes, nodes)])
    direct = oracle.compute_shortest_paths(e.as_tuple(), nodes)
    assert np.array_equal(direct[0], want[0]) and bits_equal(direct[1], want[1])
    st = forced(rt, e, want, nodes=nodes)
    assert st["multi_pred_pairs"] > 0


def test_forced_global_fold_u64_keys(rt, monkeypatch):
    """Nanosecond keys that are multiples of 2^32: the scan runs on the keys' low words, which are all
    zero, so it is the fold's comparison of the whole u64 keys that tells a tight edge from a loose one."""
    monkeypatch.setenv("SRG_LOSS_ROWS_MAX_V", "64")
    monkeypatch.setenv("SRG_LATENCY_UNIT", "1")
    g = S.graph("composite")
    e = Edges(g.num_vertices, g.src, g.dst, g.latency_ns * np.uint64(2 ** 32), g.packet_loss, directed=False)
    full = ref("composite")
    want_lat = full[0] * np.uint64(2 ** 32)
    assert np.array_equal(oracle.compute_shortest_paths(e.as_tuple(), list(range(g.num_vertices)), rows=[5])[0][0],
                          want_lat[5])
    st = forced(rt, e, (want_lat, full[1]), path=N.SRG_PATH_DENSE_U64)
    # every low word is zero here, so the scan sees a tie wherever a target has two essential
    # in-edges and the fold's exact-key check decides all of them: the count is an upper bound
    assert st["multi_pred_pairs"] >= multi_pairs("composite")


def test_forced_global_fold_large_host_table(rt, monkeypatch):
    """A 2501-vertex table, which the host entry normally ships group by group beside the scan: with
    the global fold every row must still arrive -- the device entry's bytes, and the oracle's rows."""
    monkeypatch.setenv("SRG_LOSS_ROWS_MAX_V", "64")
    V = 2501
    e = synth.random_graph(V, 0.02, 4244, lat_hi=6, parallel=0.1)
    rows = [0, 1, 1024, 2047, 2048, V - 1]
    want = oracle.compute_shortest_paths(e.as_tuple(), list(range(V)), rows=rows, mode=2)
    with options(rt, ALGORITHM=N.SRG_ALGO_DENSE, SPARSE_THRESHOLD=1.0, SCAN_MIRROR=1):
        hl, hs, hst, hk, hm = host(rt, e)
        dl, ds, dst, dk, dm = device(rt, e)
    assert (hk, hm, dk, dm) == (N.SRG_LOSS_GLOBAL_ENTRIES, 0, N.SRG_LOSS_GLOBAL_ENTRIES, 0)
    assert hl.tobytes() == dl.tobytes() and hs.tobytes() == ds.tobytes()
    exact((hl[rows], hs[rows]), want)
    assert hst["multi_pred_pairs"] == dst["multi_pred_pairs"] > 0
    assert hst["loss_rounds"] == dst["loss_rounds"]


# ---- 6. the unforced threshold -------------------------------------------------------------------

@pytest.mark.parametrize("over", [1, 0], ids=["too_long_for_lds", "longest_lds_row"])
def test_lds_threshold_unforced(rt, monkeypatch, over):
    """The smallest V whose loss rows do not fit LDS (from the library's limits) folds in global
    memory with no switch set; one vertex fewer is the longest row the LDS fold ever takes."""
    monkeypatch.delenv("SRG_LOSS_ROWS_MAX_V", raising=False)
    V = N.loss_limits()[3] + over
    e = S.ring_chords(V, 3, 31)
    nodes = np.random.default_rng(32).permutation(V)[:200].tolist()
    want = oracle.compute_shortest_paths(e.as_tuple(), nodes)
    with options(rt, ALGORITHM=N.SRG_ALGO_DENSE):
        for entry in (host, device):
            lat, loss, st, k, m = entry(rt, e, nodes)
            assert k == (N.SRG_LOSS_GLOBAL_ENTRIES if over else N.SRG_LOSS_ROWS_LDS), (entry.__name__, k)
            assert st["path_kind"] == N.SRG_PATH_DENSE_U32 and st["scan_kind"] == N.SRG_SCAN_SPARSE
            assert st["multi_pred_pairs"] > 0
            exact((lat, loss), want)


# ---- 7. the sparse algorithm at depth ------------------------------------------------------------

@pytest.mark.parametrize("bitmaps", [0, 1])
@pytest.mark.parametrize("div", [0, 1, 16])
@pytest.mark.parametrize("gen", ["chain", "chain_chords"])
def test_sparse_algorithm_depth(rt, gen, div, bitmaps):
    """Thin graphs of 2100 vertices take the sparse algorithm by themselves; its fold has 2099 hops
    to cover (chords: ties all the way), in one bucket, the default buckets and narrow ones."""
    V = 2100
    e, want, sub, want_sub = deep(gen)
    with options(rt, ALGORITHM=N.SRG_ALGO_AUTO, SPARSE_DELTA_DIV=div, SPARSE_GLOBAL_BITMAPS=bitmaps):
        lat, loss, st, k, m = host(rt, e)
        assert st["path_kind"] in SPARSE_KINDS and k == N.SRG_LOSS_NONE
        rows = [0, V // 2, V - 1]
        exact((lat[rows], loss[rows]), want)
        lat, loss, st, k, m = host(rt, e, sub)
        assert st["path_kind"] in SPARSE_KINDS
        exact((lat, loss), want_sub)


_deep = {}


def deep(gen):
    if gen not in _deep:
        V = 2100
        e = S.chain(V, seed=41) if gen == "chain" else S.chain_chords(V, 3, seed=42)
        want = oracle.compute_shortest_paths(e.as_tuple(), list(range(V)), rows=[0, V // 2, V - 1], mode=2)
        sub = np.random.default_rng(43).permutation(V)[:64].tolist()
        _deep[gen] = (e, want, sub, oracle.compute_shortest_paths(e.as_tuple(), sub))
    return _deep[gen]
