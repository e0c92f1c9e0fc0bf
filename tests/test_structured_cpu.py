"""CPU: the structured graphs (tests/structured.py) have the shapes the GPU tests rely on, measured
with numpy from exact distances against the library's own limits, and the oracle agrees bit for bit
with an independent numpy evaluation of the loss recurrence on every one of them (the restatements
DESIGN.md §8 rests on had only ever agreed on shallow tight DAGs)."""
import numpy as np
import pytest

import oracle
import structured as S
from shadow_amd import _native as N
from helpers import bits_equal

LM_T, LM_E, MIRROR_STEPS, ROWS_MAX_V = N.loss_limits()

_shapes = {}


def shape(name):
    if name not in _shapes:
        _shapes[name] = S.Shape(S.graph(name))
    return _shapes[name]


def test_limits_accessor():
    """The accessor's values are limits a test can straddle (and the LDS bound is the documented one:
    12 B per vertex + the list, within 150 KiB)."""
    assert LM_T >= 2 and LM_E >= 2 and MIRROR_STEPS >= 2
    lds = lambda v: 12 * v + LM_T * (4 + 4 + LM_E * 8) + 16  # noqa: E731
    assert lds(ROWS_MAX_V) <= 150 * 1024 < lds(ROWS_MAX_V + 1)


@pytest.mark.parametrize("name", list(S.SMALL) + list(S.COMPOSITES) + list(S.LISTS))
def test_generator_contract(name):
    """One self-loop per vertex first, integer latencies >= 1, losses in [0, 1], connected."""
    e = S.graph(name)
    V = e.num_vertices
    assert np.array_equal(e.src[:V], np.arange(V)) and np.array_equal(e.dst[:V], np.arange(V))
    assert np.all(e.src[V:] != e.dst[V:]) and not e.directed
    assert np.all(e.latency_ns >= 1) and np.all((e.packet_loss >= 0) & (e.packet_loss <= 1))
    assert shape(name).D.max() < V * 4  # every pair reachable
    again = {**S.SMALL, **S.COMPOSITES, **S.LISTS}[name]()
    assert all(np.array_equal(getattr(e, k), getattr(again, k)) for k in ("src", "dst", "latency_ns", "packet_loss"))


def test_chain_is_deep_and_unique():
    sh = shape("chain384")
    assert max(sh.depth_min) == max(sh.depth_max) == 383 and sh.depth_min[0] == 383
    assert max(sh.indeg) == 1 and max(sh.multi) == 0
    assert max(sh.depth_min) > MIRROR_STEPS + 1  # walks of every length up to and past the step limit


def test_chain_chords_ties_all_along():
    sh = shape("chain_chords300")
    assert max(sh.depth_max) == 299  # the all-unit path is tight
    assert max(sh.depth_min) >= 99  # the fewest hops: chords of 3
    assert min(sh.multi) > 290 and max(sh.indeg) == 2
    assert min(sh.multi) > LM_T  # every row overflows the list: per-thread walks only


def test_grid_depth_and_ties():
    sh = shape("grid17")
    assert max(sh.depth_min) == max(sh.depth_max) == 32
    assert sh.multi[0] == 256 and max(sh.indeg) == 2 and min(sh.multi) >= 16 * 8 * 2


def test_bipartite_list_regimes():
    """The three regimes of k_loss_rows' multi-target list, against the library's limits."""
    sh = shape("bip10_12")  # list only: every row fits, every target's edges fit
    assert max(sh.multi) <= LM_T and min(sh.multi) >= 1 and max(sh.indeg) <= LM_E and min(sh.indeg) >= 2
    sh = shape("bip33_17")  # every row fits the list, and every row has a target whose edges do not
    assert max(sh.multi) <= LM_T and min(sh.indeg) > LM_E
    assert min(sh.multi) >= 1
    sh = shape("bip20_40")  # the a side: list rows whose targets all overflow LM_E; the b side: past LM_T
    a_side = [i for i in range(60) if sh.multi[i] <= LM_T and sh.indeg[i] > LM_E]
    assert a_side == list(range(20))
    assert all(sh.multi[i] > LM_T for i in range(20, 60))
    sh = shape("bip60_40")  # both limits exceeded in every row
    assert min(sh.multi) > LM_T and min(sh.indeg) > LM_E
    sh = shape("bip20_40_lossy")
    p = S.graph("bip20_40_lossy").packet_loss[60:]
    assert (p == 1.0).sum() > 100 and (p == 0.0).sum() > 100 and ((p > 0) & (p < 1)).sum() > 100
    assert sum(m <= LM_T and d > LM_E for m, d in zip(sh.multi, sh.indeg)) == 20


@pytest.mark.parametrize("name,rows_in_list,edges_over", [
    ("list_only", "all", False), ("edges_over_33_17", "all", True), ("edges_over_20_40", "some", True),
    ("both_over", "none", True), ("lossy", "some", True)])
def test_padded_list_regimes(name, rows_in_list, edges_over):
    """The padded graphs the GPU list tests run: more than one source block, the chain rows in the
    regime of the vertex they hang off, the bipartite rows unchanged."""
    sh = shape(name)
    V = len(sh.D)
    assert V > 128
    inlist = [m <= LM_T for m in sh.multi]
    assert min(sh.multi) >= 1
    assert {"all": all(inlist), "some": any(inlist) and not all(inlist), "none": not any(inlist)}[rows_in_list]
    if edges_over:  # a list row holds a target with more tight in-edges than a list entry stores
        assert all(d > LM_E for d in sh.indeg)
        if rows_in_list != "none":
            assert any(m <= LM_T and d > LM_E for m, d in zip(sh.multi, sh.indeg))
    else:
        assert max(sh.indeg) <= LM_E
    assert sh.multi[:120] == [sh.multi[120]] * 120  # chain rows: the multi targets of the vertex they reach


@pytest.mark.parametrize("name", list(S.COMPOSITES))
def test_composite_has_every_regime(name):
    sh = shape(name)
    V = len(sh.D)
    assert V >= 385  # four 128-blocks: mirrored rows below the diagonal in three of them
    assert max(sh.depth_min) > MIRROR_STEPS + 1 and max(sh.indeg) > LM_E
    assert min(sh.multi) > 0 and max(sh.multi) > LM_T


def test_composite_inorder_keeps_chain_order():
    e = S.graph("composite_inorder")
    V = e.num_vertices
    assert np.array_equal(e.src[V:V + 129], np.arange(129)) and np.array_equal(e.dst[V:V + 129], np.arange(1, 130))
    assert not np.array_equal(S.graph("composite").src, e.src)


def test_ring_chords_is_linear_in_memory():
    e = S.ring_chords(2000, 3, 9)
    assert e.num_edges == 2000 * 5 and np.all(e.src[2000:] != e.dst[2000:])
    assert np.all((e.latency_ns[2000:] >= 1) & (e.latency_ns[2000:] <= 4))
    lat, _ = oracle.compute_shortest_paths(e.as_tuple(), list(range(2000)), rows=[0], mode=2)
    assert lat[0, 1:].min() >= 1 and lat[0].max() < 2000  # connected


@pytest.mark.parametrize("name", list(S.SMALL) + list(S.COMPOSITES) + list(S.LISTS))
def test_oracle_equals_recurrence(name):
    """oracle (mode 0 whole table, mode 2 on a few rows) == the numpy recurrence, bit for bit."""
    e = S.graph(name)
    V = e.num_vertices
    sh = shape(name)
    lat, loss = S.recurrence_loss(e, sh)
    olat, oloss = oracle.compute_shortest_paths(e.as_tuple(), list(range(V)), mode=0)
    assert np.array_equal(olat, lat)
    bad = np.argwhere(oloss.view(np.uint32) != loss.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} pairs differ, first {bad[:4].tolist()}"
    rows = sorted({0, V // 2, V - 1})
    lat2, loss2 = oracle.compute_shortest_paths(e.as_tuple(), list(range(V)), rows=rows, mode=2)
    assert np.array_equal(lat2, lat[rows]) and bits_equal(loss2, loss[rows])


def test_shape_multi_pairs_matches_rowwise_count():
    sh = shape("bip10_12")
    assert sh.multi_pairs() == sum(sh.multi) == 10 * 9 + 12 * 11
    nodes = [3, 15, 0, 21]
    assert sh.multi_pairs(nodes) == 2 * 2  # rows 3 and 0 see target 0 / 3, rows 15 and 21 each other
