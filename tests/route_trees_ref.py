"""numpy restatement of the route trees (shadow_amd/csrc/route_trees.hip.h) -- a helper, not a test.

The tree of a source row comes from routes_ref.predecessors (every in-edge, no filter); hops and
first edges by following the predecessors vertex by vertex; loads by subtree sums in decreasing hop
order with Python integers clipped at 2^64 - 1.  Independent of the GPU code: plain numpy.
"""
import numpy as np

import routes_ref as R

NONE32 = 0xFFFFFFFF
U64_MAX = 2**64 - 1


def essential_arcs(e, lat):
    """routes_ref.arcs(e) filtered to the arcs u -> v with lat(edge) == lat[u, v]; also how many arcs
    lie below their entry."""
    ei, u, v = R.arcs(e)
    w = e.latency_ns[ei].astype(np.uint64)
    d = np.asarray(lat, dtype=np.uint64)[u, v]
    keep = w == d
    return (ei[keep], u[keep], v[keep]), int((w < d).sum())


def row_tree(e, lat, loss, s, A=None):
    """(pred_edge, pred_vertex, hops, first_edge) of source s as int64 [V]; R.NONE where there is none
    (the source's own column, an unexplained vertex and everything under it: hops -1 there)."""
    V = e.num_vertices
    pe, pu, _ = R.predecessors(e, lat, loss, s, A)
    pe[s], pu[s] = R.NONE, R.NONE
    hops = np.full(V, -1, dtype=np.int64)
    first = np.full(V, R.NONE, dtype=np.int64)
    hops[s] = 0
    for t in range(V):
        if hops[t] >= 0 or pe[t] == R.NONE:
            continue
        path, cur = [], t
        while hops[cur] < 0 and pe[cur] != R.NONE and len(path) <= V:
            path.append(cur)
            cur = int(pu[cur])
        if hops[cur] < 0:
            continue  # ends at an unexplained vertex
        for x in reversed(path):
            p = int(pu[x])
            hops[x] = hops[p] + 1
            first[x] = pe[x] if p == s else first[p]
    return pe, pu, hops, first


def trees(e, lat, loss, sources=None, A=None):
    """The four u32 arrays [len(sources), V] as the library returns them (NONE32 / 0 in the source's
    column) and the list of unexplained (row, t).  Hops of an unexplained entry: 0."""
    V = e.num_vertices
    sources = np.arange(V) if sources is None else np.asarray(sources, dtype=np.int64)
    A = A if A is not None else R.arcs(e)
    out = [np.zeros((len(sources), V), dtype=np.uint32) for _ in range(4)]
    bad = []
    for i, s in enumerate(sources):
        pe, pu, hops, first = row_tree(e, lat, loss, int(s), A)
        bad += [(i, int(t)) for t in np.flatnonzero(hops < 0)]
        for o, a in zip(out, (pe, pu, hops, first)):
            o[i] = np.where(a < 0, 0 if a is hops else NONE32, a).astype(np.uint32)
    return out[0], out[1], out[2], out[3], bad


def link_loads(e, lat, loss, counts, loads=None, A=None):
    """counts u64 [V, V]; per-edge loads (u64, saturating) added onto `loads`, by subtree sums.
    Returns (loads, dict(num_pairs, total_hops, max_hops))."""
    V = e.num_vertices
    counts = np.asarray(counts, dtype=np.uint64).reshape(V, V)
    out = [0] * e.num_edges if loads is None else [int(x) for x in loads]
    selfe = R.self_edges(e)
    A = A if A is not None else R.arcs(e)
    total, hmax = 0, 0
    for s in np.flatnonzero((counts != 0).any(axis=1)):
        pe, pu, hops, _ = row_tree(e, lat, loss, int(s), A)
        sub = [int(x) for x in counts[s]]
        if sub[s]:
            assert selfe[s] != R.NONE
            out[selfe[s]] = min(out[selfe[s]] + sub[s], U64_MAX)
            total, hmax = total + 1, max(hmax, 1)
            sub[s] = 0
        nz = np.flatnonzero(counts[s] != 0)
        nz = nz[nz != s]
        assert (hops[nz] > 0).all(), "a nonzero pair is unexplained"
        total += int(hops[nz].sum())
        hmax = max(hmax, int(hops[nz].max()) if len(nz) else 0)
        for t in np.argsort(-hops, kind="stable"):
            if hops[t] <= 0 or sub[t] == 0:
                continue
            out[pe[t]] = min(out[pe[t]] + sub[t], U64_MAX)
            if pu[t] != s:
                sub[pu[t]] = min(sub[pu[t]] + sub[t], U64_MAX)
    return np.array(out, dtype=np.uint64), dict(num_pairs=int((counts != 0).sum()), total_hops=total, max_hops=hmax)
