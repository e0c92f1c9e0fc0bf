"""Structured graphs for the loss pass and the mirrored scan, and the numpy analysis that says which
branch of those kernels a graph reaches (plain numpy, seeded; no GPU).

The random and Atlas-like graphs of the other tests have tight-predecessor DAGs of depth <= 5 and
rows with either no multi-predecessor target or far more than the loss rows' list holds.  The
graphs here vary exactly those quantities: depth (chain, grid), tie width (bipartite, grid, chords)
and the number of multi-predecessor targets per row (bipartite sides).

Every generator returns shadow_amd.graph.Edges with one self-loop per vertex first (as synth's
generators), small integer latencies (ties are exact) and f32 losses in [0, 1].
"""
import numpy as np

from shadow_amd.graph import Edges


def _edges(V, src, dst, lat, rng, loss_hi):
    """Self-loops first (latency 1..49, loss U(0, 0.3)), then the given pairs with loss U(0, loss_hi)."""
    src = np.asarray(src, dtype=np.uint32)
    dst = np.asarray(dst, dtype=np.uint32)
    lat = np.asarray(lat, dtype=np.uint64)
    loop = np.arange(V, dtype=np.uint32)
    loop_lat = rng.integers(1, 50, size=V, dtype=np.uint64)
    loop_loss = rng.uniform(0.0, 0.3, size=V).astype(np.float32)
    loss = rng.uniform(0.0, loss_hi, size=len(src)).astype(np.float32)
    return Edges(V, np.concatenate([loop, src]), np.concatenate([loop, dst]), np.concatenate([loop_lat, lat]),
                 np.concatenate([loop_loss, loss]), directed=False)


def chain(V, seed=1):
    """Path 0 - 1 - ... - V-1, latency 1, loss U(0, 0.01): depth V - 1, every shortest path unique."""
    rng = np.random.default_rng(seed)
    i = np.arange(V - 1)
    return _edges(V, i, i + 1, np.ones(V - 1), rng, 0.01)


def chain_chords(V, k=3, seed=2):
    """The chain plus chords (i, i + k) of latency exactly k: nearly every pair has two tight
    predecessors, the longest tight path stays V - 1 hops."""
    rng = np.random.default_rng(seed)
    i, j = np.arange(V - 1), np.arange(V - k)
    return _edges(V, np.concatenate([i, j]), np.concatenate([i + 1, j + k]),
                  np.concatenate([np.ones(V - 1), np.full(V - k, k)]), rng, 0.01)


def bipartite(a, b, seed=3, lossy=False):
    """K_{a,b} (vertices 0..a-1 against a..a+b-1), unit latency, distinct random losses.  A same-side
    pair has as many tight predecessors as the other side has vertices: a source on the a side has
    a - 1 multi-predecessor targets of in-degree b.  lossy: a quarter of the edge losses are exactly
    1.0 and a quarter exactly 0.0 (both legal, and 1.0 is also the fold's initial value)."""
    rng = np.random.default_rng(seed)
    i, j = np.divmod(np.arange(a * b), b)
    e = _edges(a + b, i, a + j, np.ones(a * b), rng, 0.3)
    if lossy:
        u = rng.random(a * b)
        p = e.packet_loss[a + b:]
        p[u < 0.25] = 1.0
        p[u >= 0.75] = 0.0
    return e


def grid(w, h, seed=4):
    """w x h grid, unit latency: depth w + h - 2, an interior target off the source's row and column
    has two tight predecessors."""
    rng = np.random.default_rng(seed)
    y, x = np.divmod(np.arange(w * h), w)
    v = y * w + x
    right, down = v[x < w - 1], v[y < h - 1]
    src, dst = np.concatenate([right, down]), np.concatenate([right + 1, down + w])
    return _edges(w * h, src, dst, np.ones(len(src)), rng, 0.02)


def ring_chords(V, m, seed):
    """Ring 0 - 1 - ... - V-1 - 0 (latency 1) plus m * V random chords with latencies 1..4.  O(E)
    memory (no V x V mask): this is the graph of the V > 12 000 case."""
    rng = np.random.default_rng(seed)
    i = np.arange(V)
    cs = rng.integers(0, V, size=m * V)
    cd = (cs + rng.integers(1, V, size=m * V)) % V  # never a second self-loop
    lat = np.concatenate([np.ones(V, dtype=np.int64), rng.integers(1, 5, size=m * V)])
    return _edges(V, np.concatenate([i, cs]), np.concatenate([(i + 1) % V, cd]), lat, rng, 0.05)


def composite(parts, seed=5, relabel=True):
    """The parts in order, each joined to the next by one bridge edge (last vertex of one to vertex 0
    of the next, latency 1).  relabel: a seeded random permutation of the vertex numbers; without
    it a chain part's order is its index order."""
    rng = np.random.default_rng(seed)
    V = sum(p.num_vertices for p in parts)
    loops, rest, off, bridges = [], [], 0, []
    for p in parts:
        n = p.num_vertices
        assert not p.directed and np.array_equal(p.src[:n], np.arange(n)) and np.array_equal(p.dst[:n], np.arange(n))
        loops.append((p.src[:n] + off, p.dst[:n] + off, p.latency_ns[:n], p.packet_loss[:n]))
        rest.append((p.src[n:] + off, p.dst[n:] + off, p.latency_ns[n:], p.packet_loss[n:]))
        if off:
            bridges.append((off - 1, off))
        off += n
    bs = np.array([x for x, _ in bridges], dtype=np.uint32)
    bd = np.array([y for _, y in bridges], dtype=np.uint32)
    rest.append((bs, bd, np.ones(len(bs), dtype=np.uint64), rng.uniform(0.0, 0.05, size=len(bs)).astype(np.float32)))
    src, dst, lat, loss = (np.concatenate([x[k] for x in loops + rest]) for k in range(4))
    if relabel:
        perm = rng.permutation(V).astype(np.uint32)
        # the self-loops stay first and in vertex order
        order = np.concatenate([np.argsort(perm[src[:V]], kind="stable"), np.arange(V, len(src))])
        src, dst, lat, loss = perm[src][order], perm[dst][order], lat[order], loss[order]
    return Edges(V, src, dst, lat, loss, directed=False)


def padded(g, pad=120, seed=6):
    """A chain of `pad` vertices in front of g (so V > 128: more than one source block), bridged to
    g's vertex 0.  A chain row sees g as g's vertex 0 does, so it has that row's multi-predecessor
    targets and no others; the rows of g keep theirs (the chain hangs off one vertex and adds
    single-predecessor targets only)."""
    return composite([chain(pad, seed), g], seed=seed + 1, relabel=False)


def standard_composite(relabel):
    """Every regime in one table of 391 vertices (four 128-blocks): a long unique path, chords,
    the three list regimes of the loss rows, a grid."""
    parts = [chain(130, 11), chain_chords(80, 3, 12), bipartite(10, 12, 13), bipartite(33, 17, 14),
             bipartite(20, 40, 15), grid(7, 7, 16)]
    return composite(parts, seed=17, relabel=relabel)


# the graphs the CPU and GPU tests share, by name (built on demand, cached: none is changed)
SMALL = {
    "chain384": lambda: chain(384),
    "chain_chords300": lambda: chain_chords(300),
    "bip20_40": lambda: bipartite(20, 40),
    "bip33_17": lambda: bipartite(33, 17),
    "bip10_12": lambda: bipartite(10, 12),
    "bip60_40": lambda: bipartite(60, 40),
    "bip20_40_lossy": lambda: bipartite(20, 40, seed=7, lossy=True),
    "grid17": lambda: grid(17, 17),
}
COMPOSITES = {
    "composite": lambda: standard_composite(True),
    "composite_inorder": lambda: standard_composite(False),
}
# the list regimes of k_loss_rows, padded past one source block
LISTS = {
    "list_only": lambda: padded(bipartite(10, 12)),
    "edges_over_33_17": lambda: padded(bipartite(33, 17)),
    "edges_over_20_40": lambda: padded(bipartite(20, 40)),
    "both_over": lambda: padded(bipartite(60, 40)),
    "lossy": lambda: padded(bipartite(20, 40, seed=7, lossy=True)),
}
_cache = {}


def graph(name):
    if name not in _cache:
        _cache[name] = {**SMALL, **COMPOSITES, **LISTS}[name]()
    return _cache[name]


# ---- analysis from exact distances ---------------------------------------------------------------

_INF = np.iinfo(np.int64).max // 4


def weights(e):
    """(W, WL): min latency per ordered pair (INF = no edge) and the min loss among the edges of
    that latency (parallel edges: min latency, then min loss); self-loops left out."""
    V = e.num_vertices
    m = e.src != e.dst
    s, d = e.src[m].astype(np.int64), e.dst[m].astype(np.int64)
    w, p = e.latency_ns[m].astype(np.int64), e.packet_loss[m]
    if not e.directed:
        s, d, w, p = np.concatenate([s, d]), np.concatenate([d, s]), np.concatenate([w, w]), np.concatenate([p, p])
    W = np.full((V, V), _INF, dtype=np.int64)
    np.minimum.at(W, (s, d), w)
    WL = np.full((V, V), np.float32(np.inf), dtype=np.float32)
    best = w == W[s, d]
    np.minimum.at(WL, (s[best], d[best]), p[best])
    return W, WL


def distances(W):
    """numpy Floyd-Warshall."""
    D = W.copy()
    np.fill_diagonal(D, 0)
    for k in range(len(D)):
        np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :], out=D)
    return D


def tight(W, D, s):
    """tight[u, t]: (u, t) is an essential edge on a shortest path from s to t."""
    t = (D[s][:, None] + W == D[s][None, :]) & (W == D) & (W < _INF)
    t[:, s] = False
    return t


class Shape:
    """Per source row: multi (targets with >= 2 tight predecessors), indeg (largest tight in-degree
    of a target), depth_min (most hops of a fewest-hop tight path: the round in which a Jacobi fold
    first reaches the row's last target), depth_max (hops of the longest tight path)."""

    def __init__(self, e, rows=None, depth=True):
        W, self.WL = weights(e)
        D = distances(W)
        self.W, self.D = W, D
        V = e.num_vertices
        self.rows = list(range(V)) if rows is None else list(rows)
        self.multi, self.indeg, self.depth_min, self.depth_max = [], [], [], []
        for s in self.rows:
            tg = tight(W, D, s)
            cnt = tg.sum(axis=0)
            self.multi.append(int((cnt >= 2).sum()))
            self.indeg.append(int(cnt.max()))
            if not depth:
                continue
            lo, hi = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64)
            dist = D[s]
            for d in np.unique(dist)[1:]:  # increasing distance: every tight predecessor is done
                ts = np.nonzero(dist == d)[0]
                sub = tg[:, ts]
                hi[ts] = np.where(sub, hi[:, None] + 1, 0).max(axis=0)
                lo[ts] = np.where(sub, lo[:, None] + 1, V).min(axis=0)
            self.depth_min.append(int(lo.max()))
            self.depth_max.append(int(hi.max()))

    def multi_pairs(self, nodes=None):
        """Used pairs (s, t), s != t, with two or more tight predecessors: stats.multi_pred_pairs."""
        cols = np.arange(len(self.D)) if nodes is None else np.asarray(nodes)
        total = 0
        for s in (self.rows if nodes is None else nodes):
            cnt = tight(self.W, self.D, s).sum(axis=0)
            total += int((cnt[cols] >= 2).sum())
        return total


def recurrence_loss(e, shape, rows=None):
    """The loss table by the recurrence alone, independent of any Dijkstra: targets
    in increasing distance from s, L[s] = 0, L[t] = min over tight predecessors u of
    fl(1 - fl(fl(1 - L[u]) * fl(1 - p(u, t)))) in float32; the diagonal is the raw self-loop loss.
    Returns (latency u64, loss f32) rows like the oracle's."""
    V = e.num_vertices
    one = np.float32(1.0)
    Bm = one - shape.WL  # fl(1 - p); (inf where no edge, never read)
    rows = list(range(V)) if rows is None else list(rows)
    lat = np.zeros((len(rows), V), dtype=np.uint64)
    loss = np.zeros((len(rows), V), dtype=np.float32)
    for i, s in enumerate(rows):
        tg = tight(shape.W, shape.D, s)
        dist = shape.D[s]
        L = np.ones(V, dtype=np.float32)
        L[s] = 0.0
        for d in np.unique(dist)[1:]:
            ts = np.nonzero(dist == d)[0]
            sub = tg[:, ts]
            with np.errstate(invalid="ignore"):
                cand = one - (one - L)[:, None] * Bm[:, ts]
            assert cand.dtype == np.float32
            L[ts] = np.where(sub, cand, np.float32(np.inf)).min(axis=0)
        L[s] = e.packet_loss[s]
        loss[i] = L
        lat[i] = dist.astype(np.uint64)
        lat[i, s] = e.latency_ns[s]
    return lat, loss
