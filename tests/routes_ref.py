"""numpy restatement of the route rule (shadow_amd/csrc/route_rule.h) -- a helper, not a test.

The walk of one source row in float32: the in-edges of every vertex in edge order, the first one
(smallest edge index) whose label sum reproduces the table entry bit for bit:
    D[s][u] + lat(e) == D[s][v]   and   bits(1 - (1 - L[s][u]) * (1 - p(e))) == bits(L[s][v]),
the source's label being (0, +0.0), self-loops never candidates, both orientations of an undirected
edge.  The diagonal route is the first self-loop edge.  Independent of the GPU code: plain numpy.
"""
import numpy as np

NONE = np.int64(-1)
U64_MAX = 2**64 - 1


def arcs(e):
    """(edge index, u, v) for every in-arc u -> v, self-loops left out; edge order within a vertex."""
    idx = np.arange(e.num_edges, dtype=np.int64)
    m = e.src != e.dst
    ei, s, d = idx[m], e.src[m].astype(np.int64), e.dst[m].astype(np.int64)
    if e.directed:
        return ei, s, d
    return np.concatenate([ei, ei]), np.concatenate([s, d]), np.concatenate([d, s])


def self_edges(e):
    """Smallest self-loop edge index per vertex (NONE: no self-loop)."""
    out = np.full(e.num_vertices, np.iinfo(np.int64).max, dtype=np.int64)
    m = e.src == e.dst
    np.minimum.at(out, e.src[m].astype(np.int64), np.arange(e.num_edges, dtype=np.int64)[m])
    out[out == np.iinfo(np.int64).max] = NONE
    return out


def predecessors(e, lat, loss, s, A=None):
    """For source s: (pred_edge [V], pred_vertex [V], matches [V]) -- the route's edge into every
    vertex (NONE: no in-edge explains the entry), the vertex it comes from, and how many in-edges
    satisfied both equalities."""
    ei, u, v = A if A is not None else arcs(e)
    V = e.num_vertices
    one = np.float32(1.0)
    D = lat[s].astype(np.uint64).copy()
    L = loss[s].astype(np.float32).copy()
    Dv, Lv = D[v], L[v]  # the entries to explain are the table's (v != s along a walk)
    D[s], L[s] = 0, np.float32(0.0)  # the source's own label, not the diagonal
    w = e.latency_ns[ei].astype(np.uint64)
    p = e.packet_loss[ei].astype(np.float32)
    with np.errstate(over="ignore"):
        lat_ok = (Dv >= w) & ((Dv - w) == D[u])
    f = one - (one - L[u]) * (one - p)
    assert f.dtype == np.float32
    ok = lat_ok & (f.view(np.uint32) == Lv.view(np.uint32))
    big = np.iinfo(np.int64).max
    pe = np.full(V, big, dtype=np.int64)
    np.minimum.at(pe, v[ok], ei[ok])
    cnt = np.zeros(V, dtype=np.int64)
    np.add.at(cnt, v[ok], 1)
    pu = np.full(V, NONE, dtype=np.int64)
    win = ok & (pe[v] == ei)
    pu[v[win]] = u[win]
    pe[pe == big] = NONE
    return pe, pu, cnt


def trace(e, lat, loss, pairs):
    """pairs [q, 2].  Returns (offsets u64 [q + 1], hop_edges u32, hop_vertices u32, info) with
    info = dict(unexplained=[query indices], steps=walk steps, multi_steps=steps with > 1 match,
    max_hops=...).  An unexplained query gets an empty route."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    q = len(pairs)
    A = arcs(e)
    selfe = self_edges(e)
    routes = [None] * q
    unexplained, steps, multi = [], 0, 0
    for s in np.unique(pairs[:, 0]):
        qi = np.flatnonzero(pairs[:, 0] == s)
        pe, pu, cnt = predecessors(e, lat, loss, s, A)
        for i in qi:
            t = int(pairs[i, 1])
            if t == s:
                if selfe[s] == NONE:
                    unexplained.append(int(i))
                    routes[i] = ([], [])
                else:
                    routes[i] = ([int(selfe[s])], [int(s)])
                continue
            he, hv, cur, ok = [], [], t, True
            while cur != s:
                if pe[cur] == NONE or len(he) >= e.num_vertices:
                    ok = False
                    break
                steps += 1
                multi += int(cnt[cur] > 1)
                he.append(int(pe[cur]))
                hv.append(cur)
                cur = int(pu[cur])
            if not ok:
                unexplained.append(int(i))
                he, hv = [], []
            routes[i] = (he[::-1], hv[::-1])
    lens = np.array([len(r[0]) for r in routes], dtype=np.uint64)
    off = np.zeros(q + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    hop_e = np.array([x for r in routes for x in r[0]], dtype=np.uint32)
    hop_v = np.array([x for r in routes for x in r[1]], dtype=np.uint32)
    info = dict(unexplained=sorted(unexplained), steps=steps, multi_steps=multi,
                max_hops=int(lens.max()) if q else 0)
    return off, hop_e, hop_v, info


def all_pairs(V):
    """Every ordered pair, diagonal included, row-major."""
    s, t = np.divmod(np.arange(V * V), V)
    return np.stack([s, t], axis=1)


def link_loads(e, lat, loss, counts, loads=None):
    """counts u64 [V, V]; returns the per-edge loads (u64, saturating), added onto `loads`."""
    V = e.num_vertices
    counts = np.asarray(counts, dtype=np.uint64).reshape(V, V)
    out = [0] * e.num_edges if loads is None else [int(x) for x in loads]
    nz = np.argwhere(counts != 0)
    off, he, _, info = trace(e, lat, loss, nz)
    assert not info["unexplained"]
    for i, (s, t) in enumerate(nz):
        c = int(counts[s, t])
        for ed in he[int(off[i]):int(off[i + 1])]:
            out[ed] = min(out[ed] + c, U64_MAX)
    return np.array(out, dtype=np.uint64), int(sum(int(counts[s, t]) * int(off[i + 1] - off[i])
                                                   for i, (s, t) in enumerate(nz)))


def certify(e, lat, loss, pairs, off, hop_e, hop_v):
    """The self-certificate of every route: consecutive hops share a vertex, the last vertex is t,
    the latency sum is the table entry, the forward fold from +0.0f is the table loss, bit for bit.
    Returns the list of failing query indices."""
    one = np.float32(1.0)
    bad = []
    for i, (s, t) in enumerate(np.asarray(pairs, dtype=np.int64).reshape(-1, 2)):
        es = hop_e[int(off[i]):int(off[i + 1])].astype(np.int64)
        vs = hop_v[int(off[i]):int(off[i + 1])].astype(np.int64)
        if s == t:
            if not (len(es) == 1 and e.src[es[0]] == s and e.dst[es[0]] == s and vs[0] == s):
                bad.append(i)
            continue
        ok = len(es) >= 1 and vs[-1] == t
        cur, total, L = s, 0, np.float32(0.0)
        for ed, v in zip(es, vs):
            a, b = int(e.src[ed]), int(e.dst[ed])
            ok = ok and ((a == cur and b == v) or (not e.directed and b == cur and a == v)) and a != b
            total += int(e.latency_ns[ed])
            L = one - (one - L) * (one - e.packet_loss[ed])
            cur = int(v)
        ok = ok and total == int(lat[s, t]) and np.float32(L).view(np.uint32) == loss[s, t].view(np.uint32)
        if not ok:
            bad.append(i)
    return bad
