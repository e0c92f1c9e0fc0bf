"""The routes a routing table's paths take, and per-edge packet loads (srg_trace_routes_device,
srg_link_loads_device; csrc/routes.hip.h, rule in csrc/route_rule.h), pair by pair; and the route
trees of whole source rows (srg_route_trees_device, srg_link_loads_trees_device;
csrc/route_trees.hip.h, rules in csrc/route_tree_rule.h).

The reference keeps no routes (petgraph's dijkstra returns scores only, mod.rs:190-208); they are
read back from the finished table: the route's edge into a vertex is the in-edge (u, cur) with
D[s][u] + lat == D[s][cur] and bits(fold(L[s][u], loss)) == bits(L[s][cur]), smallest edge index
among the matches; the source's label is (0, +0.0), the route s -> s is the self-loop of s.  The
table must cover every vertex in NodeIndex order (a DevicePathTable of compute_shortest_paths over
all vertices, either form).

  trace_routes_device / link_loads_device   tensors already in HBM
  trace_routes / link_loads                 host arrays in, host arrays out

For one source the routes to all targets form a tree (the tie rule makes every route unique), so
a row of predecessors holds every route of that source:

  route_trees_device / link_loads_trees_device   tensors already in HBM
  route_trees / link_loads_trees                 host arrays in, host arrays out

route_trees gives, per (source row, target): the route's last edge and the vertex it comes from, its
hop count and its first edge (the forwarding table); the source's own column holds ROUTE_NONE and
0 hops.  link_loads_trees has link_loads' contract and results, computed by pushing each row's
counts up its tree, and no limit on n * n.  Both filter the in-edges to those with
lat(e) == D[u][t] first and so trust those entries of every row (include/shadow_routing.h).
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from .device import DeviceGraph
from .events import _i32, _i64
from .graph import NetGraphError, _raise


class RouteError(NetGraphError):
    """A pair whose table entry no in-edge explains (SRG_ERR_ROUTE): the table is not a shortest-path
    table of this graph.  `bad_pair`: the first such query (link loads: s * n + t)."""

    def __init__(self, code, message, bad_pair=None):
        super().__init__(code, message)
        self.bad_pair = bad_pair


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _fail(rc, err, res):
    msg = err.value.decode(errors="replace")
    if rc == N.SRG_ERR_ROUTE:
        raise RouteError(rc, msg, int(res.bad_pair))
    _raise(rc, msg)


def trace_routes_device(router, dgraph, table, src_t, dst_t, hop_capacity, out_offsets_t, out_edges_t,
                        out_vertices_t=None, stream=None, check=True):
    """dgraph: DeviceGraph; table: DevicePathTable (n == num_vertices, with packet_loss); src_t, dst_t
    int32 [q] NodeIndex values; out_offsets_t int64 [q + 1], out_edges_t / out_vertices_t int32
    [hop_capacity] (every output may be None when hop_capacity is 0: a sizing call).
    check=True: returns the result dict, raises on any error.  check=False: returns (rc, result dict,
    message) and raises nothing (a short capacity is SRG_ERR_ARG with total_hops = the need)."""
    q = src_t.numel()
    assert dst_t.numel() == q and src_t.dtype == torch.int32 and dst_t.dtype == torch.int32
    assert out_offsets_t is None or (out_offsets_t.dtype == torch.int64 and out_offsets_t.numel() == q + 1)
    assert out_edges_t is None or (out_edges_t.dtype == torch.int32 and out_edges_t.numel() >= hop_capacity)
    assert out_vertices_t is None or (out_vertices_t.dtype == torch.int32 and out_vertices_t.numel() >= hop_capacity)
    res = N.RouteResult()
    err = ctypes.create_string_buffer(1024)
    el, t = dgraph.as_struct(), table.as_struct()
    s = stream if stream is not None else torch.cuda.current_stream(dgraph.src.device)
    rc = N.lib().srg_trace_routes_device(
        router._h, ctypes.byref(el), ctypes.byref(t), _ptr(src_t), _ptr(dst_t), q, int(hop_capacity),
        _ptr(out_offsets_t), _ptr(out_edges_t), _ptr(out_vertices_t), ctypes.c_void_p(s.cuda_stream),
        ctypes.byref(res), err, len(err))
    if not check:
        return rc, res.as_dict(), err.value.decode(errors="replace")
    if rc != N.SRG_OK:
        _fail(rc, err, res)
    return res.as_dict()


def link_loads_device(router, dgraph, table, counts_t, loads_t, stream=None):
    """counts_t: int64 [n, n] holding the u64 packet counts by position (what send_packets_device
    accumulates); loads_t: int64 [num_edges], accumulated in place (saturating), untouched on error."""
    assert counts_t.dtype == torch.int64 and counts_t.numel() == table.n * table.n and counts_t.is_contiguous()
    assert loads_t.dtype == torch.int64 and loads_t.numel() == dgraph.num_edges and loads_t.is_contiguous()
    res = N.RouteResult()
    err = ctypes.create_string_buffer(1024)
    el, t = dgraph.as_struct(), table.as_struct()
    s = stream if stream is not None else torch.cuda.current_stream(counts_t.device)
    rc = N.lib().srg_link_loads_device(router._h, ctypes.byref(el), ctypes.byref(t), counts_t.data_ptr(),
                                       loads_t.data_ptr(), ctypes.c_void_p(s.cuda_stream), ctypes.byref(res), err,
                                       len(err))
    if rc != N.SRG_OK:
        _fail(rc, err, res)
    return res.as_dict()


ROUTE_NONE = N.SRG_ROUTE_NONE


def route_trees_device(router, dgraph, table, sources_t, num_sources, pred_edge_t, pred_vertex_t=None, hops_t=None,
                       first_edge_t=None, stream=None, check=True):
    """sources_t: int32 [num_sources] NodeIndex values, or None (row i = source i, num_sources <= n);
    pred_edge_t (required unless num_sources == 0), pred_vertex_t, hops_t, first_edge_t: int32
    [num_sources * n] or None.  check=True: returns the result dict, raises on any error;
    check=False: returns (rc, result dict, message).  On an error the outputs are unspecified."""
    ns = int(num_sources)
    assert sources_t is None or (sources_t.dtype == torch.int32 and sources_t.numel() >= ns)
    for o in (pred_edge_t, pred_vertex_t, hops_t, first_edge_t):
        assert o is None or (o.dtype == torch.int32 and o.numel() >= ns * table.n and o.is_contiguous())
    res = N.RouteResult()
    err = ctypes.create_string_buffer(1024)
    el, t = dgraph.as_struct(), table.as_struct()
    s = stream if stream is not None else torch.cuda.current_stream(dgraph.src.device)
    rc = N.lib().srg_route_trees_device(
        router._h, ctypes.byref(el), ctypes.byref(t), _ptr(sources_t), ns, _ptr(pred_edge_t), _ptr(pred_vertex_t),
        _ptr(hops_t), _ptr(first_edge_t), ctypes.c_void_p(s.cuda_stream), ctypes.byref(res), err, len(err))
    if not check:
        return rc, res.as_dict(), err.value.decode(errors="replace")
    if rc != N.SRG_OK:
        _fail(rc, err, res)
    return res.as_dict()


def link_loads_trees_device(router, dgraph, table, counts_t, loads_t, stream=None):
    """link_loads_device's arguments and results, by route trees."""
    assert counts_t.dtype == torch.int64 and counts_t.numel() == table.n * table.n and counts_t.is_contiguous()
    assert loads_t.dtype == torch.int64 and loads_t.numel() == dgraph.num_edges and loads_t.is_contiguous()
    res = N.RouteResult()
    err = ctypes.create_string_buffer(1024)
    el, t = dgraph.as_struct(), table.as_struct()
    s = stream if stream is not None else torch.cuda.current_stream(counts_t.device)
    rc = N.lib().srg_link_loads_trees_device(router._h, ctypes.byref(el), ctypes.byref(t), counts_t.data_ptr(),
                                             loads_t.data_ptr(), ctypes.c_void_p(s.cuda_stream), ctypes.byref(res),
                                             err, len(err))
    if rc != N.SRG_OK:
        _fail(rc, err, res)
    return res.as_dict()


def _dgraph(router, edges):
    return edges if isinstance(edges, DeviceGraph) else DeviceGraph(edges, f"cuda:{router.device}")


def trace_routes(router, edges, table, pairs):
    """edges: Edges (or a DeviceGraph); table: DevicePathTable; pairs: [q, 2] (s, t) NodeIndex values.
    Returns (offsets u64 [q + 1], hop_edges u32, hop_vertices u32, result): query i's route is
    hop_edges[offsets[i]:offsets[i + 1]], s -> t.  Sizes the hop arrays with a capacity-0 call."""
    dev = torch.device(f"cuda:{router.device}")
    dg = _dgraph(router, edges)
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    src, dst = _i32(pairs[:, 0], dev), _i32(pairs[:, 1], dev)
    off = torch.empty(len(pairs) + 1, dtype=torch.int64, device=dev)
    rc, res, msg = trace_routes_device(router, dg, table, src, dst, 0, off, None, None, check=False)
    need = 0
    he = hv = None
    if rc == N.SRG_ERR_ARG and res["total_hops"] > 0:
        need = int(res["total_hops"])
        he = torch.empty(need, dtype=torch.int32, device=dev)
        hv = torch.empty(need, dtype=torch.int32, device=dev)
        rc, res, msg = trace_routes_device(router, dg, table, src, dst, need, off, he, hv, check=False)
    if rc == N.SRG_ERR_ROUTE:
        raise RouteError(rc, msg, res["bad_pair"])
    if rc != N.SRG_OK:
        _raise(rc, msg)
    if need == 0:
        z = np.zeros(0, np.uint32)
        return off.cpu().numpy().view(np.uint64), z, z.copy(), res
    return (off.cpu().numpy().view(np.uint64), he.cpu().numpy().view(np.uint32), hv.cpu().numpy().view(np.uint32),
            res)


def link_loads(router, edges, table, counts, loads=None):
    """counts: u64 [n, n] by position (a host array, or the int64 device tensor of send_packets);
    loads: u64 [num_edges] to accumulate onto (None = zeros).  Returns (loads u64 [num_edges], result)."""
    dev = torch.device(f"cuda:{router.device}")
    dg = _dgraph(router, edges)
    if not isinstance(counts, torch.Tensor):
        counts = _i64(np.asarray(counts), dev)
    init = np.zeros(dg.num_edges, np.uint64) if loads is None else np.asarray(loads)
    loads_t = _i64(init, dev)
    res = link_loads_device(router, dg, table, counts.contiguous(), loads_t)
    return loads_t.cpu().numpy().view(np.uint64), res


def route_trees(router, edges, table, sources=None):
    """edges: Edges (or a DeviceGraph); table: DevicePathTable; sources: NodeIndex values (None: every
    vertex in order).  Returns (pred_edge, pred_vertex, hops, first_edge, result), each array u32
    [len(sources), n]; ROUTE_NONE (hops: 0) in the source's own column."""
    dev = torch.device(f"cuda:{router.device}")
    dg = _dgraph(router, edges)
    n = table.n
    if sources is None:
        src_t, ns = None, n
    else:
        sources = np.asarray(sources, dtype=np.uint32).reshape(-1)
        src_t, ns = _i32(sources, dev), len(sources)
    outs = [torch.empty(max(ns * n, 1), dtype=torch.int32, device=dev) for _ in range(4)]
    res = route_trees_device(router, dg, table, src_t, ns, *outs)
    return tuple(o[:ns * n].cpu().numpy().view(np.uint32).reshape(ns, n) for o in outs) + (res,)


def link_loads_trees(router, edges, table, counts, loads=None):
    """link_loads' arguments and results, by route trees."""
    dev = torch.device(f"cuda:{router.device}")
    dg = _dgraph(router, edges)
    if not isinstance(counts, torch.Tensor):
        counts = _i64(np.asarray(counts), dev)
    init = np.zeros(dg.num_edges, np.uint64) if loads is None else np.asarray(loads)
    loads_t = _i64(init, dev)
    res = link_loads_trees_device(router, dg, table, counts.contiguous(), loads_t)
    return loads_t.cpu().numpy().view(np.uint64), res


__all__ = ["RouteError", "ROUTE_NONE", "trace_routes_device", "link_loads_device", "trace_routes", "link_loads",
           "route_trees_device", "link_loads_trees_device", "route_trees", "link_loads_trees"]
