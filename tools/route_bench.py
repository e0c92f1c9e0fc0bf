"""Times route tracing and link loads on the bench workload's table: atlas_like(10000) (C3), the
table built once by srg_compute_shortest_paths_device and kept in HBM.  One process, one GPU.

  (c)  srg_trace_routes_device of ONE pair: the per-call fixed cost (the edge checks and the in-edge
       lists of 5 * 10^7 edges are rebuilt on every call)
  (a)  srg_trace_routes_device of `--pairs` (10^6) random pairs, hop arrays sized beforehand
  (b)  srg_link_loads_device for a counts table with `--loads` (10^6, 10^7) nonzero pairs
  (d)  srg_route_trees_device of all sources, all four outputs, with 16 lanes per target and with a
       wave per target (SRG_ROUTE_TREE_GROUP, read on every call), alternating
  (e)  srg_link_loads_trees_device for the same counts tables as (b), checked equal to (b)'s loads
       and result, and for a fully nonzero table (which (b) is not timed on)
  and the essential fraction of arcs: those with lat(e) == D[u][t], which (d) and (e) keep.  Their
  byte model: rows x essential arcs x 20 B (an entry's endpoint and latency plus the gather D[s][u];
  only the few entries whose latency fits read more)

Each variant: `--warmup` (2) calls, then `--reps` (7) timed ones; every call returns after its stream
synchronise and is timed with a host clock.  Median, min and max go out as one JSON line.

No time threshold: these are first measurements.  Beside each time, the algorithmic byte count:
entries examined x 32 B (an in-edge entry is its edge index 4, other endpoint 4, latency 8 and loss
4 read in sequence, plus the gathers D[s][u] 8 and L[s][u] 4), entries examined = passes x hops x
in-degree (V - 1 on this complete graph; both calls walk twice: validate / count, then commit), and
the fraction of the HBM rate (8 TB/s) that byte count over the median time comes to.  The lists and
the table rows are reused between the waves of one source, so most of these bytes come from L2.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENTRY_BYTES = 32
# the tree kernels test an entry's latency first: endpoint 4 + latency 8 read in sequence and the
# gather D[s][u] 8; the few entries that pass also read the loss, the edge index and L[s][u]
TREE_ENTRY_BYTES = 20
HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vertices", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=10**6)
    ap.add_argument("--loads", type=int, nargs="*", default=[10**6, 10**7], help="nonzero count entries per variant")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from shadow_amd import Router, routes, synth
    from shadow_amd import events as ev
    from shadow_amd.device import DeviceGraph, compute_shortest_paths_device
    if not torch.cuda.is_available():
        sys.exit("route_bench: no GPU (there is nothing to time without one)")
    dev = torch.device("cuda", 0)
    V = args.vertices
    e = synth.atlas_like(V, seed=V)
    router = Router(0)
    dg = DeviceGraph(e, dev)
    nodes = torch.arange(V, dtype=torch.int32, device=dev)
    lat = torch.empty((V, V), dtype=torch.int64, device=dev)
    loss = torch.empty((V, V), dtype=torch.float32, device=dev)
    compute_shortest_paths_device(router, dg, nodes, lat, loss)
    table = ev.DevicePathTable(V, latency_ns=lat, packet_loss=loss)
    rng = np.random.default_rng(7)

    def timed(fn):
        ms = []
        res = None
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize(dev)
            c0 = time.perf_counter()
            res = fn()
            t = (time.perf_counter() - c0) * 1e3
            if i >= args.warmup:
                ms.append(t)
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                "max_ms": round(max(ms), 4)}, res

    def model(stat, res, passes):
        entries = passes * int(res["total_hops"]) * (V - 1)
        b = entries * ENTRY_BYTES
        return {"pairs": int(res["num_pairs"]), "total_hops": int(res["total_hops"]), "max_hops": int(res["max_hops"]),
                "passes": passes, "entries_examined": entries, "bytes": b,
                "bytes_per_s": round(b / (stat["median_ms"] * 1e-3), 1),
                "hbm_fraction": round(b / (stat["median_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)}

    out = {"tool": "route_bench", "vertices": V, "edges": e.num_edges, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "entry_bytes": ENTRY_BYTES, "hbm_bytes_per_s": HBM_BYTES_PER_S}

    def trace_variant(q):
        pairs = rng.integers(0, V, (q, 2), dtype=np.uint32)
        src, dst = ev._i32(pairs[:, 0], dev), ev._i32(pairs[:, 1], dev)
        off = torch.empty(q + 1, dtype=torch.int64, device=dev)
        rc, res, msg = routes.trace_routes_device(router, dg, table, src, dst, 0, None, None, None, check=False)
        need = max(int(res["total_hops"]), 1)
        he = torch.empty(need, dtype=torch.int32, device=dev)
        hv = torch.empty(need, dtype=torch.int32, device=dev)
        stat, res = timed(lambda: routes.trace_routes_device(router, dg, table, src, dst, need, off, he, hv))
        return {**stat, "model": model(stat, res, 2)}

    def progress(key):  # (stderr: stdout carries the one JSON line)
        print(f"route_bench: {key} {out[key]['median_ms']} ms", file=sys.stderr, flush=True)

    out["c_trace_one_pair"] = trace_variant(1)
    progress("c_trace_one_pair")
    out["a_trace_pairs"] = trace_variant(args.pairs)
    progress("a_trace_pairs")
    count_idx, count_val, pairwise = {}, {}, {}
    for nnz in args.loads:
        counts = torch.zeros(V * V, dtype=torch.int64, device=dev)
        count_idx[nnz] = torch.from_numpy(rng.choice(V * V, nnz, replace=False))
        count_val[nnz] = torch.from_numpy(rng.integers(1, 1000, nnz, dtype=np.int64))
        counts[count_idx[nnz].to(dev)] = count_val[nnz].to(dev)
        loads = torch.zeros(e.num_edges, dtype=torch.int64, device=dev)
        stat, res = timed(lambda: routes.link_loads_device(router, dg, table, counts, loads))
        out[f"b_link_loads_{nnz}"] = {**stat, "model": model(stat, res, 2)}
        progress(f"b_link_loads_{nnz}")
        pairwise[nnz] = (loads, res)
        del counts

    # the essential fraction: arcs u -> t (both orientations of an undirected edge, no self-loops)
    # whose latency equals the table entry (u, t)
    arc = dg.src != dg.dst
    es, ed, el = dg.src[arc].long(), dg.dst[arc].long(), dg.lat[arc]
    ess = int((lat[es, ed] == el).sum())
    arcs = int(arc.sum())
    if not e.directed:
        ess += int((lat[ed, es] == el).sum())
        arcs *= 2
    out["essential_arcs"] = {"arcs": arcs, "essential": ess, "fraction": round(ess / max(arcs, 1), 6)}
    del es, ed, el, arc

    def tree_model(stat, rows):
        entries = rows * ess  # every row examines every essential arc once
        b = entries * TREE_ENTRY_BYTES
        return {"rows": rows, "entries_examined": entries, "entry_bytes": TREE_ENTRY_BYTES, "bytes": b,
                "bytes_per_s": round(b / (stat["median_ms"] * 1e-3), 1),
                "hbm_fraction": round(b / (stat["median_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)}

    outs = [torch.empty(V * V, dtype=torch.int32, device=dev) for _ in range(4)]
    for rep in range(2):  # (alternating: other work shares the machine)
        for group in ("16", "64"):
            os.environ["SRG_ROUTE_TREE_GROUP"] = group
            stat, res = timed(lambda: routes.route_trees_device(router, dg, table, None, V, *outs))
            key = f"d_route_trees_all_group{group}_run{rep}"
            out[key] = {**stat, "total_hops": int(res["total_hops"]), "max_hops": int(res["max_hops"]),
                        "model": tree_model(stat, V)}
            progress(key)
    del outs
    os.environ.pop("SRG_ROUTE_TREE_GROUP", None)

    for nnz in list(args.loads) + [V * V]:
        if nnz < V * V:
            counts = torch.zeros(V * V, dtype=torch.int64, device=dev)
            counts[count_idx[nnz].to(dev)] = count_val[nnz].to(dev)
        else:
            counts = torch.from_numpy(rng.integers(1, 1000, V * V, dtype=np.int64)).to(dev)
        loads = torch.zeros(e.num_edges, dtype=torch.int64, device=dev)
        stat, res = timed(lambda: routes.link_loads_trees_device(router, dg, table, counts, loads))
        rows = int((counts.view(V, V) != 0).any(dim=1).sum())
        key = f"e_tree_loads_{nnz}"
        out[key] = {**stat, "pairs": int(res["num_pairs"]), "total_hops": int(res["total_hops"]),
                    "max_hops": int(res["max_hops"]), "model": tree_model(stat, rows)}
        if nnz in pairwise:
            # both accumulated the same number of calls onto zeros: the loads must be equal
            pl, pres = pairwise[nnz]
            out[key]["equals_pairwise"] = bool(torch.equal(pl, loads)) and all(
                res[k] == pres[k] for k in ("num_pairs", "total_hops", "max_hops", "bad_pair"))
            out[key]["speedup_vs_pairwise"] = round(out[f"b_link_loads_{nnz}"]["median_ms"] / stat["median_ms"], 2)
        progress(key)
        del counts, loads

    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
