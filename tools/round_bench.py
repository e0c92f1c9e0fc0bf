"""Times a round on the C5 shape, two ways in one session: `--offers` (10^7) offers over `--hosts`
(10 000) hosts per 5 ms window, `--sockets` (8) socket slots per host, sizes from {40, 576, 1500}, a
tenth of the offers control packets, destinations uniform over the hosts, a `--nodes` (256) node
table with latencies of 1 - 4 ms and losses below 2 %.  A tenth of the hosts are offered twice their
bw_up and keep a backlog; every bw_down is ten times the mean arrival rate.

  round     srg_round_receive_device + srg_round_send_device (Round.receive_device / send_device)
  separate  the same round through the five calls: pop, the popped tags read back and their sizes
            gathered with numpy and uploaded, the inbound step, the outbound step, its leaving order
            read back, destinations, per-host event ids and `chance` made with numpy, the batch
            uploaded, send_packets_device, push

Each way runs `--warmup` (2) + `--reps` (7) consecutive rounds on an object of its own (window k is
[t0 + k w, t0 + (k + 1) w)), fed the same offers; a round is timed with a host clock from before the
receive half to after the send half (every call ends in its own stream synchronise).  The two ways
draw different `chance` values (the separate way uses numpy's generator: what the parent commit's
caller would do), so their drop patterns differ; the shapes are the same.  One JSON line; --out also
writes it to a file.  --only round (or separate) runs one way alone, e.g. under a kernel trace."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--offers", type=int, default=10**7)
    ap.add_argument("--hosts", type=int, default=10000)
    ap.add_argument("--sockets", type=int, default=8)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("round", "separate"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from shadow_amd import Router
    from shadow_amd import events as ev
    if not torch.cuda.is_available():
        sys.exit("round_bench: no GPU (there is nothing to time without one)")
    dev = torch.device("cuda", 0)
    n, H, K, TN = args.offers, args.hosts, args.sockets, args.nodes
    window, t0 = 5_000_000, 10**12
    rounds = args.warmup + args.reps
    sim_end = t0 + (rounds + 10) * window
    rng = np.random.default_rng(7)
    host = np.sort(rng.integers(0, H, n, dtype=np.uint32))
    t = rng.integers(0, window, n, dtype=np.uint64).astype(np.uint64)
    t = t[np.lexsort((t, host))]
    counts = np.bincount(host, minlength=H)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    control = rng.random(n) < 0.1
    size = np.where(control, 40, rng.choice(np.array([40, 576, 1500], np.uint32), n)).astype(np.uint32)
    payload = (size - 40).astype(np.uint32)
    prio0 = np.where(control, 0, np.arange(n, dtype=np.uint64) - offs[host] + 1).astype(np.uint64)
    slot = rng.integers(0, K, n, dtype=np.uint32)
    dst = rng.integers(0, H, n, dtype=np.uint32)
    local = dst == host
    offered_bits = int(n / H * float(size.mean()) * 8 / (window * 1e-9))  # per host, bit/s
    bw_up = np.full(H, offered_bits * 10, np.uint64)
    bw_up[rng.permutation(H)[:H // 10]] = offered_bits // 2
    bw_down = np.full(H, offered_bits * 10, np.uint64)
    sockets = np.full(H, K, np.uint32)
    host_node = rng.integers(0, TN, H, dtype=np.uint32)
    lat = rng.integers(1_000_000, 4_000_000, (TN, TN)).astype(np.uint64)
    loss = (rng.random((TN, TN), dtype=np.float32) * np.float32(0.02)).astype(np.float32)
    seeds = rng.integers(0, 2**63, H, dtype=np.uint64)
    table = ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss, device=dev)
    router = Router(0)
    k_t, s_t = ev._i32(slot, dev), ev._i32(size, dev)
    g_t = torch.arange(n, dtype=torch.int64, device=dev)
    o_t = ev._i64(offs, dev)
    t_base, p_base = ev._i64(t, dev), ev._i64(prio0, dev)
    data = torch.from_numpy(~control).to(dev)

    def offers_of(k):
        """Window k's times and priorities (the host's counter goes on counting)."""
        return t_base + (t0 + k * window), torch.where(data, p_base + k * int(counts.max()), p_base)

    result = {}
    if args.only in (None, "round"):
        rd = ev.Round(router, host_node, table, bw_up, bw_down, sockets, 0, seeds, 0, t0 + window, sim_end, reserve=n)
        rd.set_packets(ev._i32(dst, dev), s_t, ev._i32(payload, dev))
        recv_ms, send_ms, both_ms, last = [], [], [], None
        for k in range(rounds):
            we = t0 + (k + 1) * window
            t_t, p_t = offers_of(k)
            torch.cuda.synchronize(dev)
            c0 = time.perf_counter()
            rc, rres, msg = rd.receive_device(we)
            c1 = time.perf_counter()
            if rc != 0:
                sys.exit("round_bench: receive failed: " + msg)
            rc, sres, msg = rd.send_device(we, n, t_t, k_t, p_t, None, g_t, o_t)
            c2 = time.perf_counter()
            if rc != 0:
                sys.exit("round_bench: send failed: " + msg)
            if k >= args.warmup:
                recv_ms.append((c1 - c0) * 1e3)
                send_ms.append((c2 - c1) * 1e3)
                both_ms.append((c2 - c0) * 1e3)
            last = (rres.as_dict(), sres.as_dict())
        rd.close()
        result["round"] = {"receive": stats(recv_ms), "send": stats(send_ms), "both": stats(both_ms),
                           "last_receive": last[0], "last_send": last[1]}

    if args.only in (None, "separate"):
        q = ev.EventQueues(router, H, reserve=n)
        inb = ev.Inbound(router, bw_down, 0, t0 + window, reserve=n)
        out = ev.Outbound(router, bw_up, sockets, 0, 0, t0 + window, reserve=n)
        f_t = torch.from_numpy(local.astype(np.uint8)).to(dev)
        next_eid = np.zeros(H, np.uint64)
        nrng = np.random.default_rng(11)
        both_ms, last = [], None
        for k in range(rounds):
            we = t0 + (k + 1) * window
            t_t, p_t = offers_of(k)
            torch.cuda.synchronize(dev)
            c0 = time.perf_counter()
            # receive half: pop, sizes by tag on the host, the inbound step
            m = q.num_queued
            p_time = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
            p_tag = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
            p_off = torch.empty(H + 1, dtype=torch.int64, device=dev)
            rc, qres, msg = q.pop_device(we, m, p_time, None, None, p_tag, p_off)
            if rc != 0:
                sys.exit("round_bench: pop failed: " + msg)
            moved = int(qres["num_moved"])
            sz = ev._i32(size[p_tag[:moved].cpu().numpy()], dev)
            cap = max(inb.num_queued + moved, 1)
            i_out = (torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.int64, device=dev),
                     torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(H + 1, dtype=torch.int64, device=dev))
            rc, ires, msg = inb.step_device(we, moved, p_time, sz, p_tag, p_off, cap, *i_out)
            if rc != 0:
                sys.exit("round_bench: inbound step failed: " + msg)
            # send half: the outbound step, its leaving order through the host, send, push
            cap = max(out.num_queued + n, 1)
            o_out = (torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.int64, device=dev),
                     torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(H + 1, dtype=torch.int64, device=dev))
            rc, ores, msg = out.step_device(we, n, t_t, k_t, p_t, s_t, f_t, g_t, o_t, cap, *o_out)
            if rc != 0:
                sys.exit("round_bench: outbound step failed: " + msg)
            left = int(ores["num_sent"] + ores["num_local"])
            st = o_out[0][:left].cpu().numpy()
            tm = o_out[1][:left].cpu().numpy().view(np.uint64)
            tg = o_out[2][:left].cpu().numpy()
            oo = o_out[3].cpu().numpy()
            keep = st == 1
            src = np.repeat(np.arange(H, dtype=np.uint32), np.diff(oo))[keep]
            tags = tg[keep]
            per_host = np.bincount(src, minlength=H).astype(np.uint64)
            first = np.concatenate([[0], np.cumsum(per_host)[:-1]]).astype(np.uint64)
            eid = next_eid[src] + (np.arange(len(src), dtype=np.uint64) - first[src])
            next_eid += per_host
            d = dst[tags]
            batch = dict(src_node=host_node[src], dst_node=host_node[d], src_host=src, dst_host=d, send_time_ns=tm[keep],
                         src_event_id=eid, chance=nrng.random(len(src)), payload_size=payload[tags])
            db = ev.DeviceSendBatch(batch, H, we, t0 + window, dev)
            sres, pres, _ = q.send(db, table, tags=ev._i64(tags.astype(np.uint64), dev))
            c2 = time.perf_counter()
            if k >= args.warmup:
                both_ms.append((c2 - c0) * 1e3)
            last = {"num_popped": moved, "num_left": left, "num_sent": int(sres["num_sent"]),
                    "num_queued_events": int(pres["num_queued"])}
        q.close()
        inb.close()
        out.close()
        result["separate"] = {"both": stats(both_ms), "last": last}

    if "round" in result and "separate" in result:
        a, b = result["round"]["both"], result["separate"]["both"]
        gain = b["median_ms"] - a["median_ms"]
        spreads = (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"])
        result["gain_ms"] = round(gain, 4)
        result["spreads_ms"] = round(spreads, 4)
        result["faster_by_more_than_the_spreads"] = bool(gain > spreads)
    line = json.dumps({
        "tool": "round_bench", "offers": n, "hosts": H, "sockets_per_host": K, "table_nodes": TN, "window_ns": window,
        "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "busiest_host_offers": int(counts.max()), "local_share": round(float(local.mean()), 6), **result,
    })
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
