"""Times srg_sockets_in_step_device behind the inbound step on the C5 round shape: `--events` (10^7)
arrivals over `--hosts` (10 000) hosts in one 5 ms window go through srg_inbound_step_device (the
shape and bandwidth mix of tools/inbound_bench.py), and what it writes -- status, time, tag, host
offsets -- goes into the sockets step untouched (deliver_status 1).  8 UDP sockets per host bound to
ports 1000..1007 by wildcard keys, limits at the default receive buffer, a tenth of the packets to an
unbound port, and about as many reads as deliveries (per host as many reads as it has rows, at
sorted random times of the window, on random slots).  One process, one GPU.

9 consecutive steps on one object (the buffers carry over), the last 7 timed with a host clock; every
call ends in its own stream synchronise.  In the same session: srg_inbound_step_device on the same
arrivals (fresh object per repetition, as in inbound_bench), and the floor of any host-side
alternative: the D2H of the forwarded rows' status, time and tag into pinned memory plus an H2D of
as many status bytes.  `--skew` runs a second case without the inbound stage: 10^6 of the
deliveries, and as many reads, on one socket.  One JSON line; --out also writes it to a file.
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

SOCKETS = 8


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events", type=int, default=10**7)
    ap.add_argument("--hosts", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skew", type=int, default=0, help="rows (and reads) put on one socket in a second case")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from shadow_amd import Router
    from shadow_amd import events as ev
    if not torch.cuda.is_available():
        sys.exit("sockets_in_bench: no GPU (there is nothing to time without one)")
    dev = torch.device("cuda", 0)
    n, H = args.events, args.hosts
    window, t0 = 5_000_000, 10**12
    rng = np.random.default_rng(7)
    router = Router(0)

    def u8(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev)

    def i16(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(dev)

    def arrivals(host):
        t = (t0 + rng.integers(0, window, len(host), dtype=np.uint64)).astype(np.uint64)
        t = t[np.lexsort((t, host))]
        counts = np.bincount(host, minlength=H)
        return t, counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)

    def sockets_object(size):
        """8 bound UDP sockets per host and the packet table for `size` (total sizes by tag)."""
        m = len(size)
        sk = ev.SocketsIn(router, np.full(H, SOCKETS, np.uint32), reserve=m)
        hs = np.repeat(np.arange(H, dtype=np.uint32), SOCKETS)
        sl = np.tile(np.arange(SOCKETS, dtype=np.uint32), H)
        z = np.zeros(H * SOCKETS, np.uint32)
        sk.associate(hs, np.full(H * SOCKETS, 17), 1000 + sl, z, z, sl)
        port = np.where(rng.random(m) < 0.1, 9, 1000 + rng.integers(0, SOCKETS, m))
        sk.set_packets(u8(np.full(m, 17)), ev._i32(rng.integers(1, 2**32, m, dtype=np.uint64).astype(np.uint32), dev),
                       i16(rng.integers(1024, 65536, m)), i16(port), ev._i32(size, dev),
                       ev._i32(np.maximum(size.astype(np.int64) - 28, 0).astype(np.uint32), dev))
        return sk, port

    def reads_like(counts, slot_of_host0=None):
        host = np.repeat(np.arange(H, dtype=np.uint32), counts)
        t, _, offs = arrivals(host)
        slot = rng.integers(0, SOCKETS, len(host)).astype(np.uint32)
        if slot_of_host0 is not None:
            slot[:counts[0]] = slot_of_host0
        return ev._i64(t, dev), ev._i32(slot, dev), ev._i64(offs, dev), len(host)

    def time_steps(sk, m, st_t, tm_t, tg_t, off_t, reads):
        rt_t, rs_t, roff_t, nr = reads
        outs = (torch.empty(max(m, 1), dtype=torch.uint8, device=dev), torch.empty(max(m, 1), dtype=torch.int32, device=dev),
                torch.empty(max(nr, 1), dtype=torch.uint8, device=dev), torch.empty(max(nr, 1), dtype=torch.int64, device=dev),
                torch.empty(max(nr, 1), dtype=torch.int64, device=dev), torch.empty(max(nr, 1), dtype=torch.int32, device=dev))
        ms, results = [], []
        for rep in range(args.warmup + args.reps):
            torch.cuda.synchronize(dev)
            c0 = time.perf_counter()
            rc, res, msg = sk.step_device(m, st_t, tm_t, tg_t, off_t, 1, nr, rt_t, rs_t, None, roff_t, *outs)
            dt = (time.perf_counter() - c0) * 1e3
            if rc != 0:
                sys.exit("sockets_in_bench: step failed: " + msg)
            if rep >= args.warmup:
                ms.append(dt)
            results.append({k: int(v) for k, v in res.items() if k != "ms_total"})
        return stats(ms), results[0], results[-1]

    # ---- the C5 shape: arrivals -> inbound step -> sockets step ----
    host = np.sort(rng.integers(0, H, n, dtype=np.uint32))
    t, counts, offs = arrivals(host)
    size = rng.choice(np.array([40, 576, 1500], np.uint32), n)
    offered_bits = int(n / H * float(size.mean()) * 8 / (window * 1e-9))
    bw = np.full(H, offered_bits * 10, np.uint64)
    bw[rng.permutation(H)[:H // 10]] = offered_bits // 10
    t_t, s_t, g_t, o_t = ev._i64(t, dev), ev._i32(size, dev), torch.arange(n, dtype=torch.int64, device=dev), ev._i64(offs, dev)
    out = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
           torch.empty(n, dtype=torch.int64, device=dev), torch.empty(H + 1, dtype=torch.int64, device=dev))
    inb_ms, inb_res = [], None
    for rep in range(args.warmup + args.reps):
        inb = ev.Inbound(router, bw, 0, t0, reserve=n)
        torch.cuda.synchronize(dev)
        c0 = time.perf_counter()
        rc, inb_res, msg = inb.step_device(t0 + window, n, t_t, s_t, g_t, o_t, n, *out)
        dt = (time.perf_counter() - c0) * 1e3
        if rc != 0:
            sys.exit("sockets_in_bench: inbound step failed: " + msg)
        if rep >= args.warmup:
            inb_ms.append(dt)
        inb.close()
    m = int(inb_res["num_forwarded"] + inb_res["num_dropped"])
    leaving = np.diff(out[3].cpu().numpy().view(np.uint64)).astype(np.int64)
    sk, _ = sockets_object(size)
    step, first, last = time_steps(sk, m, out[0], out[1], out[2], out[3], reads_like(leaving))
    sk.close()
    # ---- the floor of a host-side alternative: forwarded rows down, as many status bytes up ----
    fwd = int(inb_res["num_forwarded"])
    pinned = (torch.empty(fwd, dtype=torch.uint8).pin_memory(), torch.empty(fwd, dtype=torch.int64).pin_memory(),
              torch.empty(fwd, dtype=torch.int64).pin_memory())
    up = torch.empty(fwd, dtype=torch.uint8, device=dev)
    copy_ms = []
    for rep in range(args.warmup + args.reps):
        torch.cuda.synchronize(dev)
        c0 = time.perf_counter()
        for p, d in zip(pinned, out[:3]):
            p.copy_(d[:fwd], non_blocking=True)
        torch.cuda.synchronize(dev)
        up.copy_(pinned[0], non_blocking=True)
        torch.cuda.synchronize(dev)
        if rep >= args.warmup:
            copy_ms.append((time.perf_counter() - c0) * 1e3)
    doc = {
        "tool": "sockets_in_bench", "events": n, "hosts": H, "sockets_per_host": SOCKETS, "window_ns": window,
        "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "mapping": "lookup: one thread per row; buffers: one wave64 per socket, 4 sockets per workgroup, 64 operations per pass",
        "busiest_host_rows": int(leaving.max()), "rows": m, "forwarded_rows": fwd, "reads": int(leaving.sum()),
        "step": step, "first_step": first, "last_step": last,
        "inbound_step_same_session": stats(inb_ms), "d2h_rows_plus_h2d_status": stats(copy_ms),
        "d2h_h2d_bytes": fwd * 17 + fwd,
    }
    # ---- the skewed case: `--skew` rows and reads on one socket ----
    if args.skew:
        k = args.skew
        host = np.sort(np.concatenate([np.zeros(k, np.uint32), rng.integers(1, H, n - k, dtype=np.uint32)]))
        t, counts, offs = arrivals(host)
        size = rng.choice(np.array([40, 576, 1500], np.uint32), n)
        sk, port = sockets_object(size)
        port[:k] = 1000  # host 0's rows are the first k tags
        sk._packets = sk._packets[:3] + (i16(port),) + sk._packets[4:]
        sk.set_packets(*sk._packets)
        sstep, sfirst, slast = time_steps(sk, n, None, ev._i64(t, dev), torch.arange(n, dtype=torch.int64, device=dev),
                                          ev._i64(offs, dev), reads_like(counts, slot_of_host0=0))
        sk.close()
        doc["skewed"] = {"rows_on_one_socket": k, "reads_on_one_socket": k, "rows": n, "step": sstep, "first_step": sfirst,
                         "last_step": slast}
    line = json.dumps(doc)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
