"""Times srg_outbound_step_device on the C5 round shape: `--offers` (10^7) offers over `--hosts`
(10 000) hosts in one 5 ms window, grouped by host with non-decreasing times, `--sockets` (8) socket
slots per host, sizes from {40, 576, 1500}, data priorities from a per-host counter, a tenth of the
offers control packets (priority 0, 40 B).  A tenth of the hosts are offered ten times their bw_up
(they block on tokens and keep a backlog), the rest a tenth of it.  Both qdiscs, one after the other.
One process, one GPU.

A step changes the state, so every repetition runs on a fresh srg_outbound (created outside the
timed region); the timed call ends in its own stream synchronise and is timed with a host clock.
Reported per qdisc: median / min / max over `--reps` (7) calls after `--warmup` (2), the busiest
host's offer count, what left and what stayed.  One JSON line; --out also writes it to a file.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--offers", type=int, default=10**7)
    ap.add_argument("--hosts", type=int, default=10000)
    ap.add_argument("--sockets", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from shadow_amd import Router
    from shadow_amd import events as ev
    if not torch.cuda.is_available():
        sys.exit("outbound_bench: no GPU (there is nothing to time without one)")
    dev = torch.device("cuda", 0)
    n, H, K = args.offers, args.hosts, args.sockets
    window, t0 = 5_000_000, 10**12
    rng = np.random.default_rng(7)
    host = np.sort(rng.integers(0, H, n, dtype=np.uint32))
    t = (t0 + rng.integers(0, window, n, dtype=np.uint64)).astype(np.uint64)
    t = t[np.lexsort((t, host))]
    counts = np.bincount(host, minlength=H)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    control = rng.random(n) < 0.1
    size = np.where(control, 40, rng.choice(np.array([40, 576, 1500], np.uint32), n)).astype(np.uint32)
    prio = np.where(control, 0, np.arange(n, dtype=np.uint64) - offs[host] + 1).astype(np.uint64)  # the host's counter
    slot = rng.integers(0, K, n, dtype=np.uint32)
    offered_bits = int(n / H * float(size.mean()) * 8 / (window * 1e-9))  # per host, bit/s
    bw = np.full(H, offered_bits * 10, np.uint64)
    bw[rng.permutation(H)[:H // 10]] = offered_bits // 10
    t_t, k_t, p_t, s_t = ev._i64(t, dev), ev._i32(slot, dev), ev._i64(prio, dev), ev._i32(size, dev)
    g_t = torch.arange(n, dtype=torch.int64, device=dev)
    o_t = ev._i64(offs, dev)
    out = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
           torch.empty(n, dtype=torch.int64, device=dev), torch.empty(H + 1, dtype=torch.int64, device=dev))
    router = Router(0)
    per_qdisc = {}
    for name, qdisc in (("fifo", 0), ("round_robin", 1)):
        ms, last = [], None
        for rep in range(args.warmup + args.reps):
            ob = ev.Outbound(router, bw, np.full(H, K, np.uint32), qdisc, 0, t0, reserve=n)
            torch.cuda.synchronize(dev)
            c0 = time.perf_counter()
            # (returns after its own stream synchronise)
            rc, res, msg = ob.step_device(t0 + window, n, t_t, k_t, p_t, s_t, None, g_t, o_t, n, *out)
            dt = (time.perf_counter() - c0) * 1e3
            if rc != 0:
                sys.exit("outbound_bench: step failed: " + msg)
            if rep >= args.warmup:
                ms.append(dt)
            last = res
            ob.close()
        med = statistics.median(ms)
        per_qdisc[name] = {
            "step": {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)},
            "num_sent": int(last["num_sent"]), "num_local": int(last["num_local"]), "num_queued": int(last["num_queued"]),
            "min_next_wake_ns": int(last["min_next_wake_ns"]),
            "us_per_offer_of_busiest_host": round(med * 1e3 / int(counts.max()), 3),
        }
    line = json.dumps({
        "tool": "outbound_bench", "offers": n, "hosts": H, "sockets_per_host": K, "window_ns": window, "reps": args.reps,
        "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "mapping": "one wave64 per host, 4 hosts per workgroup", "offered_bits_per_host": offered_bits,
        "overloaded_hosts": H // 10, "control_share": round(float(control.mean()), 4),
        "busiest_host_offers": int(counts.max()), "mean_host_offers": round(float(counts.mean()), 1),
        "qdisc": per_qdisc,
    })
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
