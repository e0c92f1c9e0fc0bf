"""Times srg_inbound_step_device on the C5 round shape: `--events` (10^7) arrivals over `--hosts`
(10 000) hosts in one 5 ms window, grouped by host with non-decreasing times (what
srg_event_queues_pop_device writes), sizes from {40, 576, 1500}.  A tenth of the hosts get a
bandwidth a tenth of their offered load (they block on tokens, build a backlog and drop), the rest
ten times their offered load.  One process, one GPU.

A step changes the state, so every repetition runs on a fresh srg_inbound (created outside the
timed region); the timed call ends in its own stream synchronise and is timed with a host clock.
Reported: median / min / max over `--reps` (7) calls after `--warmup` (2), the busiest host's event
count, what left and what stayed, and the achieved bytes/s against a traffic model of
MODEL_BYTES per arrival.  One JSON line; --out also writes it to a file.
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

# per arrival: validate reads time 8 + size 4; step reads time 8 + size 4, writes status 1 + time 8;
# commit reads status 1 + time 8 + tag 8 and writes 17 (left) or reads 12 more and writes 20 (kept)
MODEL_BYTES = 12 + 12 + 9 + 17 + 17
HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events", type=int, default=10**7)
    ap.add_argument("--hosts", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from shadow_amd import Router
    from shadow_amd import events as ev
    if not torch.cuda.is_available():
        sys.exit("inbound_bench: no GPU (there is nothing to time without one)")
    dev = torch.device("cuda", 0)
    n, H = args.events, args.hosts
    window, t0 = 5_000_000, 10**12
    rng = np.random.default_rng(7)
    host = np.sort(rng.integers(0, H, n, dtype=np.uint32))
    t = (t0 + rng.integers(0, window, n, dtype=np.uint64)).astype(np.uint64)
    t = t[np.lexsort((t, host))]
    size = rng.choice(np.array([40, 576, 1500], np.uint32), n)
    counts = np.bincount(host, minlength=H)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    offered_bits = int(n / H * float(size.mean()) * 8 / (window * 1e-9))  # per host, bit/s
    bw = np.full(H, offered_bits * 10, np.uint64)
    bw[rng.permutation(H)[:H // 10]] = offered_bits // 10
    t_t, s_t = ev._i64(t, dev), ev._i32(size, dev)
    g_t = torch.arange(n, dtype=torch.int64, device=dev)
    o_t = ev._i64(offs, dev)
    out = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
           torch.empty(n, dtype=torch.int64, device=dev), torch.empty(H + 1, dtype=torch.int64, device=dev))
    router = Router(0)
    ms, last = [], None
    for rep in range(args.warmup + args.reps):
        inb = ev.Inbound(router, bw, 0, t0, reserve=n)
        torch.cuda.synchronize(dev)
        c0 = time.perf_counter()
        rc, res, msg = inb.step_device(t0 + window, n, t_t, s_t, g_t, o_t, n, *out)  # returns after its synchronise
        dt = (time.perf_counter() - c0) * 1e3
        if rc != 0:
            sys.exit("inbound_bench: step failed: " + msg)
        if rep >= args.warmup:
            ms.append(dt)
        last = res
        inb.close()
    med = statistics.median(ms)
    line = json.dumps({
        "tool": "inbound_bench", "events": n, "hosts": H, "window_ns": window, "reps": args.reps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "mapping": "one wave64 per host, 4 hosts per workgroup",
        "offered_bits_per_host": offered_bits, "overloaded_hosts": H // 10,
        "busiest_host_events": int(counts.max()), "mean_host_events": round(float(counts.mean()), 1),
        "step": {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)},
        "num_forwarded": int(last["num_forwarded"]), "num_dropped": int(last["num_dropped"]),
        "num_queued": int(last["num_queued"]), "min_next_wake_ns": int(last["min_next_wake_ns"]),
        "model": {"bytes_per_arrival": MODEL_BYTES, "bytes": MODEL_BYTES * n,
                  "bytes_per_s": round(MODEL_BYTES * n / (med * 1e-3), 1),
                  "share_of_hbm_peak": round(MODEL_BYTES * n / (med * 1e-3) / HBM_BYTES_PER_S, 4)},
        "ns_per_event_of_busiest_host": round(med * 1e6 / int(counts.max()), 1),
    })
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
