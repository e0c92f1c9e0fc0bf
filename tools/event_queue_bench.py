"""Times the device-resident event queues on the C5 round: synthetic_round(10^7 events, 10 000
hosts, seed 7) against bench.py's 10k x 10k table, pushed into a backlog of `--backlog` (10) earlier
rounds, then a pop of one window.  One process, one GPU.

The earlier rounds are the same round shifted by whole windows (send times + r * runahead, the
per-source event-id counters continued), each ordered by srg_order_packet_events_device and pushed.

  (m)  srg_event_queues_push_device of round `backlog` into the backlog              (the merge)
  (s)  srg_order_packet_events_device over the concatenated backlog + batch arrays   (the re-sort:
       what the library could do before to get the same merged order)
  (p)  srg_event_queues_pop_device of one window after (m)

Default: no pops while the backlog is built (it is exactly backlog x events; the popped window is the
first one).  --round-loop pops every window on the way, as a simulation does (pop -> send -> push):
the backlog then holds what has not been delivered yet, popped prefixes are stored in front of the
hosts' segments when (m) runs, and (s) sorts as many events as (m)'s result holds.

The queues are rebuilt for every repetition (a push cannot be undone); after the warm-up the
variants alternate, one call each per repetition; every call ends in a stream synchronise and is
timed with a host clock.  Median, min and max per variant go out as one JSON line.

Yardstick for (m): its median must be below (s)'s median by more than the two variants' min-max
spreads combined.  Also reported: (m)'s bytes/s against its own traffic model, 64 B per live event
of the result (32 read + 32 written), and (p)'s against 32 B per popped event.
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

MERGE_BYTES = 64  # per live event of the merged result: 32 B read + 32 B written
POP_BYTES = 32    # per popped event


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events", type=int, default=10**7)
    ap.add_argument("--hosts", type=int, default=10000)
    ap.add_argument("--backlog", type=int, default=10, help="earlier rounds pushed before the timed one")
    ap.add_argument("--round-loop", action="store_true", help="pop every window while the backlog is built")
    ap.add_argument("--reps", type=int, default=7, help="timed calls per variant (>= 5 for a figure)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from shadow_amd import Router
    from shadow_amd import _native as N
    from shadow_amd import events as ev
    if not torch.cuda.is_available():
        sys.exit("event_queue_bench: no GPU (there is nothing to time without one)")
    dev = torch.device("cuda", 0)
    n, H, R = args.events, args.hosts, args.backlog
    runahead = 5_000_000
    b, round_end0 = ev.synthetic_round(n, H, H, seed=7, runahead=runahead)
    t0 = round_end0 - runahead
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)  # bench.py's C5 table
    lat = torch.randint(1_000_000, 100_000_000, (H, H), dtype=torch.int64, device=dev, generator=gen)
    router = Router(0)

    # round r: the same sends one window later each, the per-source counters continued
    id_step = int(b["src_event_id"].max()) + 1
    base = ev.DeviceEventBatch(b, H, round_end0, dev)
    rounds = []
    for r in range(R + 1):
        db = ev.DeviceEventBatch.__new__(ev.DeviceEventBatch)
        db.n, db.num_hosts, db.round_end_ns = n, H, round_end0 + r * runahead
        db.t = dict(base.t)
        db.t["send_time_ns"] = base.t["send_time_ns"] + r * runahead
        db.t["src_event_id"] = base.t["src_event_id"] + r * id_step
        deliver = torch.empty(n, dtype=torch.int64, device=dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        off = torch.empty(H + 1, dtype=torch.int64, device=dev)
        ev.order_packet_events_device(router, db, lat, deliver, order, off)
        rounds.append((db, deliver, order))
    del b

    def build():
        """The backlog: rounds 0 .. R-1 pushed (and, --round-loop, every window popped on the way)."""
        q = ev.EventQueues(router, H, reserve=(R + 1) * n)
        for r in range(R):
            db, deliver, order = rounds[r]
            q.push(db, deliver, order, n)
            if args.round_loop:
                pop_window(q, r)
        return q

    pop_out = {}

    def pop_window(q, r):
        """The window behind round r's barrier: [round_end_r, round_end_r + runahead)."""
        until = t0 + (r + 2) * runahead
        rc, res, msg = q.pop_device(until, 0, None, None, None, None, None)
        need = int(res["num_moved"]) if rc != 0 else 0
        if need > pop_out.get("cap", 0):
            pop_out.update(cap=need, t=torch.empty(need, dtype=torch.int64, device=dev),
                           src=torch.empty(need, dtype=torch.int32, device=dev),
                           eid=torch.empty(need, dtype=torch.int64, device=dev),
                           tag=torch.empty(need, dtype=torch.int64, device=dev),
                           off=torch.empty(H + 1, dtype=torch.int64, device=dev))
        if need == 0:
            return 0.0, res
        torch.cuda.synchronize(dev)
        c0 = time.perf_counter()
        rc, res, msg = q.pop_device(until, pop_out["cap"], pop_out["t"], pop_out["src"], pop_out["eid"], pop_out["tag"],
                                    pop_out["off"])
        ms = (time.perf_counter() - c0) * 1e3
        if rc != 0:
            sys.exit("event_queue_bench: pop failed: " + msg)
        return ms, res

    # the re-sort's input: as many events as the merge's result holds, from the rounds concatenated
    q = build()
    backlog_live = len(q)
    q.close()
    n_sort = backlog_live + n
    cat = ev.DeviceEventBatch.__new__(ev.DeviceEventBatch)
    cat.n, cat.num_hosts, cat.round_end_ns = n_sort, H, round_end0
    cat.t = {k: torch.cat([rounds[r][0].t[k] for r in range(R + 1)])[-n_sort:].contiguous() for k in base.t}
    s_deliver = torch.empty(n_sort, dtype=torch.int64, device=dev)
    s_order = torch.empty(n_sort, dtype=torch.int32, device=dev)
    s_off = torch.empty(H + 1, dtype=torch.int64, device=dev)
    last = {}

    def run_once(timed):
        q = build()
        db, deliver, order = rounds[R]
        torch.cuda.synchronize(dev)
        c0 = time.perf_counter()
        last["m"] = q.push(db, deliver, order, n)  # returns after its stream synchronise
        m = (time.perf_counter() - c0) * 1e3
        torch.cuda.synchronize(dev)
        c0 = time.perf_counter()
        last["s"] = ev.order_packet_events_device(router, cat, lat, s_deliver, s_order, s_off)
        s = (time.perf_counter() - c0) * 1e3
        p, last["p"] = pop_window(q, R if args.round_loop else 0)
        q.close()
        if timed:
            ms["m"].append(m)
            ms["s"].append(s)
            ms["p"].append(p)

    ms = {"m": [], "s": [], "p": []}
    for _ in range(args.warmup):
        run_once(False)
    for _ in range(args.reps):
        run_once(True)
    stat = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ms.items()}
    spread = {k: stat[k]["max_ms"] - stat[k]["min_ms"] for k in stat}
    live_after = int(last["m"]["num_queued"])
    popped = int(last["p"]["num_moved"])
    margin = stat["s"]["median_ms"] - stat["m"]["median_ms"]
    out = {
        "tool": "event_queue_bench", "events": n, "hosts": H, "backlog_rounds": R, "round_loop": bool(args.round_loop),
        "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "merge_tile": int(N.lib().srg_event_queues_merge_tile()),
        "backlog_live_events": backlog_live, "backlog_over_batch": round(backlog_live / n, 3),
        "m_push_merge": stat["m"], "s_resort_backlog_plus_batch": stat["s"], "p_pop_one_window": stat["p"],
        "resort": {"events": n_sort, "key_bits": last["s"]["key_bits"], "radix_passes": last["s"]["radix_passes"]},
        "yardstick": {"s_minus_m_median_ms": round(margin, 4),
                      "spreads_combined_ms": round(spread["m"] + spread["s"], 4),
                      "merge_beats_resort": margin > spread["m"] + spread["s"]},
        "merge_model": {"live_events_after": live_after, "bytes": MERGE_BYTES * live_after,
                        "bytes_per_s": round(MERGE_BYTES * live_after / (stat["m"]["median_ms"] * 1e-3), 1)},
        "pop_model": {"popped_events": popped, "bytes": POP_BYTES * popped,
                      "bytes_per_s": round(POP_BYTES * popped / (stat["p"]["median_ms"] * 1e-3), 1)
                      if stat["p"]["median_ms"] > 0 else None,
                      "min_next_event_ns_after": int(last["p"]["min_next_event_ns"])},
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
