"""Times the send batch beside the packet-event batch on the C5 round: synthetic_round(10^7 events,
10 000 hosts, seed 7) against a 10k x 10k table resident in HBM.  One process, one GPU.

  (a)  srg_order_packet_events_device                      (the bench's C5 call)
  (b)  srg_send_packets_device, loss all zero, no counts   (the same work plus the drop decision)
  (c)  srg_send_packets_device, mean loss 1 %, counts on
  (c0) as (c) without the counts                           (so that c - c0 = the counts pass)

After the warm-up the variants alternate, one call each per repetition; every call ends in a
stream synchronise and is timed with a host clock.  Median, min and max per variant go out as one
JSON line.  (b)'s outputs are compared with (a)'s before anything is timed.

The yardstick for (b) is (a) in the same run: (b) may take (a)'s median plus (a)'s own min-max
spread plus the time its extra bytes take -- 12 B read (chance, payload) + a 4 B loss gather + 1 B
status written per event -- at the byte rate k_ev_prep reaches in (a) (48 B per event: 4 x u32 +
2 x u64 read, an 8 B table gather, 8 B deliver written).  k_ev_prep's time comes from a kernel trace
taken in a run of its own (rocprofv3 --kernel-trace --stats ... -- python tools/send_batch_bench.py
--reps 2) and is passed in with --kernel-stats <its kernel_stats.csv>; without it the allowance
prices the extra bytes at the HBM peak of 8 TB/s (the tightest allowance) and says so.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PREP_BYTES = 48    # k_ev_prep<false> per event
EXTRA_BYTES = 17   # k_ev_prep<true> (the send call) on top of it


def kernel_avg_us(path):
    """{kernel name (up to its argument list): average us} from a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = (row.get("Name") or "").split("(")[0].replace("void ", "").replace("srg::", "").strip()
            if name.endswith(".kd"):
                name = name[:-3]
            if name and row.get("AverageNs"):
                out[name] = float(row["AverageNs"]) / 1e3
    return out


def distinct_pairs_per_wave(b, status, tn):
    """k_ev_counts' atomics per wave: a wave takes 64 consecutive events and issues one atomic per
    distinct (src_node, dst_node) among its sent ones."""
    import numpy as np
    n = len(status)
    pair = b["src_node"].astype(np.int64) * tn + b["dst_node"]
    pair = np.where(status.astype(bool), pair, -1)
    pad = (-n) % 64
    rows = np.sort(np.r_[pair, np.full(pad, -1, np.int64)].reshape(-1, 64), axis=1)
    new = np.c_[rows[:, :1] >= 0, (rows[:, 1:] != rows[:, :-1]) & (rows[:, 1:] >= 0)]
    return float(new.sum() / len(rows)), float((rows >= 0).sum() / len(rows))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events", type=int, default=10**7)
    ap.add_argument("--hosts", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7, help="timed calls per variant (>= 5 for a figure)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loss", type=float, default=0.01, help="mean packet loss of (c)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a traced run")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    from shadow_amd import Router
    from shadow_amd import events as ev
    if not torch.cuda.is_available():
        sys.exit("send_batch_bench: no GPU (there is nothing to time without one)")
    dev = torch.device("cuda", 0)
    n, H = args.events, args.hosts
    b, round_end, loss_host = ev.synthetic_round(n, H, H, seed=7, loss=args.loss)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)  # bench.py's C5 table
    lat = torch.randint(1_000_000, 100_000_000, (H, H), dtype=torch.int64, device=dev, generator=gen)
    loss0 = torch.zeros((H, H), dtype=torch.float32, device=dev)
    loss1 = torch.from_numpy(loss_host).to(dev)
    del loss_host
    db = ev.DeviceSendBatch(b, H, round_end, 0, dev)
    t_zero = ev.DevicePathTable(H, latency_ns=lat, packet_loss=loss0)
    t_loss = ev.DevicePathTable(H, latency_ns=lat, packet_loss=loss1)
    counts = torch.zeros((H, H), dtype=torch.int64, device=dev)

    def outputs():
        return (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
                torch.empty(n, dtype=torch.int32, device=dev), torch.empty(H + 1, dtype=torch.int64, device=dev))

    st_a, del_a, ord_a, off_a = outputs()
    st_b, del_b, ord_b, off_b = outputs()
    router = Router(0)
    last = {}

    def run_a():
        last["a"] = ev.order_packet_events_device(router, db, lat, del_a, ord_a, off_a)

    def run_b():
        last["b"] = ev.send_packets_device(router, db, t_zero, st_b, del_b, ord_b, off_b)

    def run_c():
        last["c"] = ev.send_packets_device(router, db, t_loss, st_b, del_b, ord_b, off_b, counts)

    def run_c0():
        last["c0"] = ev.send_packets_device(router, db, t_loss, st_b, del_b, ord_b, off_b)

    variants = [("a", run_a), ("b", run_b), ("c", run_c), ("c0", run_c0)]
    run_a()
    run_b()
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(del_a, del_b) and torch.equal(ord_a, ord_b) and torch.equal(off_a, off_b)
                and bool(st_b.all()) and last["b"]["num_dropped"] == 0)
    if not same:
        sys.exit("send_batch_bench: (b) differs from (a) on the same batch")
    for _ in range(args.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k, _ in variants}
    for _ in range(args.reps):
        for k, fn in variants:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()  # returns after its stream synchronise
            ms[k].append((time.perf_counter() - t0) * 1e3)
    stat = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ms.items()}
    res_c = last["c"]
    status = st_b.cpu().numpy()  # the last call was (c0): the same decisions as (c)
    pairs, sent = distinct_pairs_per_wave(b, status, H)

    kern = kernel_avg_us(args.kernel_stats) if args.kernel_stats else {}
    prep_us = kern.get("k_ev_prep<false>")
    if prep_us:
        rate = PREP_BYTES * n / (prep_us * 1e-6)
        rate_src = "k_ev_prep<false> in the kernel trace"
    else:
        rate, rate_src = 8e12, "no kernel trace given: the HBM peak of 8 TB/s (the tightest allowance)"
    spread = stat["a"]["max_ms"] - stat["a"]["min_ms"]
    extra_ms = EXTRA_BYTES * n / rate * 1e3
    allowance = stat["a"]["median_ms"] + spread + extra_ms
    out = {
        "tool": "send_batch_bench", "events": n, "hosts": H, "table_n": H, "reps": args.reps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0),
        "a_order_packet_events": stat["a"], "b_send_no_loss_no_counts": stat["b"],
        "c_send_loss_counts": stat["c"], "c0_send_loss_no_counts": stat["c0"],
        "b_equals_a_outputs": same,
        "b_yardstick": {"a_median_ms": stat["a"]["median_ms"], "a_spread_ms": round(spread, 4),
                        "prep_bytes_per_s": round(rate, 1), "prep_rate_source": rate_src,
                        "extra_bytes_ms": round(extra_ms, 4), "allowed_ms": round(allowance, 4),
                        "b_within": stat["b"]["median_ms"] <= allowance},
        "c": {"mean_loss": args.loss, "num_sent": res_c["num_sent"], "num_dropped": res_c["num_dropped"],
              "key_bits": res_c["key_bits"], "radix_passes": res_c["radix_passes"],
              "counts_pass_ms": round(stat["c"]["median_ms"] - stat["c0"]["median_ms"], 4),
              "counts_share": round((stat["c"]["median_ms"] - stat["c0"]["median_ms"]) / stat["c"]["median_ms"], 4),
              "sent_events_per_wave": round(sent, 2), "distinct_pairs_per_wave": round(pairs, 2)},
        "kernels_avg_us": {k: round(v, 2) for k, v in kern.items() if k.startswith(("k_ev_", "k_rs_"))},
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
