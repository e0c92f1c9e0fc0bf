"""The scenarios the inbound tests share (test_inbound_cpu.py, test_inbound_gpu.py): each is
(name, bw_down_bits, sim_start_ns, bootstrap_end_ns, steps), steps = [(until_ns, [per-host list of
(time, size, tag)])].  Everything is fixed data: the window grids are fixed, and windows in which a
host can have neither an arrival nor a forward task (as inbound_ref.py finds while the list is
built) are left out, the way the round loop skips them with next_window."""
import random

import inbound_ref as R

MS = 1_000_000
SIM_START = 1_000 * MS
U64 = R.U64
OVERLOAD_SEED = 9  # found on the CPU: with it the overload scenario alone reaches every branch counter
CHUNK_COUNTS = (0, 1, 63, 64, 65, 129)  # per-host arrivals per step: the step kernel's chunk edges


def windowed(bw, bootstrap_end, arrivals, width, end, sim_start=SIM_START):
    """arrivals: per-host lists; windows [k * width, (k + 1) * width) from sim_start to `end`."""
    ref = R.Inbound(bw, sim_start, bootstrap_end)
    pos = [0] * len(bw)
    steps, w = [], sim_start
    while w < end:
        until = w + width
        per_host = []
        for h, a in enumerate(arrivals):
            j = pos[h]
            while j < len(a) and a[j][0] < until:
                j += 1
            per_host.append(a[pos[h]:j])
            pos[h] = j
        due = any(hh.pending and hh.wake < until for hh in ref.hosts)
        if due or any(per_host):
            steps.append((until, per_host))
            flat = [e for a in per_host for e in a]
            offs = [0]
            for a in per_host:
                offs.append(offs[-1] + len(a))
            ref.step(until, [e[0] for e in flat], [e[1] for e in flat], [e[2] for e in flat], offs)
        w = until
    assert all(p == len(a) for p, a in zip(pos, arrivals))
    return steps


def overload(width, seed=OVERLOAD_SEED):
    """One 1 Mbit/s host, two bursts of 300 packets, 1 s of silence between them, the bootstrap end
    20 ms after the first arrival."""
    t0 = SIM_START + 5 * MS
    arr = R.overload_arrivals(seed, t0)
    return ("overload_%dms" % (width // MS), [1_000_000], SIM_START, t0 + 20 * MS,
            windowed([1_000_000], t0 + 20 * MS, [arr], width, arr[-1][0] + 4_000 * MS))


def overload_one_step(seed=OVERLOAD_SEED):
    t0 = SIM_START + 5 * MS
    arr = R.overload_arrivals(seed, t0)
    return ("overload_one_step", [1_000_000], SIM_START, t0 + 20 * MS, [(arr[-1][0] + 4_000 * MS, [arr])])


def chunk_edges(num_hosts):
    """Per-host arrivals per step of 0, 1, 63, 64, 65, 129; slow hosts keep a backlog that crosses a
    chunk edge between steps."""
    rng = random.Random(1000 + num_hosts)
    bws = (U64, 1_000_000, 10_000_000, 7_999, 100_000_000)
    bw = [bws[h % len(bws)] for h in range(num_hosts)]
    steps, tag = [], 0
    width = 20 * MS
    for k in range(4):
        w = SIM_START + k * width
        per_host = []
        for h in range(num_hosts):
            n = CHUNK_COUNTS[(h + k) % len(CHUNK_COUNTS)]
            ts = sorted(w + rng.randrange(0, width // (250_000)) * 250_000 for _ in range(n))
            per_host.append([(t, rng.choice((0, 40, 576, 1500)), (tag := tag + 1)) for t in ts])
        steps.append((w + width, per_host))
    steps.append((SIM_START + 3_000 * MS, [[] for _ in range(num_hosts)]))  # the drain
    return ("chunk_edges_%d" % num_hosts, bw, SIM_START, SIM_START + 30 * MS, steps)


def boundaries():
    """Hand-made edges, one host each (all in one instance):
    0  1 Mbit/s: the second 1500 B packet blocks for 11 refills; the task lands exactly on the first
       step's `until` (stays pending), an arrival comes exactly at that wake time (a refill boundary)
       and is enqueued before the task
    1  7 999 bit/s (max(1, ...) = 1 token per ms, capacity 1501): unlimited at bootstrap_end - 1,
       limited at bootstrap_end; a 1501 B packet (the whole capacity) waits 1500 refills and passes
    2  unlimited
    3  1 Mbit/s, size-0 packets behind a blocked packet and on an empty bucket"""
    S, B = SIM_START, SIM_START + 50 * MS
    bw = [1_000_000, 7_999, U64, 1_000_000]
    t = B + 300_000  # 0.3 ms past a refill boundary
    wake = B + 11 * MS
    steps = [
        (B, [[], [(B - 1, 1500, 100), (B - 1, 1500, 101), (B - 1, 1500, 102)], [(S, 1500, 200)], []]),
        (wake, [[(t, 1500, 1), (t, 1500, 2)], [(B, 1500, 103), (B, 1501, 104)],
                [(B + k * 1000, 1500, 201 + k) for k in range(70)], [(t, 1500, 300), (t, 1500, 301), (t, 0, 302)]]),
        (wake + 5 * MS, [[(wake, 1500, 3), (wake, 40, 4)], [], [], [(wake, 0, 303)]]),
        (B + 5_000 * MS, [[], [], [], []]),
    ]
    return ("boundaries", bw, S, B, steps)


def all_scenarios():
    return ([overload_one_step(), overload(50 * MS), overload(1 * MS), boundaries()] +
            [chunk_edges(h) for h in (1, 3, 64, 65)])


def flatten(per_host):
    """-> time, size, tag, host_offsets lists"""
    flat = [e for a in per_host for e in a]
    offs = [0]
    for a in per_host:
        offs.append(offs[-1] + len(a))
    return [e[0] for e in flat], [e[1] for e in flat], [e[2] for e in flat], offs


def run_ref(scn):
    """-> (per-step (status, time, tag, offsets, result), per-step list of host states)"""
    _, bw, sim_start, boot, steps = scn
    ref = R.Inbound(bw, sim_start, boot)
    outs, states = [], []
    for until, per_host in steps:
        outs.append(ref.step(until, *flatten(per_host)))
        states.append([ref.host_state(h) for h in range(len(bw))])
    return outs, states


def concat_by_host(outs, num_hosts):
    """The per-host concatenation over steps of what left: {host: [(status, time, tag)]}."""
    acc = {h: [] for h in range(num_hosts)}
    for st, tm, tg, oo, _ in outs:
        for h in range(num_hosts):
            acc[h] += [(int(st[j]), int(tm[j]), int(tg[j])) for j in range(int(oo[h]), int(oo[h + 1]))]
    return acc
