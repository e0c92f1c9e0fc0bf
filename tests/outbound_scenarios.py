"""The scenarios the outbound tests share (test_outbound_cpu.py, test_outbound_gpu.py): each is
(name, bw_up_bits, sockets_per_host, qdisc, sim_start_ns, bootstrap_end_ns, steps), steps =
[(until_ns, [per-host list of offers (time, slot, priority, size, flags, tag)])].  Everything is fixed
data: seeded generators, fixed window grids; windows in which a host can have neither an offer nor a
forward task (as outbound_ref.py finds while the list is built) are left out, the way the round loop
skips them with next_window."""
import json
import os
import random
import subprocess

import outbound_ref as R

MS = 1_000_000
SIM_START = 1_000 * MS
U64 = R.U64
LOCAL, BARRIER = R.OFFER_LOCAL, R.OFFER_BARRIER
OVERLOAD_SEED = 3  # picked on the CPU: with it the scenarios reach every branch counter of outbound_ref.py
CHUNK_COUNTS = (0, 1, 63, 64, 65, 129)  # per-host offers per step: the step kernel's chunk edges
SHAPE_SOCKETS = (1, 2, 3, 7, 64, 65, 130)
HERE = os.path.dirname(os.path.abspath(__file__))


def flatten(per_host):
    """-> time, slot, priority, size, flags, tag, host_offsets lists"""
    flat = [e for a in per_host for e in a]
    offs = [0]
    for a in per_host:
        offs.append(offs[-1] + len(a))
    return tuple([e[k] for e in flat] for k in range(6)) + (offs,)


def windowed(bw, sockets, qdisc, bootstrap_end, offers, width, end, sim_start=SIM_START):
    """offers: per-host lists; windows [k * width, (k + 1) * width) from sim_start to `end`."""
    ref = R.Outbound(bw, sockets, qdisc, sim_start, bootstrap_end)
    pos = [0] * len(bw)
    steps, w = [], sim_start
    while w < end:
        until = w + width
        per_host = []
        for h, a in enumerate(offers):
            j = pos[h]
            while j < len(a) and a[j][0] < until:
                j += 1
            per_host.append(a[pos[h]:j])
            pos[h] = j
        due = any(hh.pending and hh.wake < until for hh in ref.hosts)
        if due or any(per_host):
            steps.append((until, per_host))
            ref.step(until, *flatten(per_host))
        w = until
    assert all(p == len(a) for p, a in zip(pos, offers))
    return steps


def burst_offers(seed, t0, sockets, n=300, bursts=2, control=0.15, local=0.03, barrier=0.3, unique=True, tag0=0):
    """One host's offers: `bursts` bursts of n packets over `sockets` sockets, sizes from {40, 576,
    1500}, gaps from {0, 0, 0.5, 1, 3} ms (so offers land on the bucket's refill boundaries, where
    the wakes are), 1 s of silence between the bursts.  Data priorities come from a counter, control
    packets (priority 0, 40 B) are a `control` share; the barrier bit sits on the first offer of a
    share `barrier` of the events (an event: the offers between two gaps)."""
    rng = random.Random(seed)
    out, t, prio, first = [], t0, 0, True
    for _ in range(bursts):
        for _ in range(n):
            prio += 1
            ctl = rng.random() < control
            fl = (LOCAL if rng.random() < local else 0) | (BARRIER if first and rng.random() < barrier else 0)
            out.append((t, rng.randrange(sockets), 0 if ctl else (prio if unique else rng.randrange(1, 6)),
                        40 if ctl else rng.choice((40, 576, 1500)), fl, tag0 + len(out)))
            gap = rng.choice((0, 0, 500_000, 1_000_000, 3_000_000))
            first = gap > 0
            t += gap
        t += 1_000 * MS
        first = True
    return out


def overload(width, qdisc, seed=OVERLOAD_SEED):
    """One 1 Mbit/s host, two bursts of 300 packets over 5 sockets with control packets, the bootstrap
    end 20 ms after the first offer; width None: one step."""
    t0 = SIM_START + 5 * MS
    arr = burst_offers(seed, t0, 5)
    end = arr[-1][0] + 4_000 * MS
    name = "overload_q%d_%s" % (qdisc, "one_step" if width is None else "%dms" % (width // MS))
    steps = [(end, [arr])] if width is None else windowed([1_000_000], [5], qdisc, t0 + 20 * MS, [arr], width, end)
    return (name, [1_000_000], [5], qdisc, SIM_START, t0 + 20 * MS, steps)


def chunk_edges(num_hosts, qdisc):
    """Per-host offers per step of 0, 1, 63, 64, 65, 129; slow hosts keep a backlog that crosses a
    chunk edge between steps."""
    rng = random.Random(2000 + num_hosts)
    bws = (U64, 1_000_000, 10_000_000, 7_999, 100_000_000)
    bw = [bws[h % len(bws)] for h in range(num_hosts)]
    sockets = [(1, 2, 5, 8)[h % 4] for h in range(num_hosts)]
    steps, tag, prio = [], 0, [0] * num_hosts
    width = 20 * MS
    for k in range(4):
        w = SIM_START + k * width
        per_host = []
        for h in range(num_hosts):
            n = CHUNK_COUNTS[(h + k) % len(CHUNK_COUNTS)]
            ts = sorted(w + rng.randrange(0, width // 250_000) * 250_000 for _ in range(n))
            a = []
            for t in ts:
                prio[h] += 1
                ctl = rng.random() < 0.1
                fl = (LOCAL if rng.random() < 0.05 else 0) | (BARRIER if rng.random() < 0.2 else 0)
                tag += 1
                a.append((t, rng.randrange(sockets[h]), 0 if ctl else prio[h], rng.choice((0, 40, 576, 1500)), fl, tag))
            per_host.append(a)
        steps.append((w + width, per_host))
    steps.append((SIM_START + 3_000 * MS, [[] for _ in range(num_hosts)]))  # the drain
    return ("chunk_edges_%d_q%d" % (num_hosts, qdisc), bw, sockets, qdisc, SIM_START, SIM_START + 30 * MS, steps)


def shapes(qdisc):
    """Hosts with 1, 2, 3, 7, 64, 65, 130 sockets at 1 Mbit/s: every socket is offered two packets in
    the same nanosecond, so the whole heap (or ring) is built before the first task runs; the steps cut
    the drain where the structure is still large."""
    rng = random.Random(77 + qdisc)
    t = SIM_START + 2 * MS
    per_host, tag = [], 0
    for n in SHAPE_SOCKETS:
        slots = list(range(n)) * 2
        rng.shuffle(slots)
        prios = rng.sample(range(1, 10 * n + 10), 2 * n)
        a = []
        for s, p in zip(slots, prios):
            tag += 1
            a.append((t, s, 0 if rng.random() < 0.1 else p, rng.choice((40, 60, 120)), 0, tag))
        per_host.append(a)
    nobody = [[] for _ in SHAPE_SOCKETS]
    steps = [(t + 1, per_host)] + [(t + d * MS, nobody) for d in (5, 30, 120, 1_000)]
    return ("shapes_q%d" % qdisc, [1_000_000] * len(SHAPE_SOCKETS), list(SHAPE_SOCKETS), qdisc, SIM_START, SIM_START, steps)


def boundaries(qdisc):
    """Hand-made edges, one host each (all in one instance):
    0  1 Mbit/s: the second 1500 B packet blocks for 11 refills; the task lands exactly on the first
       step's `until` (stays pending); the next step's first offer comes exactly at that wake time with
       the barrier bit (the task runs first), a second one without it
    1  7 999 bit/s (max(1, ...) = 1 token per ms, capacity 1501): unlimited at bootstrap_end - 1,
       limited at bootstrap_end; a 1501 B packet (the whole capacity) waits 1500 refills and passes
    2  unlimited, 70 offers in one step
    3  1 Mbit/s: local packets of any size pass without tokens, but wait behind the cached packet;
       size-0 packets on an empty bucket
    4  1 Mbit/s: the same as host 0 without the barrier bit"""
    S, B = SIM_START, SIM_START + 50 * MS
    bw = [1_000_000, 7_999, U64, 1_000_000, 1_000_000]
    sockets = [3, 2, 4, 3, 3]
    t = B + 300_000  # 0.3 ms past a refill boundary
    wake = B + 11 * MS
    h0 = [(t, 0, 1, 1500, 0, 1), (t, 1, 2, 1500, 0, 2), (t, 2, 3, 40, 0, 3)]
    steps = [
        (B, [[], [(B - 1, 0, 1, 1500, 0, 100), (B - 1, 1, 2, 1500, 0, 101), (B - 1, 0, 3, 1500, 0, 102)],
             [(S, 0, 1, 1500, 0, 200)], [], []]),
        (wake, [h0, [(B, 0, 4, 1500, 0, 103), (B, 1, 5, 1501, 0, 104)],
                [(B + k * 1000, k % 4, 0 if k % 7 == 0 else 2 + k, 1500, LOCAL if k % 5 == 0 else 0, 201 + k)
                 for k in range(70)],
                [(t, 0, 1, 1500, 0, 300), (t, 1, 2, 1500, 0, 301), (t, 2, 3, 9000, LOCAL, 302), (t, 2, 4, 0, 0, 303)],
                [(e[0], e[1], e[2], e[3], e[4], 400 + e[5]) for e in h0]]),
        (wake + 5 * MS, [[(wake, 0, 0, 40, BARRIER, 4), (wake, 1, 0, 40, 0, 5)], [], [], [(wake, 0, 0, 0, 0, 304)],
                         [(wake, 0, 0, 40, 0, 404), (wake, 1, 0, 40, 0, 405)]]),
        (B + 5_000 * MS, [[], [], [], [], []]),
    ]
    return ("boundaries_q%d" % qdisc, bw, sockets, qdisc, S, B, steps)


# ---- the scenarios whose qdisc operations the reference's own queue code has replayed -----------
# (tests/golden/qdisc_reference.json holds each host's traced script and that program's output)
TRICKLE_BW = 7_999  # max(1, 999 // 1000) = 1 token per 1 ms refill, capacity 1501


def trickle_offers(seed, t0, sockets, tie, unique, wakes):
    """One 7 999 bit/s host whose time axis is turned into an arbitrary offer / select interleaving.
    t0 is a refill boundary at which the bucket is full (nothing removed tokens before).  A 1501 B
    packet at t0 takes the whole bucket.  At t0 + 0.5 ms every socket gets one packet (the whole heap
    or ring stands before the next select); from then on the balance is 0 at every refill boundary
    while packets are queued, so the task at t0 + k ms sends the cached 1 B packet with the refill's
    one token, selects exactly one more and blocks on it.  Offers lie strictly between the wakes, 1 to
    3 per ms for 25 ms, then 0 or 1, and so on; a size-0 packet always conforms and a local one needs
    no tokens, so either gives a second select in the same task; after a quiet stretch that empties
    the qdisc the idle refills give short runs.  `tie` is the share of priority-0 (control) packets;
    data priorities are a counter (unique) or drawn from 1..5.  Tags count from 1."""
    rng = random.Random(seed)
    out, prio = [(t0, 0, 1, 1501, 0, 1)], 1

    def add(t, slot, size, flags):
        nonlocal prio
        prio += 1
        ctl = rng.random() < tie
        out.append((t, slot, 0 if ctl else (prio if unique else rng.randrange(1, 6)), size, flags, len(out) + 1))

    slots = list(range(sockets))
    rng.shuffle(slots)
    for slot in slots:
        add(t0 + 500_000, slot, 1, 0)
    for k in range(1, wakes + 1):
        n = rng.choice((1, 1, 2, 2, 3)) if (k // 25) % 2 == 0 else rng.choice((0, 0, 0, 1, 1))
        for j in range(n):
            add(t0 + k * MS + 200_000 * (j + 1), rng.randrange(sockets), 0 if rng.random() < 0.12 else 1,
                LOCAL if rng.random() < 0.04 else 0)
    return out


def batch_offers(seed, times, sockets, tie, unique, barrier_in=()):
    """Batch-then-drain: at each of `times` 1.5 * sockets + 6 offers of 1500 B arrive in one
    nanosecond (sockets repeat, so a socket holds several packets and control packets enter queued
    sockets), and where nothing limits the host the one task at that time drains them all.  A batch
    whose index is in `barrier_in` carries the barrier bit on its middle offer: the task runs there,
    and the rest of the batch meets an empty qdisc."""
    rng = random.Random(seed)
    out, prio = [], 0
    for b, t in enumerate(times):
        n = sockets * 3 // 2 + 6
        for j in range(n):
            prio += 1
            ctl = rng.random() < tie
            out.append((t, rng.randrange(sockets), 0 if ctl else (prio if unique else rng.randrange(1, 6)), 1500,
                        BARRIER if b in barrier_in and j == n // 2 else 0, len(out) + 1))
    return out


QDISC_TRICKLE_HOSTS = ((1, 0.5, True), (2, 0.1, False), (3, 0.0, True), (7, 0.5, False), (64, 0.1, True),
                       (65, 0.0, False), (130, 0.1, True))  # (sockets, tie, unique)
QDISC_BATCH_HOSTS = ((2, 0.5, False), (7, 0.1, True), (65, 0.1, False))


def qdisc_trickle_offers(qdisc):
    """-> (name, qdisc, bw, sockets, bootstrap_end, per-host offers, a time by which everything has left)"""
    t0 = SIM_START + 3 * MS
    bw, sockets, offers = [], [], []
    for i, (n, tie, unique) in enumerate(QDISC_TRICKLE_HOSTS):
        bw.append(TRICKLE_BW)
        sockets.append(n)
        offers.append(trickle_offers(500 + 10 * qdisc + i, t0, n, tie, unique, wakes=100))
    for i, (n, tie, unique) in enumerate(QDISC_BATCH_HOSTS):
        bw.append(U64)
        sockets.append(n)
        offers.append(batch_offers(600 + 10 * qdisc + i, (t0 + 250_000, t0 + 40 * MS + 1), n, tie, unique, barrier_in=(1,)))
    return "qdisc_trickle_q%d" % qdisc, qdisc, bw, sockets, SIM_START, offers, t0 + 2_000 * MS


def qdisc_bootstrap_offers(qdisc):
    """Limited hosts before bootstrap_end: two batches drain at once, whatever their size; past it the
    same hosts trickle."""
    boot = SIM_START + 20 * MS
    bw, sockets, offers = [], [], []
    for i, (n, tie, unique) in enumerate(((3, 0.5, True), (7, 0.1, False), (64, 0.0, True))):
        bw.append(TRICKLE_BW)
        sockets.append(n)
        a = batch_offers(700 + 10 * qdisc + i, (SIM_START + 2 * MS, boot - 1), n, tie, unique, barrier_in=(0,))
        b = trickle_offers(800 + 10 * qdisc + i, boot + 2 * MS, n, tie, unique, wakes=40)
        offers.append(a + [(e[0], e[1], e[2], e[3], e[4], len(a) + e[5]) for e in b])
    return "qdisc_bootstrap_q%d" % qdisc, qdisc, bw, sockets, boot, offers, boot + 1_000 * MS


def qdisc_scenario(spec, width=10 * MS):
    """Windows of `width` while offers arrive (None: everything in one step), then one step to `far`,
    after which nothing is queued."""
    name, qdisc, bw, sockets, boot, offers, far = spec
    nobody = [[] for _ in bw]
    if width is None:
        return (name + "_one_step", bw, sockets, qdisc, SIM_START, boot, [(far, offers)])
    last = max(a[-1][0] for a in offers)
    end = SIM_START + ((last - SIM_START) // width + 1) * width
    steps = windowed(bw, sockets, qdisc, boot, offers, width, end) + [(far, nobody)]
    return (name, bw, sockets, qdisc, SIM_START, boot, steps)


def qdisc_specs(qdisc):
    return [qdisc_trickle_offers(qdisc), qdisc_bootstrap_offers(qdisc)]


def qdisc_scenarios():
    return [qdisc_scenario(spec) for q in (R.QDISC_FIFO, R.QDISC_ROUND_ROBIN) for spec in qdisc_specs(q)]


def trace_ref(scn, drained=True):
    """-> (per-host (script, output) texts in the reference program's format, the reference's outs)"""
    _, bw, sockets, qdisc, sim_start, boot, steps = scn
    ref = R.Outbound(bw, sockets, qdisc, sim_start, boot, trace=True)
    outs = [ref.step(until, *flatten(per_host)) for until, per_host in steps]
    assert not drained or outs[-1][4]["num_queued"] == 0
    return [(R.trace_script(qdisc, n, h.trace), R.trace_output(h.trace)) for n, h in zip(sockets, ref.hosts)], outs


def free_script(seed, qdisc, sockets, tie, unique):
    """A free-form script for the reference program: offers and selects interleaved with no time axis.
    20 ops with offers and selects even, an offer to every socket in a shuffled order (after it every
    socket is queued), 100 + sockets ops with offers and selects even again, then selects until one
    finds the qdisc empty."""
    rng = random.Random(seed)
    lines, prio, queued = ["%d %d" % (qdisc, sockets)], 0, 0

    def select():
        nonlocal queued
        lines.append("s")
        queued -= queued > 0

    def offer(slot):
        nonlocal prio, queued
        prio += 1
        ctl = rng.random() < tie
        lines.append("o %d %d %d" % (slot, 0 if ctl else (prio if unique else rng.randrange(1, 6)), prio))
        queued += 1

    slots = list(range(sockets))
    rng.shuffle(slots)
    for phase in (20, None, 100 + sockets):
        if phase is None:
            for slot in slots:
                offer(slot)
            continue
        for _ in range(phase):
            if rng.random() < 0.5:
                select()
            else:
                offer(rng.randrange(sockets))
    lines += ["s"] * (queued + 1)
    return "\n".join(lines) + "\n"


FREE_SOCKETS = (1, 2, 3, 7, 64, 65, 130)
FREE_TIES = (0.0, 0.1, 0.5)


def free_scripts(seed0, count):
    """`count` scripts per qdisc: sockets, tie share and priority mode cycle at different periods (7, 3,
    2), so every value and, from 42 on, every combination occurs."""
    return [dict(seed=seed0 + k, qdisc=q, sockets=FREE_SOCKETS[k % 7], tie=FREE_TIES[k % 3], unique=k % 2 == 0,
                 script=free_script(seed0 + k, q, FREE_SOCKETS[k % 7], FREE_TIES[k % 3], k % 2 == 0))
            for q in (R.QDISC_FIFO, R.QDISC_ROUND_ROBIN) for k in range(count)]


def kat_script(k):
    """A KAT's one host traced over its steps (some end with packets queued) -> (script, output)."""
    return trace_ref(kat_scenario(k), drained=False)[0][0]


def run_qdisc_ref(exe, scripts):
    """Feeds the scripts to the reference program (oracle/_ref/qdisc_ref) in one process, an "e" line
    after each -> the output text per script."""
    r = subprocess.run([exe], input="".join(sc + "e\n" for sc in scripts), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    outs = r.stdout.split("e\n")
    assert len(outs) == len(scripts) + 1 and outs[-1] == ""
    return outs[:-1]


def load_qdisc_reference():
    with open(os.path.join(HERE, "golden", "qdisc_reference.json")) as f:
        return json.load(f)


def load_kats():
    with open(os.path.join(HERE, "golden", "outbound_kats.json")) as f:
        return json.load(f)["tests"]


def kat_scenario(k):
    return ("kat_" + k["name"], [k["bw"]], [k["sockets"]], k["qdisc"], k["sim_start"], k["bootstrap_end"],
            [(s["until"], [[tuple(o) for o in s["offers"]]]) for s in k["steps"]])


def all_scenarios():
    out = [kat_scenario(k) for k in load_kats()]
    for q in (R.QDISC_FIFO, R.QDISC_ROUND_ROBIN):
        out += [overload(None, q), overload(50 * MS, q), overload(1 * MS, q), boundaries(q), shapes(q)]
        out += [chunk_edges(h, q) for h in (1, 3, 64, 65)]
    return out + qdisc_scenarios()


def run_ref(scn):
    """-> (per-step (status, time, tag, offsets, result), per-step host states, per-step qdisc arrays)"""
    _, bw, sockets, qdisc, sim_start, boot, steps = scn
    ref = R.Outbound(bw, sockets, qdisc, sim_start, boot)
    outs, states, orders = [], [], []
    for until, per_host in steps:
        outs.append(ref.step(until, *flatten(per_host)))
        states.append([ref.host_state(h) for h in range(len(bw))])
        orders.append([ref.host_order(h) for h in range(len(bw))])
    return outs, states, orders


def concat_by_host(outs, num_hosts):
    """The per-host concatenation over steps of what left: {host: [(status, time, tag)]}."""
    acc = {h: [] for h in range(num_hosts)}
    for st, tm, tg, oo, _ in outs:
        for h in range(num_hosts):
            acc[h] += [(int(st[j]), int(tm[j]), int(tg[j])) for j in range(int(oo[h]), int(oo[h + 1]))]
    return acc


# ---- the properties' cases (test_outbound_cpu.py) ----------------------------------------------
def property_case(seed, sockets, control, unique=True):
    """200 offers of one 1 Mbit/s host past its bootstrap; -> (offers without any barrier bit, the same
    with the bit on the first offer of every event, until)."""
    arr = [(t, s, p, z, fl & ~BARRIER, g)
           for t, s, p, z, fl, g in burst_offers(seed, SIM_START + 5 * MS, sockets, n=200, bursts=1, control=control,
                                                 local=0.0, barrier=0.0, unique=unique)]
    with_b, prev = [], None
    for e in arr:
        with_b.append((e[0], e[1], e[2], e[3], e[4] | (BARRIER if e[0] != prev else 0), e[5]))
        prev = e[0]
    return arr, with_b, arr[-1][0] + 4_000 * MS


def run_one_host(offers, until, sockets, qdisc, host_cls=None):
    host = (host_cls or R.Host)(1_000_000, sockets, qdisc, SIM_START, SIM_START)
    return host.step(until, offers)
