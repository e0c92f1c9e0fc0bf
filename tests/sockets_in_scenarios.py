"""Scenarios shared by tests/test_sockets_in_cpu.py (restatement vs sockets_in_rule.h) and
tests/test_sockets_in_gpu.py (restatement vs the device step).  A scenario is a dict:
  name, sockets_per_host, packets (protocol, src_ip, src_port, dst_port, total, payload: lists by tag),
  ops: a list of
    ("configure", entries)        entries as SocketsInRef.configure takes them
    ("associate", entries)        may be refused: the record holds the error code
    ("disassociate", entries)
    ("step", status | None, time, tag, host_off, deliver_status, r_time, r_slot, r_flags, r_host_off)
    ("reset", host)               host_counters(host, reset=True)
run_ref() applies them to the restatement and returns one record per op."""
import random

import sockets_in_ref as R

UDP_PROTO, TCP_PROTO = 17, 6
HDR = 28  # CONFIG_HEADER_SIZE_UDPIP
SIZES = (0, 1, 63, 64, 65, 129)
MODES = ("deliveries", "reads", "alternating")


class Builder:
    """Collects packets (a fresh tag per delivery) and per-host delivery / read lists for one step."""

    def __init__(self, sockets_per_host):
        self.nsock = list(sockets_per_host)
        self.H = len(self.nsock)
        self.pk = [[] for _ in range(6)]
        self.ops = []
        self.new_step()

    def new_step(self):
        self.d = [[] for _ in range(self.H)]  # (status, time, tag)
        self.r = [[] for _ in range(self.H)]  # (time, slot, flags)

    def packet(self, proto, sip, sport, dport, payload, total=None):
        for col, v in zip(self.pk, (proto, sip, sport, dport, payload + HDR if total is None else total, payload)):
            col.append(v)
        return len(self.pk[0]) - 1

    def deliver(self, h, t, tag, status=1):
        self.d[h].append((status, t, tag))

    def read(self, h, t, slot, flags=0):
        self.r[h].append((t, slot, flags))

    def end_step(self, deliver_status=1, with_status=True):
        st, tm, tg, off, rt, rs, rf, roff = [], [], [], [0], [], [], [], [0]
        for h in range(self.H):
            for s, t, g in self.d[h]:
                st.append(s), tm.append(t), tg.append(g)
            off.append(len(tm))
            for t, s, f in self.r[h]:
                rt.append(t), rs.append(s), rf.append(f)
            roff.append(len(rt))
        self.ops.append(("step", st if with_status else None, tm, tg, off, deliver_status, rt, rs, rf, roff))
        self.new_step()

    def scenario(self, name):
        return dict(name=name, sockets_per_host=self.nsock, packets=self.pk, ops=self.ops)


def wildcard_assoc(b, proto=UDP_PROTO):
    return [(h, proto, 1000 + s, 0, 0, s) for h in range(b.H) for s in range(b.nsock[h])]


def wave_sizes(H, spp, steps, seed=1):
    """Every socket sees op counts 0, 1, 63, 64, 65, 129 as pure deliveries, pure reads and
    alternating (strictly increasing times, so the chain really alternates); elsewhere ties are
    frequent.  Limits are small enough that buffers fill inside runs; a tenth of the packets go to
    an unknown port."""
    rng = random.Random(seed * 1000 + H * 10 + spp)
    b = Builder([spp] * H)
    b.ops.append(("associate", wildcard_assoc(b)))
    b.ops.append(("configure", [(h, s, R.UDP, 0, 0, 0, 100 * ((h * spp + s) % 7 * 10 + 5)) for h in range(H) for s in range(spp)]))
    t = [10**9] * H
    for step in range(steps):
        for h in range(H):
            seqs = []
            for s in range(spp):
                c = h * spp + s + step
                n, mode = SIZES[c % 6], MODES[(c // 6) % 3]
                seqs.append([(s, mode, "d" if mode == "deliveries" or (mode == "alternating" and i % 2 == 0) else "r")
                             for i in range(n)])
            last_read = (None, True)
            while any(seqs):
                for q in seqs:
                    if not q:
                        continue
                    s, mode, kind = q.pop(0)
                    t[h] += 1 if mode == "alternating" else rng.choice((0, 0, 1))
                    if kind == "d":
                        port = 9 if rng.random() < 0.1 else 1000 + s
                        b.deliver(h, t[h], b.packet(UDP_PROTO, 0x0A000001 + h, 4000 + s, port, rng.choice((0, 100, 100, 100))))
                    else:
                        f = rng.choice((0, 0, R.READ_PEEK, R.READ_FIRST))
                        if last_read[0] == t[h] and not last_read[1]:
                            f &= ~R.READ_FIRST
                        last_read = (t[h], bool(f & R.READ_FIRST))
                        b.read(h, t[h], s, f)
            if spp == 0:  # a host without sockets still receives: every packet finds no socket
                t[h] += 1
                b.deliver(h, t[h], b.packet(UDP_PROTO, 1, 2, 1000, 50))
        b.end_step(with_status=step % 2 == 0)
    return b.scenario("wave_sizes_H%d_S%d" % (H, spp))


def run_boundaries():
    """Runs that straddle a 64-operation boundary; a buffer that fills in the middle of a run and one
    that fills exactly at a run's last element; a host with deliveries only to unknown ports; a step
    with no deliveries; a step with no reads; a step with nothing."""
    b = Builder([2, 1, 1])
    b.ops.append(("associate", wildcard_assoc(b)))
    # host 0 slot 0: 50 deliveries, 30 reads, 70 deliveries (the run crosses op 64 and op 128), 40 reads
    b.ops.append(("configure", [(0, 0, R.UDP, 0, 0, 0, 10**6), (0, 1, R.UDP, 0, 0, 0, 100 * 40), (1, 0, R.UDP, 0, 0, 0, 100 * 70)]))
    t = 5 * 10**9
    for n, kind in ((50, "d"), (30, "r"), (70, "d"), (40, "r")):
        for _ in range(n):
            t += 1
            if kind == "d":
                b.deliver(0, t, b.packet(UDP_PROTO, 7, 7, 1000, 100))
            else:
                b.read(0, t, 0)
    # host 0 slot 1: fills in the middle of one run of 100 (limit 4000, 100 each: 40 accepted)
    for _ in range(100):
        t += 1
        b.deliver(0, t, b.packet(UDP_PROTO, 7, 7, 1001, 100))
    # host 1: a run of exactly 70 with limit 7000: the last one is accepted, nothing refused; then one more
    for i in range(70):
        b.deliver(1, t + i, b.packet(UDP_PROTO, 7, 7, 1000, 100))
    # host 2: only unknown ports
    for i in range(5):
        b.deliver(2, t + i, b.packet(UDP_PROTO, 7, 7, 4242, 10))
    b.end_step()
    b.deliver(1, t + 100, b.packet(UDP_PROTO, 7, 7, 1000, 100))  # now full: refused
    b.end_step()  # (a step with no reads)
    b.read(0, t + 200, 0), b.read(0, t + 200, 1), b.read(1, t + 200, 0, R.READ_PEEK), b.read(1, t + 200, 0)
    b.end_step()  # (a step with no deliveries)
    b.end_step()  # (a step with nothing)
    return b.scenario("run_boundaries")


def tables(per_host, seed=3):
    """per_host associations on each of two hosts (the same keys on both, different slots), keys that
    differ in exactly one field, half removed and every key looked up again, then reassociated."""
    rng = random.Random(seed)
    b = Builder([4, 4])
    base = (UDP_PROTO, 5000, 0x0A0A0A0A, 6000)
    keys = [base, (TCP_PROTO,) + base[1:], (base[0], 5001) + base[2:], base[:2] + (0x0A0A0A0B, base[3]), base[:3] + (6001,),
            (UDP_PROTO, 5000, 0, 0)]
    while len(keys) < per_host:
        k = (rng.choice((UDP_PROTO, TCP_PROTO)), rng.randrange(1, 65536), rng.randrange(1, 2**32), rng.randrange(1, 65536))
        if k not in keys:
            keys.append(k)
    keys = keys[:per_host]
    entries = [(h, p, lp, pip, pp, (i + h) % 4) for h in range(2) for i, (p, lp, pip, pp) in enumerate(keys)]
    b.ops.append(("associate", entries))

    def look_up_all(t):
        for h in range(2):
            for p, lp, pip, pp in keys:
                # the key's own packet; for a wildcard key a packet from anywhere
                b.deliver(h, t, b.packet(p, pip or 77, pp or 88, lp, 10))
            b.deliver(h, t, b.packet(UDP_PROTO, 1, 1, 1, 10))  # nobody's
        b.end_step(with_status=False)
    look_up_all(10**9)
    half = [e[:5] for e in entries[::2]]
    b.ops.append(("disassociate", half))
    look_up_all(10**9 + 1)
    b.ops.append(("disassociate", half))  # all missing now
    b.ops.append(("associate", [e for e in entries[::2]]))
    b.ops.append(("associate", [entries[0]]))  # refused: exists
    look_up_all(10**9 + 2)
    return b.scenario("tables_%d" % per_host)


def skipped_rows(deliver_status):
    """The same interleaved status bytes read with deliver_status 1 and 2."""
    b = Builder([2, 2])
    b.ops.append(("associate", wildcard_assoc(b)))
    t = 10**9
    for h in range(2):
        for i in range(150):
            b.deliver(h, t + i // 3, b.packet(UDP_PROTO, 3, 3, 1000 + i % 2, 20 * (i % 3)), status=(0, 1, 2, 1)[(i + h) % 4])
        for i in range(20):
            b.read(h, t + 5 * i, i % 2, R.READ_FIRST if i % 3 == 0 else 0)
    b.end_step(deliver_status=deliver_status)
    return b.scenario("skipped_rows_%d" % deliver_status)


def several_steps(seed=5):
    """8 steps on one object: buffers carry messages across steps; configure in between lowers a limit
    below len_bytes, sets and clears a peer, and turns a slot EXTERNAL and back; counters are reset
    in the middle."""
    rng = random.Random(seed)
    b = Builder([3, 2, 0, 1])
    b.ops.append(("associate", wildcard_assoc(b) + [(0, UDP_PROTO, 1000, 0x01020304, 555, 2)]))
    t = 10**9
    for step in range(8):
        if step == 2:
            b.ops.append(("configure", [(0, 0, R.UDP, 0, 0, 0, 150), (1, 0, R.UDP, 1, 0x01020304, 555, R.DEFAULT_LIMIT)]))
        if step == 3:
            b.ops.append(("configure", [(0, 1, R.EXTERNAL, 0, 0, 0, 0), (1, 1, R.UDP, 0, 0, 0, 0)]))
            b.ops.append(("reset", 0))
        if step == 5:
            b.ops.append(("configure", [(0, 1, R.UDP, 0, 0, 0, 500), (1, 0, R.UDP, 0, 0, 0, R.DEFAULT_LIMIT),
                                        (0, 0, R.UDP, 0, 0, 0, 10**5), (0, 0, R.UDP, 0, 0, 0, 3000)]))
        for h in (0, 1, 3):
            for _ in range(rng.randrange(20, 90)):
                t += rng.choice((0, 1))
                s = rng.randrange(b.nsock[h])
                if rng.random() < 0.6:
                    sip, sport = rng.choice(((0x01020304, 555), (0x01020304, 556), (0x01020305, 555)))
                    b.deliver(h, t, b.packet(UDP_PROTO, sip, sport, 1000 + s, rng.choice((0, 40, 1472))))
                elif not (h == 0 and s == 1 and step in (3, 4)):  # (no reads on the EXTERNAL slot)
                    b.read(h, t, s, rng.choice((0, 0, R.READ_PEEK)))
            t += 1
        b.end_step(with_status=False)
    return b.scenario("several_steps")


def errors():
    """Every refused call, each followed by a valid step.  ("step_raw" carries arrays as given.)"""
    b = Builder([2, 1])
    b.ops.append(("associate", wildcard_assoc(b)))
    b.ops.append(("configure", [(1, 0, R.EXTERNAL, 0, 0, 0, 0)]))
    t = 10**9
    g = [b.packet(UDP_PROTO, 1, 1, 1000, 100) for _ in range(8)]

    def good():
        b.deliver(0, t, g[0]), b.deliver(0, t + 1, g[1]), b.deliver(1, t, g[2]), b.read(0, t + 1, 0)
        b.end_step()
    good()
    bad = [
        ("step", [1, 1], [t, t], [g[0], g[1]], [0, 3, 2], 1, [], [], [], [0, 0, 0]),           # offsets not monotone
        ("step", [1, 1], [t, t], [g[0], g[1]], [0, 1, 1], 1, [], [], [], [0, 0, 0]),           # ... not ending at n
        ("step", [1], [t], [g[0]], [0, 1, 1], 1, [t], [0], [0], [0, 0, 2]),                    # read offsets
        ("step", [1, 1], [t, t], [g[0], 10**6], [0, 2, 2], 1, [], [], [], [0, 0, 0]),          # tag >= num_packets
        ("step", [1], [t], [g[0]], [0, 1, 1], 1, [t], [0], [4], [0, 1, 1]),                    # unknown flag
        ("step", [1], [t], [g[0]], [0, 1, 1], 1, [t], [2], [0], [0, 1, 1]),                    # slot >= sockets_per_host
        ("step", [1], [t], [g[0]], [0, 1, 1], 1, [t], [0], [0], [0, 0, 1]),                    # read on an EXTERNAL slot
        ("step", [1], [t], [g[0]], [0, 1, 1], 1, [t, t], [0, 1], [0, R.READ_FIRST], [0, 2, 2]),  # contradiction
        ("step", [1, 1], [t + 1, t], [g[0], g[1]], [0, 2, 2], 1, [], [], [], [0, 0, 0]),       # delivery backward
        ("step", [1], [t], [g[0]], [0, 1, 1], 1, [t + 1, t], [0, 0], [0, 0], [0, 2, 2]),       # read backward
    ]
    for op in bad:
        b.ops.append(op)
        good()
    # a skipped row may carry any tag and any time
    b.ops.append(("step", [0, 1, 0], [t + 9, t, 0], [10**9, g[3], 10**9], [0, 3, 3], 1, [], [], [], [0, 0, 0]))
    b.ops.append(("associate", [(0, UDP_PROTO, 1000, 0, 0, 1)]))            # duplicate
    b.ops.append(("associate", [(0, UDP_PROTO, 7, 0, 0, 0), (0, UDP_PROTO, 7, 0, 0, 1)]))  # duplicate inside the batch
    b.ops.append(("associate", [(0, UDP_PROTO, 8, 0, 0, 2)]))               # slot out of range
    b.ops.append(("associate", [(2, UDP_PROTO, 8, 0, 0, 0)]))               # host out of range
    b.ops.append(("configure", [(0, 0, R.UDP, 0, 0, 0, 5), (0, 2, R.UDP, 0, 0, 0, 5)]))  # second entry bad: none applied
    b.ops.append(("configure", [(0, 0, 2, 0, 0, 0, 5)]))                    # unknown kind
    good()
    return b.scenario("errors")


def no_table():
    b = Builder([1])
    b.pk = None
    b.ops.append(("step", None, [], [], [0, 0], 1, [], [], [], [0, 0]))
    return dict(name="no_table", sockets_per_host=[1], packets=None, ops=b.ops)


def all_scenarios():
    out = [wave_sizes(H, spp, 18 if H * max(spp, 1) <= 24 else 3) for H in (1, 3, 64, 65) for spp in (0, 1, 8)]
    out += [run_boundaries(), tables(1), tables(2), tables(1000), skipped_rows(1), skipped_rows(2), several_steps(),
            errors(), no_table()]
    return out


def run_ref(scn):
    """-> (ref, records): one record per op -- ("ok", outputs...) or ("err", code)."""
    ref = R.SocketsInRef(scn["sockets_per_host"])
    if scn["packets"] is not None:
        ref.set_packets(*scn["packets"])
    recs = []
    for op in scn["ops"]:
        try:
            if op[0] == "step":
                recs.append(("ok",) + tuple(ref.step(*op[1:])))
            elif op[0] == "reset":
                recs.append(("ok", ref.host_counters(op[1], reset=True)))
            else:
                getattr(ref, op[0])(op[1])
                recs.append(("ok",))
        except R.RefError as e:
            recs.append(("err", e.code))
        recs[-1] = recs[-1] + (snapshot(ref),)
    return ref, recs


def snapshot(ref):
    return ([[s.state() for s in hs] for hs in ref.socks], [dict(c) for c in ref.counters])
