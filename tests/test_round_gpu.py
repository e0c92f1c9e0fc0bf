"""GPU: a round on the device (srg_round_*, shadow_amd/csrc/round.hip.h) against tests/round_ref.py.
After every call every output array, every result field, every host's inbound state, outbound state
and qdisc order (through the part views), its generator words and its next event id are compared
exactly.  The closed loop of test_outbound_gpu.py through Round.receive / Round.send; the same seeded
rounds through the five separate calls with `chance` and ids made on the host; the draw kernel's
chunk edges (hosts 1, 3, 64, 65; 0, 1, 63, 64, 65, 129 leaving packets per host and step; a host
that never draws; a step without offers); the draw rule's cases; set_host_rng; every error with a
check that nothing moved and that the next valid round equals the restatement's."""
import numpy as np
import pytest

import outbound_ref as OR
import round_ref as RR
from shadow_amd import _native as N
from shadow_amd import events as ev
from shadow_amd.graph import NetGraphError

pytestmark = pytest.mark.gpu

U64 = 2**64 - 1
MS = 1_000_000
SEND_KEYS = ("num_leaving", "num_sent", "num_dropped", "num_local", "num_after_end", "num_no_host", "num_queued_outbound",
             "num_queued_events", "min_used_latency_ns", "min_next_event_ns", "min_inbound_wake_ns",
             "min_outbound_wake_ns", "next_start_ns")
RECV_KEYS = ("num_popped", "num_leaving", "num_forwarded", "num_dropped", "num_queued_inbound", "num_queued_events",
             "min_next_event_ns", "min_inbound_wake_ns", "min_outbound_wake_ns", "next_start_ns")


def u64(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def flatten(per_host):
    """per host [(time, slot, prio, flags, tag)] -> the six arrays of a send."""
    cols = [[], [], [], [], []]
    offs = [0]
    for mine in per_host:
        for e in mine:
            for c, v in zip(cols, e):
                c.append(v)
        offs.append(len(cols[0]))
    return cols + [offs]


class Both:
    """The device object and the restatement, fed alike and compared after every call."""

    def __init__(self, router, host_node, lat, loss, bw_up, bw_down, sockets, qdisc, seeds, sim_start, boot, sim_end):
        import torch
        self.torch = torch
        self.dev = torch.device(f"cuda:{router.device}")
        self.H, self.sim_start = len(host_node), sim_start
        table = ev.DevicePathTable.from_arrays(latency_ns=np.asarray(lat, np.uint64),
                                               packet_loss=None if loss is None else np.asarray(loss, np.float32),
                                               device=self.dev)
        self.rd = ev.Round(router, host_node, table, bw_up, bw_down, sockets, qdisc, seeds, sim_start, boot, sim_end)
        self.ref = RR.Round(host_node, np.asarray(lat).tolist(), None if loss is None else np.asarray(loss, np.float32),
                            bw_up, bw_down, sockets, qdisc, seeds, sim_start, boot, sim_end)
        self.dst, self.size, self.payload = [], [], []
        self.ref.set_packets(self.dst, self.size, self.payload)
        self.uploaded = -1

    def add_packet(self, dst, size, payload):
        self.dst.append(dst)
        self.size.append(size)
        self.payload.append(payload)
        return len(self.dst) - 1

    def upload(self):
        if self.uploaded != len(self.dst):
            self.rd.set_packets(ev._i32(np.array(self.dst, np.uint32), self.dev),
                                ev._i32(np.array(self.size, np.uint32), self.dev),
                                ev._i32(np.array(self.payload, np.uint32), self.dev))
            self.uploaded = len(self.dst)

    def check_states(self):
        rd, ref, H = self.rd, self.ref, self.H
        for h in range(H):
            for view, part in ((rd.inbound, ref.inb), (rd.outbound, ref.out)):
                exp = dict(part.host_state(h))
                if exp["last_refill_ns"] is None:  # an unlimited host has no bucket: the record keeps sim_start
                    exp["last_refill_ns"] = self.sim_start
                assert view.host_state(h) == exp, h
            assert rd.outbound.host_order(h) == ref.out.host_order(h), h
            assert rd.host_rng(h) == ref.host_rng(h), h

    def send(self, until, per_host):
        self.upload()
        time, slot, prio, flags, tag, offs = flatten(per_host)
        e = self.ref.send(until, time, slot, prio, flags, tag, offs)
        d = self.rd.send(until, np.array(time, np.uint64), np.array(slot, np.uint32), np.array(prio, np.uint64),
                         np.array(flags, np.uint8), np.array(tag, np.uint64), np.array(offs, np.uint64))
        assert u64(d["host_offsets"]) == e["host_offsets"], "host offsets"
        assert d["status"].cpu().numpy().tolist() == e["status"], "status"
        assert u64(d["time"]) == e["time"] and u64(d["tag"]) == e["tag"]
        for k in SEND_KEYS:
            assert d[k] == e[k], k
        self.check_states()
        return e

    def receive(self, until):
        self.upload()
        e = self.ref.receive(until)
        d = self.rd.receive(until)
        for k in ("popped_time", "popped_tag", "popped_host_offsets", "time", "tag", "host_offsets"):
            assert u64(d[k]) == e[k], k
        assert d["status"].cpu().numpy().tolist() == e["status"], "status"
        for k in RECV_KEYS:
            assert d[k] == e[k], k
        self.check_states()
        return e

    def refused(self, code, until, per_host=None, arrays=None):
        """A send both sides refuse with `code`; nothing moved on either."""
        self.upload()
        time, slot, prio, flags, tag, offs = arrays if arrays is not None else flatten(per_host)
        with pytest.raises(RR.RoundRefError) as e:
            self.ref.send(until, time, slot, prio, flags, tag, offs)
        assert e.value.code == code
        n = len(time)
        rc, res, msg = self.rd.send_device(
            until, n, ev._i64(np.array(time, np.uint64), self.dev), ev._i32(np.array(slot, np.uint32), self.dev),
            ev._i64(np.array(prio, np.uint64), self.dev),
            self.torch.from_numpy(np.array(flags, np.uint8)).to(self.dev), ev._i64(np.array(tag, np.uint64), self.dev),
            ev._i64(np.array(offs, np.uint64), self.dev))
        assert rc == code, (rc, msg)
        assert msg
        m = self.ref._minima()
        for k in ("num_queued_events", "min_next_event_ns", "min_inbound_wake_ns", "min_outbound_wake_ns", "next_start_ns"):
            assert getattr(res, k) == m[k], k
        self.check_states()

    def refused_receive(self, code, until):
        """A receive both sides refuse with `code`; nothing moved on either."""
        self.upload()
        with pytest.raises(RR.RoundRefError) as e:
            self.ref.receive(until)
        assert e.value.code == code
        rc, res, msg = self.rd.receive_device(until)
        assert rc == code, (rc, msg)
        assert msg
        m = self.ref._minima()
        for k in ("num_queued_events", "min_next_event_ns", "min_inbound_wake_ns", "min_outbound_wake_ns", "next_start_ns"):
            assert getattr(res, k) == m[k], k
        self.check_states()

    def close(self):
        self.rd.close()


# ---- the closed loop's setup (test_outbound_gpu.py::test_closed_round_loop) ---------------------
H, TN, RUNAHEAD, T0 = 23, 6, 5_000_000, 10**12
BWS = [U64, 1_000_000, 8_000_000, 50_000_000, 7_999]
BOOT = T0 + 7_000_000
SIM_END = T0 + 10**9


def loop_setup():
    rng = np.random.default_rng(23)
    lat = rng.integers(1_000_000, 4_000_000, (TN, TN)).astype(np.uint64)
    loss = (rng.random((TN, TN), dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    host_node = rng.integers(0, TN, H, dtype=np.uint32)
    bw_up = [BWS[h % len(BWS)] for h in range(H)]
    bw_down = [BWS[(h + 2) % len(BWS)] for h in range(H)]
    sockets = [1 + h % 4 for h in range(H)]
    seeds = rng.integers(0, 2**63, H, dtype=np.uint64)
    return rng, lat, loss, host_node, bw_up, bw_down, sockets, seeds


def loop_offers(rng, ws, we, sockets, prio, add_packet):
    """One window's seeded offers; the packets enter the pool through add_packet."""
    offers = []
    for h in range(H):
        ts = np.sort(ws + rng.integers(0, (we - ws) // 250_000, rng.integers(0, 40)) * 250_000)
        mine = []
        for t in ts.tolist():
            prio[h] += 1
            ctl = rng.random() < 0.1
            size = 40 if ctl else int(rng.integers(41, 1501))
            x = rng.random()
            dst = h if x < 0.03 else RR.NO_HOST if x < 0.05 else int(rng.integers(0, H))
            fl = OR.OFFER_BARRIER if rng.random() < 0.2 else 0
            g = add_packet(dst, size, size - 40)
            mine.append((t, int(rng.integers(0, sockets[h])), 0 if ctl else prio[h], fl, g))
        offers.append(mine)
    return offers


@pytest.mark.parametrize("qdisc", [OR.QDISC_FIFO, OR.QDISC_ROUND_ROBIN], ids=["fifo", "rr"])
def test_closed_loop(router, qdisc):
    """8 rounds: receive(window end), the window's seeded offers, send(window end), next_window on
    the result's next_start_ns.  Every call against the restatement."""
    rng, lat, loss, host_node, bw_up, bw_down, sockets, seeds = loop_setup()
    b = Both(router, host_node, lat, loss, bw_up, bw_down, sockets, qdisc, seeds, 0, BOOT, SIM_END)
    b.check_states()
    prio, start = [0] * H, T0
    tot = dict(num_sent=0, num_dropped=0, num_local=0, num_no_host=0, num_popped=0)
    for rnd in range(8):
        win = ev.next_window(start, RUNAHEAD, SIM_END)
        assert win is not None
        ws, we = win
        r = b.receive(we)
        s = b.send(we, loop_offers(rng, ws, we, sockets, prio, b.add_packet))
        for k in tot:
            tot[k] += r.get(k, 0) if k == "num_popped" else s[k]
        start = s["next_start_ns"]
    assert tot["num_sent"] > 500 and tot["num_popped"] > 300 and tot["num_dropped"] > 5
    assert tot["num_local"] > 5 and tot["num_no_host"] > 5
    b.close()


def test_same_answers_as_the_separate_calls(router):
    """The same seeded rounds twice on the device: through Round, and through Outbound.step ->
    send_packets_device -> push -> pop -> Inbound.step with `chance` and the event ids produced on the
    host by round_ref's generator and draw rule.  Popped order, times, tags and the inbound outputs
    are identical."""
    import torch
    outs = []
    for separate in (False, True):
        rng, lat, loss, host_node, bw_up, bw_down, sockets, seeds = loop_setup()
        dev = torch.device(f"cuda:{router.device}")
        dst, size, payload = [], [], []

        def add_packet(d, s, p):
            dst.append(d)
            size.append(s)
            payload.append(p)
            return len(dst) - 1
        if separate:
            table = ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss, device=dev)
            q = ev.EventQueues(router, H)
            inb = ev.Inbound(router, bw_down, 0, BOOT)
            out = ev.Outbound(router, bw_up, sockets, OR.QDISC_FIFO, 0, BOOT)
            gens = [RR.Xoshiro256PlusPlus.seed_from_u64(s) for s in seeds]
            next_eid = [0] * H
        else:
            table = ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss, device=dev)
            rd = ev.Round(router, host_node, table, bw_up, bw_down, sockets, OR.QDISC_FIFO, seeds, 0, BOOT, SIM_END)
        prio, start, log = [0] * H, T0, []
        for rnd in range(6):
            ws, we = ev.next_window(start, RUNAHEAD, SIM_END)
            if separate:
                t_a, _, _, g_a, off_a, _ = q.pop(we)
                i_st, i_tm, i_tg, i_off, i_res = inb.step(we, t_a, np.array([size[g] for g in g_a.tolist()], np.uint32),
                                                          g_a, off_a)
                log.append((t_a.tolist(), g_a.tolist(), off_a.tolist(), i_st.cpu().numpy().tolist(), u64(i_tm), u64(i_tg),
                            u64(i_off)))
            else:
                d = rd.receive(we)
                log.append((u64(d["popped_time"]), u64(d["popped_tag"]), u64(d["popped_host_offsets"]),
                            d["status"].cpu().numpy().tolist(), u64(d["time"]), u64(d["tag"]), u64(d["host_offsets"])))
            offers = loop_offers(rng, ws, we, sockets, prio, add_packet)
            time, slot, pr, fl, tag, offs = flatten(offers)
            if not separate:
                rd.set_packets(ev._i32(np.array(dst, np.uint32), dev), ev._i32(np.array(size, np.uint32), dev),
                               ev._i32(np.array(payload, np.uint32), dev))
                d = rd.send(we, np.array(time, np.uint64), np.array(slot, np.uint32), np.array(pr, np.uint64),
                            np.array(fl, np.uint8), np.array(tag, np.uint64), np.array(offs, np.uint64))
                start = d["next_start_ns"]
                continue
            owner = np.repeat(np.arange(H), np.diff(offs)).tolist()
            fl = [f | (OR.OFFER_LOCAL if dst[g] == h else 0) for f, g, h in zip(fl, tag, owner)]
            o_st, o_tm, o_tg, o_off, _ = out.step(we, np.array(time, np.uint64), np.array(slot, np.uint32),
                                                  np.array(pr, np.uint64), np.array([size[g] for g in tag], np.uint32),
                                                  np.array(fl, np.uint8), np.array(tag, np.uint64), np.array(offs, np.uint64))
            o_st, o_tm, o_tg, o_off = o_st.cpu().numpy().tolist(), u64(o_tm), u64(o_tg), u64(o_off)
            rows = []  # (src, dst, time, eid, chance, payload, tag) of the drawing packets
            for h in range(H):
                pk = [(o_st[j], o_tm[j], dst[o_tg[j]],
                       float(loss[host_node[h], host_node[dst[o_tg[j]]]]) if dst[o_tg[j]] < H else 0.0, payload[o_tg[j]])
                      for j in range(o_off[h], o_off[h + 1])]
                res, next_eid[h] = RR.draw_host(gens[h], next_eid[h], pk, True, BOOT, SIM_END)
                for j, (c, chance, eid) in zip(range(o_off[h], o_off[h + 1]), res):
                    if chance is not None:
                        rows.append((h, dst[o_tg[j]], o_tm[j], eid if eid is not None else 0, chance, payload[o_tg[j]],
                                     o_tg[j]))
            if rows:
                src = np.array([r[0] for r in rows], np.uint32)
                dd = np.array([r[1] for r in rows], np.uint32)
                batch = dict(src_node=host_node[src], dst_node=host_node[dd], src_host=src, dst_host=dd,
                             send_time_ns=np.array([r[2] for r in rows], np.uint64),
                             src_event_id=np.array([r[3] for r in rows], np.uint64),
                             chance=np.array([r[4] for r in rows], np.float64),
                             payload_size=np.array([r[5] for r in rows], np.uint32))
                db = ev.DeviceSendBatch(batch, H, we, BOOT, dev)
                q.send(db, table, tags=ev._i64(np.array([r[6] for r in rows], np.uint64), dev))
            start = min(q.min_next_event_ns, inb.min_next_wake_ns, out.min_next_wake_ns)
        outs.append(log)
        if separate:
            q.close()
            inb.close()
            out.close()
        else:
            rd.close()
    assert outs[0] == outs[1]
    assert sum(len(x[0]) for x in outs[0]) > 200


# ---- the draw kernel's chunk edges ---------------------------------------------------------------
CHUNK_COUNTS = (0, 1, 63, 64, 65, 129)


@pytest.mark.parametrize("num_hosts", [1, 3, 64, 65])
def test_chunk_edges(router, num_hosts):
    """Unlimited hosts, so what is offered leaves in the same step: per host and step 0, 1, 63, 64, 65
    or 129 leaving packets, rotated over hosts and steps.  Host 0 never draws (its packets are local
    or go to no host); the last step has no offers at all.  Two nodes with loss 0.5 between them."""
    n = num_hosts
    lat = np.array([[1 * MS, 2 * MS], [2 * MS, 1 * MS]], np.uint64)
    loss = np.array([[0.0, 0.5], [0.5, 0.25]], np.float32)
    host_node = [h % 2 for h in range(n)]
    b = Both(router, host_node, lat, loss, [U64] * n, [U64] * n, [2] * n, OR.QDISC_FIFO, [1000 + h for h in range(n)],
             0, 0, 10**15)
    rnd = np.random.default_rng(n)
    prio = 0
    for step in range(len(CHUNK_COUNTS) + 1):
        ws, we = T0 + step * 5 * MS, T0 + (step + 1) * 5 * MS
        b.receive(we)
        offers = []
        for h in range(n):
            k = CHUNK_COUNTS[(h + step) % len(CHUNK_COUNTS)] if step < len(CHUNK_COUNTS) else 0
            mine = []
            for i in range(k):
                prio += 1
                x = rnd.random()
                if h == 0:
                    dst = 0 if x < 0.5 else RR.NO_HOST
                else:
                    dst = RR.NO_HOST if x < 0.1 else int(rnd.integers(0, n))
                size = int(rnd.integers(40, 1501))
                mine.append((ws + i * 1000, i % 2, prio, 0, b.add_packet(dst, size, size - 40)))
            offers.append(mine)
        e = b.send(we, offers)
        if step == len(CHUNK_COUNTS):
            assert e["num_leaving"] == 0
        assert all(c in (RR.LOCAL, RR.NO_DST) for c in e["status"][e["host_offsets"][0]:e["host_offsets"][1]])
    assert b.ref.host_rng(0) == (RR.Xoshiro256PlusPlus.seed_from_u64(1000).s, 0)
    b.receive(T0 + 100 * MS)
    b.close()


# ---- the draw rule ---------------------------------------------------------------------------------
def advanced(seed, k):
    g = RR.Xoshiro256PlusPlus.seed_from_u64(seed)
    for _ in range(k):
        g.next_u64()
    return g.s


@pytest.mark.parametrize("loss_value", [0.0, 1.0], ids=["loss0", "loss1"])
def test_draw_rule(router, loss_value):
    """3 unlimited hosts on 2 nodes, the bootstrap ends inside the window, the simulation shortly
    after.  Host 0 sends to host 1 before and after the bootstrap end, with and without payload, to
    no host, to itself, and after the simulation's end."""
    boot, end = T0 + 2 * MS, T0 + 4 * MS
    lat = np.full((2, 2), MS, np.uint64)
    loss = np.full((2, 2), loss_value, np.float32)
    seeds = [5, 6, 7]
    b = Both(router, [0, 1, 1], lat, loss, [U64] * 3, [U64] * 3, [1] * 3, OR.QDISC_FIFO, seeds, 0, boot, end)
    spec = [(boot - 1, 1, 100), (boot - 1, 1, 0), (boot, 1, 100), (boot, 1, 0), (boot + 1, 1, 1), (boot + 2, RR.NO_HOST, 9),
            (boot + 3, 0, 9), (end - 1, 1, 100), (end, 1, 100), (end, RR.NO_HOST, 100), (end + 1, 0, 100), (end + 2, 2, 0)]
    offers = [[(t, 0, i + 1, 0, b.add_packet(d, p + 40, p)) for i, (t, d, p) in enumerate(spec)],
              [(boot + 5, 0, 1, 0, b.add_packet(2, 140, 100))], []]
    e = b.send(T0 + 5 * MS, offers)
    D = RR.DROPPED if loss_value == 1.0 else RR.SENT
    S, L, A, X = RR.SENT, RR.LOCAL, RR.AFTER_END, RR.NO_DST
    assert e["status"] == [S, S, D, S, D, X, L, D, A, A, L, A, D]
    draws0 = 6
    assert b.rd.host_rng(0) == (advanced(5, draws0), e["status"][:12].count(S))
    assert b.rd.host_rng(1) == (advanced(6, 1), 0 if loss_value == 1.0 else 1)
    assert b.rd.host_rng(2) == (advanced(7, 0), 0)
    assert e["num_dropped"] == (4 if loss_value == 1.0 else 0) and e["num_after_end"] == 3 and e["num_no_host"] == 1
    b.receive(T0 + 20 * MS)
    b.close()


def test_set_host_rng(router):
    """Between two rounds the caller steps host 1's generator by k (its other draws) and adds its
    local events' ids; device and restatement agree afterwards."""
    lat = np.full((1, 1), MS, np.uint64)
    loss = np.full((1, 1), 0.5, np.float32)
    b = Both(router, [0, 0], lat, loss, [U64] * 2, [U64] * 2, [1] * 2, OR.QDISC_FIFO, [41, 42], 0, 0, 10**15)

    def offers(ws, n):
        return [[(ws + i, 0, i + 1, 0, b.add_packet(1 - h, 140, 100)) for i in range(n)] for h in range(2)]
    b.send(T0 + MS, offers(T0, 70))
    words, eid = b.rd.host_rng(1)
    g = RR.Xoshiro256PlusPlus(words)
    for _ in range(13):
        g.next_u64()
    b.rd.set_host_rng(1, g.s, eid + 1000)
    b.ref.set_host_rng(1, g.s, eid + 1000)
    assert b.rd.host_rng(1) == (g.s, eid + 1000)
    b.check_states()
    b.receive(T0 + 3 * MS)
    e = b.send(T0 + 3 * MS, offers(T0 + 2 * MS, 70))
    assert e["num_sent"] > 40 and e["num_dropped"] > 40
    b.receive(T0 + 9 * MS)
    with pytest.raises(NetGraphError):
        b.rd.set_host_rng(1, [0, 0, 0, 0], 0)
    with pytest.raises(NetGraphError):
        b.rd.host_rng(2)
    b.close()


# ---- errors ------------------------------------------------------------------------------------------
def test_errors_leave_everything(router):
    """4 hosts on 2 nodes; host 1's downstream bucket holds 1000 + 1500 bytes; host 0's upstream link
    is slow, so it carries a backlog and a pending task across the failing calls.  Every failing call
    also carries valid offers of hosts 0 and 2 that would have moved sockets, buckets, generators,
    counters and queues."""
    lat = np.array([[1 * MS, 2 * MS], [2 * MS, 1 * MS]], np.uint64)
    loss = np.array([[0.0, 0.3], [0.3, 0.0]], np.float32)
    b = Both(router, [0, 1, 1, 0], lat, loss, [1_000_000, U64, U64, U64], [U64, 8_000_000, U64, U64], [2, 1, 2, 1],
             OR.QDISC_ROUND_ROBIN, [1, 2, 3, 4], 0, 0, 10**15)
    prio = [0]

    def pkt(t, slot, dst, size=1000, flags=0):
        prio[0] += 1
        return (t, slot, prio[0], flags, b.add_packet(dst, size, size - 40))
    w1 = T0 + 5 * MS
    b.send(w1, [[pkt(T0 + i * 1000, i % 2, 1 + i % 2) for i in range(8)], [pkt(T0 + 4 * MS, 0, 0)],
                [pkt(T0 + 4 * MS + 900_000, 0, 1), pkt(T0 + 4 * MS + 900_000, 1, 3)], []])
    assert b.ref.out.host_state(0)["queued"] > 0 and b.ref.out.host_state(0)["pending"]
    w2 = w1 + 5 * MS

    def valid():
        return [pkt(w1 + 1000, 0, 2), pkt(w1 + 2000, 1, 1)], [pkt(w1 + 1000, 0, 0), pkt(w1 + 3000, 1, 3)]
    # a tag >= num_packets
    h0, h2 = valid()
    b.refused(N.SRG_ERR_ARG, w2, [h0, [(w1 + 5, 0, 99, 0, len(b.dst) + 3)], h2, []])
    # a dst_host that is neither valid nor SRG_NO_HOST
    h0, h2 = valid()
    b.refused(N.SRG_ERR_ARG, w2, [h0, [pkt(w1 + 5, 0, 4)], h2, []])
    # a packet above its destination's downstream capacity (host 3 -> host 1: 2501 > 1000 + 1500)
    h0, h2 = valid()
    b.refused(N.SRG_ERR_ARG, w2, [h0, [], h2, [pkt(w1 + 5, 0, 1, size=2501)]])
    # a flag bit other than the barrier
    h0, h2 = valid()
    b.refused(N.SRG_ERR_ARG, w2, [h0, [pkt(w1 + 5, 0, 0, flags=OR.OFFER_LOCAL)], h2, []])
    h0, h2 = valid()
    b.refused(N.SRG_ERR_ARG, w2, [h0, [pkt(w1 + 5, 0, 0, flags=4)], h2, []])
    # what the outbound step itself refuses: a slot, offsets
    h0, h2 = valid()
    b.refused(N.SRG_ERR_ARG, w2, [h0, [pkt(w1 + 5, 1, 0)], h2, []])
    h0, h2 = valid()
    arrays = flatten([h0, [], h2, []])
    arrays[5] = [0, 3, 2, 4, 4]
    b.refused(N.SRG_ERR_ARG, w2, arrays=arrays)
    # a receive whose inbound step fails (until_ns outside the time domain) after the pop took every
    # queued event: head and last_popped are put back, and the receive below pops the same events
    assert b.ref._minima()["num_queued_events"] > 0
    b.refused_receive(N.SRG_ERR_ARG, 2**62 + 1)
    # the same upper boundaries are accepted: 2500 bytes to host 1, and a packet to SRG_NO_HOST
    b.receive(w2)
    h0, h2 = valid()
    e = b.send(w2, [h0, [pkt(w1 + 5, 0, RR.NO_HOST)], h2, [pkt(w1 + 5, 0, 1, size=2500)]])
    assert e["num_no_host"] == 1
    w3 = w2 + 5 * MS
    r = b.receive(w3)
    late = max(range(4), key=lambda h: b.ref.last_popped[h])
    assert r["num_popped"] > 0 and b.ref.last_popped[late] >= w2
    # a send with until_ns below the last receive's.  Host 3's last offer was at w1 + 5, so the
    # outbound step accepts two offers shortly after it, lets them leave and commits; they would be
    # delivered about 1 ms after w1, before the last event `late` popped (at w2 or later): the push
    # is SRG_ERR_TIME_BACKWARD, and the outbound step, the generator and the counter are rolled back
    b.refused(N.SRG_ERR_TIME_BACKWARD, w1 + 2000,
              [[], [], [], [pkt(w1 + 10, 0, late, size=40), pkt(w1 + 20, 0, late, size=40)]])
    # the next valid round equals the restatement's
    h0, h2 = valid()
    h0 = [(w3 + 1000,) + h0[0][1:], (w3 + 2000,) + h0[1][1:]]
    h2 = [(w3 + 1000,) + h2[0][1:], (w3 + 3000,) + h2[1][1:]]
    w4 = w3 + 5 * MS
    e = b.send(w4, [h0, [pkt(w3 + 5, 0, 0)], h2, [pkt(w3 + 10, 0, late)]])
    assert e["num_leaving"] > 0
    b.receive(w4 + 50 * MS)
    b.close()
