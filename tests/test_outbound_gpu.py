"""GPU: the hosts' outbound path (srg_outbound_*, shadow_amd/csrc/outbound.hip.h) against
tests/outbound_ref.py, the plain-Python restatement of the reference that the hand-derived KATs pin
(test_outbound_cpu.py).  After every step every output array, every result field, every host's state
and its qdisc array (srg_outbound_host_order) are compared exactly, for both qdiscs: the KATs as
steps; the overload scenario as one step, as 50 ms windows and as 1 ms windows, with identical
concatenated outputs; hosts 1, 3, 64, 65 with 0, 1, 63, 64, 65, 129 offers per host and step and a
backlog across a chunk edge; 1, 2, 3, 7, 64, 65, 130 sockets per host, all queued at once; the
hand-made boundaries (a wake exactly at `until`, a barrier offer as the first offer of the next step,
the bootstrap boundary, local packets, an unlimited host); the time-domain scenarios qdisc_*, whose
leaving order is also compared directly with what the reference's own compiled heap and queue code
selected (tests/golden/qdisc_reference.json).  Then every error with a check that nothing
moved, the backlog's growth past reserve_packets, and an 8-round closed loop offers -> Outbound.step ->
send_packets -> EventQueues.push -> pop -> Inbound.step -> next_window with both wakes folded in."""
import heapq

import numpy as np
import pytest

import inbound_ref as IR
import inbound_scenarios as IS
import outbound_ref as R
import outbound_scenarios as S
from shadow_amd import _native as N
from shadow_amd import events as ev
from shadow_amd.graph import NetGraphError

pytestmark = pytest.mark.gpu

U64 = 2**64 - 1


def u64(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def check_states(out, ref, sim_start):
    for h in range(out.num_hosts):
        exp = dict(ref.host_state(h))
        if exp["last_refill_ns"] is None:  # an unlimited host has no bucket: the record keeps sim_start
            exp["last_refill_ns"] = sim_start
        assert out.host_state(h) == exp, h
        assert out.host_order(h) == ref.host_order(h), h


def arrays(per_host):
    time, slot, prio, size, flags, tag, offs = S.flatten(per_host)
    return (np.array(time, np.uint64), np.array(slot, np.uint32), np.array(prio, np.uint64), np.array(size, np.uint32),
            np.array(flags, np.uint8), np.array(tag, np.uint64), np.array(offs, np.uint64))


def step_both(out, ref, until, per_host, sim_start):
    e_st, e_tm, e_tg, e_off, e_res = ref.step(until, *S.flatten(per_host))
    st, tm, tg, off, res = out.step(until, *arrays(per_host))
    assert u64(off) == e_off, "host offsets"
    assert st.cpu().numpy().tolist() == e_st, "status"
    assert u64(tm) == e_tm, "leave times"
    assert u64(tg) == e_tg, "tags"
    for k, v in e_res.items():
        assert res[k] == v, k
    assert out.num_queued == e_res["num_queued"] and out.min_next_wake_ns == e_res["min_next_wake_ns"]
    check_states(out, ref, sim_start)
    return st.cpu().numpy().tolist(), u64(tm), u64(tg), u64(off), res


def run_scenario(router, scn, reserve=0):
    _, bw, sockets, qdisc, sim_start, boot, steps = scn
    out = ev.Outbound(router, bw, sockets, qdisc, sim_start, boot, reserve)
    ref = R.Outbound(bw, sockets, qdisc, sim_start, boot)
    check_states(out, ref, sim_start)
    outs = [step_both(out, ref, until, per_host, sim_start) for until, per_host in steps]
    out.close()
    return outs


SCENARIOS = [s for s in S.all_scenarios() if not s[0].startswith("overload")]


@pytest.mark.parametrize("scn", SCENARIOS, ids=lambda s: s[0])
def test_scenarios_match_the_reference(router, scn):
    run_scenario(router, scn)


@pytest.mark.parametrize("qdisc", [R.QDISC_FIFO, R.QDISC_ROUND_ROBIN], ids=["fifo", "rr"])
def test_overload_in_one_step_and_in_windows(router, qdisc):
    """One 1 Mbit/s host, two bursts of 300 packets over 5 sockets with control packets: one step,
    50 ms windows and 1 ms windows, each step against the reference, and the device's concatenated
    outputs identical."""
    a, b, c = (S.concat_by_host(run_scenario(router, S.overload(w, qdisc)), 1) for w in (None, 50 * S.MS, 1 * S.MS))
    assert a == b == c and len(a[0]) == 600


def tags_by_host(router, scn):
    """The device alone: -> per host, the tags that left, concatenated over the steps."""
    _, bw, sockets, qdisc, sim_start, boot, steps = scn
    out = ev.Outbound(router, bw, sockets, qdisc, sim_start, boot)
    outs = []
    for until, per_host in steps:
        st, tm, tg, off, res = out.step(until, *arrays(per_host))
        outs.append((st.cpu().numpy().tolist(), u64(tm), u64(tg), u64(off), res))
    assert out.num_queued == 0 and out.min_next_wake_ns == U64
    out.close()
    left = S.concat_by_host(outs, len(bw))
    return [[g for _, _, g in left[h]] for h in range(len(bw))]


@pytest.mark.parametrize("width", [None, 3 * S.MS], ids=["one_step", "3ms_windows"])
@pytest.mark.parametrize("qdisc", [R.QDISC_FIFO, R.QDISC_ROUND_ROBIN], ids=["fifo", "rr"])
def test_device_leaves_in_the_reference_programs_order(router, qdisc, width):
    """The qdisc_* scenarios of one qdisc (two instances: their bootstrap ends differ), as one step and
    in 3 ms windows, with no restatement in between: per host, the tags the device lets leave are the
    tag column the reference's compiled queue code printed for that host's operations, in its order.
    Reads tests/golden/ only."""
    recorded = {x["name"]: x["hosts"] for x in S.load_qdisc_reference()["scenarios"]}
    specs = S.qdisc_specs(qdisc)
    assert len(specs) == 2 and all(spec[0] in recorded for spec in specs)
    for spec in specs:
        got = tags_by_host(router, S.qdisc_scenario(spec, width))
        hosts = recorded[spec[0]]
        assert len(got) == len(hosts)
        for h, e in enumerate(hosts):
            exp = [int(ln.split()[1]) for ln in e["output"].splitlines() if ln != "-"]
            assert exp and got[h] == exp, (spec[0], h)


def test_scenarios_reach_every_branch():
    R.reset_counters()
    for scn in S.all_scenarios():
        S.run_ref(scn)
    assert all(R.COUNTERS[k] > 0 for k in R.BRANCHES), R.COUNTERS


def test_backlog_grows_past_the_reserve(router):
    """reserve_packets = 8.  300 packets of 1500 B are offered to a 1 Mbit/s host in one nanosecond: the
    full bucket (1625) lets one leave, the second is cached, 298 stay in the sockets.  200 more arrive
    1 ms later, when the cached packet still lacks tokens: 498 in the sockets.  Then the drain."""
    S0, MS = S.SIM_START, S.MS
    a = [(S0 + MS, i % 4, i + 1, 1500, 0, i) for i in range(300)]
    b = [(S0 + 2 * MS, i % 4, 301 + i, 1500, 0, 1000 + i) for i in range(200)]
    for qdisc in (R.QDISC_FIFO, R.QDISC_ROUND_ROBIN):
        scn = ("growth", [1_000_000, U64], [4, 1], qdisc, S0, S0,
               [(S0 + MS + 1, [a, []]), (S0 + 3 * MS, [b, [(S0 + 2 * MS, 0, 1, 40, 0, 5000)]]),
                (S0 + 10_000 * MS, [[], []])])
        outs = run_scenario(router, scn, reserve=8)
        assert [o[4]["num_queued"] for o in outs] == [299, 499, 0]
        assert [len(o[0]) for o in outs] == [1, 1, 499]


def test_errors_leave_the_state(router):
    import torch
    S0, MS = S.SIM_START, S.MS
    bw, sockets = [1_000_000, U64, 1_000_000], [2, 1, 3]
    with pytest.raises(NetGraphError):
        ev.Outbound(router, bw, sockets, 2, S0, S0)
    out = ev.Outbound(router, bw, sockets, R.QDISC_FIFO, S0, S0)
    ref = R.Outbound(bw, sockets, R.QDISC_FIFO, S0, S0)
    first = [[(S0 + MS, 0, 1, 1500, 0, 1), (S0 + 2 * MS, 1, 2, 1500, 0, 2), (S0 + 2 * MS, 0, 3, 1500, 0, 3)],
             [(S0 + 3 * MS, 0, 1, 99, 0, 4)], []]
    step_both(out, ref, S0 + 5 * MS, first, S0)
    until = S0 + 9 * MS
    dev = out.dev

    def refused(code, offers, offs, until=until, capacity=None):
        """offers: [(time, slot, size, flags)]"""
        n = len(offers)
        t_t = ev._i64(np.array([o[0] for o in offers], np.uint64), dev)
        k_t = ev._i32(np.array([o[1] for o in offers], np.uint32), dev)
        p_t = ev._i64(np.arange(10, 10 + n, dtype=np.uint64), dev)
        s_t = ev._i32(np.array([o[2] for o in offers], np.uint32), dev)
        f_t = torch.tensor([o[3] for o in offers], dtype=torch.uint8, device=dev)
        g_t = ev._i64(np.arange(90, 90 + n, dtype=np.uint64), dev)
        o_t = ev._i64(np.array(offs, np.uint64), dev)
        cap = out.num_queued + n if capacity is None else capacity
        o = [torch.zeros(max(cap, 1), dtype=d, device=dev) for d in (torch.uint8, torch.int64, torch.int64)]
        ooff = torch.zeros(len(bw) + 1, dtype=torch.int64, device=dev)
        queued, wake = out.num_queued, out.min_next_wake_ns
        rc, res, msg = out.step_device(until, n, t_t, k_t, p_t, s_t, f_t, g_t, o_t, cap, o[0], o[1], o[2], ooff)
        assert rc == code, (rc, msg)
        assert msg
        assert out.num_queued == queued and out.min_next_wake_ns == wake
        check_states(out, ref, S0)
        return res

    t = S0 + 6 * MS
    refused(N.SRG_ERR_TIME_BACKWARD, [(S0 + MS, 0, 40, 0)], [0, 1, 1, 1])              # before host 0's last offer
    refused(N.SRG_ERR_TIME_BACKWARD, [(t, 0, 40, 0), (t - 1, 0, 40, 0)], [0, 0, 0, 2])  # decreasing inside a slice
    refused(N.SRG_ERR_ARG, [(until, 0, 40, 0)], [0, 1, 1, 1])                          # time >= until
    refused(N.SRG_ERR_ARG, [(S0 - 1, 0, 40, 0)], [0, 0, 0, 1])                         # below the simulation start
    refused(N.SRG_ERR_ARG, [(2**62, 0, 40, 0)], [0, 0, 0, 1], until=2**62)             # at the domain's end
    refused(N.SRG_ERR_ARG, [(t, 0, 40, 0)], [0, 0, 0, 1], until=2**62 + 1)             # until outside the domain
    refused(N.SRG_ERR_ARG, [(t, 0, 40, 0), (t, 0, 40, 0)], [0, 2, 1, 2])               # offsets not monotone
    refused(N.SRG_ERR_ARG, [(t, 0, 40, 0), (t, 0, 40, 0)], [0, 1, 1, 1])               # offsets not ending at n
    refused(N.SRG_ERR_ARG, [(t, 0, 1626, 0)], [0, 0, 0, 1])                            # above the capacity, not local
    refused(N.SRG_ERR_ARG, [(t, 3, 40, 0)], [0, 0, 0, 1])                              # slot == sockets_per_host
    refused(N.SRG_ERR_ARG, [(t, 1, 40, 0)], [0, 0, 1, 1])                              # host 1 has one slot
    refused(N.SRG_ERR_ARG, [(t, 0, 40, 4)], [0, 0, 0, 1])                              # an unknown flag bit
    # capacity short: the need is reported, nothing moved; host 0's blocked packet leaves before `far`
    far = S0 + 100 * MS
    e = R.Outbound(bw, sockets, R.QDISC_FIFO, S0, S0)
    e.step(S0 + 5 * MS, *S.flatten(first))
    need = len(e.step(far, [t], [0], [10], [40], [0], [90], [0, 0, 0, 1])[0])
    assert need >= 3
    res = refused(N.SRG_ERR_ARG, [(t, 0, 40, 0)], [0, 0, 0, 1], until=far, capacity=need - 1)
    assert res["num_sent"] + res["num_local"] == need
    rc, res, _ = out.step_device(far, 0, None, None, None, None, None, None, ev._i64(np.zeros(4, np.uint64), dev), 0, None,
                                 None, None, None)
    assert rc == N.SRG_ERR_ARG and res["num_sent"] + res["num_local"] == need - 1  # a sizing call
    check_states(out, ref, S0)
    # the next step runs as if none of them had happened; a local packet above the capacity is accepted
    step_both(out, ref, far, [[], [], [(t, 0, 10, 40, 0, 90), (t, 2, 11, 9000, R.OFFER_LOCAL, 91)]], S0)
    with pytest.raises(NetGraphError):
        out.host_state(3)
    with pytest.raises(NetGraphError):
        out.host_order(3)
    out.close()


def send_reference(b, lat, loss, round_end, boot):
    """worker.rs:374-424 for one batch: (status, deliver)."""
    a, d = b["src_node"].astype(np.int64), b["dst_node"].astype(np.int64)
    send = b["send_time_ns"].astype(np.uint64)
    rel = (np.float32(1) - loss[a, d]).astype(np.float64)
    drop = (send >= np.uint64(boot)) & (b["chance"] >= rel) & (b["payload_size"] > 0)
    deliver = np.maximum(send + lat[a, d], np.uint64(round_end))
    return (~drop).astype(np.uint8), deliver


def test_closed_round_loop(router):
    """8 rounds on a small routing table: the window's packet events are popped and run through the
    inbound step; the window's seeded offers run through the outbound step; what left for the router
    is sent at the step's times, in leaving order (event ids and `chance` drawn in that order), and
    pushed; next_window takes the minimum of the queues' next event and both paths' wakes.  Every
    stage is compared with its restatement."""
    import torch
    H, TN, runahead, t0 = 23, 6, 5_000_000, 10**12
    rng = np.random.default_rng(23)
    lat = rng.integers(1_000_000, 4_000_000, (TN, TN)).astype(np.uint64)
    loss = (rng.random((TN, TN), dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    host_node = rng.integers(0, TN, H, dtype=np.uint32)
    bws = [U64, 1_000_000, 8_000_000, 50_000_000, 7_999]
    bw_up = [bws[h % len(bws)] for h in range(H)]
    bw_down = [bws[(h + 2) % len(bws)] for h in range(H)]
    sockets = [1 + h % 4 for h in range(H)]
    boot = t0 + 7_000_000
    dev = torch.device(f"cuda:{router.device}")
    table = ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss, device=dev)
    q = ev.EventQueues(router, H)
    inb = ev.Inbound(router, bw_down, 0, boot)
    out = ev.Outbound(router, bw_up, sockets, R.QDISC_FIFO, 0, boot)
    ref_q = [[] for _ in range(H)]
    ref_in = IR.Inbound(bw_down, 0, boot)
    ref_out = R.Outbound(bw_up, sockets, R.QDISC_FIFO, 0, boot)
    pkt_dst, pkt_size = [], []  # by tag
    prio, next_eid = [0] * H, [1] * H
    start, total_sent, total_in = t0, 0, 0
    for rnd in range(8):
        win = ev.next_window(start, runahead, t0 + 10**9)
        assert win is not None
        ws, we = win
        # the window's packet events: pop, then the hosts' inbound path
        t_a, _, _, g_a, off_a, _ = q.pop(we)
        per_host = []
        for h in range(H):
            mine = []
            while ref_q[h] and ref_q[h][0][0] < we:
                e = heapq.heappop(ref_q[h])
                mine.append((e[0], pkt_size[e[3]], e[3]))
            per_host.append(mine)
        e_time, e_size, e_tag, e_off = IS.flatten(per_host)
        assert t_a.tolist() == e_time and g_a.tolist() == e_tag and off_a.tolist() == e_off, rnd
        i_st, i_tm, i_tg, i_off, i_res = inb.step(we, t_a, np.array(e_size, np.uint32), g_a, off_a)
        r_st, r_tm, r_tg, r_off, r_res = ref_in.step(we, e_time, e_size, e_tag, e_off)
        assert (i_st.cpu().numpy().tolist(), u64(i_tm), u64(i_tg), u64(i_off)) == (r_st, r_tm, r_tg, r_off), rnd
        total_in += len(r_st)
        # the window's offers: the hosts' outbound path
        offers = []
        for h in range(H):
            ts = np.sort(ws + rng.integers(0, (we - ws) // 250_000, rng.integers(0, 40)) * 250_000)
            mine = []
            for t in ts.tolist():
                prio[h] += 1
                ctl = rng.random() < 0.1
                size = 40 if ctl else int(rng.integers(41, 1501))
                fl = (R.OFFER_LOCAL if rng.random() < 0.03 else 0) | (R.OFFER_BARRIER if rng.random() < 0.2 else 0)
                mine.append((t, int(rng.integers(0, sockets[h])), 0 if ctl else prio[h], size, fl, len(pkt_dst)))
                pkt_dst.append(h if fl & R.OFFER_LOCAL else int(rng.integers(0, H)))
                pkt_size.append(size)
            offers.append(mine)
        o_st, o_tm, o_tg, o_off, o_res = step_both(out, ref_out, we, offers, 0)
        # what left for the router is sent at the step's times, in each host's leaving order
        src = np.repeat(np.arange(H, dtype=np.uint32), np.diff(np.array(o_off, np.int64)))
        keep = np.array(o_st, np.uint8) == 1
        tags = np.array(o_tg, np.uint64)[keep]
        n = int(keep.sum())
        total_sent += n
        if n:
            src = src[keep]
            dst = np.array([pkt_dst[g] for g in tags.tolist()], np.uint32)
            eid = np.empty(n, np.uint64)
            for i, h in enumerate(src.tolist()):
                eid[i] = next_eid[h]
                next_eid[h] += 1
            batch = dict(src_node=host_node[src], dst_node=host_node[dst], src_host=src, dst_host=dst,
                         send_time_ns=np.array(o_tm, np.uint64)[keep], src_event_id=eid, chance=rng.random(n),
                         payload_size=np.array([pkt_size[g] - 40 for g in tags.tolist()], np.uint32))
            db = ev.DeviceSendBatch(batch, H, we, boot, dev)
            status = torch.empty(n, dtype=torch.uint8, device=dev)
            deliver = torch.empty(n, dtype=torch.int64, device=dev)
            order = torch.empty(n, dtype=torch.int32, device=dev)
            hoff = torch.empty(H + 1, dtype=torch.int64, device=dev)
            sres = ev.send_packets_device(router, db, table, status, deliver, order, hoff)
            e_status, e_deliver = send_reference(batch, lat, loss, we, boot)
            sent = e_status != 0
            assert status.cpu().numpy().tolist() == e_status.tolist() and sres["num_sent"] == int(sent.sum()), rnd
            assert np.array_equal(deliver.cpu().numpy().view(np.uint64)[sent], e_deliver[sent]), rnd
            q.push(db, deliver, order, sres["num_sent"], ev._i64(tags, dev))
            for i in np.flatnonzero(sent):
                heapq.heappush(ref_q[int(dst[i])], (int(e_deliver[i]), int(src[i]), int(eid[i]), int(tags[i])))
        wakes = [hh.wake for hh in ref_out.hosts if hh.pending]
        e_next = min(min((x[0][0] for x in ref_q if x), default=U64), r_res["min_next_wake_ns"], min(wakes, default=U64))
        start = min(q.min_next_event_ns, inb.min_next_wake_ns, out.min_next_wake_ns)
        assert start == e_next, rnd
    assert total_sent > 500 and total_in > 300
    q.close()
    inb.close()
    out.close()
