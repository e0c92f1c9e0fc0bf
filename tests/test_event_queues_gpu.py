"""The device-resident per-host packet-event queues (srg_event_queues_*, event_queue.hip.h): a
round's events merged in, a window's events popped out, across rounds.  Every comparison is exact
against RefQueues below, a literal restatement of EventQueue (event_queue.rs:10-55), Host::execute's
pop loop (host.rs:809-818), Host::next_event_time (:866-868) and the manager's minimum
(manager.rs:416-435, 459-464): one heapq per host.  Nothing expected is derived from the library."""
import heapq

import numpy as np
import pytest

from shadow_amd import _native as N
from shadow_amd import events as ev
from shadow_amd.graph import NetGraphError

pytestmark = pytest.mark.gpu

U64_MAX = 2**64 - 1


class RefOrderPanic(Exception):
    pass


class RefTimeBackward(Exception):
    pass


class RefQueues:
    """heapq of (time, src_host, event_id, tag) per host.  push checks the whole batch before it
    changes anything (the library's calls are atomic)."""

    def __init__(self, num_hosts):
        self.q = [[] for _ in range(num_hosts)]
        self.last_popped = [0] * num_hosts
        self.keys = set()

    def push(self, events):
        """events: iterable of (dst, time, src, event_id, tag)."""
        events = list(events)
        new = set()
        for dst, t, src, eid, _ in events:
            if t < self.last_popped[dst]:
                raise RefTimeBackward((dst, t))           # assert!(time >= last_popped_event_time)
            k = (dst, t, src, eid)
            if k in self.keys or k in new:
                raise RefOrderPanic(k)                    # PanickingOrd: no relative order
            new.add(k)
        for dst, t, src, eid, tag in events:
            heapq.heappush(self.q[dst], (t, src, eid, tag))
        self.keys |= new

    def pop(self, until):
        out = []
        for h, q in enumerate(self.q):
            mine = []
            while q and q[0][0] < until:
                e = heapq.heappop(q)
                self.keys.discard((h, e[0], e[1], e[2]))
                self.last_popped[h] = e[0]
                mine.append(e)
            out.append(mine)
        return out

    def __len__(self):
        return sum(len(q) for q in self.q)

    def min_next(self):
        return min((q[0][0] for q in self.q if q), default=U64_MAX)


def ref_next_window(min_next, runahead, end_time):
    assert runahead != 0
    start = min_next
    end = min(min(start + runahead, U64_MAX), end_time)
    return (start, end) if start < end else None


def _t64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _t32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to("cuda:0")


def queue_order(dst, t, src, eid):
    """The order srg_order_packet_events_device writes: by (dst_host, time, src_host, event_id)."""
    return np.lexsort((eid, src, t, dst)).astype(np.uint32)


def raw_push(q, H, dst, t, src, eid, tag=None, order=None):
    """A batch of given deliver times pushed through a given order (default: its queue order)."""
    dst, src = np.asarray(dst, np.uint32), np.asarray(src, np.uint32)
    t, eid = np.asarray(t, np.uint64), np.asarray(eid, np.uint64)
    n = len(t)
    z32, z64 = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    db = ev.DeviceEventBatch(dict(src_node=z32, dst_node=z32, src_host=src, dst_host=dst, send_time_ns=z64,
                                  src_event_id=eid), H, 0)
    order = queue_order(dst, t, src, eid) if order is None else np.asarray(order, np.uint32)
    return q.push(db, _t64(t), _t32(order), len(order), _t64(tag) if tag is not None else None)


def events_of(dst, t, src, eid, tag=None):
    tag = range(len(t)) if tag is None else tag
    return [(int(a), int(b), int(c), int(d), int(e)) for a, b, c, d, e in zip(dst, t, src, eid, tag)]


def push_both(q, ref, H, dst, t, src, eid, tag=None):
    res = raw_push(q, H, dst, t, src, eid, tag)
    ref.push(events_of(dst, t, src, eid, tag))
    assert res["num_moved"] == len(t)
    check_state(q, ref, res)
    return res


def check_state(q, ref, res=None):
    assert len(q) == len(ref), "num_queued"
    assert q.min_next_event_ns == ref.min_next(), "min_next_event_ns"
    if res is not None:
        assert res["num_queued"] == len(ref) and res["min_next_event_ns"] == ref.min_next()


def pop_both(q, ref, until):
    t, src, eid, tag, off, res = q.pop(until)
    exp = ref.pop(until)
    e_off = np.cumsum([0] + [len(x) for x in exp]).astype(np.uint64)
    flat = [e for mine in exp for e in mine]
    assert np.array_equal(off, e_off), "host offsets"
    assert res["num_moved"] == len(flat) == len(t)
    assert t.tolist() == [e[0] for e in flat], "times"
    assert src.tolist() == [e[1] for e in flat], "src hosts"
    assert eid.tolist() == [e[2] for e in flat], "event ids"
    assert tag.tolist() == [e[3] for e in flat], "tags"
    check_state(q, ref, res)
    return len(flat)


def rand_events(rng, n, H, t_lo, t_hi, hosts=None, id0=0):
    """n events with unique (src, id); dst among `hosts` (default: all)."""
    dst = rng.choice(np.arange(H) if hosts is None else np.asarray(hosts), n).astype(np.uint32)
    t = rng.integers(t_lo, t_hi, n, dtype=np.uint64)
    src = rng.integers(0, H, n, dtype=np.uint32)
    eid = (id0 + rng.permutation(n)).astype(np.uint64)
    tag = rng.integers(0, 2**63, n, dtype=np.uint64) * 2 + 1
    return dst, t, src, eid, tag


@pytest.fixture(scope="module")
def T():
    return int(N.lib().srg_event_queues_merge_tile())


def test_single_push_pop_everything(router, T):
    for n in (1, 63, 65, T - 1, T, T + 1, 2 * T + 1):
        q, ref = ev.EventQueues(router, 5), RefQueues(5)
        rng = np.random.default_rng(100 + n)
        # few distinct times: plenty of ties that only src_host / event id break
        push_both(q, ref, 5, *rand_events(rng, n, 5, 1000, 1040))
        assert pop_both(q, ref, U64_MAX) == n
        assert len(q) == 0 and q.min_next_event_ns == U64_MAX
        q.close()


def test_default_tag_is_the_event_index(router):
    q, ref = ev.EventQueues(router, 3), RefQueues(3)
    dst, t, src, eid, _ = rand_events(np.random.default_rng(5), 200, 3, 10, 500)
    push_both(q, ref, 3, dst, t, src, eid, None)
    pop_both(q, ref, U64_MAX)
    q.close()


# ---- multi-round -------------------------------------------------------------------------------
MR = dict(H=7, rounds=8, sends=1500, window=1000, tn=5, seed=11, t0=10**6, end=10**12)


def multi_round_trace():
    """The whole scenario on the CPU reference: per round the batch the hosts send, and what the
    reference queues give.  7 hosts, 8 rounds, 1500 sends per round, window = runahead = 1000 ns,
    latencies uniform in [500, 6000) on a 5 x 5 table, mean loss 5 %."""
    p = MR
    rng = np.random.default_rng(p["seed"])
    H, tn = p["H"], p["tn"]
    lat = rng.integers(500, 6000, (tn, tn), dtype=np.uint64)
    loss = (rng.random((tn, tn), dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    host_node = rng.integers(0, tn, H, dtype=np.uint32)
    next_id = np.zeros(H, np.uint64)
    ref = RefQueues(H)
    window = (p["t0"], p["t0"] + p["window"])
    rounds = []
    for r in range(p["rounds"]):
        ws, we = window
        popped = ref.pop(we)
        n = p["sends"]
        src = rng.integers(0, H, n, dtype=np.uint32)
        dst = rng.integers(0, H, n, dtype=np.uint32)
        send = np.sort(rng.integers(ws, we, n, dtype=np.uint64))
        eid = np.empty(n, np.uint64)
        for i in range(n):  # Host::get_new_event_id: one counter per source host, in send order
            eid[i] = next_id[src[i]]
            next_id[src[i]] += 1
        chance = rng.random(n)
        payload = np.where(rng.random(n) < 0.1, 0, rng.integers(1, 1461, n)).astype(np.uint32)
        tags = (np.arange(n, dtype=np.uint64) + np.uint64((r + 1) * 10**6))
        a, d = host_node[src].astype(np.int64), host_node[dst].astype(np.int64)
        # worker.rs:374-414, as tests/test_send_packets_gpu.py restates it
        rel = (np.float32(1) - loss[a, d]).astype(np.float64)
        drop = (chance >= rel) & (payload > 0)
        deliver = np.maximum(send + lat[a, d], np.uint64(we))
        keep = np.flatnonzero(~drop)
        backlog_before = len(ref)
        ref.push(events_of(dst[keep], deliver[keep], src[keep], eid[keep], tags[keep]))
        window = ref_next_window(ref.min_next(), p["window"], p["end"])
        rounds.append(dict(ws=ws, we=we, popped=popped, popped_rounds={int(e[3]) // 10**6 for m in popped for e in m},
                           batch=dict(src_node=host_node[src], dst_node=host_node[dst], src_host=src, dst_host=dst,
                                      send_time_ns=send, src_event_id=eid, chance=chance, payload_size=payload),
                           tags=tags, num_sent=len(keep), queued=len(ref), backlog_before=backlog_before,
                           min_next=ref.min_next(), next_window=window))
        assert window is not None
    return lat, loss, rounds


def test_multi_round_matches_the_reference(router, T):
    lat, loss, rounds = multi_round_trace()
    # the scenario does what it is for: a window's pops interleave six earlier pushes, and the
    # resident array a merge reads (the last push's result, its popped prefixes still stored) is
    # longer than two tiles
    assert max(len(r["popped_rounds"]) for r in rounds) == 6
    assert max(r["queued"] for r in rounds[:-1]) > 2 * T
    H = MR["H"]
    table = ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss)
    q = ev.EventQueues(router, H)
    for r in rounds:
        t, src, eid, tag, off, res = q.pop(r["we"])
        flat = [e for m in r["popped"] for e in m]
        assert np.array_equal(off, np.cumsum([0] + [len(m) for m in r["popped"]]).astype(np.uint64))
        assert (t.tolist(), src.tolist(), eid.tolist(), tag.tolist()) == (
            [e[0] for e in flat], [e[1] for e in flat], [e[2] for e in flat], [e[3] for e in flat])
        db = ev.DeviceSendBatch(r["batch"], H, r["we"], 0)
        sres, qres, status = q.send(db, table, tags=_t64(r["tags"]))
        assert sres["num_sent"] == r["num_sent"] == qres["num_moved"] and sres["num_dropped"] > 0
        assert qres["num_queued"] == r["queued"] == len(q)
        assert qres["min_next_event_ns"] == r["min_next"] == q.min_next_event_ns
        assert ev.next_window(q.min_next_event_ns, MR["window"], MR["end"]) == r["next_window"]
    q.close()


# ---- merge placement ---------------------------------------------------------------------------
def spaced_backlog(n, hosts):
    """n events, times 1000, 1010, ...: round-robin over `hosts`, so there is room in front of each."""
    i = np.arange(n)
    return (np.asarray(hosts, np.uint32)[i % len(hosts)], (1000 + 10 * i).astype(np.uint64),
            (i % 3).astype(np.uint32), i.astype(np.uint64), (i + 7 * 10**6).astype(np.uint64))


def test_merge_placement_single_events(router, T):
    """One event in front of everything, behind everything, and landing exactly at merged rank
    T - 1, T, T + 1, 2T - 1, 2T, 2T + 1 of a backlog of 2T + 1."""
    H, n = 6, 2 * T + 1
    q, ref = ev.EventQueues(router, H), RefQueues(H)
    b = spaced_backlog(n, [1, 2, 3, 4])  # hosts 0 and H - 1 empty
    push_both(q, ref, H, *b)
    S = sorted(events_of(*b))  # the backlog in queue order; one more event arrives per step below
    extra = [(0, 5, 0, 0, 900), (H - 1, 5, 0, 1, 901)]  # in front of / behind everything (empty hosts)
    extra += [(S[0][0], S[0][1] - 1, 0, 2, 902), (S[-1][0], S[-1][1] + 1, 0, 3, 903)]  # ... inside used hosts
    for k, rank in enumerate((T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)):
        # the event that ends at merged rank `rank`: just in front of the backlog event there now
        cur = sorted(set(S) | {e for e in extra})
        at = cur[rank]
        extra.append((at[0], at[1] - 1, 0, 10 + k, 910 + k))
        assert sorted(set(S) | set(extra)).index(extra[-1]) == rank
    for e in extra:
        push_both(q, ref, H, [e[0]], [e[1]], [e[2]], [e[3]], [e[4]])
    assert pop_both(q, ref, U64_MAX) == n + len(extra)
    q.close()


def test_merge_placement_batches(router, T):
    H = 6
    rng = np.random.default_rng(21)
    q, ref = ev.EventQueues(router, H), RefQueues(H)
    # an empty batch into an empty queue, then a push into the empty queue
    res = raw_push(q, H, [], [], [], [])
    assert res["num_moved"] == 0 and res["num_queued"] == 0 and res["min_next_event_ns"] == U64_MAX
    push_both(q, ref, H, *rand_events(rng, 2 * T + 1, H, 1000, 9000, hosts=[1, 2, 3, 4]))
    # an empty batch changes nothing
    res = raw_push(q, H, [], [], [], [])
    assert res["num_moved"] == 0
    check_state(q, ref, res)
    # a batch larger than the backlog, everything to one host
    push_both(q, ref, H, *rand_events(rng, 3 * T + 5, H, 1000, 9000, hosts=[2], id0=10**6))
    # a batch that uses the two hosts left empty so far, and only those
    push_both(q, ref, H, *rand_events(rng, 300, H, 1000, 9000, hosts=[0, H - 1], id0=2 * 10**6))
    pop_both(q, ref, 5000)
    pop_both(q, ref, U64_MAX)
    assert len(q) == 0
    q.close()


# ---- full-width compares -----------------------------------------------------------------------
def test_full_width_compares(router):
    H = 70000  # hosts past 16 bits
    q, ref = ev.EventQueues(router, H), RefQueues(H)
    B = 1 << 40
    ev1 = [  # (dst, time, src, id, tag)
        (3, 7 + 2 * B, 1, 1, 1), (3, 7 + B, 1, 2, 2),            # time differs only in bits >= 32
        (4, 50, 1, 9 + 2 * B, 3), (4, 50, 1, 9 + B, 4),          # event id differs only in bits >= 32
        (5, 60, 70000, 5, 5), (5, 60, 69999, 6, 6),              # src_host at equal time
        (65536 + 3, 1, 0, 0, 7), (65535, 2, 0, 0, 8), (65536, 3, 0, 0, 9), (69999, 4, 0, 0, 10),
    ]
    ev2 = [(3, 7, 1, 3, 11), (3, 7 + 3 * B, 1, 4, 12), (4, 50, 1, 9, 13), (4, 50, 1, 9 + 3 * B, 14),
           (5, 60, 3, 7, 15), (5, 60 + (1 << 32), 0, 8, 16), (3 + 65536, 1 + B, 0, 0, 17), (3, 6 + B, 9, 9, 18)]
    for batch in (ev1, ev2):  # the second push merges into the first
        push_both(q, ref, H, *(np.array(c, dtype=np.uint64) for c in zip(*batch)))
    pop_both(q, ref, 7 + B + 1)  # a window edge above 2^32
    pop_both(q, ref, U64_MAX)
    assert len(q) == 0
    q.close()


# ---- pop boundary ------------------------------------------------------------------------------
def test_pop_boundary(router, T):
    H = 4
    rng = np.random.default_rng(31)
    q, ref = ev.EventQueues(router, H), RefQueues(H)
    push_both(q, ref, H, *rand_events(rng, T + 300, H, 1000, 3000))
    push_both(q, ref, H, [1, 2], [2000, 2000], [0, 0], [10**7, 10**7 + 1], [41, 42])
    assert pop_both(q, ref, 1000) == 0            # nothing is earlier than the first event
    n1 = pop_both(q, ref, 2000)                   # time == until stays
    assert n1 > 0 and ref.min_next() == 2000
    assert pop_both(q, ref, 2000) == 0            # again: nothing
    n2 = pop_both(q, ref, 2001)                   # until + 1 takes it
    assert n2 >= 2
    pop_both(q, ref, 2500)                        # a pop after a partial pop
    # pop, push, pop: the merge drops the popped prefixes; new events from the last popped time on
    lp = max(ref.last_popped)
    push_both(q, ref, H, *rand_events(rng, T + 50, H, lp, 4000, id0=2 * 10**7))
    pop_both(q, ref, 2800)
    push_both(q, ref, H, *rand_events(rng, 77, H, max(ref.last_popped), 4000, id0=3 * 10**7))
    pop_both(q, ref, U64_MAX)
    assert len(q) == 0 and q.min_next_event_ns == U64_MAX
    q.close()


def test_push_at_the_last_popped_time_in_front_of_popped_events(router):
    """time == last_popped is accepted, and by (src_host, event id) such an event may sort in front
    of events that were already popped at that time and are still stored."""
    H = 3
    q, ref = ev.EventQueues(router, H), RefQueues(H)
    push_both(q, ref, H, [1, 1, 1, 2], [100, 100, 200, 100], [5, 6, 1, 4], [1, 2, 3, 4], [11, 12, 13, 14])
    assert pop_both(q, ref, 150) == 3
    assert ref.last_popped == [0, 100, 100]
    push_both(q, ref, H, [1, 1, 1, 2, 0], [100, 100, 100, 100, 0], [1, 5, 7, 0, 0], [9, 0, 0, 0, 0],
              [21, 22, 23, 24, 25])
    assert pop_both(q, ref, 101) == 5
    assert pop_both(q, ref, U64_MAX) == 1
    q.close()


# ---- errors leave the state unchanged ----------------------------------------------------------
def test_errors_leave_the_queues_unchanged(router, T):
    H = 5
    rng = np.random.default_rng(41)
    q, ref = ev.EventQueues(router, H), RefQueues(H)
    dst, t, src, eid, tag = rand_events(rng, 2 * T + 9, H, 1000, 5000)
    push_both(q, ref, H, dst, t, src, eid, tag)
    pop_both(q, ref, 2000)
    lp = ref.last_popped[2]
    assert lp > 0
    k = int(np.flatnonzero(t >= 2000)[len(t) // 3])  # a resident, live event

    # a key equal to a resident one (among other, fine events): no order
    d2, t2, s2, e2, g2 = rand_events(rng, 500, H, 2000, 5000, id0=10**6)
    d2[100], t2[100], s2[100], e2[100] = dst[k], t[k], src[k], eid[k]
    with pytest.raises(RefOrderPanic):
        ref.push(events_of(d2, t2, s2, e2, g2))
    with pytest.raises(ev.EventOrderError) as e:
        raw_push(q, H, d2, t2, s2, e2, g2)
    assert e.value.code == N.SRG_ERR_EVENT_ORDER
    check_state(q, ref)

    # time = last_popped - 1: the push assert; time = last_popped is accepted
    with pytest.raises(RefTimeBackward):
        ref.push([(2, lp - 1, 0, 5 * 10**6, 1)])
    with pytest.raises(ev.TimeBackwardError) as e:
        raw_push(q, H, [2, 3], [lp - 1, 4000], [0, 0], [5 * 10**6, 5 * 10**6 + 1], [1, 2])
    assert e.value.code == N.SRG_ERR_TIME_BACKWARD
    check_state(q, ref)
    push_both(q, ref, H, [2], [lp], [0], [5 * 10**6], [77])

    # order: unsorted, an entry >= num_events, a repeated entry; dst_host >= num_hosts
    d3, t3, s3, e3, g3 = rand_events(rng, 300, H, 3000, 5000, id0=2 * 10**6)
    good = queue_order(d3, t3, s3, e3)
    swapped = good.copy()
    swapped[[150, 151]] = swapped[[151, 150]]
    too_big = good.copy()
    too_big[64] = 300
    repeated = good.copy()
    repeated[10] = repeated[9]
    for order in (swapped, too_big, repeated):
        with pytest.raises(NetGraphError) as e:
            raw_push(q, H, d3, t3, s3, e3, g3, order=order)
        assert e.value.code == N.SRG_ERR_ARG
        check_state(q, ref)
    d4 = d3.copy()
    d4[7] = H
    with pytest.raises(NetGraphError) as e:
        raw_push(q, H, d4, t3, s3, e3, g3)
    assert e.value.code == N.SRG_ERR_ARG
    check_state(q, ref)

    # out_capacity one short: SRG_ERR_ARG, num_moved = the count needed, nothing popped
    import torch
    need = sum(1 for hq in ref.q for e in hq if e[0] < 3500)
    assert need > 2

    def outs(n):
        return (torch.empty(n, dtype=torch.int64, device="cuda:0"), torch.empty(n, dtype=torch.int32, device="cuda:0"),
                torch.empty(n, dtype=torch.int64, device="cuda:0"), torch.empty(n, dtype=torch.int64, device="cuda:0"),
                torch.empty(H + 1, dtype=torch.int64, device="cuda:0"))
    rc, res, msg = q.pop_device(3500, need - 1, *outs(need - 1))
    assert rc == N.SRG_ERR_ARG and res["num_moved"] == need
    check_state(q, ref)
    rc, res, msg = q.pop_device(3500, need, *outs(need))
    assert rc == N.SRG_OK and res["num_moved"] == need
    ref.pop(3500)
    check_state(q, ref, res)

    # everything that remains equals the reference without the failed calls
    pop_both(q, ref, U64_MAX)
    assert len(q) == 0
    q.close()


# ---- growth ------------------------------------------------------------------------------------
def test_growth_keeps_the_contents(router, T):
    H = 9
    rng = np.random.default_rng(51)
    q, ref = ev.EventQueues(router, H, reserve=0), RefQueues(H)
    for i, n in enumerate((100, 900, 3 * T)):  # each push outgrows the set it builds into
        push_both(q, ref, H, *rand_events(rng, n, H, 1000, 9000, id0=i * 10**6))
    pop_both(q, ref, 4000)
    push_both(q, ref, H, *rand_events(rng, 4 * T, H, 4000, 9000, id0=5 * 10**6))
    pop_both(q, ref, U64_MAX)
    assert len(q) == 0
    q.close()
