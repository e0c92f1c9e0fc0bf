"""The handles of the five resident classes (EventQueues, Inbound, Outbound, SocketsIn, Round): close()
twice, raw calls and read-backs on a closed object, an object dropped without close(); and the
round's rollback of the outbound part through its snapshot.  2 hosts with 1 socket each."""
import gc

import numpy as np
import pytest

from shadow_amd import _native as N
from shadow_amd import events as ev
from shadow_amd.graph import NetGraphError

pytestmark = pytest.mark.gpu

U64 = 2**64 - 1
MS = 1_000_000
T0 = 10**12
SENTINEL = 0x5A
H = 2


def table(router):
    import torch
    lat = np.array([[1 * MS, 2 * MS], [2 * MS, 1 * MS]], np.uint64)
    loss = np.array([[0.0, 0.0], [0.3, 0.0]], np.float32)
    return ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss, device=torch.device(f"cuda:{router.device}"))


def make_round(router, bw_up=(1_000_000, U64)):
    return ev.Round(router, [0, 1], table(router), list(bw_up), [U64, U64], [1, 1], 0, [1, 2], 0, 0, 10**15)


def sentinels(dev, *shapes):
    """uint8 / int64 output tensors filled with a value no call writes"""
    import torch
    return [torch.full((n,), SENTINEL, dtype=dt, device=dev) for n, dt in shapes]


def untouched(ts):
    return all(bool((t == SENTINEL).all()) for t in ts)


# ---- one entry per class: make, a step that must succeed, the raw call on a closed object, its read-backs ----
def queues_step(q):
    import torch
    b = ev.DeviceEventBatch(dict(src_node=[0], dst_node=[1], src_host=[0], dst_host=[1], send_time_ns=[T0],
                                 src_event_id=[1]), H, T0 + MS, q.dev)
    res = q.push(b, ev._i64(np.array([T0 + 2 * MS], np.uint64), q.dev), torch.zeros(1, dtype=torch.int32, device=q.dev), 1)
    assert res["num_moved"] == 1 and q.num_queued == 1
    t, src, eid, tag, off, res = q.pop(T0 + 3 * MS)
    assert t.tolist() == [T0 + 2 * MS] and off.tolist() == [0, 0, 1] and q.num_queued == 0


def queues_raw(q):
    import torch
    outs = sentinels(q.dev, (4, torch.int64), (4, torch.int32), (4, torch.int64), (4, torch.int64), (H + 1, torch.int64))
    rc, res, msg = q.pop_device(T0, 4, *outs)
    return rc, outs


def inbound_step(q):
    status, time, tag, off, res = q.step(T0 + MS, [T0], [1000], [7], [0, 0, 1])
    assert res["num_forwarded"] == 1 and tag.cpu().tolist() == [7] and off.cpu().tolist() == [0, 0, 1]


def inbound_raw(q):
    import torch
    outs = sentinels(q.dev, (4, torch.uint8), (4, torch.int64), (4, torch.int64), (H + 1, torch.int64))
    off = torch.zeros(H + 1, dtype=torch.int64, device=q.dev)
    rc, res, msg = q.step_device(T0, 0, None, None, None, off, 4, *outs)
    return rc, outs


def outbound_step(q):
    status, time, tag, off, res = q.step(T0 + MS, [T0], [0], [1], [1000], None, [7], [0, 1, 1])
    assert res["num_sent"] == 1 and tag.cpu().tolist() == [7] and off.cpu().tolist() == [0, 1, 1]


def outbound_raw(q):
    import torch
    outs = sentinels(q.dev, (4, torch.uint8), (4, torch.int64), (4, torch.int64), (H + 1, torch.int64))
    off = torch.zeros(H + 1, dtype=torch.int64, device=q.dev)
    rc, res, msg = q.step_device(T0, 0, None, None, None, None, None, None, off, 4, *outs)
    return rc, outs


def sockets_packets(q):
    z8, z16, z32 = np.zeros(1, np.uint8), np.zeros(1, np.int16), np.zeros(1, np.uint32)
    import torch
    q.set_packets(torch.from_numpy(z8).to(q.dev), ev._i32(z32, q.dev), torch.from_numpy(z16).to(q.dev),
                  torch.from_numpy(z16).to(q.dev), ev._i32(np.array([1000], np.uint32), q.dev),
                  ev._i32(np.array([960], np.uint32), q.dev))


def sockets_step(q):
    sockets_packets(q)
    st, slot, *_, res = q.step([1], [T0], [0], [0, 0, 1])
    assert st.tolist() == [N.SRG_RCV_NO_SOCKET] and res["num_no_socket"] == 1


def sockets_raw(q):
    import torch
    outs = sentinels(q.dev, (4, torch.uint8), (4, torch.int32))
    off = torch.zeros(H + 1, dtype=torch.int64, device=q.dev)
    one = torch.zeros(1, dtype=torch.int64, device=q.dev)
    rc, res, msg = q.step_device(1, None, one, one, off, 1, 0, None, None, None, None, *outs, None, None, None, None)
    return rc, outs


def round_step(r):
    r.set_packets(ev._i32(np.array([1], np.uint32), r.dev), ev._i32(np.array([1000], np.uint32), r.dev),
                  ev._i32(np.array([960], np.uint32), r.dev))
    d = r.send(T0 + MS, [T0], [0], [1], None, [0], [0, 1, 1])
    assert d["num_leaving"] == 1 and d["tag"].cpu().tolist() == [0]


def round_raw(r):
    rc, res, msg = r.receive_device(T0)
    assert res.num_popped == 0 and not res.status_dev
    rc2, res2, msg2 = r.send_device(T0, 0, None, None, None, None, None, ev._i64(np.zeros(H + 1, np.uint64), r.dev))
    assert rc2 == rc and res2.num_leaving == 0 and not res2.status_dev
    return rc, []


CASES = {
    "queues": (lambda router: ev.EventQueues(router, H), queues_step, queues_raw, []),
    "inbound": (lambda router: ev.Inbound(router, [U64, U64], 0, 0), inbound_step, inbound_raw,
                [lambda q: q.host_state(0)]),
    "outbound": (lambda router: ev.Outbound(router, [U64, U64], [1, 1], 0, 0, 0), outbound_step, outbound_raw,
                 [lambda q: q.host_state(0), lambda q: q.host_order(0)]),
    "sockets_in": (lambda router: ev.SocketsIn(router, [1, 1]), sockets_step, sockets_raw,
                   [lambda q: q.socket_state(0, 0), lambda q: q.host_counters(0)]),
    "round": (make_round, round_step, round_raw, [lambda r: r.host_rng(0)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_handle(router, name):
    make, step, raw, readbacks = CASES[name]
    q = make(router)
    step(q)
    counters = {k: getattr(q, k) for k in ("num_queued", "min_next_event_ns", "min_next_wake_ns", "num_buffered_messages")
                if hasattr(q, k)}
    q.close()
    assert q._h is None
    q.close()  # a no-op
    assert q._h is None
    rc, outs = raw(q)  # the null-handle check, in front of everything
    assert rc == N.SRG_ERR_ARG
    assert untouched(outs)
    assert counters == {k: getattr(q, k) for k in counters}
    for rb in readbacks:
        with pytest.raises(NetGraphError) as e:
            rb(q)
        assert e.value.code == N.SRG_ERR_ARG
    del q  # (__del__ on a closed object: nothing left to destroy)
    gc.collect()


@pytest.mark.parametrize("name", sorted(CASES))
def test_dropped_without_close(router, name):
    """The object's only reference goes: __del__ destroys it, once.  A second object on the same router
    afterwards is created and stepped as usual."""
    make, step, raw, readbacks = CASES[name]
    q = make(router)
    step(q)
    del q
    gc.collect()
    q2 = make(router)
    step(q2)
    for rb in readbacks:
        rb(q2)
    q2.close()


# ---- the round's rollback of the outbound part ---------------------------------------------------
def upload(r, dst):
    n = len(dst)
    r.set_packets(ev._i32(np.array(dst, np.uint32), r.dev), ev._i32(np.full(n, 1000, np.uint32), r.dev),
                  ev._i32(np.full(n, 960, np.uint32), r.dev))


def send_arrays(r, until, time, tag, offs):
    n = len(time)
    return r.send_device(until, n, ev._i64(np.array(time, np.uint64), r.dev), ev._i32(np.zeros(n, np.uint32), r.dev),
                         ev._i64(np.array(tag, np.uint64) + np.uint64(1), r.dev), None, ev._i64(np.array(tag, np.uint64), r.dev),
                         ev._i64(np.array(offs, np.uint64), r.dev))


def send_dict(r, until, time, tag, offs):
    n = len(time)
    d = r.send(until, np.array(time, np.uint64), np.zeros(n, np.uint32), np.array(tag, np.uint64) + np.uint64(1), None,
               np.array(tag, np.uint64), np.array(offs, np.uint64))
    d.pop("ms_total")
    return {k: (v.cpu().tolist() if hasattr(v, "cpu") else v) for k, v in d.items()}


def states(r):
    return [r.outbound.host_state(h) for h in range(H)], [r.outbound.host_order(h) for h in range(H)]


def test_send_failing_behind_the_outbound_commit(router):
    """Host 0's slow link keeps packets of the first send inside the outbound part.  The packet table
    is then rewritten under them: a queued packet's dst_host becomes 7.  The next send's offers are
    valid, its outbound step commits, and only the count over the leaving packets refuses the
    destination: the outbound part is put back from its snapshot.  With the table repaired, the same
    send gives what a fresh Round fed the two valid sends gives."""
    first = dict(until=T0 + 5 * MS, time=[T0 + i * 1000 for i in range(8)], tag=list(range(8)), offs=[0, 8, 8])
    second = dict(until=T0 + 20 * MS, time=[T0 + 5 * MS + 1000, T0 + 5 * MS + 2000], tag=[8, 9], offs=[0, 1, 2])
    dst = [1] * 8 + [1, 0]
    a = make_round(router)
    upload(a, dst)
    d1 = send_dict(a, **first)
    assert d1["num_queued_outbound"] > 0 and a.outbound.host_state(0)["queued"] > 0
    before = states(a)
    cached = a.outbound.host_state(0)["cached_tag"]  # the packet the relay holds: the next to leave
    assert a.outbound.host_state(0)["has_cached"] and cached not in d1["tag"]
    bad = list(dst)
    bad[cached] = 7
    upload(a, bad)
    rc, res, msg = send_arrays(a, **second)
    assert rc == N.SRG_ERR_ARG and "packet table changed" in msg, (rc, msg)
    assert states(a) == before
    # a send refused in front of the outbound step reports the host-side counters as they are now
    rc, res, msg = send_arrays(a, second["until"], [second["time"][0]], [len(dst)], [0, 1, 1])
    assert rc == N.SRG_ERR_ARG and "tag" in msg, (rc, msg)
    for k in ("num_queued_outbound", "num_queued_events", "min_next_event_ns", "min_outbound_wake_ns", "next_start_ns"):
        assert getattr(res, k) == d1[k], k
    assert states(a) == before
    upload(a, dst)
    d2 = send_dict(a, **second)
    fresh = make_round(router)
    upload(fresh, dst)
    assert send_dict(fresh, **first) == d1
    assert send_dict(fresh, **second) == d2
    assert d2["num_leaving"] > 0
    assert states(a) == states(fresh)
    assert [a.host_rng(h) for h in range(H)] == [fresh.host_rng(h) for h in range(H)]
    a.close()
    fresh.close()
