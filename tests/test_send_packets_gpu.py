"""The whole per-packet tail of Worker::send_packet as one batch (srg_send_packets_device,
events.hip.h k_ev_prep<true> / k_ev_counts): drop decision, latency from either table form, deliver
times, per-host pop order, packet counts.  Every comparison is exact (integers) against the numpy
restatement below of worker.rs:374-424, event.rs:84-155 and mod.rs:449-456."""
import numpy as np
import pytest

import oracle
from shadow_amd import _native as N
from shadow_amd import events as ev
from shadow_amd.graph import NetGraphError

pytestmark = pytest.mark.gpu

U64_MAX = 2**64 - 1
T0 = 10**12


def numpy_reference(b, lat, loss, num_hosts, round_end, boot=0):
    """lat u64 [tn, tn]; loss f32 [tn, tn] or None.  Returns (status, deliver, order, host_offsets,
    min_next_event, min_used_latency, counts)."""
    a, d = b["src_node"].astype(np.int64), b["dst_node"].astype(np.int64)
    send = b["send_time_ns"].astype(np.uint64)
    n = len(send)
    if loss is None:
        drop = np.zeros(n, bool)
    else:
        rel = (np.float32(1) - loss[a, d]).astype(np.float64)
        drop = (send >= np.uint64(boot)) & (b["chance"] >= rel) & (b["payload_size"] > 0)
    idx = np.flatnonzero(~drop)
    l = lat[a[idx], d[idx]]
    deliver = np.full(n, U64_MAX, np.uint64)
    deliver[idx] = np.maximum(send[idx] + l, np.uint64(round_end))
    o = np.lexsort((b["src_event_id"][idx], b["src_host"][idx], deliver[idx], b["dst_host"][idx]))
    order = idx[o].astype(np.uint32)
    off = np.searchsorted(b["dst_host"][order], np.arange(num_hosts + 1), side="left").astype(np.uint64)
    counts = np.zeros(lat.shape, np.uint64)
    np.add.at(counts, (a[idx], d[idx]), np.uint64(1))
    mn = int(deliver[idx].min()) if len(idx) else U64_MAX
    ml = int(l.min()) if len(idx) else U64_MAX
    return (~drop).astype(np.uint8), deliver, order, off, mn, ml, counts


def rand_send_batch(n, H, tn, seed, id_span=10**6, t_span=10**6, loss_hi=0.6):
    """A batch with unique (src_host, event_id), a u64 latency table and a loss table uniform in
    [0, loss_hi): about loss_hi / 2 of the packets with a payload are dropped."""
    rng = np.random.default_rng(seed)
    b = dict(src_node=rng.integers(0, tn, n, dtype=np.uint32), dst_node=rng.integers(0, tn, n, dtype=np.uint32),
             src_host=rng.integers(0, H, n, dtype=np.uint32), dst_host=rng.integers(0, H, n, dtype=np.uint32),
             send_time_ns=(T0 + rng.integers(0, t_span, n, dtype=np.uint64)).astype(np.uint64))
    b["src_event_id"] = (rng.permutation(max(n, 1))[:n].astype(np.uint64) * max(1, id_span // max(n, 1)) + 5)
    b["chance"] = rng.random(n)
    b["payload_size"] = np.where(rng.random(n) < 0.1, 0, rng.integers(1, 1461, n)).astype(np.uint32)
    lat = rng.integers(10**5, 10**7, (tn, tn), dtype=np.uint64)
    loss = (rng.random((tn, tn), dtype=np.float32) * np.float32(loss_hi)).astype(np.float32)
    return b, lat, loss


def counts_tensor(tn, init=None):
    import torch
    c = np.zeros((tn, tn), np.uint64) if init is None else np.ascontiguousarray(init, dtype=np.uint64)
    return torch.from_numpy(c.view(np.int64).copy()).to("cuda:0")


def counts_host(t):
    return t.cpu().numpy().view(np.uint64)


def check(router, b, lat, loss, H, re, boot=0, table=None, with_counts=True):
    """One call against `table` (default: the u64 form of lat + loss); everything compared."""
    tn = lat.shape[0]
    table = table or ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss)
    counts = counts_tensor(tn) if with_counts else None
    status, deliver, order, off, res = ev.send_packets(router, b, table, H, re, boot, counts)
    e_status, e_deliver, e_order, e_off, e_mn, e_ml, e_counts = numpy_reference(b, lat, loss, H, re, boot)
    assert np.array_equal(status, e_status), "status"
    assert np.array_equal(deliver, e_deliver), "deliver times"
    assert len(order) == res["num_sent"] == int(e_status.sum()), "num_sent"
    assert res["num_dropped"] == len(e_status) - int(e_status.sum())
    assert np.array_equal(order, e_order), "order"
    assert np.array_equal(off, e_off) and int(off[H]) == res["num_sent"], "host offsets"
    assert res["min_next_event_ns"] == e_mn and res["min_used_latency_ns"] == e_ml
    if with_counts:
        assert np.array_equal(counts_host(counts), e_counts), "packet counts"
    return status, deliver, order, off, res


@pytest.mark.parametrize("n", [1, 63, 65])
def test_wave_edges(router, n):
    b, lat, loss = rand_send_batch(n, 5, 4, 10 + n)
    check(router, b, lat, loss, 5, T0 + 300_000)


def test_three_tiles_thirty_percent_loss_and_counts(router):
    """5000 events = two radix tiles of 2048 and a partial third; the counts equal np.add.at."""
    b, lat, loss = rand_send_batch(5000, 37, 9, 2)
    *_, res = check(router, b, lat, loss, 37, T0 + 300_000)
    assert 0.2 < res["num_dropped"] / 5000 < 0.4


def test_none_dropped_equals_order_packet_events(router):
    """Loss all 0: the new entry gives what the pinned old one's oracle gives on the same batch."""
    b, lat, loss = rand_send_batch(5000, 37, 9, 3)
    loss[:] = 0
    re = T0 + 300_000
    status, deliver, order, off, res = check(router, b, lat, loss, 37, re)
    assert res["num_dropped"] == 0 and status.all()
    o_deliver, o_order, o_off, o_mn, o_ml = oracle.order_packet_events(b, lat, 37, re)
    assert np.array_equal(deliver, np.asarray(o_deliver)) and np.array_equal(order, np.asarray(o_order))
    assert np.array_equal(off, np.asarray(o_off))
    assert res["min_next_event_ns"] == o_mn and res["min_used_latency_ns"] == o_ml
    # and no loss table at all: no decision, the same result
    t = ev.DevicePathTable.from_arrays(latency_ns=lat)
    b2 = {k: v for k, v in b.items() if k not in ("chance", "payload_size")}
    got = ev.send_packets(router, b2, t, 37, re)
    assert np.array_equal(got[1], deliver) and np.array_equal(got[2], order) and got[4]["num_dropped"] == 0


def test_all_dropped_and_bootstrap(router):
    b, lat, loss = rand_send_batch(3000, 11, 6, 4)
    loss[:] = 1
    b["payload_size"][:] = 7
    status, deliver, order, off, res = check(router, b, lat, loss, 11, T0 + 300_000)
    assert res["num_sent"] == 0 and len(order) == 0 and off.tolist() == [0] * 12
    assert res["min_next_event_ns"] == U64_MAX and res["min_used_latency_ns"] == U64_MAX
    assert not status.any() and (deliver == U64_MAX).all()
    # the same batch while bootstrapping: nothing is dropped
    boot = int(b["send_time_ns"].max()) + 1
    *_, res = check(router, b, lat, loss, 11, T0 + 300_000, boot=boot)
    assert res["num_dropped"] == 0
    # send == bootstrap_end is eligible again
    *_, res = check(router, b, lat, loss, 11, T0 + 300_000, boot=int(b["send_time_ns"].min()))
    assert res["num_sent"] == 0


def fixed_batch(k):
    """k events on one pair of a 2 x 2 table; loss 0.5 everywhere: chance 0.9 drops, 0.1 sends."""
    b = dict(src_node=np.zeros(k, np.uint32), dst_node=np.ones(k, np.uint32), src_host=np.full(k, 3, np.uint32),
             dst_host=np.full(k, 2, np.uint32), send_time_ns=np.full(k, T0, np.uint64),
             src_event_id=np.arange(1, k + 1, dtype=np.uint64), chance=np.full(k, 0.1),
             payload_size=np.full(k, 100, np.uint32))
    lat = np.array([[5, 7], [9, 3]], np.uint64)
    loss = np.full((2, 2), 0.5, np.float32)
    return b, lat, loss


def test_dropped_events_have_no_order(router):
    """Two dropped events equal in every key field are fine; the same two sent have no order."""
    b, lat, loss = fixed_batch(3)
    b["src_event_id"][:] = [4, 4, 9]
    b["chance"][:2] = 0.9
    *_, res = check(router, b, lat, loss, 4, 0)
    assert res["num_sent"] == 1 and res["num_dropped"] == 2
    b["chance"][:2] = 0.1
    with pytest.raises(ev.EventOrderError):
        ev.send_packets(router, b, ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss), 4, 0)


def test_dropped_event_never_reaches_the_add(router):
    """send = 2^64 - 1 overflows send + delay only when the packet is sent."""
    b, lat, loss = fixed_batch(3)
    b["send_time_ns"][1] = U64_MAX
    b["chance"][1] = 0.9
    *_, res = check(router, b, lat, loss, 4, 0)
    assert res["num_sent"] == 2
    b["chance"][1] = 0.1
    with pytest.raises(NetGraphError) as e:
        ev.send_packets(router, b, ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss), 4, 0)
    assert e.value.code == N.SRG_ERR_LATENCY_RANGE


def test_wide_key(router):
    b, lat, loss = rand_send_batch(20000, 100, 30, 5, id_span=2**45, t_span=2**40, loss_hi=0.22)
    *_, res = check(router, b, lat, loss, 100, T0 + 2**40 // 3)
    assert res["key_bits"] > 64
    assert 0.05 < res["num_dropped"] / 20000 < 0.15


def test_key_table_equals_u64_table(router):
    rng = np.random.default_rng(6)
    b, _, loss = rand_send_batch(5000, 37, 9, 6)
    b["dst_node"][::7] = b["src_node"][::7]  # self pairs: the diagonal
    key = rng.integers(100, 10**4, (9, 9), dtype=np.uint32)
    diag = rng.integers(1, 10**9, 9, dtype=np.uint64) * 2 + 1  # odd: never key * 1000
    wide = key.astype(np.uint64) * np.uint64(1000)
    wide[np.arange(9), np.arange(9)] = diag
    assert not np.any(diag == key[np.arange(9), np.arange(9)].astype(np.uint64) * np.uint64(1000))
    re = T0 + 300_000
    got_w = check(router, b, wide, loss, 37, re)
    got_k = check(router, b, wide, loss, 37, re,
                  table=ev.DevicePathTable.from_arrays(key=key, diag=diag, unit=1000, packet_loss=loss))
    for w, k in zip(got_w[:4], got_k[:4]):
        assert np.array_equal(w, k)
    assert (b["src_node"] == b["dst_node"]).sum() > 700


def test_counts_hot_pair_accumulates(router):
    b, lat, loss = fixed_batch(4096)
    loss[:] = 0
    t = ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss)
    counts = counts_tensor(2)
    ev.send_packets(router, b, t, 4, 0, counts=counts)
    assert counts_host(counts).tolist() == [[0, 4096], [0, 0]]
    ev.send_packets(router, b, t, 4, 0, counts=counts)
    assert counts_host(counts).tolist() == [[0, 8192], [0, 0]]


def test_counts_saturate(router):
    b, lat, loss = fixed_batch(10)
    loss[:] = 0
    t = ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss)
    counts = counts_tensor(2, [[1, U64_MAX - 2], [U64_MAX, 0]])
    ev.send_packets(router, b, t, 4, 0, counts=counts)
    assert counts_host(counts).tolist() == [[1, U64_MAX], [U64_MAX, 0]]
    # several waves on a counter that is about to wrap: 200 events, 4 waves, room for 5
    b, lat, loss = fixed_batch(200)
    loss[:] = 0
    counts = counts_tensor(2, [[0, U64_MAX - 5], [0, 0]])
    ev.send_packets(router, b, t, 4, 0, counts=counts)
    assert counts_host(counts).tolist() == [[0, U64_MAX], [0, 0]]


def test_counts_null_is_accepted(router):
    b, lat, loss = rand_send_batch(1000, 7, 5, 8)
    check(router, b, lat, loss, 7, T0 + 300_000, with_counts=False)


def test_end_to_end_routing_info(router):
    """A RoutingInfo built on the GPU keeps its u32 keys; they are uploaded as they are, the batch
    matches the reference on the table's u64 view, and the batch counts merge into packet_count."""
    from shadow_amd import generate_routing_info, synth
    g = synth.random_graph(60, 0.2, 9, lat_lo=10**5, lat_hi=10**7)
    ids = list(range(59, -1, -1))  # position p holds GML id 59 - p
    ri = generate_routing_info(g, ids, True, router)
    assert ri.key_tables() is not None
    t = ev.DevicePathTable.from_routing_info(ri)
    assert t.key is not None and t.latency_ns is None
    lat, loss, gml = ri.tables()
    assert gml.tolist() == ids
    b, re, _ = ev.synthetic_round(50000, 60, 60, seed=9, runahead=2 * 10**6, loss=0.1)
    b["src_node"], b["dst_node"] = b["src_host"].copy(), b["dst_host"].copy()
    counts = counts_tensor(60)
    status, deliver, order, off, res = ev.send_packets(router, b, t, 60, re, 0, counts)
    e = numpy_reference(b, lat, loss, 60, re)
    for got, exp in zip((status, deliver, order, off), e[:4]):
        assert np.array_equal(got, exp)
    assert res["min_next_event_ns"] == e[4] and res["min_used_latency_ns"] == e[5]
    assert 0 < res["num_dropped"] < 50000
    c = counts_host(counts)
    assert np.array_equal(c, e[6])
    pa, pb = (int(x) for x in np.unravel_index(np.argmax(c), c.shape))
    ri.increment_packet_count(ids[pa], ids[pb])
    assert ri.packet_count(ids[pa], ids[pb]) == 1
    ri.add_packet_counts(counts)
    assert ri.packet_count(ids[pa], ids[pb]) == int(c[pa, pb]) + 1
    ri.increment_packet_count(ids[pa], ids[pb])
    assert ri.packet_count(ids[pa], ids[pb]) == int(c[pa, pb]) + 2
    assert ri.packet_count(ids[3], ids[5]) == int(c[3, 5])
    ri.close()


def test_argument_errors(router):
    b, lat, loss = rand_send_batch(100, 7, 5, 9)
    key, diag = lat.astype(np.uint32), np.ones(5, np.uint64)

    def refused(table, batch=b):
        with pytest.raises(NetGraphError) as e:
            ev.send_packets(router, batch, table, 7, 0)
        assert e.value.code == N.SRG_ERR_ARG

    refused(ev.DevicePathTable.from_arrays(latency_ns=lat, key=key, diag=diag, unit=1))  # both
    none = ev.DevicePathTable.from_arrays(latency_ns=lat)
    none.latency_ns = None
    refused(none)                                                                        # neither
    refused(ev.DevicePathTable.from_arrays(key=key, unit=1))                             # keys, no diag
    refused(ev.DevicePathTable.from_arrays(key=key, diag=diag, unit=0))                  # unit < 1
    no_chance = {k: v for k, v in b.items() if k != "chance"}
    refused(ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss), no_chance)  # loss, no chance
    # the range checks apply to dropped events too: dst_host is the caller's to resolve
    loss1 = np.ones_like(loss)
    bad = dict(b, dst_host=b["dst_host"].copy(), payload_size=np.full(100, 9, np.uint32))
    bad["dst_host"][4] = 7
    refused(ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss1), bad)
