"""GPU: interface receive (srg_sockets_in_*, shadow_amd/csrc/sockets_in.hip.h) against
tests/sockets_in_ref.py, the plain-Python restatement that the hand-worked KATs pin
(test_sockets_in_cpu.py).  After every call of every scenario of sockets_in_scenarios.py every output
row, the result struct, every socket's state and every host's counters are compared exactly: hosts
1, 3, 64, 65 with 0, 1, 8 sockets and 0, 1, 63, 64, 65, 129 operations per socket and step as pure
deliveries, pure reads and alternating; runs across a 64-operation boundary, buffers that fill in the
middle of a run and exactly at its end; tables of 1, 2 and 1 000 associations per host with removal
and reassociation; skipped rows under both deliver_status values; 8 steps with configure between
them; every refused call followed by a valid step.  Then the composition: Round.receive ->
SocketsIn.step_device on the result's borrowed arrays, Round.send -> a second step over its local
rows, against round_ref.py chained with sockets_in_ref.py."""
import numpy as np
import pytest

import sockets_in_ref as R
import sockets_in_scenarios as S
from shadow_amd import _native as N
from shadow_amd import events as ev
from shadow_amd.graph import NetGraphError

pytestmark = pytest.mark.gpu


def upload_packets(sk, pk, dev):
    import torch

    def t(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    sk.set_packets(t(pk[0], np.uint8), ev._i32(pk[1], dev), t(np.array(pk[2], np.uint16).view(np.int16), np.int16),
                   t(np.array(pk[3], np.uint16).view(np.int16), np.int16), ev._i32(pk[4], dev), ev._i32(pk[5], dev))


def check_state(sk, snap):
    socks, counters = snap
    for h, hs in enumerate(socks):
        for slot, exp in enumerate(hs):
            assert sk.socket_state(h, slot) == exp, (h, slot)
        assert sk.host_counters(h) == counters[h], h


def columns(entries, n):
    return [[e[i] for e in entries] for i in range(n)]


def apply_op(sk, op):
    """-> ("ok", outputs...) or ("err", code), as sockets_in_scenarios.run_ref records them"""
    try:
        if op[0] == "step":
            _, status, time, tag, off, ds, rt, rs, rf, roff = op
            out = sk.step(status, np.array(time, np.uint64), np.array(tag, np.uint64), np.array(off, np.uint64), ds,
                          np.array(rt, np.uint64), np.array(rs, np.uint32), np.array(rf, np.uint8), np.array(roff, np.uint64))
            return ("ok",) + out
        if op[0] == "reset":
            return ("ok", sk.host_counters(op[1], reset=True))
        n = {"configure": 7, "associate": 6, "disassociate": 5}[op[0]]
        getattr(sk, op[0])(*columns(op[1], n))
        return ("ok",)
    except NetGraphError as e:
        return ("err", e.code)


def compare(got, exp, where):
    assert got[0] == exp[0], (where, got[:2], exp[:2])
    if exp[0] == "err":
        assert got[1] == exp[1], where
    elif len(exp) == 2:  # a counters read-back
        assert got[1] == exp[1], where
    elif len(exp) > 2:
        for k, name in enumerate(("status", "slot", "read status", "read tag", "read time", "read payload"), 1):
            assert [int(x) for x in got[k]] == list(exp[k]), (where, name)
        for k, v in exp[7].items():
            assert got[7][k] == v, (where, k)


@pytest.mark.parametrize("scn", S.all_scenarios(), ids=lambda s: s["name"])
def test_scenarios_match_the_restatement(router, scn):
    _, recs = S.run_ref(scn)
    sk = ev.SocketsIn(router, scn["sockets_per_host"])
    if scn["packets"] is not None:
        upload_packets(sk, scn["packets"], sk.dev)
    for i, (op, rec) in enumerate(zip(scn["ops"], recs)):
        compare(apply_op(sk, op), rec[:-1], (scn["name"], i, op[0]))
        check_state(sk, rec[-1])
    sk.close()


def test_message_store_grows_from_a_small_reserve(router):
    """reserve_messages 1, then 300 messages: the store reallocates and keeps every message."""
    b = S.Builder([1])
    b.ops.append(("associate", S.wildcard_assoc(b)))
    for i in range(300):
        b.deliver(0, 10 + i, b.packet(S.UDP_PROTO, 1, 1, 1000, 7))
    b.end_step()
    for i in range(300):
        b.read(0, 1000 + i, 0)
    b.end_step()
    scn = b.scenario("grow")
    _, recs = S.run_ref(scn)
    sk = ev.SocketsIn(router, [1], reserve=1)
    upload_packets(sk, scn["packets"], sk.dev)
    for i, (op, rec) in enumerate(zip(scn["ops"], recs)):
        compare(apply_op(sk, op), rec[:-1], ("grow", i))
        check_state(sk, rec[-1])
    assert recs[1][7]["num_buffered_messages"] == 300 and recs[2][7]["num_read"] == 300
    sk.close()


def test_round_composition(router):
    """The closed loop of test_round_gpu.py (23 hosts, 6 nodes): each round's receive result goes into
    SocketsIn.step_device through its borrowed device pointers, without a copy; the send result's
    local rows (SRG_ROUND_LOCAL) go through a second step.  Against round_ref.py chained with
    sockets_in_ref.py."""
    import torch
    import test_round_gpu as TR
    import outbound_ref as OR
    rng, lat, loss, host_node, bw_up, bw_down, sockets, seeds = TR.loop_setup()
    b = TR.Both(router, host_node, lat, loss, bw_up, bw_down, sockets, OR.QDISC_FIFO, seeds, 0, TR.BOOT, TR.SIM_END)
    H, dev = TR.H, b.dev
    nsock = [3] * H
    sk = ev.SocketsIn(router, nsock)
    ref = R.SocketsInRef(nsock)
    assoc = [(h, 17, 1000 + s, 0, 0, s) for h in range(H) for s in range(2)]  # port 1002 stays unbound
    sk.associate(*columns(assoc, 6))
    ref.associate(assoc)
    cfg = [(h, 1, R.EXTERNAL if h % 3 == 0 else R.UDP, 0, 0, 0, 4000) for h in range(H)]
    sk.configure(*columns(cfg, 7))
    ref.configure(cfg)
    prio, start = [0] * H, TR.T0
    seen = dict.fromkeys(R.RESULT_KEYS, 0)

    def step_both(res, e, deliver_status, reads):
        n = len(b.dst)
        tags = np.arange(n)
        pk = [[17] * n, (tags * 7 + 1).tolist(), (tags % 50 + 1).tolist(), (1000 + tags % 3).tolist(), b.size, b.payload]
        upload_packets(sk, pk, dev)
        ref.set_packets(*pk)
        rt, rs, rf, roff = reads
        exp = ref.step(e["status"], e["time"], e["tag"], e["host_offsets"], deliver_status, rt, rs, rf, roff)
        m, nr = int(res.num_leaving), len(rt)
        o_st = torch.empty(max(m, 1), dtype=torch.uint8, device=dev)
        o_sl = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        q_st = torch.empty(max(nr, 1), dtype=torch.uint8, device=dev)
        q = [torch.empty(max(nr, 1), dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.int32)]
        rc, got, msg = sk.step_device(
            m, res.status_dev, res.time_ns_dev, res.tag_dev, res.host_offsets_dev, deliver_status, nr,
            ev._i64(np.array(rt, np.uint64), dev), ev._i32(np.array(rs, np.uint32), dev),
            torch.from_numpy(np.array(rf, np.uint8)).to(dev), ev._i64(np.array(roff, np.uint64), dev), o_st, o_sl, q_st, *q)
        assert rc == N.SRG_OK, msg
        assert o_st[:m].cpu().numpy().tolist() == exp[0]
        assert o_sl[:m].cpu().numpy().view(np.uint32).tolist() == exp[1]
        assert q_st[:nr].cpu().numpy().tolist() == exp[2]
        assert q[0][:nr].cpu().numpy().view(np.uint64).tolist() == exp[3]
        assert q[1][:nr].cpu().numpy().view(np.uint64).tolist() == exp[4]
        assert q[2][:nr].cpu().numpy().view(np.uint32).tolist() == exp[5]
        for k, v in exp[6].items():
            assert got[k] == v, k
            seen[k] += v
        check_state(sk, S.snapshot(ref))

    for rnd in range(8):
        ws, we = ev.next_window(start, TR.RUNAHEAD, TR.SIM_END)
        e = b.ref.receive(we)
        b.upload()
        rc, res, msg = b.rd.receive_device(we)
        assert rc == N.SRG_OK, msg
        # each host reads slot 0 twice at the window's end, after its deliveries
        rt = [we] * (2 * H)
        step_both(res, e, 1, (rt, [0] * (2 * H), [0, R.READ_PEEK] * H, list(range(0, 2 * H + 1, 2))))
        offers = TR.loop_offers(rng, ws, we, sockets, prio, b.add_packet)
        time, slot, pr, flags, tag, offs = TR.flatten(offers)
        e = b.ref.send(we, time, slot, pr, flags, tag, offs)
        b.upload()
        rc, res, msg = b.rd.send_device(
            we, len(time), ev._i64(np.array(time, np.uint64), dev), ev._i32(np.array(slot, np.uint32), dev),
            ev._i64(np.array(pr, np.uint64), dev), torch.from_numpy(np.array(flags, np.uint8)).to(dev),
            ev._i64(np.array(tag, np.uint64), dev), ev._i64(np.array(offs, np.uint64), dev))
        assert rc == N.SRG_OK, msg
        step_both(res, e, N.SRG_ROUND_LOCAL, ([], [], [], [0] * (H + 1)))
        start = e["next_start_ns"]
    assert seen["num_buffered"] > 100 and seen["num_no_socket"] > 50 and seen["num_external"] > 10
    assert seen["num_skipped"] > 100 and seen["num_read"] > 50
    sk.close()
    b.close()
