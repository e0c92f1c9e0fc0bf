"""GPU: the hosts' inbound path (srg_inbound_*, shadow_amd/csrc/inbound.hip.h) against
tests/inbound_ref.py, the plain-Python restatement of the reference that the golden KATs pin
(test_inbound_cpu.py).  Every output array, every result field and every host's state are compared
exactly, after every step of every scenario of inbound_scenarios.py: the overload scenario as one
step, as 50 ms windows and as 1 ms windows; hosts 1, 3, 64, 65 with 0, 1, 63, 64, 65, 129 arrivals
per host and step and a backlog across a chunk edge; the hand-made boundaries (a task exactly at
`until`, an arrival exactly at a pending wake time and on a refill boundary, the bootstrap boundary,
an unlimited host, max(1, ...) at 7 999 bit/s, size-0 packets, a packet of the bucket's whole
capacity that needs 1500 refills).  Then the control law on the device against math.sqrt, every
error with a check that nothing moved, and an 8-round loop send_packets -> EventQueues.push -> pop
-> Inbound.step -> next_window with the wake folded in."""
import heapq
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import inbound_ref as R
import inbound_scenarios as S
from shadow_amd import _native as N
from shadow_amd import events as ev
from shadow_amd.graph import NetGraphError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = 2**64 - 1


def u64(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def check_states(inb, ref, sim_start):
    for h in range(inb.num_hosts):
        exp = dict(ref.host_state(h))
        if exp["last_refill_ns"] is None:  # an unlimited host has no bucket: the record keeps sim_start
            exp["last_refill_ns"] = sim_start
        assert inb.host_state(h) == exp, h


def step_both(inb, ref, until, per_host, sim_start):
    time, size, tag, offs = S.flatten(per_host)
    e_st, e_tm, e_tg, e_off, e_res = ref.step(until, time, size, tag, offs)
    st, tm, tg, off, res = inb.step(until, np.array(time, np.uint64), np.array(size, np.uint32), np.array(tag, np.uint64),
                                    np.array(offs, np.uint64))
    assert u64(off) == e_off, "host offsets"
    assert st.cpu().numpy().tolist() == e_st, "status"
    assert u64(tm) == e_tm, "leave times"
    assert u64(tg) == e_tg, "tags"
    for k, v in e_res.items():
        assert res[k] == v, k
    assert inb.num_queued == e_res["num_queued"] and inb.min_next_wake_ns == e_res["min_next_wake_ns"]
    check_states(inb, ref, sim_start)
    return e_st, e_tm, e_tg, e_off, e_res


@pytest.mark.parametrize("scn", S.all_scenarios(), ids=lambda s: s[0])
def test_scenarios_match_the_reference(router, scn):
    _, bw, sim_start, boot, steps = scn
    inb = ev.Inbound(router, bw, sim_start, boot)
    ref = R.Inbound(bw, sim_start, boot)
    check_states(inb, ref, sim_start)
    for until, per_host in steps:
        step_both(inb, ref, until, per_host, sim_start)
    inb.close()


def test_scenarios_reach_every_branch_and_windows_agree():
    """The coverage condition over the scenarios used above, and the overload scenario's three
    window widths leaving the same packets at the same times (the device equals the reference step
    by step above, so the reference's concatenations stand for it)."""
    for k in R.COUNTERS:
        R.COUNTERS[k] = 0
    outs = {s[0]: S.run_ref(s)[0] for s in S.all_scenarios()}
    assert all(R.COUNTERS[k] > 0 for k in R.BRANCHES), R.COUNTERS
    a, b, c = (S.concat_by_host(outs[k], 1) for k in ("overload_one_step", "overload_50ms", "overload_1ms"))
    assert a == b == c and len(a[0]) == 600


def test_control_law_on_the_device():
    """round(1e8 / sqrt(count)) as the device computes it (f64 sqrt, f64 divide, round half away from
    zero) for counts 0..4096 and twenty counts up to 2^32, from the test build's kernel."""
    lib = os.path.join(os.path.dirname(HERE), "shadow_amd", "libshadow_routing_testhooks.so")
    assert os.path.exists(lib), "build the libraries first (python shadow_amd/build.py)"
    big = [2**32, 2**32 - 1, 2**31 + 1, 2**31, 2**30 + 12345, 3 * 2**29, 10**9 + 7, 999999937, 2**28 - 1, 123456789,
           10**8, 10**8 + 1, 99999999, 2**24 + 1, 16777213, 10**7 + 19, 5000011, 1000003, 65537, 4099]
    counts = list(range(0, 4097)) + big
    env = dict(os.environ, SRG_LIB_PATH=lib)
    p = subprocess.run([sys.executable, "-u", os.path.join(HERE, "inbound_law_run.py"), json.dumps(counts)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    exp = [R.control_law(0, c) for c in counts]
    bad = [(c, g, e) for c, g, e in zip(counts, got, exp) if g != e]
    assert not bad, bad[:10]
    assert exp[0] == exp[1] == 100_000_000 and exp[4] == 50_000_000
    assert exp[2] == int(math.floor(1e8 / math.sqrt(2.0) + 0.5))


def test_errors_leave_the_state(router):
    S0, MS = S.SIM_START, S.MS
    bw = [1_000_000, U64, 1_000_000]
    inb = ev.Inbound(router, bw, S0, S0)
    ref = R.Inbound(bw, S0, S0)
    first = [[(S0 + MS, 1500, 1), (S0 + 2 * MS, 1500, 2), (S0 + 2 * MS, 1500, 3)], [(S0 + 3 * MS, 99, 4)], []]
    step_both(inb, ref, S0 + 5 * MS, first, S0)
    until = S0 + 9 * MS

    def refused(code, time, size, tag, offs, until=until, capacity=None):
        import torch
        dev = inb.dev
        t_t, s_t, g_t, o_t = ev._i64(np.array(time, np.uint64), dev), ev._i32(np.array(size, np.uint32), dev), \
            ev._i64(np.array(tag, np.uint64), dev), ev._i64(np.array(offs, np.uint64), dev)
        cap = inb.num_queued + len(time) if capacity is None else capacity
        out = [torch.zeros(max(cap, 1), dtype=d, device=dev) for d in (torch.uint8, torch.int64, torch.int64)]
        ooff = torch.zeros(len(bw) + 1, dtype=torch.int64, device=dev)
        queued, wake = inb.num_queued, inb.min_next_wake_ns
        rc, res, msg = inb.step_device(until, len(time), t_t, s_t, g_t, o_t, cap, out[0], out[1], out[2], ooff)
        assert rc == code, (rc, msg)
        assert msg
        assert inb.num_queued == queued and inb.min_next_wake_ns == wake
        check_states(inb, ref, S0)
        return res

    t = S0 + 6 * MS
    refused(N.SRG_ERR_TIME_BACKWARD, [S0 + MS], [40], [9], [0, 1, 1, 1])          # before host 0's last arrival
    refused(N.SRG_ERR_TIME_BACKWARD, [t, t - 1], [40, 40], [9, 10], [0, 0, 0, 2])  # decreasing inside a slice
    refused(N.SRG_ERR_ARG, [until], [40], [9], [0, 1, 1, 1])                       # time >= until
    refused(N.SRG_ERR_ARG, [S0 - 1], [40], [9], [0, 0, 0, 1])                      # below the simulation start
    refused(N.SRG_ERR_ARG, [2**62], [40], [9], [0, 0, 0, 1], until=2**62)          # at the domain's end
    refused(N.SRG_ERR_ARG, [t], [40], [9], [0, 0, 0, 1], until=2**62 + 1)          # until outside the domain
    refused(N.SRG_ERR_ARG, [t, t], [40, 40], [9, 10], [0, 2, 1, 2])                # offsets not monotone
    refused(N.SRG_ERR_ARG, [t, t], [40, 40], [9, 10], [0, 1, 1, 1])                # offsets not ending at n
    refused(N.SRG_ERR_ARG, [t], [1626], [9], [0, 0, 0, 1])                         # above the bucket's capacity
    # capacity short: the need is reported, nothing moved; host 0's blocked packet leaves before `far`
    far = S0 + 100 * MS
    e = R.Inbound(bw, S0, S0)
    e.step(S0 + 5 * MS, *S.flatten(first))
    need = len(e.step(far, [t], [40], [9], [0, 0, 0, 1])[0])
    assert need >= 2
    res = refused(N.SRG_ERR_ARG, [t], [40], [9], [0, 0, 0, 1], until=far, capacity=need - 1)
    assert res["num_forwarded"] + res["num_dropped"] == need
    rc, res, _ = inb.step_device(far, 0, None, None, None, ev._i64(np.zeros(4, np.uint64), inb.dev), 0, None, None, None,
                                 None)
    assert rc == N.SRG_ERR_ARG and res["num_forwarded"] + res["num_dropped"] == need - 1  # a sizing call
    check_states(inb, ref, S0)
    # the next step runs as if none of them had happened
    step_both(inb, ref, far, [[], [], [(t, 40, 9)]], S0)
    with pytest.raises(NetGraphError):
        inb.host_state(3)
    inb.close()


def test_round_loop(router):
    """8 rounds of send_packets -> EventQueues.push -> pop -> Inbound.step -> next_window, the pop's
    device tensors feeding the step without a copy; against heapq queues feeding inbound_ref.py."""
    import torch
    H, TN, n, runahead, t0 = 37, 8, 1500, 5_000_000, 10**12
    rng = np.random.default_rng(11)
    lat = rng.integers(1_000_000, 4_000_000, (TN, TN)).astype(np.uint64)
    bws = [U64, 1_000_000, 8_000_000, 50_000_000, 7_999]
    bw = [bws[h % len(bws)] for h in range(H)]
    boot = t0 + 7_000_000
    q = ev.EventQueues(router, H)
    inb = ev.Inbound(router, bw, 0, boot)
    ref_q = [[] for _ in range(H)]
    ref = R.Inbound(bw, 0, boot)
    dev = inb.dev
    sizes_all = torch.zeros(0, dtype=torch.int32, device=dev)
    sizes_host = []
    start, total_left = t0, 0
    for rnd in range(8):
        win = ev.next_window(start, runahead, t0 + 10**9)
        assert win is not None
        ws, we = win
        # pop the window, run the hosts' inbound path
        off = torch.empty(H + 1, dtype=torch.int64, device=dev)
        rc, res, msg = q.pop_device(we, 0, None, None, None, None, off)
        m = int(res["num_moved"]) if rc == N.SRG_ERR_ARG else 0
        t_t = torch.empty(max(m, 1), dtype=torch.int64, device=dev)[:m]
        g_t = torch.empty(max(m, 1), dtype=torch.int64, device=dev)[:m]
        if m:
            rc, res, msg = q.pop_device(we, m, t_t, None, None, g_t, off)
        assert rc == N.SRG_OK, msg
        s_t = sizes_all[g_t] if m else torch.empty(0, dtype=torch.int32, device=dev)
        st, tm, tg, ooff, ires = inb.step(we, t_t, s_t, g_t, off)
        per_host = []
        for h in range(H):
            mine = []
            while ref_q[h] and ref_q[h][0][0] < we:
                e = heapq.heappop(ref_q[h])
                mine.append((e[0], sizes_host[e[3]], e[3]))
            per_host.append(mine)
        e_st, e_tm, e_tg, e_off, e_res = ref.step(we, *S.flatten(per_host))
        assert u64(ooff) == e_off and st.cpu().numpy().tolist() == e_st and u64(tm) == e_tm and u64(tg) == e_tg, rnd
        for k, v in e_res.items():
            assert ires[k] == v, (rnd, k)
        total_left += len(e_st)
        # the round's sends, at the barrier
        batch, _, loss = ev.synthetic_round(n, H, TN, seed=100 + rnd, t0=ws, runahead=we - ws, loss=0.05)
        db = ev.DeviceSendBatch(batch, H, we, boot, dev)
        table = ev.DevicePathTable.from_arrays(latency_ns=lat, packet_loss=loss, device=dev)
        base = len(sizes_host)
        size = (batch["payload_size"] + 40).astype(np.uint32)
        sizes_host += size.tolist()
        sizes_all = torch.cat([sizes_all, ev._i32(size, dev)])
        tags = ev._i64(np.arange(base, base + n, dtype=np.uint64), dev)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        deliver = torch.empty(n, dtype=torch.int64, device=dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        hoff = torch.empty(H + 1, dtype=torch.int64, device=dev)
        sres = ev.send_packets_device(router, db, table, status, deliver, order, hoff)
        q.push(db, deliver, order, sres["num_sent"], tags)
        sent = status.cpu().numpy() != 0
        dl = deliver.cpu().numpy().view(np.uint64)
        for i in np.flatnonzero(sent):
            heapq.heappush(ref_q[int(batch["dst_host"][i])],
                           (int(dl[i]), int(batch["src_host"][i]), int(batch["src_event_id"][i]), base + int(i)))
        e_next = min(min((x[0][0] for x in ref_q if x), default=U64), e_res["min_next_wake_ns"])
        start = min(q.min_next_event_ns, inb.min_next_wake_ns)  # a pending forward task is a local event
        assert start == e_next, rnd
    assert total_left > 1000
    q.close()
    inb.close()
