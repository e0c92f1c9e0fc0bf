"""CPU side of the round driver (per-host RNG, draw rule, event ids):
1. tests/round_ref.py's Xoshiro256++ and SplitMix64 give the generator's published vector, the
   state of seed_from_u64(0) and the chance values of tests/golden/round_kats.json;
2. shadow_amd/csrc/round_rule.h, the header the kernels run, replays the vectors and a draw scenario
   with every status through tests/cpp/round_rule_check.cpp (g++, -Werror, -ffp-contract=off,
   ASan + UBSan) and agrees with round_ref.py line by line;
3. the draw rule's cases on the restatement: loss 0 / loss 1, payload 0, the bootstrap boundary, the
   packets that do not draw; the generator advances by exactly the number of drawing packets and a
   packet dropped by loss takes no event id;
4. round_ref.Round restores itself on an error;
5. the new ctypes structs have the C sizes and the binding names every srg_round_* function.
The GPU side: tests/test_round_gpu.py."""
import ctypes
import json
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

import round_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def kats():
    with open(os.path.join(HERE, "golden", "round_kats.json")) as f:
        return json.load(f)


def test_generator_vectors():
    k = kats()
    g = R.Xoshiro256PlusPlus(k["state"])
    assert [g.next_u64() for _ in k["outputs"]] == k["outputs"]
    assert k["outputs"][0] == 41943041 and k["outputs"][9] == 10450023813501588000
    s = R.Xoshiro256PlusPlus.seed_from_u64(k["seed"]).s
    assert ["%016x" % x for x in s] == k["seed_state_hex"]
    assert k["seed_state_hex"][0] == "e220a8397b1dcdaf"
    g = R.Xoshiro256PlusPlus(k["state"])
    assert ["%016x" % f64_bits(g.gen_f64()) for _ in k["chance_bits_hex"]] == k["chance_bits_hex"]
    assert all(0.0 <= float(c) < 1.0 for c in k["chance_repr"])
    # 53 bits: the largest value is 1 - 2^-53, never 1.0
    assert (M := (2**64 - 1) >> 11) * (1.0 / (1 << 53)) == 1.0 - 2.0**-53 and M == 2**53 - 1


@pytest.fixture(scope="module")
def rule_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("round") / "round_rule_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(HERE, "cpp", "round_rule_check.cpp")], check=True)
    return str(exe)


def run_check(exe, text, tmp_path):
    p = tmp_path / "script.txt"
    p.write_text(text)
    r = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


BOOT, END = 5_000, 9_000


def draw_scenario(seed=11, n=300):
    """One host's leaving packets with every status: local, after the end, no host, drawing before
    and after the bootstrap end, payload 0, losses 0, 1 and in between."""
    rnd = random.Random(seed)
    pk = []
    for i in range(n):
        st = 2 if rnd.random() < 0.1 else 1
        t = rnd.choice([BOOT - 1, BOOT, BOOT + 1, END - 1, END, END + 7, rnd.randrange(0, END)])
        dst = R.NO_HOST if rnd.random() < 0.1 else rnd.randrange(0, 5)
        loss = float(np.float32(rnd.choice([0.0, 1.0, 0.5, 1e-9, rnd.random()])))
        payload = 0 if rnd.random() < 0.2 else rnd.randrange(1, 1461)
        pk.append((st, t, dst, loss, payload))
    return pk


def ref_host_lines(seed, eid, have_loss, pk):
    g = R.Xoshiro256PlusPlus.seed_from_u64(seed)
    res, eid = R.draw_host(g, eid, pk, have_loss, BOOT, END)
    lines = ["P %d %d %d" % (c, 0 if ch is None else f64_bits(ch), -1 if e is None else e) for c, ch, e in res]
    return lines + ["G %d %d %d %d %d" % (*g.s, eid)], res


def test_header_matches_restatement(rule_check, tmp_path):
    k = kats()
    pk = draw_scenario()
    text = ["state %d %d %d %d %d" % (*k["state"], 10), "seed 0", "seed 18446744073709551615", "chance 7 20"]
    exp = ["U %d" % x for x in k["outputs"]]
    for s in (0, 2**64 - 1):
        exp.append("W %d %d %d %d" % tuple(R.Xoshiro256PlusPlus.seed_from_u64(s).s))
    g = R.Xoshiro256PlusPlus.seed_from_u64(7)
    exp += ["C %d" % f64_bits(g.gen_f64()) for _ in range(20)]
    seen = set()
    for have_loss in (1, 0):
        text.append("host 99 5 %d %d %d %d" % (have_loss, BOOT, END, len(pk)))
        text += ["%d %d %d %d %d" % (st, t, dst, f32_bits(loss), pay) for st, t, dst, loss, pay in pk]
        lines, res = ref_host_lines(99, 5, bool(have_loss), pk)
        exp += lines
        seen |= {c for c, _, _ in res}
    assert seen == {R.DROPPED, R.SENT, R.LOCAL, R.AFTER_END, R.NO_DST}
    got = run_check(rule_check, "\n".join(text) + "\n", tmp_path)
    assert len(got) == len(exp)
    for i, (a, b) in enumerate(zip(got, exp)):
        assert a == b, i
    assert got[10] == "W %d %d %d %d" % tuple(int(x, 16) for x in k["seed_state_hex"])


def steps_between(seed, words):
    g = R.Xoshiro256PlusPlus.seed_from_u64(seed)
    for n in range(10_000):
        if g.s == list(words):
            return n
        g.next_u64()
    raise AssertionError("state not reached")


def test_draw_rule_cases():
    def run(pk, have_loss=True):
        g = R.Xoshiro256PlusPlus.seed_from_u64(3)
        res, eid = R.draw_host(g, 0, pk, have_loss, BOOT, END)
        return [c for c, _, _ in res], [e for _, _, e in res], eid, steps_between(3, g.s)
    # loss 0: nothing is dropped; every status-1 packet inside the simulation draws and takes an id
    st, ids, eid, adv = run([(1, BOOT + i, 1, 0.0, 100) for i in range(10)])
    assert st == [R.SENT] * 10 and ids == list(range(10)) and eid == 10 and adv == 10
    # loss 1: dropped past the bootstrap end when the payload is > 0; never with payload 0; never before it
    pk = [(1, BOOT - 1, 1, 1.0, 100), (1, BOOT, 1, 1.0, 100), (1, BOOT, 1, 1.0, 0), (1, BOOT + 1, 1, 1.0, 1)]
    st, ids, eid, adv = run(pk)
    assert st == [R.SENT, R.DROPPED, R.SENT, R.DROPPED] and ids == [0, None, 1, None] and eid == 2 and adv == 4
    # without a loss table nothing is dropped, the draws still happen
    st, ids, eid, adv = run(pk, have_loss=False)
    assert st == [R.SENT] * 4 and eid == 4 and adv == 4
    # after the end and without a host: no draw, no id; the end is checked first; local never draws
    pk = [(1, END, 1, 0.0, 9), (1, END, R.NO_HOST, 0.0, 9), (1, END - 1, R.NO_HOST, 0.0, 9), (2, 10, 0, 0.0, 9),
          (2, END + 1, 0, 0.0, 9), (1, END - 1, 2, 0.0, 9)]
    st, ids, eid, adv = run(pk)
    assert st == [R.AFTER_END, R.AFTER_END, R.NO_DST, R.LOCAL, R.LOCAL, R.SENT] and eid == 1 and adv == 1


def small_round():
    """3 hosts on 2 nodes, no loss table; host 1's downstream bucket holds 1000 + 1500 bytes."""
    lat = [[1000, 2000], [2000, 1000]]
    r = R.Round([0, 1, 1], lat, None, [R.U64] * 3, [R.U64, 8_000_000, R.U64], [2, 1, 1], 0, [1, 2, 3], 0, 0, 10**9)
    dst, size, payload = [1, 2, 0, 1, R.NO_HOST, 2], [100, 200, 300, 2501, 50, 60], [60, 160, 260, 2461, 10, 20]
    r.set_packets(dst, size, payload)
    return r


def snapshot(r):
    return ([r.host_rng(h) for h in range(r.H)], [sorted(q) for q in r.q], list(r.last_popped),
            [r.out.host_state(h) for h in range(r.H)], [r.inb.host_state(h) for h in range(r.H)])


def test_restatement_round_and_errors():
    r = small_round()
    d = r.send(10_000, [9_900, 9_900, 9_900], [0, 1, 0], [1, 2, 1], None, [0, 1, 2], [0, 2, 3, 3])
    assert d["num_leaving"] == 3 and d["num_sent"] == 3 and d["min_next_event_ns"] == 11_900
    assert [r.host_rng(h)[1] for h in range(3)] == [2, 1, 0]
    before = snapshot(r)
    for args, code in (
            ((20_000, [10_100], [0], [3], None, [6], [0, 1, 1, 1]), R.ERR_ARG),   # tag >= num_packets
            ((20_000, [10_100], [0], [3], [1], [5], [0, 1, 1, 1]), R.ERR_ARG),    # the local bit is derived
            ((20_000, [10_100], [0], [3], None, [3], [0, 1, 1, 1]), R.ERR_ARG),   # above host 1's downstream bucket
            ((20_000, [10_100], [0], [3], None, [5], [0, 1, 1, 2]), R.ERR_ARG)):  # offsets
        with pytest.raises(R.RoundRefError) as e:
            r.send(*args)
        assert e.value.code == code and snapshot(r) == before
    rc = r.receive(12_001)
    assert rc["num_popped"] == 3 and r.last_popped == [11_900] * 3
    # a send whose window end lies below the last popped time: host 2 -> host 1 arrives at 11 400,
    # the push is refused after the outbound step ran, everything is restored
    before = snapshot(r)
    with pytest.raises(R.RoundRefError) as e:
        r.send(10_500, [10_400], [0], [9], None, [0], [0, 0, 0, 1])
    assert e.value.code == R.ERR_TIME_BACKWARD and snapshot(r) == before
    d = r.send(12_001, [10_400], [0], [9], None, [0], [0, 0, 0, 1])
    assert d["num_sent"] == 1 and r.host_rng(2)[1] == 1


def test_struct_sizes_and_binding_names():
    from shadow_amd import _native as N
    assert ctypes.sizeof(N.RoundReceiveResult) == 18 * 8
    assert ctypes.sizeof(N.RoundSendResult) == 18 * 8
    assert N.RoundSendResult.ms_total.offset == 17 * 8 and N.RoundReceiveResult.ms_total.offset == 17 * 8
    for name in ("srg_round_create", "srg_round_destroy", "srg_round_set_packets", "srg_round_receive_device",
                 "srg_round_send_device", "srg_round_host_rng", "srg_round_set_host_rng", "srg_round_queues",
                 "srg_round_inbound", "srg_round_outbound"):
        assert name in N.EXPORTS
        assert hasattr(N.lib(), name)  # a missing symbol fails here
