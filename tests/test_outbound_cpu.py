"""CPU side of the hosts' outbound path (socket qdisc + upstream token bucket):
1. tests/outbound_ref.py, the plain-Python restatement of the reference, passes the hand-derived KATs
   (tests/golden/outbound_kats.json);
2. shadow_amd/csrc/outbound_rule.h, the header the kernels run, replays the KATs and the shared
   scenarios (outbound_scenarios.py) through tests/cpp/outbound_rule_check.cpp (g++, -Werror,
   -ffp-contract=off, ASan + UBSan) and agrees with outbound_ref.py line by line: outputs, results,
   per-host state and the heap or queue array;
3. errors leave the state unchanged;
4. the scenarios reach every branch counter of outbound_ref.py;
5. the barrier bit: irrelevant for the FIFO qdisc with unique increasing priorities (where the heap
   is also the "smallest queued priority" model), relevant with control packets and for round robin;
6. the overload scenario in one step, 50 ms windows and 1 ms windows leaves the same packets at the
   same times;
7. the new ctypes structs have the C sizes;
8. the qdisc against the reference's own compiled code.  tests/golden/qdisc_reference.json holds offer /
   select scripts with the output of oracle/_ref/qdisc_ref, which is the reference's priority_queue.c
   and network_queuing_disciplines.c compiled from a checkout (oracle/ref_qdisc/): free interleavings,
   the operations outbound_ref.py performs on the time-domain scenarios qdisc_* (its trace hook), and
   those of the KATs.  Where the program is built the fixture regenerates byte for byte and 420 further
   scripts agree with SocketHeap / SocketRing; without it the fixture replays through those classes,
   the header's leaving order on the qdisc_* scenarios is the program's selection order, the scripts
   reach the heap's special cases at 65 and 129 queued sockets, and three plausible wrong heaps each
   fail on the fixture.  Pinned this way: heap, comparator, round-robin queue.  Still restated (in
   the driver too): the sockets' FIFOs, wantsSend, the selection loop, relay and bucket.
The GPU side: tests/test_outbound_gpu.py."""
import ctypes
import heapq
import os
import shutil
import subprocess

import pytest

import outbound_ref as R
import outbound_scenarios as S

HERE = os.path.dirname(os.path.abspath(__file__))
STATE_KEYS = ("balance", "last_refill_ns", "pending", "wake_ns", "has_cached", "cached_tag", "queued", "qdisc_len")


def test_reference_restatement_passes_kats():
    kats = S.load_kats()
    assert len(kats) == 7
    for k in kats:
        outs, states, orders = S.run_ref(S.kat_scenario(k))
        for i, step in enumerate(k["steps"]):
            st, tm, tg, _, _ = outs[i]
            assert [list(x) for x in zip(st, tm, tg)] == step["out"], (k["name"], i)
            assert orders[i][0] == step["order"], (k["name"], i)
            for key, v in step.get("state", {}).items():
                assert states[i][0][key] == v, (k["name"], i, key)


@pytest.fixture(scope="module")
def rule_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("outbound") / "outbound_rule_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(HERE, "cpp", "outbound_rule_check.cpp")], check=True)
    return str(exe)


def run_check(exe, text, tmp_path):
    p = tmp_path / "scenario.txt"
    p.write_text(text)
    r = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def scenario_text(scn):
    _, bw, sockets, qdisc, sim_start, boot, steps = scn
    out = ["%d %d %d %d" % (len(bw), qdisc, sim_start, boot)] + ["%d %d" % (b, n) for b, n in zip(bw, sockets)]
    for until, per_host in steps:
        out.append("step %d %d" % (until, sum(len(a) for a in per_host)))
        for h, a in enumerate(per_host):
            out += ["%d %d %d %d %d %d %d" % ((h,) + tuple(e)) for e in a]
    return "\n".join(out) + "\n"


def ref_lines(scn):
    bw, sim_start = scn[1], scn[4]
    outs, states, orders = S.run_ref(scn)
    lines = []
    for (st, tm, tg, oo, res), hs, os_ in zip(outs, states, orders):
        for h in range(len(bw)):
            lines += ["L %d %d %d %d" % (h, st[j], tm[j], tg[j]) for j in range(oo[h], oo[h + 1])]
        lines.append("R %d %d %d %d" % (res["num_sent"], res["num_local"], res["num_queued"], res["min_next_wake_ns"]))
        for h, s in enumerate(hs):
            s = dict(s)
            if s["last_refill_ns"] is None:  # an unlimited host has no bucket: the header keeps sim_start
                s["last_refill_ns"] = sim_start
            lines.append("S %d " % h + " ".join(str(s[k]) for k in STATE_KEYS))
            lines.append(" ".join(["O %d" % h] + [str(x) for x in os_[h]]))
    return lines


@pytest.mark.parametrize("scn", S.all_scenarios(), ids=lambda s: s[0])
def test_header_matches_reference_on_scenarios(rule_check, tmp_path, scn):
    got = run_check(rule_check, scenario_text(scn), tmp_path)
    ref = ref_lines(scn)
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (scn[0], i)


def test_header_passes_kats(rule_check, tmp_path):
    """The header's lines against the KATs' own expectations (not through outbound_ref.py)."""
    for k in S.load_kats():
        got = run_check(rule_check, scenario_text(S.kat_scenario(k)), tmp_path)
        exp = []
        for step in k["steps"]:
            exp += ["L 0 %d %d %d" % tuple(o) for o in step["out"]]
            exp.append(" ".join(["O 0"] + [str(x) for x in step["order"]]))
        assert [g for g in got if g[0] in "LO"] == exp, k["name"]


def test_header_errors_leave_the_state(rule_check, tmp_path):
    S0, MS = S.SIM_START, S.MS
    u = S0 + 9 * MS
    text = ("1 0 %d %d\n1000000 2\n" % (S0, S0) +
            "step %d 2\n0 %d 0 1 1500 0 1\n0 %d 1 2 1500 0 2\n" % (S0 + 5 * MS, S0 + MS, S0 + 2 * MS) +
            "step %d 1\n0 %d 0 3 40 0 3\n" % (u, S0 + MS) +             # earlier than the last offer
            "step %d 1\n0 %d 0 3 40 0 4\n" % (u, u) +                   # not below until
            "step %d 1\n0 %d 0 3 40 0 5\n" % (u, S0 - 1) +              # below the simulation start
            "step %d 1\n0 %d 0 3 1626 0 6\n" % (u, S0 + 6 * MS) +       # above the bucket's capacity, not local
            "step %d 1\n0 %d 2 3 40 0 7\n" % (u, S0 + 6 * MS) +         # slot out of range
            "step %d 1\n0 %d 0 3 40 4 8\n" % (u, S0 + 6 * MS))          # an unknown flag bit
    got = run_check(rule_check, text, tmp_path)
    states = [g for g in got if g[0] in "SO"]
    errors = [g for g in got if g.startswith("E ")]
    assert errors == ["E 12", "E 1", "E 1", "E 1", "E 1", "E 1"]
    assert len(states) == 14 and len(set(states)) == 2
    ref = R.Outbound([1_000_000], [2], 0, S0, S0)
    ref.step(S0 + 5 * MS, [S0 + MS, S0 + 2 * MS], [0, 1], [1, 2], [1500, 1500], [0, 0], [1, 2], [0, 2])
    before = (ref.host_state(0), ref.host_order(0))
    for code, o in ((12, (S0 + MS, 0, 40, 0)), (1, (u, 0, 40, 0)), (1, (S0 - 1, 0, 40, 0)), (1, (S0 + 6 * MS, 0, 1626, 0)),
                    (1, (S0 + 6 * MS, 2, 40, 0)), (1, (S0 + 6 * MS, 0, 40, 4))):
        with pytest.raises(R.OutboundRefError) as e:
            ref.step(u, [o[0]], [o[1]], [3], [o[2]], [o[3]], [9], [0, 1])
        assert e.value.code == code
        assert (ref.host_state(0), ref.host_order(0)) == before
    with pytest.raises(R.OutboundRefError):
        R.Outbound([1], [1], 2, 0, 0)


def test_scenarios_reach_every_branch():
    R.reset_counters()
    for scn in S.all_scenarios():
        S.run_ref(scn)
    assert all(R.COUNTERS[k] > 0 for k in R.BRANCHES), R.COUNTERS


class MinPriorityHost(R.Host):
    """The independent model: no qdisc structure, the interface sends the smallest queued priority."""

    def offer(self, t, slot, pkt):
        self.sockets[slot].add(pkt)
        if not self.pending:
            self.pending, self.wake, self.wake_from_block = True, t, False
        self.last_time = max(self.last_time, t)

    def interface_pop(self):
        live = [s for s in self.sockets if s.has_data()]
        if not live:
            return None
        return min(live, key=lambda s: s.peek_priority()).pull()


PROPERTY_CASES = [(seed, sockets) for sockets in (1, 2, 5) for seed in range(300)]  # 300 seeds per socket count


def test_fifo_unique_priorities_ignore_the_barrier():
    for seed, sockets in PROPERTY_CASES:
        plain, barred, until = S.property_case(seed, sockets, control=0.0)
        a = S.run_one_host(plain, until, sockets, R.QDISC_FIFO)
        assert len(a) == 200
        assert S.run_one_host(barred, until, sockets, R.QDISC_FIFO) == a, (seed, sockets)
        assert S.run_one_host(plain, until, sockets, R.QDISC_FIFO, MinPriorityHost) == a, (seed, sockets)


@pytest.mark.parametrize("qdisc,control", [(R.QDISC_FIFO, 0.15), (R.QDISC_ROUND_ROBIN, 0.0)], ids=["fifo_control", "rr"])
def test_the_barrier_changes_outputs(qdisc, control):
    differ = 0
    for seed, sockets in PROPERTY_CASES:
        plain, barred, until = S.property_case(seed, sockets, control=control)
        a, b = (S.run_one_host(o, until, sockets, qdisc) for o in (plain, barred))
        assert len(a) == len(b) == 200 and sorted(x[2] for x in a) == sorted(x[2] for x in b)
        differ += a != b
    assert differ >= 1, differ


@pytest.mark.parametrize("qdisc", [R.QDISC_FIFO, R.QDISC_ROUND_ROBIN])
def test_overload_windows_agree(qdisc):
    """One step, 50 ms windows and 1 ms windows leave the same packets at the same times."""
    a, b, c = (S.concat_by_host(S.run_ref(S.overload(w, qdisc))[0], 1) for w in (None, 50 * S.MS, 1 * S.MS))
    assert a == b == c and len(a[0]) == 600


def test_struct_sizes():
    from shadow_amd import _native as N
    assert ctypes.sizeof(N.OutboundResult) == 4 * 8 + 8
    assert ctypes.sizeof(N.OutboundHostState) == 5 * 8 + 4 + 4
    assert N.OutboundHostState.qdisc_len.offset == 40 and N.OutboundHostState.has_cached.offset == 45


# ---- 8. the qdisc against the reference's own compiled code -------------------------------------
QDISC_REF_EXE = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "qdisc_ref")
FREE_SEED, FREE_COUNT = 1000, 10  # tests/golden/make_qdisc_reference.py
EXTRA_SEED, EXTRA_COUNT = 50_000, 210  # per qdisc: 5 of every (sockets, tie, priority mode)


@pytest.fixture(scope="module")
def qref():
    return S.load_qdisc_reference()


def fixture_entries(doc):
    """-> [(id, script, output)]"""
    out = [("free_%d_q%d" % (e["seed"], e["qdisc"]), e["script"], e["output"]) for e in doc["free"]]
    for scn in doc["scenarios"]:
        out += [("%s_host%d" % (scn["name"], h), e["script"], e["output"]) for h, e in enumerate(scn["hosts"])]
    return out + [("kat_" + e["name"], e["script"], e["output"]) for e in doc["kats"]]


def tags_of(output):
    return [int(ln.split()[1]) for ln in output.splitlines() if ln != "-"]


def test_qdisc_fixture_is_what_the_generators_give(qref):
    """The fixture's scripts are today's: the free scripts of its seeds, the traces of today's
    scenarios and KATs.  (Their outputs are the reference program's: the regeneration test.)"""
    assert [e["script"] for e in qref["free"]] == [e["script"] for e in S.free_scripts(FREE_SEED, FREE_COUNT)]
    scns = S.qdisc_scenarios()
    assert [x["name"] for x in qref["scenarios"]] == [scn[0] for scn in scns]
    for x, scn in zip(qref["scenarios"], scns):
        assert [e["script"] for e in x["hosts"]] == [sc for sc, _ in S.trace_ref(scn)[0]], scn[0]
    kats = S.load_kats()
    assert [e["name"] for e in qref["kats"]] == [k["name"] for k in kats]
    assert [e["script"] for e in qref["kats"]] == [S.kat_script(k)[0] for k in kats]
    assert os.path.getsize(os.path.join(HERE, "golden", "qdisc_reference.json")) <= \
        os.path.getsize(os.path.join(HERE, "golden", "routing_vectors.json"))


def test_qdisc_reference_program_regenerates_the_fixture(qref):
    if not os.path.exists(QDISC_REF_EXE):
        pytest.skip("oracle/_ref/qdisc_ref is not built (no reference checkout)")
    entries = fixture_entries(qref)
    got = S.run_qdisc_ref(QDISC_REF_EXE, [sc for _, sc, _ in entries])
    for (name, _, out), g in zip(entries, got):
        assert g == out, name
    extra = S.free_scripts(EXTRA_SEED, EXTRA_COUNT)
    assert len(extra) >= 400
    R.reset_counters()
    got = S.run_qdisc_ref(QDISC_REF_EXE, [e["script"] for e in extra])
    for e, g in zip(extra, got):
        assert R.replay_script(e["script"]) == g, (e["seed"], e["qdisc"], e["sockets"], e["tie"], e["unique"])
    selects = sum(g.count("\n") for g in got)
    print("qdisc_ref: %d fixture scripts reproduced; %d further scripts, %d selects agree; reached %s"
          % (len(entries), len(extra), selects, {k: R.COUNTERS[k] for k in QDISC_BRANCHES[0] + QDISC_BRANCHES[1]}))
    assert selects == sum(e["script"].count("s\n") for e in extra)
    # every (sockets, tie, priority mode) five times per qdisc: each special case is met many times over
    assert all(R.COUNTERS[k] >= 100 for k in QDISC_BRANCHES[0] + QDISC_BRANCHES[1][-1:])


def test_qdisc_fixture_replays_through_the_restatement(qref):
    entries = fixture_entries(qref)
    assert len(entries) == 2 * FREE_COUNT + 26 + 7
    for name, script, out in entries:
        assert R.replay_script(script) == out, name


QDISC_BRANCHES = {0: ("control_into_queued_socket", "priority0_tie", "right_child_taken", "socket_pushed_back",
                      "select_65_queued", "select_129_queued"),
                  1: ("control_into_queued_socket", "socket_pushed_back", "select_65_queued", "select_129_queued",
                      "round_robin_rotation")}


@pytest.mark.parametrize("qdisc", [R.QDISC_FIFO, R.QDISC_ROUND_ROBIN], ids=["fifo", "rr"])
def test_qdisc_fixture_reaches_the_special_cases(qref, qdisc):
    """Free scripts and time-domain scenarios (not the KATs), per qdisc, by outbound_ref.py's counters."""
    R.reset_counters()
    for e in qref["free"]:
        if e["qdisc"] == qdisc:
            R.replay_script(e["script"])
    for scn in qref["scenarios"]:
        for e in scn["hosts"]:
            if int(e["script"].split()[0]) == qdisc:
                R.replay_script(e["script"])
    assert all(R.COUNTERS[k] > 0 for k in QDISC_BRANCHES[qdisc]), R.COUNTERS
    used = {(e["sockets"], e["tie"], e["unique"]) for e in qref["free"] if e["qdisc"] == qdisc}
    assert {u[0] for u in used} == set(S.FREE_SOCKETS) and {u[1] for u in used} == set(S.FREE_TIES)
    assert {u[2] for u in used} == {True, False}


def test_qdisc_scenarios_leave_every_packet(qref):
    for x, scn in zip(qref["scenarios"], S.qdisc_scenarios()):
        traced, outs = S.trace_ref(scn)
        left = S.concat_by_host(outs, len(scn[1]))
        for h, e in enumerate(x["hosts"]):
            offered = [o[5] for _, per_host in scn[6] for o in per_host[h]]
            assert sorted(g for _, _, g in left[h]) == sorted(offered) and offered, (scn[0], h)
            assert [g for _, _, g in left[h]] == tags_of(e["output"]), (scn[0], h)
        assert outs[-1][4]["num_queued"] == 0 and outs[-1][4]["min_next_wake_ns"] == R.U64, scn[0]


@pytest.mark.parametrize("scn", S.qdisc_scenarios(), ids=lambda s: s[0])
def test_header_leaves_in_the_reference_programs_order(rule_check, tmp_path, qref, scn):
    """The header's leaving packets per host (sent and local), concatenated over the steps, are the
    packets the reference program selected, in its order.  (That every line equals outbound_ref.py's:
    test_header_matches_reference_on_scenarios.)"""
    got = run_check(rule_check, scenario_text(scn), tmp_path)
    hosts = next(x["hosts"] for x in qref["scenarios"] if x["name"] == scn[0])
    left = {h: [] for h in range(len(hosts))}
    for ln in got:
        if ln.startswith("L "):
            _, h, status, _, tag = ln.split()
            assert status in ("1", "2")
            left[int(h)].append(int(tag))
    for h, e in enumerate(hosts):
        assert left[h] == tags_of(e["output"]), (scn[0], h)


class StoredKeyHeap(R.SocketHeap):
    """Wrong model 1: the key is stored when the socket is pushed, and the smallest stored key leaves
    (the oldest of equal ones)."""

    def __init__(self):
        super().__init__()
        self.pushes = 0

    def find(self, s):
        return any(x[2] is s for x in self.heap)

    def push(self, s):
        self.pushes += 1
        heapq.heappush(self.heap, (s.peek_priority(), self.pushes, s))

    def pop(self):
        return heapq.heappop(self.heap)[2]


class TieBySlotHeap(R.SocketHeap):
    """Wrong model 2: the reference's heap with a strict order, equal keys broken by the lower slot."""

    def _smaller(self, i, j):
        a, b = self.heap[i], self.heap[j]
        return (a.peek_priority(), a.slot) < (b.peek_priority(), b.slot)


def model_host(heap_cls, resift=False):
    class ModelHost(R.Host):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            if self.qdisc == R.QDISC_FIFO:
                self.q = heap_cls()

        def offer(self, t, slot, pkt):
            """Wrong model 3 (resift): a queued socket whose key changes is sifted down, then up."""
            s = self.sockets[slot]
            before = s.peek_priority() if resift and s.has_data() else None
            super().offer(t, slot, pkt)
            if before is not None and s.peek_priority() != before:
                self.q._down(self.q.heap.index(s))
                self.q._up(self.q.heap.index(s))
    return ModelHost


@pytest.mark.parametrize("model", [model_host(StoredKeyHeap), model_host(TieBySlotHeap), model_host(R.SocketHeap, resift=True)],
                         ids=["stored_keys_global_minimum", "tie_by_lower_slot", "resift_on_key_change"])
def test_qdisc_fixture_catches_a_wrong_heap(qref, model):
    entries = [e for e in fixture_entries(qref) if e[1].startswith("0 ")]
    wrong = [name for name, script, out in entries if R.replay_script(script, model) != out]
    assert wrong, "the fixture does not tell this model from the reference"
    # and the harness itself is sound: the plain classes through the same path agree everywhere
    assert all(R.replay_script(script, model_host(R.SocketHeap)) == out for _, script, out in entries)
