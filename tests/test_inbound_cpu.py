"""CPU side of the hosts' inbound path (CoDel router queue + token-bucket relay):
1. tests/inbound_ref.py, the plain-Python restatement of the reference, passes every golden KAT
   (tests/golden/inbound_kats.json: the reference's own unit tests as operation lists);
2. shadow_amd/csrc/inbound_rule.h, the header the kernels run, replays the same KATs and the shared
   scenarios (inbound_scenarios.py) through tests/cpp/inbound_rule_check.cpp (g++, -Werror,
   -ffp-contract=off, ASan + UBSan) and agrees with inbound_ref.py line by line;
3. the scenarios reach every branch counter of inbound_ref.py;
4. the new ctypes structs have the C sizes.
The GPU side: tests/test_inbound_gpu.py."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

import inbound_ref as R
import inbound_scenarios as S

HERE = os.path.dirname(os.path.abspath(__file__))


def load_kats():
    with open(os.path.join(HERE, "golden", "inbound_kats.json")) as f:
        return json.load(f)


def check_kat(test, records):
    for i, (step, rec) in enumerate(zip(test["steps"], records)):
        for k, v in step["expect"].items():
            assert rec[k] == v, (test["name"], i, step["op"], k, rec[k], v)


def test_reference_restatement_passes_kats():
    kats = load_kats()
    assert len(kats["tests"]) == 9
    for t in kats["tests"]:
        check_kat(t, R.run_kat([s["op"] for s in t["steps"]], kats["packet_size"]))


@pytest.fixture(scope="module")
def rule_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("inbound") / "inbound_rule_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(HERE, "cpp", "inbound_rule_check.cpp")], check=True)
    return str(exe)


def run_check(exe, mode, text, tmp_path):
    p = tmp_path / (mode + ".txt")
    p.write_text(text)
    r = subprocess.run([exe, mode, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_header_passes_kats(rule_check, tmp_path):
    kats = load_kats()
    for t in kats["tests"]:
        lines = []
        for s in t["steps"]:
            op = list(s["op"])
            code = R.KAT_OPS.index(op[0])
            args = op[1:]
            if op[0] == "cq_push":
                args = args + [kats["packet_size"]]
            lines.append(" ".join(str(x) for x in [code] + args + [0] * (4 - len(args))))
        got = run_check(rule_check, "kat", "\n".join(lines) + "\n", tmp_path)
        ref = R.run_kat([s["op"] for s in t["steps"]], kats["packet_size"])
        assert got == R.kat_lines(ref), t["name"]
        check_kat(t, [dict(zip(R.KAT_FIELDS, (int(x) for x in g.split()))) for g in got])


def scenario_text(scn):
    _, bw, sim_start, boot, steps = scn
    out = ["%d %d %d" % (len(bw), sim_start, boot), " ".join(str(b) for b in bw)]
    for until, per_host in steps:
        out.append("step %d %d" % (until, sum(len(a) for a in per_host)))
        for h, a in enumerate(per_host):
            out += ["%d %d %d %d" % (h, t, s, g) for t, s, g in a]
    return "\n".join(out) + "\n"


STATE_KEYS = ("balance", "last_refill_ns", "mode", "has_interval_end", "interval_end_ns", "has_drop_next", "drop_next_ns",
              "current_drop_count", "previous_drop_count", "bytes_stored", "queued", "pending", "wake_ns", "has_cached",
              "cached_tag")


def ref_lines(scn):
    _, bw, sim_start, _, _ = scn
    outs, states = S.run_ref(scn)
    lines = []
    for (st, tm, tg, oo, res), hs in zip(outs, states):
        for h in range(len(bw)):
            lines += ["L %d %d %d %d" % (h, st[j], tm[j], tg[j]) for j in range(oo[h], oo[h + 1])]
        lines.append("R %d %d %d %d" % (res["num_forwarded"], res["num_dropped"], res["num_queued"],
                                        res["min_next_wake_ns"]))
        for h, s in enumerate(hs):
            s = dict(s)
            if s["last_refill_ns"] is None:  # an unlimited host has no bucket: the header keeps sim_start
                s["last_refill_ns"] = sim_start
            lines.append("S %d " % h + " ".join(str(s[k]) for k in STATE_KEYS))
    return lines


@pytest.mark.parametrize("scn", S.all_scenarios(), ids=lambda s: s[0])
def test_header_matches_reference_on_scenarios(rule_check, tmp_path, scn):
    got = run_check(rule_check, "scenario", scenario_text(scn), tmp_path)
    ref = ref_lines(scn)
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (scn[0], i)


def test_header_errors_leave_the_state(rule_check, tmp_path):
    S0 = S.SIM_START
    text = ("1 %d %d\n1000000\n" % (S0, S0) +
            "step %d 2\n0 %d 1500 1\n0 %d 1500 2\n" % (S0 + 5 * S.MS, S0 + S.MS, S0 + 2 * S.MS) +
            "step %d 1\n0 %d 40 3\n" % (S0 + 9 * S.MS, S0 + S.MS) +            # earlier than the last arrival
            "step %d 1\n0 %d 40 4\n" % (S0 + 9 * S.MS, S0 + 9 * S.MS) +        # not below until
            "step %d 1\n0 %d 40 5\n" % (S0 + 9 * S.MS, S0 - 1) +               # below the simulation start
            "step %d 1\n0 %d 1626 6\n" % (S0 + 9 * S.MS, S0 + 6 * S.MS))       # above the bucket's capacity
    got = run_check(rule_check, "scenario", text, tmp_path)
    states = [g for g in got if g.startswith("S ")]
    errors = [g for g in got if g.startswith("E ")]
    assert errors == ["E 12", "E 1", "E 1", "E 1"]
    assert len(states) == 5 and len(set(states)) == 1


def test_scenarios_reach_every_branch():
    for k in R.COUNTERS:
        R.COUNTERS[k] = 0
    for scn in S.all_scenarios():
        S.run_ref(scn)
    assert all(R.COUNTERS[k] > 0 for k in R.BRANCHES), R.COUNTERS


def test_overload_windows_agree():
    """One step, 50 ms windows and 1 ms windows leave the same packets at the same times."""
    a, b, c = (S.concat_by_host(S.run_ref(s)[0], 1) for s in (S.overload_one_step(), S.overload(50 * S.MS),
                                                              S.overload(1 * S.MS)))
    assert a == b == c and len(a[0]) == 600


def test_struct_sizes():
    from shadow_amd import _native as N
    assert ctypes.sizeof(N.InboundResult) == 4 * 8 + 8
    assert ctypes.sizeof(N.InboundHostState) == 10 * 8 + 8
    assert N.InboundHostState.mode.offset == 80 and N.InboundHostState.has_cached.offset == 84
