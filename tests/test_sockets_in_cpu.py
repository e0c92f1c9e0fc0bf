"""CPU side of interface receive (socket lookup, UDP receive buffers, tracker input counters):
1. tests/sockets_in_ref.py, the plain-Python restatement of the reference, passes every hand-worked
   KAT (tests/golden/sockets_in_kats.json);
2. shadow_amd/csrc/sockets_in_rule.h, the header the kernels run, replays the same KATs and the shared
   scenarios (sockets_in_scenarios.py) through tests/cpp/sockets_in_rule_check.cpp (g++, -Werror,
   -ffp-contract=off, ASan + UBSan) and agrees with sockets_in_ref.py line by line;
3. the scenarios reach every branch counter of sockets_in_ref.py;
4. the restatement rolls back on every error;
5. the new ctypes structs have the C sizes.
The GPU side: tests/test_sockets_in_gpu.py."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

import sockets_in_ref as R
import sockets_in_scenarios as S

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTER_KEYS = R.COUNTER_KEYS


def load_kats():
    with open(os.path.join(HERE, "golden", "sockets_in_kats.json")) as f:
        return json.load(f)["tests"]


def kat_scenario(t):
    def op(o):
        if o[0] == "step":
            return tuple(o)
        if o[0] == "reset":
            return ("reset", o[1])
        return (o[0], [tuple(e) for e in o[1]])
    return dict(name=t["name"], sockets_per_host=t["sockets_per_host"], packets=[list(c) for c in zip(*t["packets"])],
                ops=[op(s["op"]) for s in t["ops"]])


def check_kat(t, recs):
    assert len(recs) == len(t["ops"])
    for i, (s, rec) in enumerate(zip(t["ops"], recs)):
        exp, where = s["expect"], (t["name"], i)
        if "error" in exp:
            assert rec[0] == "err" and rec[1] == exp["error"], where
        else:
            assert rec[0] == "ok", where
        if "status" in exp:
            assert list(rec[1]) == exp["status"] and list(rec[2]) == exp["slot"], where
        if "reads" in exp:
            assert [list(r) for r in zip(rec[3], rec[4], rec[5], rec[6])] == exp["reads"], where
        if "counters_read" in exp:
            assert [rec[1][k] for k in COUNTER_KEYS] == exp["counters_read"], where
        socks, counters = rec[-1]
        for k, v in exp.get("sockets", {}).items():
            h, slot = (int(x) for x in k.split(","))
            assert [socks[h][slot]["len_bytes"], socks[h][slot]["num_messages"]] == v, (where, k)
        for h, v in exp.get("counters", {}).items():
            assert [counters[int(h)][k] for k in COUNTER_KEYS] == v, (where, h)


def test_restatement_passes_kats():
    kats = load_kats()
    assert len(kats) == 4
    for t in kats:
        check_kat(t, S.run_ref(kat_scenario(t))[1])


@pytest.fixture(scope="module")
def rule_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("sockets_in") / "sockets_in_rule_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(HERE, "cpp", "sockets_in_rule_check.cpp")], check=True)
    return str(exe)


def scenario_text(scn):
    pk = scn["packets"]
    out = [str(len(scn["sockets_per_host"])), " ".join(str(x) for x in scn["sockets_per_host"]),
           str(-1 if pk is None else len(pk[0]))]
    if pk is not None:
        out += [" ".join(str(x) for x in row) for row in zip(*pk)]
    for op in scn["ops"]:
        if op[0] == "step":
            _, status, time, tag, off, ds, rt, rs, rf, roff = op
            out.append("step %d %d %d %d" % (len(time), status is not None, ds, len(rt)))
            out += ["%d %d %d" % (0 if status is None else status[i], time[i], tag[i]) for i in range(len(time))]
            out.append(" ".join(str(x) for x in off))
            out += ["%d %d %d" % (rt[j], rs[j], rf[j]) for j in range(len(rt))]
            out.append(" ".join(str(x) for x in roff))
        elif op[0] == "reset":
            out.append("reset %d" % op[1])
        else:
            out.append("%s %d" % (op[0], len(op[1])))
            out += [" ".join(str(x) for x in e) for e in op[1]]
    return "\n".join(out) + "\n"


def ref_lines(scn, recs):
    lines = []
    for op, rec in zip(scn["ops"], recs):
        if rec[0] == "err":
            lines.append("E %d" % rec[1])
        elif op[0] == "step":
            st, sl, rs, rg, rt, rp, res = rec[1:8]
            lines += ["D %d %d %d" % (i, st[i], sl[i]) for i in range(len(st))]
            lines += ["R %d %d %d %d %d" % (j, rs[j], rg[j], rt[j], rp[j]) for j in range(len(rs))]
            lines.append("T " + " ".join(str(res[k]) for k in R.RESULT_KEYS))
        elif op[0] == "reset":
            lines.append("C %d " % op[1] + " ".join(str(rec[1][k]) for k in COUNTER_KEYS))
        socks, counters = rec[-1]
        for h, hs in enumerate(socks):
            lines += ["S %d %d %d %d %d %d %d %d %d" % (h, i, s["len_bytes"], s["num_messages"], s["soft_limit_bytes"],
                                                       s["peer_ip"], s["peer_port"], s["kind"], s["has_peer"])
                      for i, s in enumerate(hs)]
            lines.append("H %d " % h + " ".join(str(counters[h][k]) for k in COUNTER_KEYS))
    return lines


def header_agrees(exe, scn, tmp_path):
    p = tmp_path / "scenario.txt"
    p.write_text(scenario_text(scn))
    r = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    _, recs = S.run_ref(scn)
    ref = ref_lines(scn, recs)
    assert len(got) == len(ref), scn["name"]
    for i, (g, e) in enumerate(zip(got, ref)):
        assert g == e, (scn["name"], i)
    return recs


def test_header_passes_kats(rule_check, tmp_path):
    for t in load_kats():
        check_kat(t, header_agrees(rule_check, kat_scenario(t), tmp_path))


@pytest.mark.parametrize("scn", S.all_scenarios(), ids=lambda s: s["name"])
def test_header_matches_restatement_on_scenarios(rule_check, tmp_path, scn):
    header_agrees(rule_check, scn, tmp_path)


def test_scenarios_reach_every_branch():
    for k in R.COUNTERS:
        R.COUNTERS[k] = 0
    for scn in S.all_scenarios():
        S.run_ref(scn)
    assert all(R.COUNTERS[k] > 0 for k in R.BRANCHES), {k: v for k, v in R.COUNTERS.items() if v == 0}


def test_restatement_rolls_back_on_every_error():
    """Each refused call of the errors scenario (and the step without a packet table) leaves the
    snapshot exactly as the previous operation left it."""
    seen = set()
    for scn in (S.errors(), S.no_table()):
        ref, recs = S.run_ref(scn)
        prev = S.snapshot(R.SocketsInRef(scn["sockets_per_host"]))
        for op, rec in zip(scn["ops"], recs):
            if rec[0] == "err":
                assert rec[-1] == prev, op[0]
                seen.add((op[0], rec[1]))
            prev = rec[-1]
    assert seen == {("step", R.ERR_ARG), ("step", R.ERR_TIME_BACKWARD), ("associate", R.ERR_ARG), ("configure", R.ERR_ARG)}
    # the associations too: a refused batch adds none of its keys
    ref = R.SocketsInRef([2])
    ref.associate([(0, 17, 1, 0, 0, 0)])
    with pytest.raises(R.RefError):
        ref.associate([(0, 17, 2, 0, 0, 0), (0, 17, 1, 0, 0, 1)])
    assert ref.assoc == {(0, 17, 1, 0, 0): 0}


def test_struct_sizes():
    from shadow_amd import _native as N
    assert ctypes.sizeof(N.SocketsInResult) == 9 * 8 + 8
    assert ctypes.sizeof(N.SocketsInSocketState) == 3 * 8 + 8
    assert N.SocketsInSocketState.peer_port.offset == 28 and N.SocketsInSocketState.has_peer.offset == 31
    assert ctypes.sizeof(N.SocketsInHostCounters) == 5 * 8
