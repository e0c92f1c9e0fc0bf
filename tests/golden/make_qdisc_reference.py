"""Writes tests/golden/qdisc_reference.json: offer / select scripts for a host's socket qdisc, each
with what oracle/_ref/qdisc_ref printed for it.  That program is the reference's own heap, comparator
and round-robin queue, compiled from a reference checkout (oracle/Makefile, oracle/ref_qdisc/); it
must have been built (python __graft_entry__.py, or oracle.build_qdisc_ref()).  The scripts:
  free       seeded interleavings with no time axis (outbound_scenarios.free_scripts)
  scenarios  per host, the operations outbound_ref.py performs on the time-domain scenarios
             outbound_scenarios.qdisc_scenarios() (its trace hook)
  kats       the same for the hand-derived KATs of outbound_kats.json
Nothing here computes an expected output: all of them are the program's.  Where outbound_ref.py's own
trace differs from them the script stops with the first difference.

    python tests/golden/make_qdisc_reference.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle  # noqa: E402
import outbound_scenarios as S  # noqa: E402

FREE_SEED, FREE_COUNT = 1000, 10  # per qdisc


def main():
    exe = oracle.build_qdisc_ref()
    if exe is None:
        sys.exit("oracle/_ref/qdisc_ref is not built and no reference checkout was found")
    free = S.free_scripts(FREE_SEED, FREE_COUNT)
    scenarios = []
    for scn in S.qdisc_scenarios():
        traced, _ = S.trace_ref(scn)
        scenarios.append(dict(name=scn[0], hosts=[dict(script=sc, restated=out) for sc, out in traced]))
    kats = []
    for k in S.load_kats():
        sc, out = S.kat_script(k)
        kats.append(dict(name=k["name"], script=sc, restated=out))
    entries = free + [h for s in scenarios for h in s["hosts"]] + kats
    for e, out in zip(entries, S.run_qdisc_ref(exe, [e["script"] for e in entries])):
        restated = e.pop("restated", None)
        if restated is not None and restated != out:
            sys.exit("outbound_ref.py and the reference program differ on:\n" + e["script"])
        e["output"] = out
    doc = dict(
        comment="Offer / select scripts for one host's socket qdisc and the output of the reference's own queue code for "
                "each (oracle/_ref/qdisc_ref: utility/priority_queue.c and host/network/network_queuing_disciplines.c "
                "compiled from a reference checkout, driven by oracle/ref_qdisc/driver.c). Script: '<qdisc 0 fifo | 1 "
                "round robin> <sockets>', then 'o <slot> <priority> <tag>' (the packet enters the socket, then wantsSend) "
                "and 's' (one selection step). Output: '<slot> <tag>' per 's', '-' on an empty qdisc. free: seeded "
                "interleavings; scenarios: per host, the operations of the time-domain scenarios of "
                "tests/outbound_scenarios.py; kats: those of tests/golden/outbound_kats.json. Written by "
                "tests/golden/make_qdisc_reference.py.",
        free=free, scenarios=scenarios, kats=kats)
    path = os.path.join(HERE, "qdisc_reference.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d bytes, %d scripts, %d selects" % (path, os.path.getsize(path), len(entries),
                                                    sum(e["script"].count("s\n") for e in entries)))


if __name__ == "__main__":
    main()
