"""CPU: the device-resident event queues' C ABI (include/shadow_routing.h) -- symbols, the ctypes
layout of srg_queue_result against the compiler, null arguments refused before any device work,
srg_next_window (controller.rs:88-112) -- and tests/cpp/evq_merge_check.cpp, which replays the
merge kernels' partition + per-tile sequential merge on the host from shadow_amd/csrc/evq_merge.h
against std::merge.  The GPU side: tests/test_event_queues_gpu.py."""
import ctypes
import os
import shutil
import subprocess

import pytest

from shadow_amd import _native as N
from shadow_amd import events as ev
from shadow_amd.graph import NetGraphError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = 2**64 - 1

NEW = ("srg_event_queues_create", "srg_event_queues_destroy", "srg_event_queues_merge_tile",
       "srg_event_queues_push_device", "srg_event_queues_pop_device", "srg_next_window")


def test_new_symbols_exported():
    L = N.lib()
    for name in NEW:
        assert name in N.EXPORTS, name
        assert hasattr(L, name), name
    assert N.SRG_ERR_TIME_BACKWARD == 12
    assert issubclass(ev.TimeBackwardError, NetGraphError)
    tile = L.srg_event_queues_merge_tile()
    assert tile >= 64 and tile % 64 == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_queue_result_layout_matches_the_compiler(tmp_path):
    assert ctypes.sizeof(N.QueueResult) == 32
    fs = ["num_moved", "num_queued", "min_next_event_ns", "ms_total"]
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "shadow_routing.h"', "int main() {",
             'std::printf("%zu", sizeof(srg_queue_result));']
    lines += [f'std::printf(" %zu", offsetof(srg_queue_result, {f}));' for f in fs]
    lines.append('std::printf(" %d\\n", SRG_ERR_TIME_BACKWARD); return 0; }')
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert [int(x) for x in out] == ([ctypes.sizeof(N.QueueResult)] + [getattr(N.QueueResult, f).offset for f in fs]
                                     + [N.SRG_ERR_TIME_BACKWARD])


def test_null_arguments_are_refused_without_a_gpu():
    """The pointer checks come before any device work: no context, no queues, no call."""
    L = N.lib()
    err = ctypes.create_string_buffer(256)
    h = ctypes.c_void_p()
    assert L.srg_event_queues_create(None, 4, 0, ctypes.byref(h), err, len(err)) == N.SRG_ERR_ARG
    assert b"null" in err.value and not h.value
    assert L.srg_event_queues_create(None, 4, 0, None, err, len(err)) == N.SRG_ERR_ARG
    res = N.QueueResult()
    rc = L.srg_event_queues_push_device(None, None, None, None, 0, None, None, ctypes.byref(res), err, len(err))
    assert rc == N.SRG_ERR_ARG and b"null" in err.value
    rc = L.srg_event_queues_pop_device(None, 5, 0, None, None, None, None, None, None, ctypes.byref(res), err, len(err))
    assert rc == N.SRG_ERR_ARG and b"null" in err.value
    L.srg_event_queues_destroy(None)  # a no-op, must not crash


def test_next_window():
    # the plain step
    assert ev.next_window(1000, 50, 10**9) == (1000, 1050)
    # saturation at UINT64_MAX (checked_add ... unwrap_or(MAX)), then the clamp has nothing to cut
    assert ev.next_window(U64_MAX - 10, 50, U64_MAX) == (U64_MAX - 10, U64_MAX)
    assert ev.next_window(U64_MAX - 50, 50, U64_MAX) == (U64_MAX - 50, U64_MAX)
    # the clamp to end_time
    assert ev.next_window(1000, 50, 1020) == (1000, 1020)
    # start == end: over; so is an empty queue (min_next = UINT64_MAX) and a start past the end
    assert ev.next_window(1020, 50, 1020) is None
    assert ev.next_window(U64_MAX, 50, U64_MAX) is None
    assert ev.next_window(2000, 50, 1020) is None
    # runahead 0: the reference's assert_ne!
    with pytest.raises(NetGraphError) as e:
        ev.next_window(1000, 0, 10**9)
    assert e.value.code == N.SRG_ERR_ARG
    ws, we = ctypes.c_uint64(7), ctypes.c_uint64(8)
    assert N.lib().srg_next_window(1000, 0, 10**9, ctypes.byref(ws), ctypes.byref(we)) == -N.SRG_ERR_ARG
    assert N.lib().srg_next_window(1000, 5, 10**9, None, None) == -N.SRG_ERR_ARG
    # no window: the outputs are left alone
    assert N.lib().srg_next_window(1020, 50, 1020, ctypes.byref(ws), ctypes.byref(we)) == 0
    assert (ws.value, we.value) == (7, 8)
    assert N.lib().srg_next_window(1000, 50, 10**9, ctypes.byref(ws), ctypes.byref(we)) == 1
    assert (ws.value, we.value) == (1000, 1050)


def _sanitizers_link(tmp_path):
    """A trial compile: are the address / undefined sanitizer runtimes present for g++?"""
    src = tmp_path / "trial.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", str(tmp_path / "trial"), str(src)],
                       capture_output=True)
    return r.returncode == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_merge_path_against_std_merge(tmp_path):
    """A stand-alone program (its own main), sanitized where the runtimes are installed."""
    exe = tmp_path / "evq_merge_check"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if _sanitizers_link(tmp_path) else []
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san +
                   ["-o", str(exe), os.path.join(ROOT, "tests", "cpp", "evq_merge_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"
