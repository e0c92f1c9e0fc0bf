"""CPU: the send batch's C ABI (include/shadow_routing.h) -- the library exports the new entry points
and the ctypes mirrors of srg_path_table_dev, srg_send_batch and srg_send_result have the C layout."""
import ctypes
import os
import shutil
import subprocess

import pytest

from shadow_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("srg_send_packets_device", "srg_routing_info_key_tables", "srg_routing_info_add_packet_counts")


def test_new_symbols_exported():
    L = N.lib()
    for name in NEW:
        assert name in N.EXPORTS, name
        assert hasattr(L, name), name


def test_send_struct_layouts():
    # srg_path_table_dev: u32 n, u32 reserved, three pointers, u64 unit, one pointer
    assert ctypes.sizeof(N.PathTableDev) == 4 + 4 + 3 * 8 + 8 + 8
    assert N.PathTableDev.latency_ns.offset == 8 and N.PathTableDev.unit_ns.offset == 32
    assert N.PathTableDev.packet_loss.offset == 40
    # srg_send_batch: srg_event_batch (u64, six pointers, u32, u32, u64 = 72 B), two pointers, u64
    assert ctypes.sizeof(N.EventBatch) == 72
    assert ctypes.sizeof(N.SendBatch) == 72 + 8 + 8 + 8
    assert N.SendBatch.chance.offset == 72 and N.SendBatch.bootstrap_end_ns.offset == 88
    # srg_send_result: srg_event_result (u64, u64, u32, u32, f64 = 32 B), u64, u64
    assert ctypes.sizeof(N.EventResult) == 32
    assert ctypes.sizeof(N.SendResult) == 32 + 8 + 8
    assert N.SendResult.num_sent.offset == 32 and N.SendResult.num_dropped.offset == 40


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_send_struct_layouts_match_the_compiler(tmp_path):
    """sizeof / offsetof as the C compiler lays the header's structs out, against ctypes."""
    fields = {"srg_path_table_dev": (N.PathTableDev, ["n", "latency_ns", "latency_key", "diag_ns", "unit_ns",
                                                      "packet_loss"]),
              "srg_send_batch": (N.SendBatch, ["ev", "chance", "payload_size", "bootstrap_end_ns"]),
              "srg_send_result": (N.SendResult, ["ev", "num_sent", "num_dropped"])}
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "shadow_routing.h"', "int main() {"]
    for name, (_, fs) in fields.items():
        lines.append(f'std::printf("%zu", sizeof({name}));')
        lines += [f'std::printf(" %zu", offsetof({name}, {f}));' for f in fs]
        lines.append('std::printf("\\n");')
    lines.append("return 0; }")
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert len(out) == len(fields)
    for row, (name, (cls, fs)) in zip(out, fields.items()):
        assert [int(x) for x in row.split()] == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fs], name


def test_null_arguments_are_refused_without_a_gpu():
    """The pointer checks come before any device work: no context, no call."""
    err = ctypes.create_string_buffer(256)
    rc = N.lib().srg_send_packets_device(None, None, None, None, None, None, None, None, None, None, err, len(err))
    assert rc == N.SRG_ERR_ARG and b"null" in err.value
    assert N.lib().srg_routing_info_key_tables(None, None, None, None, None, None) == 0
    N.lib().srg_routing_info_add_packet_counts(None, None)  # a no-op, must not crash
