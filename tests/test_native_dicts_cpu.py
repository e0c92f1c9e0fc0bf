"""as_dict() of every result and state struct of shadow_amd/_native.py: the exact key list, in order,
and the type of every value, on a zero-initialised instance.  The lists are literals: what callers
(tests, tools, bench.py) have always seen, not something computed from _fields_."""
import ctypes

import pytest

from shadow_amd import _native as N

F = "ms_total"  # the one double of most structs

EXPECTED = {
    "EventResult": ["min_next_event_ns", "min_used_latency_ns", "key_bits", "radix_passes", "ms_total"],
    "SendResult": ["min_next_event_ns", "min_used_latency_ns", "key_bits", "radix_passes", "ms_total", "num_sent",
                   "num_dropped"],
    "QueueResult": ["num_moved", "num_queued", "min_next_event_ns", "ms_total"],
    "InboundResult": ["num_forwarded", "num_dropped", "num_queued", "min_next_wake_ns", "ms_total"],
    "InboundHostState": ["balance", "last_refill_ns", "interval_end_ns", "drop_next_ns", "current_drop_count",
                         "previous_drop_count", "bytes_stored", "queued", "wake_ns", "cached_tag", "mode",
                         "has_interval_end", "has_drop_next", "pending", "has_cached"],
    "OutboundResult": ["num_sent", "num_local", "num_queued", "min_next_wake_ns", "ms_total"],
    "OutboundHostState": ["balance", "last_refill_ns", "wake_ns", "cached_tag", "queued", "qdisc_len", "pending",
                          "has_cached"],
    "RoundReceiveResult": ["num_popped", "num_leaving", "num_forwarded", "num_dropped", "num_queued_inbound",
                           "num_queued_events", "min_next_event_ns", "min_inbound_wake_ns", "min_outbound_wake_ns",
                           "next_start_ns", "ms_total"],
    "RoundSendResult": ["num_leaving", "num_sent", "num_dropped", "num_local", "num_after_end", "num_no_host",
                        "num_queued_outbound", "num_queued_events", "min_used_latency_ns", "min_next_event_ns",
                        "min_inbound_wake_ns", "min_outbound_wake_ns", "next_start_ns", "ms_total"],
    "SocketsInResult": ["num_skipped", "num_no_socket", "num_external", "num_peer_mismatch", "num_full", "num_buffered",
                        "num_read", "num_would_block", "num_buffered_messages", "ms_total"],
    "SocketsInSocketState": ["len_bytes", "num_messages", "soft_limit_bytes", "peer_ip", "peer_port", "kind", "has_peer"],
    "SocketsInHostCounters": ["packets_control", "packets_data", "bytes_control_header", "bytes_data_header",
                              "bytes_data_payload"],
    "RouteResult": ["num_pairs", "total_hops", "bad_pair", "max_hops", "reserved", "ms_total"],
    "Stats": ["ms_total", "ms_h2d", "ms_build", "ms_fw", "ms_scan", "ms_loss", "ms_extract", "ms_d2h", "path_kind",
              "loss_rounds", "multi_pred_pairs", "relaxations", "essential_edges", "scan_kind", "table_keys",
              "prof_launches", "prof_kernel_ms", "prof_relaxations", "ms_exchange", "nranks", "rank", "local_sources",
              "ms_host_register", "d2h_overlapped_bytes", "min_latency_ns", "latency_unit_ns", "fw_overlap_pivots",
              "fw_overlap_kept", "d2h_key_rows", "reserved0", "ms_key_widen"],
}

# every other value is an int
FLOATS = {name: {F} for name in EXPECTED}
FLOATS["InboundHostState"] = FLOATS["OutboundHostState"] = set()
FLOATS["SocketsInSocketState"] = FLOATS["SocketsInHostCounters"] = set()
FLOATS["Stats"] = {"ms_total", "ms_h2d", "ms_build", "ms_fw", "ms_scan", "ms_loss", "ms_extract", "ms_d2h",
                   "prof_kernel_ms", "ms_exchange", "ms_host_register", "ms_key_widen"}


def test_every_struct_with_as_dict_is_listed():
    have = {name for name, c in vars(N).items()
            if isinstance(c, type) and issubclass(c, ctypes.Structure) and hasattr(c, "as_dict")}
    assert have == set(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_as_dict_keys_and_types(name):
    d = getattr(N, name)().as_dict()
    assert list(d) == EXPECTED[name]
    for k, v in d.items():
        assert type(v) is (float if k in FLOATS[name] else int), (k, type(v))
        assert v == 0
