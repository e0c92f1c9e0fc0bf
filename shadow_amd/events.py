"""Stretch row f4: one scheduling round's cross-host packet-event batch on the GPU.

Host-side mirror of the reference's per-packet path, batched (srg_order_packet_events_device,
include/shadow_routing.h):
  Worker::send_packet      src/main/core/worker.rs:391-424  latency lookup, deliver time raised
                                                            to the round end, runahead / next
                                                            event bookkeeping
  push_packet_to_host      worker.rs:644-654                one EventQueue per destination host
  EventQueue / Event order event_queue.rs:38-49, event.rs:84-155
  min next event           manager.rs:459-464
The latency table is the dense routing table (RoutingInfo's backing store), e.g. the
`latency_ns` matrix of a PathTable, kept in HBM.  torch tensors are only HBM containers here.

send_packets / send_packets_device (srg_send_packets_device) start higher up, at the drop decision
(worker.rs:374-390: chance >= 1.0f32 - packet_loss, payload > 0, not bootstrapping), take the
table in either form a RoutingInfo keeps (DevicePathTable), and count the sent packets per node
pair (increment_packet_count, worker.rs:395).  Only the RNG draw stays with the caller: `chance`.

EventQueues (srg_event_queues_*) keeps the per-host packet-event queues themselves in HBM across
rounds: push merges a round's ordered batch into the backlog, pop takes a window's events out in
the reference's order (event_queue.rs:10-55, host.rs:809-818), next_window is the controller's step
(controller.rs:88-112).

Round (srg_round_*) joins the stages on the device: receive = pop -> sizes by tag -> inbound step,
send = offers -> outbound step -> draw -> send -> push, with each host's Xoshiro256++ generator
(host.rs:233) and event-id counter (host.rs:690) in HBM, so `chance` no longer comes from the caller.
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from .graph import NetGraphError, _raise

FIELDS_U32 = ("src_node", "dst_node", "src_host", "dst_host")
FIELDS_U64 = ("send_time_ns", "src_event_id")


class EventOrderError(NetGraphError):
    """Two events with no relative order: the reference's PanickingOrd unwrap panic."""


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)


def _i64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)


def _u8(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev)


def _ptr(t):
    """A device tensor, a raw device pointer (int, e.g. a borrowed pointer of a Round result) or None."""
    return t.data_ptr() if isinstance(t, torch.Tensor) else (int(t) if t else None)


def _dev_t(a, up, dev):
    """a as it is when it is a device tensor or None; a host array or host tensor is uploaded by up (_i32, _i64, _u8)."""
    if a is None or (isinstance(a, torch.Tensor) and a.is_cuda):
        return a
    return up(a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a), dev)


class DeviceEventBatch:
    """An event batch resident in HBM (uint32/uint64 data held in int32/int64 tensors)."""

    def __init__(self, batch, num_hosts, round_end_ns, device="cuda:0"):
        dev = torch.device(device)
        self.n = len(batch["send_time_ns"])
        self.num_hosts = int(num_hosts)
        self.round_end_ns = int(round_end_ns)
        self.t = {k: _i32(batch[k], dev) for k in FIELDS_U32}
        self.t.update({k: _i64(batch[k], dev) for k in FIELDS_U64})

    def as_struct(self):
        p = {k: v.data_ptr() for k, v in self.t.items()}
        return N.EventBatch(self.n, p["src_node"], p["dst_node"], p["src_host"], p["dst_host"], p["send_time_ns"],
                            p["src_event_id"], self.num_hosts, 0, self.round_end_ns)


def order_packet_events_device(router, dbatch, table_t, out_deliver_t, out_order_t, out_host_off_t, stream=None):
    """table_t int64 [tn, tn]; outputs int64[n], int32[n], int64[num_hosts + 1] on the GPU."""
    assert table_t.dtype == torch.int64 and table_t.dim() == 2 and table_t.shape[0] == table_t.shape[1]
    assert out_deliver_t.numel() == dbatch.n and out_order_t.numel() == dbatch.n
    assert out_host_off_t.numel() == dbatch.num_hosts + 1
    res = N.EventResult()
    err = ctypes.create_string_buffer(1024)
    b = dbatch.as_struct()
    s = stream if stream is not None else torch.cuda.current_stream(table_t.device)
    rc = N.lib().srg_order_packet_events_device(
        router._h, ctypes.byref(b), table_t.data_ptr(), table_t.shape[0], out_deliver_t.data_ptr(),
        out_order_t.data_ptr(), out_host_off_t.data_ptr(), ctypes.c_void_p(s.cuda_stream), ctypes.byref(res), err,
        len(err))
    if rc == N.SRG_ERR_EVENT_ORDER:
        raise EventOrderError(rc, err.value.decode(errors="replace"))
    if rc != N.SRG_OK:
        _raise(rc, err.value.decode(errors="replace"))
    return res.as_dict()


def order_packet_events(router, batch, table, num_hosts, round_end_ns, device=None):
    """Host arrays in, host arrays out: (deliver u64[n], order u32[n], host_offsets u64[H+1], result)."""
    dev = torch.device(device or f"cuda:{router.device}")
    db = DeviceEventBatch(batch, num_hosts, round_end_ns, dev)
    tab = _i64(np.asarray(table), dev)
    n = db.n
    deliver = torch.empty(max(n, 1), dtype=torch.int64, device=dev)[:n]
    order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    off = torch.empty(db.num_hosts + 1, dtype=torch.int64, device=dev)
    res = order_packet_events_device(router, db, tab, deliver, order, off)
    torch.cuda.synchronize(dev)
    return (deliver.cpu().numpy().view(np.uint64), order.cpu().numpy().view(np.uint32),
            off.cpu().numpy().view(np.uint64), res)


class DeviceSendBatch(DeviceEventBatch):
    """A DeviceEventBatch plus what the drop decision reads: batch["chance"] f64 [n] (the host's
    draws, program order) and batch["payload_size"] u32 [n]; both may be absent when the table has
    no packet_loss."""

    def __init__(self, batch, num_hosts, round_end_ns, bootstrap_end_ns=0, device="cuda:0"):
        super().__init__(batch, num_hosts, round_end_ns, device)
        dev = torch.device(device)
        self.bootstrap_end_ns = int(bootstrap_end_ns)
        self.chance = self.payload = None
        if batch.get("chance") is not None:
            self.chance = torch.from_numpy(np.ascontiguousarray(batch["chance"], dtype=np.float64)).to(dev)
        if batch.get("payload_size") is not None:
            self.payload = _i32(batch["payload_size"], dev)

    def as_send_struct(self):
        return N.SendBatch(self.as_struct(), self.chance.data_ptr() if self.chance is not None else None,
                           self.payload.data_ptr() if self.payload is not None else None, self.bootstrap_end_ns)


class DevicePathTable:
    """A routing table resident in HBM, by node position, in either form (srg_path_table_dev):
    u64 latencies, or u32 keys + the diagonal's raw latencies + the unit; packet_loss optional."""

    def __init__(self, n, latency_ns=None, key=None, diag=None, unit=1, packet_loss=None):
        self.n, self.unit = int(n), int(unit)
        self.latency_ns, self.key, self.diag, self.packet_loss = latency_ns, key, diag, packet_loss

    @classmethod
    def from_arrays(cls, latency_ns=None, key=None, diag=None, unit=1, packet_loss=None, device="cuda:0"):
        dev = torch.device(device)
        first = latency_ns if latency_ns is not None else key
        if first is None:
            raise ValueError("latency_ns or key is required")
        return cls(np.asarray(first).shape[0],
                   _i64(np.asarray(latency_ns), dev) if latency_ns is not None else None,
                   _i32(np.asarray(key), dev) if key is not None else None,
                   _i64(np.asarray(diag), dev) if diag is not None else None, unit,
                   torch.from_numpy(np.ascontiguousarray(packet_loss, dtype=np.float32)).to(dev)
                   if packet_loss is not None else None)

    @classmethod
    def from_routing_info(cls, ri, device="cuda:0"):
        """Uploads the u32 keys when the RoutingInfo kept them (no u64 widening on the host), else u64."""
        kt = ri.key_tables()
        if kt is not None:
            key, diag, unit, loss = kt
            return cls.from_arrays(key=key, diag=diag, unit=unit, packet_loss=loss, device=device)
        lat, loss, _ = ri.tables()
        return cls.from_arrays(latency_ns=lat, packet_loss=loss, device=device)

    def as_struct(self):
        return N.PathTableDev(self.n, 0, _ptr(self.latency_ns), _ptr(self.key), _ptr(self.diag), self.unit,
                              _ptr(self.packet_loss))


def send_packets_device(router, dbatch, table, out_status_t, out_deliver_t, out_order_t, out_host_off_t, counts_t=None,
                        stream=None):
    """dbatch: DeviceSendBatch; table: DevicePathTable; outputs uint8[n], int64[n], int32[n] (the first
    num_sent entries are written), int64[num_hosts + 1]; counts_t: int64 [tn, tn] accumulated in place."""
    assert out_status_t.dtype == torch.uint8 and out_status_t.numel() == dbatch.n
    assert out_deliver_t.numel() == dbatch.n and out_order_t.numel() == dbatch.n
    assert out_host_off_t.numel() == dbatch.num_hosts + 1
    assert counts_t is None or (counts_t.dtype == torch.int64 and counts_t.numel() == table.n * table.n
                                and counts_t.is_contiguous())
    res = N.SendResult()
    err = ctypes.create_string_buffer(1024)
    b, t = dbatch.as_send_struct(), table.as_struct()
    s = stream if stream is not None else torch.cuda.current_stream(out_host_off_t.device)
    rc = N.lib().srg_send_packets_device(
        router._h, ctypes.byref(b), ctypes.byref(t), out_status_t.data_ptr(), out_deliver_t.data_ptr(),
        out_order_t.data_ptr(), out_host_off_t.data_ptr(), counts_t.data_ptr() if counts_t is not None else None,
        ctypes.c_void_p(s.cuda_stream), ctypes.byref(res), err, len(err))
    if rc == N.SRG_ERR_EVENT_ORDER:
        raise EventOrderError(rc, err.value.decode(errors="replace"))
    if rc != N.SRG_OK:
        _raise(rc, err.value.decode(errors="replace"))
    return res.as_dict()


def send_packets(router, batch, table, num_hosts, round_end_ns, bootstrap_end_ns=0, counts=None, device=None):
    """Host arrays in, host arrays out: (status u8[n], deliver u64[n], order u32[num_sent],
    host_offsets u64[H+1], result).  table: a DevicePathTable; counts: a persistent int64 [tn, tn]
    tensor on the device that accumulates the packet counts (None = not counted)."""
    dev = torch.device(device or f"cuda:{router.device}")
    db = DeviceSendBatch(batch, num_hosts, round_end_ns, bootstrap_end_ns, dev)
    n = db.n
    status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[:n]
    deliver = torch.empty(max(n, 1), dtype=torch.int64, device=dev)[:n]
    order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    off = torch.empty(db.num_hosts + 1, dtype=torch.int64, device=dev)
    res = send_packets_device(router, db, table, status, deliver, order, off, counts)
    torch.cuda.synchronize(dev)
    return (status.cpu().numpy(), deliver.cpu().numpy().view(np.uint64),
            order[:res["num_sent"]].cpu().numpy().view(np.uint32), off.cpu().numpy().view(np.uint64), res)


def synthetic_round(n, num_hosts, table_n, seed=7, t0=10**12, runahead=5_000_000, loss=None, zero_payload=0.1):
    """n events, send times uniform in one round window [t0, t0 + runahead),
    src/dst hosts uniform, per-source monotone event ids, hosts mapped to table rows.

    loss (a mean drop probability in [0, 0.5], default None = as before): the batch also gets what
    send_packets reads -- "chance" (f64 uniform in [0, 1), one draw per packet) and "payload_size"
    (u32, a `zero_payload` share of them 0: bare ACKs) -- and a third value is returned, the
    packet_loss table f32 [table_n, table_n], uniform in [0, 2 loss).  These come from a generator
    of their own, so the six base arrays are the same with and without."""
    rng = np.random.default_rng(seed)
    src_host = rng.integers(0, num_hosts, n, dtype=np.uint32)
    dst_host = rng.integers(0, num_hosts, n, dtype=np.uint32)
    host_node = rng.integers(0, table_n, num_hosts, dtype=np.uint32)
    send = (t0 + rng.integers(0, runahead, n, dtype=np.uint64)).astype(np.uint64)
    # per-source monotone counters (Host::get_new_event_id) in send order
    order = np.lexsort((send, src_host))
    eid = np.empty(n, dtype=np.uint64)
    starts = np.r_[0, np.flatnonzero(np.diff(src_host[order])) + 1]
    counts = np.diff(np.r_[starts, n])
    eid[order] = (np.arange(n) - np.repeat(starts, counts)).astype(np.uint64) + 1
    batch = dict(src_node=host_node[src_host], dst_node=host_node[dst_host], src_host=src_host, dst_host=dst_host,
                 send_time_ns=send, src_event_id=eid)
    if loss is None:
        return batch, t0 + runahead
    rng2 = np.random.default_rng([seed, 0x5E9D])
    batch["chance"] = rng2.random(n)
    batch["payload_size"] = np.where(rng2.random(n) < zero_payload, 0, rng2.integers(1, 1461, n)).astype(np.uint32)
    table = (rng2.random((table_n, table_n), dtype=np.float32) * np.float32(2.0 * loss)).astype(np.float32)
    return batch, t0 + runahead, table


class TimeBackwardError(NetGraphError):
    """A pushed event earlier than its host's last popped event: EventQueue::push's assert!
    (event_queue.rs:33)."""


def _raise_queue(rc, msg):
    if rc == N.SRG_ERR_EVENT_ORDER:
        raise EventOrderError(rc, msg)
    if rc == N.SRG_ERR_TIME_BACKWARD:
        raise TimeBackwardError(rc, msg)
    _raise(rc, msg)


def next_window(min_next_event_ns, runahead_ns, end_time_ns):
    """The controller's window step (controller.rs:88-112, srg_next_window): (start, end), or None
    when the simulation is over.  runahead 0 is the reference's assert_ne!: NetGraphError."""
    ws, we = ctypes.c_uint64(), ctypes.c_uint64()
    rc = N.lib().srg_next_window(int(min_next_event_ns), int(runahead_ns), int(end_time_ns), ctypes.byref(ws),
                                 ctypes.byref(we))
    if rc < 0:
        _raise(-rc, "srg_next_window: runahead must not be zero")
    return (int(ws.value), int(we.value)) if rc else None


class _Stage:
    """A resident object of the native library behind a handle: created by one srg_*_create, destroyed
    once by cls._destroy (the name of its srg_*_destroy), called with the handle in front."""
    _destroy = None
    _h = None

    def _create(self, fn, router, *args):
        """fn(router handle, *args, &handle, err, len): sets router, dev and _h, or raises."""
        self.router = router
        self.dev = torch.device(f"cuda:{router.device}")
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(1024)
        rc = fn(router._h, *args, ctypes.byref(h), err, len(err))
        if rc != N.SRG_OK:
            _raise(rc, err.value.decode(errors="replace"))
        self._h = h

    def close(self):
        if self._h:
            getattr(N.lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, fn, result_struct, *args, stream=None):
        """A raw *_device call fn(handle, *args, stream, &result, err, len) -> (rc, result struct,
        message); raises nothing."""
        res = result_struct()
        err = ctypes.create_string_buffer(1024)
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        rc = fn(self._h, *args, ctypes.c_void_p(s.cuda_stream), ctypes.byref(res), err, len(err))
        return rc, res, err.value.decode(errors="replace")


class EventQueues(_Stage):
    """The per-host packet-event queues, resident in HBM across rounds (srg_event_queues_*,
    event_queue.hip.h).  The round loop: pop(window_end) -> the hosts run -> send() at the barrier
    -> next_window(queues.min_next_event_ns, runahead, end_time).  Local events stay with the host."""

    _destroy = "srg_event_queues_destroy"

    def __init__(self, router, num_hosts, reserve=0):
        self.num_hosts = int(num_hosts)
        self._create(N.lib().srg_event_queues_create, router, self.num_hosts, int(reserve))
        self.num_queued = 0
        self.min_next_event_ns = 2**64 - 1

    def __len__(self):
        return self.num_queued

    def _moved(self, rc, res):
        if rc == N.SRG_OK:
            self.num_queued, self.min_next_event_ns = int(res.num_queued), int(res.min_next_event_ns)

    def push(self, dbatch, deliver_t, order_t, num_order, tags_t=None, stream=None):
        """dbatch: the DeviceEventBatch / DeviceSendBatch that order_packet_events_device /
        send_packets_device took; deliver_t, order_t: what it wrote; num_order: n / num_sent;
        tags_t: int64 [n] on the device (None: an event's tag is its index)."""
        b = dbatch.as_struct()
        rc, res, msg = self._call(N.lib().srg_event_queues_push_device, N.QueueResult, ctypes.byref(b),
                                  deliver_t.data_ptr(), order_t.data_ptr(), int(num_order), _ptr(tags_t), stream=stream)
        if rc != N.SRG_OK:
            _raise_queue(rc, msg)
        self._moved(rc, res)
        return res.as_dict()

    def pop_device(self, until_ns, capacity, out_time_t, out_src_t, out_id_t, out_tag_t, out_off_t, stream=None):
        """Raw call; returns (rc, result dict, message) and raises nothing: a short capacity is
        SRG_ERR_ARG with num_moved = the count needed."""
        rc, res, msg = self._call(N.lib().srg_event_queues_pop_device, N.QueueResult, int(until_ns), int(capacity),
                                  _ptr(out_time_t), _ptr(out_src_t), _ptr(out_id_t), _ptr(out_tag_t), _ptr(out_off_t),
                                  stream=stream)
        self._moved(rc, res)
        return rc, res.as_dict(), msg

    def pop(self, until_ns):
        """Pops every event with time < until_ns.  Returns host arrays (time u64, src_host u32,
        src_event_id u64, tag u64, host_offsets u64 [H + 1], result): grouped by host, each host's
        slice in pop order.  Sized with a capacity-0 call first."""
        dev = self.dev
        off = torch.empty(self.num_hosts + 1, dtype=torch.int64, device=dev)
        rc, res, msg = self.pop_device(until_ns, 0, None, None, None, None, off)
        n = 0
        if rc == N.SRG_ERR_ARG and res["num_moved"] > 0:
            n = int(res["num_moved"])
            t = torch.empty(n, dtype=torch.int64, device=dev)
            src = torch.empty(n, dtype=torch.int32, device=dev)
            eid = torch.empty(n, dtype=torch.int64, device=dev)
            tag = torch.empty(n, dtype=torch.int64, device=dev)
            rc, res, msg = self.pop_device(until_ns, n, t, src, eid, tag, off)
        if rc != N.SRG_OK:
            _raise_queue(rc, msg)
        if n == 0:
            z = np.zeros(0, np.uint64)
            return z, np.zeros(0, np.uint32), z.copy(), z.copy(), off.cpu().numpy().view(np.uint64), res
        return (t.cpu().numpy().view(np.uint64), src.cpu().numpy().view(np.uint32), eid.cpu().numpy().view(np.uint64),
                tag.cpu().numpy().view(np.uint64), off.cpu().numpy().view(np.uint64), res)

    def send(self, dbatch, table, counts=None, tags=None):
        """send_packets_device, then push: the round's sent events enter the queues, the dropped
        ones never do.  tags: int64 [n] tensor on the device, or None.  Returns (send result,
        queue result, status uint8 tensor)."""
        dev, n = self.dev, dbatch.n
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[:n]
        deliver = torch.empty(max(n, 1), dtype=torch.int64, device=dev)[:n]
        order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        off = torch.empty(dbatch.num_hosts + 1, dtype=torch.int64, device=dev)
        sres = send_packets_device(self.router, dbatch, table, status, deliver, order, off, counts)
        qres = self.push(dbatch, deliver, order, sres["num_sent"], tags)
        return sres, qres, status


class Inbound(_Stage):
    """The hosts' inbound path, resident in HBM across steps (srg_inbound_*, inbound.hip.h): per host
    the router's CoDel queue (codel_queue.rs:125-319) and the inbound relay with its token bucket
    (relay/mod.rs:111-288, token_bucket.rs:68-157).  step() takes what EventQueues.pop returned, plus
    each packet's total size; the caller folds min_next_wake_ns into the minimum it hands to
    next_window: a pending forward task is a local event of its host."""

    _destroy = "srg_inbound_destroy"

    def __init__(self, router, bw_down_bits, sim_start_ns, bootstrap_end_ns, reserve=0):
        bw = np.ascontiguousarray(bw_down_bits, dtype=np.uint64)
        self.num_hosts = int(bw.shape[0])
        self._create(N.lib().srg_inbound_create, router, self.num_hosts, bw.ctypes.data, int(sim_start_ns),
                     int(bootstrap_end_ns), int(reserve))
        self.num_queued = 0
        self.min_next_wake_ns = 2**64 - 1

    def step_device(self, until_ns, num_arrivals, time_t, size_t, tag_t, host_off_t, capacity, out_status_t, out_time_t,
                    out_tag_t, out_off_t, stream=None):
        """Raw call; returns (rc, result dict, message) and raises nothing: a short capacity is
        SRG_ERR_ARG with num_forwarded + num_dropped = the count needed.  time_t, tag_t, host_off_t
        int64 and size_t int32 tensors on the device, as EventQueues.pop_device wrote them;
        outputs uint8 / int64 / int64 [capacity] and int64 [num_hosts + 1]."""
        rc, res, msg = self._call(N.lib().srg_inbound_step_device, N.InboundResult, int(until_ns), int(num_arrivals),
                                  _ptr(time_t), _ptr(size_t), _ptr(tag_t), _ptr(host_off_t), int(capacity),
                                  _ptr(out_status_t), _ptr(out_time_t), _ptr(out_tag_t), _ptr(out_off_t), stream=stream)
        if rc == N.SRG_OK:
            self.num_queued, self.min_next_wake_ns = int(res.num_queued), int(res.min_next_wake_ns)
        return rc, res.as_dict(), msg

    def step(self, until_ns, time, size, tag, host_offsets):
        """Device tensors (or host arrays, uploaded) in; returns device tensors (status uint8, time
        int64, tag int64, host_offsets int64 [H + 1], result).  Sized by num_queued + arrivals,
        which always suffices."""
        dev = self.dev
        time_t, size_t, tag_t = _dev_t(time, _i64, dev), _dev_t(size, _i32, dev), _dev_t(tag, _i64, dev)
        off_t = _dev_t(host_offsets, _i64, dev)
        n = int(time_t.numel())
        cap = self.num_queued + n
        status = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        otime = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        otag = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        ooff = torch.empty(self.num_hosts + 1, dtype=torch.int64, device=dev)
        rc, res, msg = self.step_device(until_ns, n, time_t, size_t, tag_t, off_t, max(cap, 1), status, otime, otag, ooff)
        if rc != N.SRG_OK:
            _raise_queue(rc, msg)
        m = res["num_forwarded"] + res["num_dropped"]
        return status[:m], otime[:m], otag[:m], ooff, res

    def host_state(self, h):
        out = N.InboundHostState()
        rc = N.lib().srg_inbound_host_state(self._h, int(h), ctypes.byref(out))
        if rc != N.SRG_OK:
            _raise(rc, "srg_inbound_host_state: host out of range")
        return out.as_dict()


class Outbound(_Stage):
    """The hosts' outbound path, resident in HBM across steps (srg_outbound_*, outbound.hip.h): per
    host the sockets' control and data FIFOs, the interface's qdisc structure (the reference's socket
    heap restated literally, or the round-robin queue: network_interface.c:205-294,
    utility/priority_queue.c:87-175) and relay_inet_out with its token bucket (relay/mod.rs:111-288).
    step() takes the offers of a window (one per packet a socket hands to the interface, in each
    host's execution order) and returns what left: status 1 packets go to send_packets_device with
    the returned time as their send_time_ns.  The caller folds min_next_wake_ns into the minimum it
    hands to next_window: a pending forward task is a local event of its host."""

    _destroy = "srg_outbound_destroy"

    def __init__(self, router, bw_up_bits, sockets_per_host, qdisc, sim_start_ns, bootstrap_end_ns, reserve=0):
        bw = np.ascontiguousarray(bw_up_bits, dtype=np.uint64)
        ns = np.ascontiguousarray(sockets_per_host, dtype=np.uint32)
        if bw.shape != ns.shape:
            _raise(N.SRG_ERR_ARG, "bw_up_bits and sockets_per_host differ in length")
        self.num_hosts = int(bw.shape[0])
        self.sockets_per_host = ns
        self._create(N.lib().srg_outbound_create, router, self.num_hosts, bw.ctypes.data, ns.ctypes.data, int(qdisc),
                     int(sim_start_ns), int(bootstrap_end_ns), int(reserve))
        self.num_queued = 0
        self.min_next_wake_ns = 2**64 - 1

    def step_device(self, until_ns, num_offers, time_t, socket_t, priority_t, size_t, flags_t, tag_t, host_off_t, capacity,
                    out_status_t, out_time_t, out_tag_t, out_off_t, stream=None):
        """Raw call; returns (rc, result dict, message) and raises nothing: a short capacity is
        SRG_ERR_ARG with num_sent + num_local = the count needed.  time_t, priority_t, tag_t,
        host_off_t int64, socket_t, size_t int32 and flags_t uint8 (or None) tensors on the device;
        outputs uint8 / int64 / int64 [capacity] and int64 [num_hosts + 1]."""
        rc, res, msg = self._call(N.lib().srg_outbound_step_device, N.OutboundResult, int(until_ns), int(num_offers),
                                  _ptr(time_t), _ptr(socket_t), _ptr(priority_t), _ptr(size_t), _ptr(flags_t), _ptr(tag_t),
                                  _ptr(host_off_t), int(capacity), _ptr(out_status_t), _ptr(out_time_t), _ptr(out_tag_t),
                                  _ptr(out_off_t), stream=stream)
        if rc == N.SRG_OK:
            self.num_queued, self.min_next_wake_ns = int(res.num_queued), int(res.min_next_wake_ns)
        return rc, res.as_dict(), msg

    def step(self, until_ns, time, socket, priority, size, flags, tag, host_offsets):
        """Device tensors (or host arrays, uploaded) in; returns device tensors (status uint8, time
        int64, tag int64, host_offsets int64 [H + 1], result).  Sized by num_queued + offers, which
        always suffices."""
        dev = self.dev
        time_t, sock_t, prio_t = _dev_t(time, _i64, dev), _dev_t(socket, _i32, dev), _dev_t(priority, _i64, dev)
        size_t, flags_t = _dev_t(size, _i32, dev), _dev_t(flags, _u8, dev)
        tag_t, off_t = _dev_t(tag, _i64, dev), _dev_t(host_offsets, _i64, dev)
        n = int(time_t.numel())
        cap = max(self.num_queued + n, 1)
        status = torch.empty(cap, dtype=torch.uint8, device=dev)
        otime = torch.empty(cap, dtype=torch.int64, device=dev)
        otag = torch.empty(cap, dtype=torch.int64, device=dev)
        ooff = torch.empty(self.num_hosts + 1, dtype=torch.int64, device=dev)
        rc, res, msg = self.step_device(until_ns, n, time_t, sock_t, prio_t, size_t, flags_t, tag_t, off_t, cap, status,
                                        otime, otag, ooff)
        if rc != N.SRG_OK:
            _raise_queue(rc, msg)
        m = res["num_sent"] + res["num_local"]
        return status[:m], otime[:m], otag[:m], ooff, res

    def host_state(self, h):
        out = N.OutboundHostState()
        rc = N.lib().srg_outbound_host_state(self._h, int(h), ctypes.byref(out))
        if rc != N.SRG_OK:
            _raise(rc, "srg_outbound_host_state: host out of range")
        return out.as_dict()

    def host_order(self, h):
        """The host's heap array (or round-robin queue from its head) as a list of slots."""
        if not 0 <= int(h) < self.num_hosts:
            _raise(N.SRG_ERR_ARG, "srg_outbound_host_order: host out of range")
        cap = max(int(self.sockets_per_host[int(h)]), 1)
        buf = (ctypes.c_uint32 * cap)()
        n = ctypes.c_uint32()
        rc = N.lib().srg_outbound_host_order(self._h, int(h), buf, cap, ctypes.byref(n))
        if rc != N.SRG_OK:
            _raise(rc, "srg_outbound_host_order: host out of range")
        return [int(buf[i]) for i in range(int(n.value))]


class SocketsIn(_Stage):
    """Interface receive, resident in HBM across steps (srg_sockets_in_*, sockets_in.hip.h): what the
    inbound relay's dst.push(packet) does (relay/mod.rs:261-271) -- the interface's socket lookup
    (network_interface.c:140-202), the UDP sockets' receive buffers (udp.rs:108-168, 1081-1157) and the
    tracker's remote-in counters (tracker.c:188-252) -- plus the recvmsg side of the buffers
    (udp.rs:497-546).  step_device() takes the arrays Inbound.step_device / Round.receive_device wrote
    (deliver_status 1) or Round.send_device wrote (deliver_status SRG_ROUND_LOCAL) untouched."""

    _destroy = "srg_sockets_in_destroy"

    def __init__(self, router, sockets_per_host, reserve=0):
        ns = np.ascontiguousarray(sockets_per_host, dtype=np.uint32)
        self.num_hosts = int(ns.shape[0])
        self.sockets_per_host = ns
        self._packets = None
        self._create(N.lib().srg_sockets_in_create, router, self.num_hosts, ns.ctypes.data, int(reserve))
        self.num_buffered_messages = 0

    def set_packets(self, protocol_t, src_ip_t, src_port_t, dst_port_t, total_size_t, payload_size_t):
        """The packet table by tag, borrowed: uint8, int32 (u32 data), int16 (u16), int16, int32, int32
        tensors [num_packets] on the device."""
        ts = (protocol_t, src_ip_t, src_port_t, dst_port_t, total_size_t, payload_size_t)
        n = int(protocol_t.numel())
        assert all(int(t.numel()) == n for t in ts)
        assert [t.element_size() for t in ts] == [1, 4, 2, 2, 4, 4]
        self._packets = ts
        rc = N.lib().srg_sockets_in_set_packets(self._h, n, *[t.data_ptr() if n else None for t in ts])
        if rc != N.SRG_OK:
            _raise(rc, "srg_sockets_in_set_packets: null argument")

    def _batch(self, fn, cols, dtypes):
        arrs = [np.ascontiguousarray(c, dtype=d) for c, d in zip(cols, dtypes)]
        n = int(arrs[0].shape[0])
        if any(int(a.shape[0]) != n for a in arrs):
            _raise(N.SRG_ERR_ARG, "the batch's arrays differ in length")
        err = ctypes.create_string_buffer(1024)
        rc = fn(self._h, n, *[a.ctypes.data for a in arrs], err, len(err))
        if rc != N.SRG_OK:
            _raise(rc, err.value.decode(errors="replace"))

    def configure(self, host, slot, kind, has_peer, peer_ip, peer_port, soft_limit_bytes):
        """Host arrays [n]: sets each (host, slot)'s kind, peer and soft limit; all or nothing."""
        self._batch(N.lib().srg_sockets_in_configure, (host, slot, kind, has_peer, peer_ip, peer_port, soft_limit_bytes),
                    (np.uint32, np.uint32, np.uint8, np.uint8, np.uint32, np.uint16, np.uint64))

    def associate(self, host, protocol, local_port, peer_ip, peer_port, slot):
        """Host arrays [n]; a key that exists already raises and adds nothing."""
        self._batch(N.lib().srg_sockets_in_associate, (host, protocol, local_port, peer_ip, peer_port, slot),
                    (np.uint32, np.uint8, np.uint16, np.uint32, np.uint16, np.uint32))

    def disassociate(self, host, protocol, local_port, peer_ip, peer_port):
        """Host arrays [n]; a missing key is a no-op."""
        self._batch(N.lib().srg_sockets_in_disassociate, (host, protocol, local_port, peer_ip, peer_port),
                    (np.uint32, np.uint8, np.uint16, np.uint32, np.uint16))

    def step_device(self, num_rows, status, time, tag, host_off, deliver_status, num_reads, r_time, r_slot, r_flags,
                    r_host_off, out_status, out_slot, out_r_status, out_r_tag, out_r_time, out_r_payload, stream=None):
        """Raw call; returns (rc, result dict, message) and raises nothing.  Every array is a device
        tensor, a raw device pointer (int, e.g. a borrowed pointer of a Round result) or None."""
        rc, res, msg = self._call(N.lib().srg_sockets_in_step_device, N.SocketsInResult, int(num_rows), _ptr(status),
                                  _ptr(time), _ptr(tag), _ptr(host_off), int(deliver_status), int(num_reads), _ptr(r_time),
                                  _ptr(r_slot), _ptr(r_flags), _ptr(r_host_off), _ptr(out_status), _ptr(out_slot),
                                  _ptr(out_r_status), _ptr(out_r_tag), _ptr(out_r_time), _ptr(out_r_payload), stream=stream)
        if rc == N.SRG_OK:
            self.num_buffered_messages = int(res.num_buffered_messages)
        return rc, res.as_dict(), msg

    def step(self, status, time, tag, host_offsets, deliver_status=1, r_time=None, r_slot=None, r_flags=None,
             r_host_offsets=None):
        """Host arrays in (status / r_flags may be None; no reads: leave r_time None), host arrays out:
        (out_status u8, out_slot u32, read_status u8, read_tag u64, read_time u64, read_payload u32,
        result)."""
        dev = self.dev
        n = int(len(time))
        nr = 0 if r_time is None else int(len(r_time))
        time_t, tag_t, off_t = _i64(time, dev), _i64(tag, dev), _i64(host_offsets, dev)
        rt_t = _i64(r_time, dev) if nr else None
        rs_t = _i32(r_slot, dev) if nr else None
        ro_t = _i64(r_host_offsets, dev) if r_host_offsets is not None else None
        o_st = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        o_sl = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        q_st = torch.empty(max(nr, 1), dtype=torch.uint8, device=dev)
        q_tag = torch.empty(max(nr, 1), dtype=torch.int64, device=dev)
        q_time = torch.empty(max(nr, 1), dtype=torch.int64, device=dev)
        q_pay = torch.empty(max(nr, 1), dtype=torch.int32, device=dev)
        rc, res, msg = self.step_device(n, _dev_t(status, _u8, dev), time_t, tag_t, off_t, deliver_status, nr, rt_t, rs_t,
                                        _dev_t(r_flags, _u8, dev) if nr else None, ro_t, o_st, o_sl, q_st, q_tag, q_time,
                                        q_pay)
        if rc != N.SRG_OK:
            _raise_queue(rc, msg)
        return (o_st[:n].cpu().numpy(), o_sl[:n].cpu().numpy().view(np.uint32), q_st[:nr].cpu().numpy(),
                q_tag[:nr].cpu().numpy().view(np.uint64), q_time[:nr].cpu().numpy().view(np.uint64),
                q_pay[:nr].cpu().numpy().view(np.uint32), res)

    def socket_state(self, h, slot):
        out = N.SocketsInSocketState()
        rc = N.lib().srg_sockets_in_socket_state(self._h, int(h), int(slot), ctypes.byref(out))
        if rc != N.SRG_OK:
            _raise(rc, "srg_sockets_in_socket_state: host or slot out of range")
        return out.as_dict()

    def host_counters(self, h, reset=False):
        out = N.SocketsInHostCounters()
        rc = N.lib().srg_sockets_in_host_counters(self._h, int(h), ctypes.byref(out), 1 if reset else 0)
        if rc != N.SRG_OK:
            _raise(rc, "srg_sockets_in_host_counters: host out of range")
        return out.as_dict()


class _Borrowed:
    """A device array the native library owns, seen through __cuda_array_interface__."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def _borrowed(ptr, n, typestr, dtype, dev):
    """-> an owned copy (int64 / uint8 tensor) of n elements at the borrowed device pointer."""
    if not n or not ptr:
        return torch.empty(0, dtype=dtype, device=dev)
    return torch.as_tensor(_Borrowed(ptr, n, typestr), device=dev).clone()


class _PartView:
    """A part of a Round seen through its borrowed handle: the read-backs only."""

    def __init__(self, handle, base, owner):
        self._h, self._base, self._owner = handle, base, owner
        self.num_hosts = owner.num_hosts
        self.sockets_per_host = owner.sockets_per_host

    def host_state(self, h):
        return self._base.host_state(self, h)

    def host_order(self, h):
        return self._base.host_order(self, h)


class Round(_Stage):
    """A round on the device (srg_round_*, round.hip.h): the event queues, the inbound and the outbound
    path, each host's Xoshiro256++ generator (host.rs:233) and event-id counter (host.rs:690) and the
    hosts' nodes in HBM, over the caller's packet table indexed by tag.  A round is
    receive(window_end) -> the hosts run -> send(window_end, offers) -> next_window(result
    ["next_start_ns"], ...).  An error leaves everything as it was.  The part views give host_state /
    host_order of the round's own parts; stepping a part is not possible through them."""
    _destroy = "srg_round_destroy"

    def __init__(self, router, host_node, table, bw_up_bits, bw_down_bits, sockets_per_host, qdisc, node_seed,
                 sim_start_ns, bootstrap_end_ns, sim_end_ns, reserve=0):
        hn = np.ascontiguousarray(host_node, dtype=np.uint32)
        up = np.ascontiguousarray(bw_up_bits, dtype=np.uint64)
        down = np.ascontiguousarray(bw_down_bits, dtype=np.uint64)
        ns = np.ascontiguousarray(sockets_per_host, dtype=np.uint32)
        seed = np.ascontiguousarray(node_seed, dtype=np.uint64)
        if not (hn.shape == up.shape == down.shape == ns.shape == seed.shape):
            _raise(N.SRG_ERR_ARG, "the per-host arrays differ in length")
        self.num_hosts = int(hn.shape[0])
        self.sockets_per_host = ns
        self.table = table  # (keeps the borrowed device arrays alive)
        self._packets = None
        t = table.as_struct()
        L = N.lib()
        self._create(L.srg_round_create, router, self.num_hosts, hn.ctypes.data, ctypes.byref(t), up.ctypes.data,
                     down.ctypes.data, ns.ctypes.data, int(qdisc), seed.ctypes.data, int(sim_start_ns),
                     int(bootstrap_end_ns), int(sim_end_ns), int(reserve))
        h = self._h
        self.queues = _PartView(ctypes.c_void_p(L.srg_round_queues(h)), EventQueues, self)
        self.inbound = _PartView(ctypes.c_void_p(L.srg_round_inbound(h)), Inbound, self)
        self.outbound = _PartView(ctypes.c_void_p(L.srg_round_outbound(h)), Outbound, self)

    def set_packets(self, dst_host_t, total_size_t, payload_size_t):
        """int32 tensors [num_packets] on the device (u32 data), indexed by tag; borrowed."""
        n = int(dst_host_t.numel())
        assert int(total_size_t.numel()) == n and int(payload_size_t.numel()) == n
        self._packets = (dst_host_t, total_size_t, payload_size_t)
        rc = N.lib().srg_round_set_packets(self._h, n, dst_host_t.data_ptr() if n else None,
                                           total_size_t.data_ptr() if n else None,
                                           payload_size_t.data_ptr() if n else None)
        if rc != N.SRG_OK:
            _raise(rc, "srg_round_set_packets: null argument")

    def receive_device(self, until_ns, stream=None):
        """Raw call; returns (rc, RoundReceiveResult, message) and raises nothing."""
        return self._call(N.lib().srg_round_receive_device, N.RoundReceiveResult, int(until_ns), stream=stream)

    def receive(self, until_ns):
        """pop(until) -> sizes -> inbound step.  Returns a dict: the result fields, the popped events
        (popped_time, popped_tag, popped_host_offsets) and the inbound step's outputs (status uint8,
        time, tag, host_offsets), as owned device tensors."""
        rc, res, msg = self.receive_device(until_ns)
        if rc != N.SRG_OK:
            _raise_queue(rc, msg)
        d, dev, H1 = res.as_dict(), self.dev, self.num_hosts + 1
        d["popped_time"] = _borrowed(res.popped_time_ns_dev, res.num_popped, "<i8", torch.int64, dev)
        d["popped_tag"] = _borrowed(res.popped_tag_dev, res.num_popped, "<i8", torch.int64, dev)
        d["popped_host_offsets"] = _borrowed(res.popped_host_offsets_dev, H1, "<i8", torch.int64, dev)
        d["status"] = _borrowed(res.status_dev, res.num_leaving, "|u1", torch.uint8, dev)
        d["time"] = _borrowed(res.time_ns_dev, res.num_leaving, "<i8", torch.int64, dev)
        d["tag"] = _borrowed(res.tag_dev, res.num_leaving, "<i8", torch.int64, dev)
        d["host_offsets"] = _borrowed(res.host_offsets_dev, H1, "<i8", torch.int64, dev)
        return d

    def send_device(self, until_ns, num_offers, time_t, socket_t, priority_t, flags_t, tag_t, host_off_t, counts_t=None,
                    stream=None):
        """Raw call; returns (rc, RoundSendResult, message) and raises nothing.  time_t, priority_t,
        tag_t, host_off_t int64, socket_t int32, flags_t uint8 (or None) tensors on the device."""
        return self._call(N.lib().srg_round_send_device, N.RoundSendResult, int(until_ns), int(num_offers), _ptr(time_t),
                          _ptr(socket_t), _ptr(priority_t), _ptr(flags_t), _ptr(tag_t), _ptr(host_off_t), _ptr(counts_t),
                          stream=stream)

    def send(self, until_ns, time, socket, priority, flags, tag, host_offsets, counts=None):
        """offers -> outbound step -> draw -> send -> push.  Device tensors (or host arrays, uploaded)
        in.  Returns a dict: the result fields and, per leaving packet grouped by host in leaving
        order, status (uint8, SRG_ROUND_*), time, tag and host_offsets as owned device tensors."""
        dev = self.dev
        time_t, sock_t, prio_t = _dev_t(time, _i64, dev), _dev_t(socket, _i32, dev), _dev_t(priority, _i64, dev)
        flags_t, tag_t, off_t = _dev_t(flags, _u8, dev), _dev_t(tag, _i64, dev), _dev_t(host_offsets, _i64, dev)
        rc, res, msg = self.send_device(until_ns, int(time_t.numel()), time_t, sock_t, prio_t, flags_t, tag_t, off_t, counts)
        if rc != N.SRG_OK:
            _raise_queue(rc, msg)
        d = res.as_dict()
        d["status"] = _borrowed(res.status_dev, res.num_leaving, "|u1", torch.uint8, dev)
        d["time"] = _borrowed(res.time_ns_dev, res.num_leaving, "<i8", torch.int64, dev)
        d["tag"] = _borrowed(res.tag_dev, res.num_leaving, "<i8", torch.int64, dev)
        d["host_offsets"] = _borrowed(res.host_offsets_dev, self.num_hosts + 1, "<i8", torch.int64, dev)
        return d

    def host_rng(self, h):
        """-> ([s0, s1, s2, s3], next_event_id) of host h."""
        w = (ctypes.c_uint64 * 4)()
        e = ctypes.c_uint64()
        rc = N.lib().srg_round_host_rng(self._h, int(h), w, ctypes.byref(e))
        if rc != N.SRG_OK:
            _raise(rc, "srg_round_host_rng: host out of range")
        return [int(x) for x in w], int(e.value)

    def set_host_rng(self, h, words, next_event_id):
        w = (ctypes.c_uint64 * 4)(*[int(x) for x in words])
        rc = N.lib().srg_round_set_host_rng(self._h, int(h), w, int(next_event_id))
        if rc != N.SRG_OK:
            _raise(rc, "srg_round_set_host_rng: host out of range, or the all-zero state")
