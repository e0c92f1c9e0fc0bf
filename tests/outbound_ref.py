"""A plain-Python restatement of a host's outbound path, written from the reference and independent of
shadow_amd/csrc/outbound_rule.h: its own heap class, deques and event loop.

  host/descriptor/socket.c:198-199,437-442,466-467   a socket's control and data FIFOs, its next packet
  host.rs:1003-1017                                   notify_socket_has_packets
  host/network/network_interface.c:205-294,344-370    the two selection steps, wantsSend
  host/network/network_queuing_disciplines.c:22-160   the round-robin queue, the FIFO comparator
  utility/priority_queue.c:87-175                     the binary heap (push, pop, heapify up / down)
  network/relay/mod.rs:111-288                        notify, the forward task, create_token_bucket
  network/relay/token_bucket.rs:68-157                TokenBucket (inbound_ref.py's: the same struct)

Pinned by the reference's own compiled code (oracle/_ref/qdisc_ref, built from a checkout by
oracle/ref_qdisc/; its recorded answers are tests/golden/qdisc_reference.json): SocketHeap with its
comparator and SocketRing.  Still restated, there as here: Socket's two FIFOs, wantsSend (Host.offer),
the selection loop (Host.interface_pop), the relay and the bucket.  Host(..., trace=True) records the
host's offers and selects; trace_script / trace_output give them in that program's format.

The order between an offer and a forward task of the same nanosecond is the caller's (event ids):
OFFER_BARRIER on an offer says that a task due at the offer's time runs before it.
COUNTERS counts the branches the tests must reach.
"""
from collections import deque

from inbound_ref import create_token_bucket

U64 = 2**64 - 1
TIME_END = 2**62
QDISC_FIFO, QDISC_ROUND_ROBIN = 0, 1
OFFER_LOCAL, OFFER_BARRIER = 1, 2

ERR_ARG = 1
ERR_TIME_BACKWARD = 12

BRANCHES = ("bootstrap_forward", "local_exempt", "local_behind_cached", "token_block", "block_multi_refill",
            "offer_at_wake_barrier", "offer_at_wake_no_barrier", "barrier_nothing_pending", "wake_at_window_end",
            "control_before_data", "control_into_queued_socket", "priority0_tie", "right_child_taken",
            "socket_pushed_back", "socket_leaves", "round_robin_rotation", "unlimited_host",
            "select_65_queued", "select_129_queued")
COUNTERS = {k: 0 for k in BRANCHES}


def hit(name):
    COUNTERS[name] += 1


def reset_counters():
    for k in COUNTERS:
        COUNTERS[k] = 0


class OutboundRefError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class Socket:
    """socket.c: packets are (priority, size, flags, tag); priority 0 is a control packet."""

    def __init__(self, slot):
        self.slot = slot
        self.control, self.data = deque(), deque()

    def add(self, pkt):  # socket.c:437-442
        (self.control if pkt[0] == 0 else self.data).append(pkt)

    def has_data(self):
        return bool(self.control) or bool(self.data)

    def peek_priority(self):  # socket.c:198-199
        return self.control[0][0] if self.control else self.data[0][0]

    def pull(self):  # socket.c:466-467
        if self.control:
            if self.data:
                hit("control_before_data")
            return self.control.popleft()
        return self.data.popleft()

    def __len__(self):
        return len(self.control) + len(self.data)


class SocketHeap:
    """priority_queue.c over sockets with network_queuing_disciplines.c:82-94 as the comparator: the
    keys are read from the sockets when two entries are compared, never stored."""

    def __init__(self):
        self.heap = []

    def __len__(self):
        return len(self.heap)

    def _smaller(self, i, j):  # _compareSocket(...) < 0: +1 only for pa > pb
        pa, pb = self.heap[i].peek_priority(), self.heap[j].peek_priority()
        if pa == 0 and pb == 0:
            hit("priority0_tie")
        return not pa > pb

    def _swap(self, i, j):
        self.heap[i], self.heap[j] = self.heap[j], self.heap[i]

    def _up(self, i):
        while i > 0 and self._smaller(i, (i - 1) // 2):
            self._swap(i, (i - 1) // 2)
            i = (i - 1) // 2

    def _down(self, i):
        while 2 * i + 1 < len(self.heap):
            c = 2 * i + 1
            if c + 1 < len(self.heap) and self._smaller(c + 1, c):
                hit("right_child_taken")
                c += 1
            if not self._smaller(c, i):
                break
            self._swap(i, c)
            i = c

    def find(self, s):
        return any(x is s for x in self.heap)

    def push(self, s):
        assert not self.find(s)
        self.heap.append(s)
        self._up(len(self.heap) - 1)

    def pop(self):
        s = self.heap[0]
        self._swap(0, len(self.heap) - 1)
        self.heap.pop()
        self._down(0)
        return s

    def order(self):
        return [s.slot for s in self.heap]


class SocketRing:
    """The round-robin discipline: a plain queue of sockets."""

    def __init__(self):
        self.q = deque()

    def __len__(self):
        return len(self.q)

    def find(self, s):
        return any(x is s for x in self.q)

    def push(self, s):
        self.q.append(s)

    def pop(self):
        return self.q.popleft()

    def order(self):
        return [s.slot for s in self.q]


class Host:
    """One host's internet interface (sockets + qdisc) and relay_inet_out."""

    def __init__(self, bw_up_bits, num_sockets, qdisc, sim_start, bootstrap_end, trace=False):
        self.trace = [] if trace else None  # ("o", slot, priority, tag) | ("s", slot, tag) | ("s", None, None)
        self.sockets = [Socket(i) for i in range(num_sockets)]
        self.qdisc = qdisc
        self.q = SocketHeap() if qdisc == QDISC_FIFO else SocketRing()
        self.bucket = None if bw_up_bits == U64 else create_token_bucket(bw_up_bits // 8, sim_start)
        self.bootstrap_end = bootstrap_end
        self.pending, self.wake, self.wake_from_block = False, 0, False
        self.next_packet = None
        self.last_time = sim_start
        self.out = []

    def interface_pop(self):  # network_interface.c:205-294
        if not len(self.q):
            if self.trace is not None:
                self.trace.append(("s", None, None))
            return None
        if len(self.q) >= 65:
            hit("select_65_queued")
        if len(self.q) >= 129:
            hit("select_129_queued")
        s = self.q.pop()
        pkt = s.pull()
        if self.trace is not None:
            self.trace.append(("s", s.slot, pkt[3]))
        if s.has_data():
            hit("socket_pushed_back")
            if self.qdisc == QDISC_ROUND_ROBIN and len(self.q):
                hit("round_robin_rotation")
            self.q.push(s)
        else:
            hit("socket_leaves")
        return pkt

    def run_forward_task(self, now):  # relay/mod.rs:166-273
        self.pending = False
        self.last_time = now
        while True:
            pkt, self.next_packet = self.next_packet, None
            if pkt is None:
                pkt = self.interface_pop()
            if pkt is None:
                return  # Idle
            local = bool(pkt[2] & OFFER_LOCAL)
            if now < self.bootstrap_end:
                hit("bootstrap_forward")
            elif local:
                hit("local_exempt")
            elif self.bucket is None:
                hit("unlimited_host")
            else:
                ok, dur = self.bucket.conforming_remove(pkt[1], now)
                if not ok:
                    hit("token_block")
                    if dur > 1_000_000:
                        hit("block_multi_refill")
                    if any(p[2] & OFFER_LOCAL for s in self.sockets for p in list(s.control) + list(s.data)):
                        hit("local_behind_cached")
                    self.next_packet = pkt
                    self.pending, self.wake, self.wake_from_block = True, now + dur, True
                    return
            self.out.append((2 if local else 1, now, pkt[3]))

    def offer(self, t, slot, pkt):  # host.rs:1003-1017
        if self.trace is not None:
            self.trace.append(("o", slot, pkt[0], pkt[3]))
        s = self.sockets[slot]
        in_q = self.q.find(s)
        assert in_q == s.has_data()
        if in_q and pkt[0] == 0:
            hit("control_into_queued_socket")
        s.add(pkt)
        if not in_q:
            self.q.push(s)
        if not self.pending:
            self.pending, self.wake, self.wake_from_block = True, t, False
        self.last_time = max(self.last_time, t)

    def step(self, until, offers):
        """offers: [(time, slot, priority, size, flags, tag)] in execution order; returns
        [(status, time, tag)] in leaving order."""
        self.out = []
        for t, slot, prio, size, flags, tag in offers:
            barrier = bool(flags & OFFER_BARRIER)
            if barrier and not (self.pending and self.wake == t):
                hit("barrier_nothing_pending")
            if self.pending and self.wake == t and self.wake_from_block:
                hit("offer_at_wake_barrier" if barrier else "offer_at_wake_no_barrier")
            while self.pending and (self.wake < t or (self.wake == t and barrier)):
                self.run_forward_task(self.wake)
            self.offer(t, slot, (prio, size, flags & OFFER_LOCAL, tag))
        while self.pending and self.wake < until:
            self.run_forward_task(self.wake)
        if self.pending and self.wake == until:
            hit("wake_at_window_end")
        return self.out

    def state(self):
        b = self.bucket
        return dict(balance=b.balance if b else 0, last_refill_ns=b.last_refill if b else None,
                    wake_ns=self.wake if self.pending else 0,
                    cached_tag=self.next_packet[3] if self.next_packet is not None else 0,
                    queued=sum(len(s) for s in self.sockets), qdisc_len=len(self.q), pending=int(self.pending),
                    has_cached=int(self.next_packet is not None))


class Outbound:
    def __init__(self, bw_up_bits, sockets_per_host, qdisc, sim_start, bootstrap_end, trace=False):
        if qdisc not in (QDISC_FIFO, QDISC_ROUND_ROBIN):
            raise OutboundRefError(ERR_ARG, "qdisc")
        self.sim_start = sim_start
        self.hosts = [Host(int(b), int(n), qdisc, sim_start, bootstrap_end, trace)
                      for b, n in zip(bw_up_bits, sockets_per_host)]

    def validate(self, until, time, slot, size, flags, offs):
        H, n = len(self.hosts), len(time)
        if until > TIME_END:
            raise OutboundRefError(ERR_ARG, "until")
        if len(offs) != H + 1 or offs[0] != 0 or offs[H] != n or any(offs[h] > offs[h + 1] for h in range(H)):
            raise OutboundRefError(ERR_ARG, "offsets")
        if any(t < self.sim_start or t >= TIME_END or t >= until for t in time):
            raise OutboundRefError(ERR_ARG, "time")
        if any(f & ~(OFFER_LOCAL | OFFER_BARRIER) for f in flags):
            raise OutboundRefError(ERR_ARG, "flags")
        for h in range(H):
            host = self.hosts[h]
            for j in range(offs[h], offs[h + 1]):
                if slot[j] >= len(host.sockets):
                    raise OutboundRefError(ERR_ARG, "slot")
                # (not the reference's: such a packet never conforms, the relay would reschedule for ever)
                if host.bucket is not None and not flags[j] & OFFER_LOCAL and size[j] > host.bucket.capacity:
                    raise OutboundRefError(ERR_ARG, "size")
        for h in range(H):
            prev = self.hosts[h].last_time
            for j in range(offs[h], offs[h + 1]):
                if time[j] < prev:
                    raise OutboundRefError(ERR_TIME_BACKWARD, "backward")
                prev = time[j]

    def step(self, until, time, slot, prio, size, flags, tag, offs):
        """Returns (status, time, tag, host_offsets, result) as lists."""
        time, slot, prio, size, flags, tag, offs = ([int(x) for x in a] for a in (time, slot, prio, size, flags, tag, offs))
        self.validate(until, time, slot, size, flags, offs)
        st, tm, tg, oo = [], [], [], [0]
        for h, host in enumerate(self.hosts):
            out = host.step(until, [(time[j], slot[j], prio[j], size[j], flags[j], tag[j])
                                    for j in range(offs[h], offs[h + 1])])
            for s, t, g in out:
                st.append(s)
                tm.append(t)
                tg.append(g)
            oo.append(len(st))
        wakes = [h.wake for h in self.hosts if h.pending]
        res = dict(num_sent=sum(1 for s in st if s == 1), num_local=sum(1 for s in st if s == 2),
                   num_queued=sum(sum(len(s) for s in h.sockets) + (h.next_packet is not None) for h in self.hosts),
                   min_next_wake_ns=min(wakes) if wakes else U64)
        return st, tm, tg, oo, res

    def host_state(self, h):
        return self.hosts[h].state()

    def host_order(self, h):
        return self.hosts[h].q.order()


# ---- the trace: a host's qdisc operations as a script for oracle/_ref/qdisc_ref ---------------
def trace_script(qdisc, num_sockets, trace):
    """A host's trace (Host(..., trace=True).trace) in the reference program's script format:
    "<qdisc> <sockets>", then "o <slot> <priority> <tag>" per offer and "s" per selection step."""
    return "".join(["%d %d\n" % (qdisc, num_sockets)] +
                   ["s\n" if e[0] == "s" else "o %d %d %d\n" % e[1:] for e in trace])


def trace_output(trace):
    """What the reference program prints for that script if it selects as the trace did: "<slot> <tag>"
    per selection step, "-" for one on an empty qdisc."""
    return "".join("-\n" if e[1] is None else "%d %d\n" % e[1:] for e in trace if e[0] == "s")


def replay_script(text, host_cls=Host):
    """Runs a script through Socket and SocketHeap / SocketRing (a host with no relay: offer and
    interface_pop only) -> the output text."""
    lines = text.splitlines()
    qdisc, num_sockets = (int(x) for x in lines[0].split())
    host = host_cls(U64, num_sockets, qdisc, 0, 0, trace=True)
    for ln in lines[1:]:
        if ln == "s":
            host.interface_pop()
        else:
            op, slot, prio, tag = ln.split()
            assert op == "o"
            host.offer(0, int(slot), (int(prio), 0, 0, int(tag)))
    assert trace_script(qdisc, num_sockets, host.trace) == text
    return trace_output(host.trace)
