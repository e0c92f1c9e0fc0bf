"""Plain-Python restatement of what lies behind the inbound relay on a host, one operation at a
time, with a counter per branch (COUNTERS / BRANCHES):
  networkinterface_associate / _disassociate   network_interface.c:77-117
  networkinterface_push                        network_interface.c:140-202
  UdpSocket::push_in_packet                    udp.rs:108-168
  MessageBuffer                                udp.rs:1081-1157
  UdpSocket::recvmsg                           udp.rs:497-546
  _tracker_updateCounters                      tracker.c:188-219
It is the yardstick of shadow_amd/csrc/sockets_in_rule.h (through tests/cpp/sockets_in_rule_check.cpp)
and of the device step (tests/test_sockets_in_gpu.py).  Nothing here is vectorised or clever: a host's
deliveries and reads are merged with two cursors and applied in that order."""
import copy

UDP, EXTERNAL = 0, 1
SKIPPED, NO_SOCKET, RCV_EXTERNAL, PEER_MISMATCH, FULL, BUFFERED = range(6)
READ_PEEK, READ_FIRST = 1, 2
NO_SLOT = 0xFFFFFFFF
DEFAULT_LIMIT = 174760  # CONFIG_RECV_BUFFER_SIZE
ERR_ARG, ERR_TIME_BACKWARD = 1, 12

BRANCHES = (
    "assoc_new", "assoc_duplicate", "disassoc_found", "disassoc_missing",
    "skipped", "lookup_specific", "lookup_wildcard", "lookup_none",
    "count_control", "count_data", "external", "no_peer", "peer_ok", "peer_ip_differs", "peer_port_differs",
    "full", "buffered", "buffered_past_limit",
    "read_empty", "read_pop", "read_peek", "read_before_delivery_earlier", "read_before_delivery_first",
    "read_after_delivery_tie", "limit_changed_nonempty",
    "err_offsets", "err_tag", "err_no_table", "err_flag", "err_slot", "err_external_read", "err_contradict",
    "err_backward_delivery", "err_backward_read", "err_config", "err_assoc_range",
)
COUNTERS = {k: 0 for k in BRANCHES}


def hit(k):
    COUNTERS[k] += 1


class RefError(Exception):
    def __init__(self, code, what):
        super().__init__(what)
        self.code = code


class Socket:
    def __init__(self):
        self.kind, self.has_peer, self.peer_ip, self.peer_port = UDP, 0, 0, 0
        self.limit, self.len = DEFAULT_LIMIT, 0
        self.msgs = []  # (tag, recv_time, payload)

    def state(self):
        return dict(len_bytes=self.len, num_messages=len(self.msgs), soft_limit_bytes=self.limit, peer_ip=self.peer_ip,
                    peer_port=self.peer_port, kind=self.kind, has_peer=self.has_peer)


COUNTER_KEYS = ("packets_control", "packets_data", "bytes_control_header", "bytes_data_header", "bytes_data_payload")
RESULT_KEYS = ("num_skipped", "num_no_socket", "num_external", "num_peer_mismatch", "num_full", "num_buffered", "num_read",
               "num_would_block", "num_buffered_messages")


def read_before(t_read, flags, t_delivery):
    """Does the read run before the delivery?  (the merge's one question)"""
    if t_read < t_delivery:
        hit("read_before_delivery_earlier")
        return True
    if t_read == t_delivery and flags & READ_FIRST:
        hit("read_before_delivery_first")
        return True
    if t_read == t_delivery:
        hit("read_after_delivery_tie")
    return False


class SocketsInRef:
    def __init__(self, sockets_per_host):
        self.nsock = [int(x) for x in sockets_per_host]
        self.H = len(self.nsock)
        self.socks = [[Socket() for _ in range(n)] for n in self.nsock]
        self.counters = [dict.fromkeys(COUNTER_KEYS, 0) for _ in range(self.H)]
        self.assoc = {}
        self.packets = None

    # ---- host-side calls ----
    def set_packets(self, protocol, src_ip, src_port, dst_port, total, payload):
        self.packets = [tuple(int(x) for x in p) for p in zip(protocol, src_ip, src_port, dst_port, total, payload)]

    def _check_slot(self, h, slot, counter):
        if not 0 <= h < self.H or not 0 <= slot < self.nsock[h]:
            hit(counter)
            raise RefError(ERR_ARG, "host or slot out of range")

    def configure(self, entries):
        """entries: (host, slot, kind, has_peer, peer_ip, peer_port, limit); all or nothing"""
        for h, slot, kind, has_peer, _, _, _ in entries:
            self._check_slot(h, slot, "err_config")
            if kind not in (UDP, EXTERNAL) or has_peer not in (0, 1):
                hit("err_config")
                raise RefError(ERR_ARG, "unknown kind or has_peer")
        for h, slot, kind, has_peer, pip, pport, limit in entries:
            s = self.socks[h][slot]
            if s.msgs and limit != s.limit:
                hit("limit_changed_nonempty")
            s.kind, s.has_peer, s.peer_ip, s.peer_port, s.limit = kind, has_peer, pip, pport, limit

    def associate(self, entries):
        """entries: (host, protocol, local_port, peer_ip, peer_port, slot); all or nothing"""
        add = {}
        for h, proto, lport, pip, pport, slot in entries:
            self._check_slot(h, slot, "err_assoc_range")
            k = (h, proto, lport, pip, pport)
            if k in self.assoc or k in add:
                hit("assoc_duplicate")
                raise RefError(ERR_ARG, "the key is already associated")
            hit("assoc_new")
            add[k] = slot
        self.assoc.update(add)

    def disassociate(self, entries):
        for k in entries:
            if self.assoc.pop(tuple(k), None) is None:
                hit("disassoc_missing")
            else:
                hit("disassoc_found")

    def socket_state(self, h, slot):
        self._check_slot(h, slot, "err_config")
        return self.socks[h][slot].state()

    def host_counters(self, h, reset=False):
        if not 0 <= h < self.H:
            raise RefError(ERR_ARG, "host out of range")
        out = dict(self.counters[h])
        if reset:
            self.counters[h] = dict.fromkeys(COUNTER_KEYS, 0)
        return out

    # ---- one operation ----
    def lookup(self, h, proto, dport, sip, sport):
        slot = self.assoc.get((h, proto, dport, sip, sport))
        if slot is not None:
            hit("lookup_specific")
            return slot
        slot = self.assoc.get((h, proto, dport, 0, 0))
        if slot is not None:
            hit("lookup_wildcard")
            return slot
        hit("lookup_none")
        return None

    def deliver(self, h, tag, t):
        """-> (status, slot)"""
        proto, sip, sport, dport, total, payload = self.packets[tag]
        slot = self.lookup(h, proto, dport, sip, sport)
        if slot is None:
            return NO_SOCKET, NO_SLOT
        c = self.counters[h]
        if payload > 0:
            hit("count_data")
            c["packets_data"] += 1
            c["bytes_data_header"] += total - payload
            c["bytes_data_payload"] += payload
        else:
            hit("count_control")
            c["packets_control"] += 1
            c["bytes_control_header"] += total - payload
        s = self.socks[h][slot]
        if s.kind == EXTERNAL:
            hit("external")
            return RCV_EXTERNAL, slot
        if s.has_peer:
            if s.peer_ip != sip:
                hit("peer_ip_differs")
                return PEER_MISMATCH, slot
            if s.peer_port != sport:
                hit("peer_port_differs")
                return PEER_MISMATCH, slot
            hit("peer_ok")
        else:
            hit("no_peer")
        if not s.len < s.limit:  # has_space
            hit("full")
            return FULL, slot
        s.len += payload
        s.msgs.append((tag, t, payload))
        hit("buffered_past_limit" if s.len > s.limit else "buffered")
        return BUFFERED, slot

    def read(self, h, slot, flags):
        """-> (status, tag, recv_time, payload)"""
        s = self.socks[h][slot]
        if not s.msgs:
            hit("read_empty")
            return 0, 0, 0, 0
        tag, t, payload = s.msgs[0]
        if flags & READ_PEEK:
            hit("read_peek")
        else:
            hit("read_pop")
            s.msgs.pop(0)
            s.len -= payload
        return 1, tag, t, payload

    # ---- a step ----
    def step(self, status, time, tag, host_off, deliver_status, r_time=(), r_slot=(), r_flags=None, r_host_off=None):
        """-> (out_status, out_slot, read_status, read_tag, read_time, read_payload, result); raises
        RefError with everything as it was"""
        snap = (copy.deepcopy(self.socks), copy.deepcopy(self.counters))
        try:
            return self._step(status, time, tag, host_off, deliver_status, r_time, r_slot, r_flags, r_host_off)
        except RefError:
            self.socks, self.counters = snap
            raise

    def _step(self, status, time, tag, host_off, deliver_status, r_time, r_slot, r_flags, r_host_off):
        n, nr, H = len(time), len(r_time), self.H
        if self.packets is None:
            hit("err_no_table")
            raise RefError(ERR_ARG, "no packet table")
        if r_host_off is None:
            r_host_off = [0] * (H + 1)
        if r_flags is None:
            r_flags = [0] * nr
        for off, cnt in ((host_off, n), (r_host_off, nr)):
            off = [int(x) for x in off]
            if len(off) != H + 1 or off[0] != 0 or off[-1] != cnt or any(a > b for a, b in zip(off, off[1:])):
                hit("err_offsets")
                raise RefError(ERR_ARG, "offsets")
        is_delivery = [status is None or int(status[i]) == deliver_status for i in range(n)]
        if any(d and int(tag[i]) >= len(self.packets) for i, d in enumerate(is_delivery)):
            hit("err_tag")
            raise RefError(ERR_ARG, "tag")
        # the reads' own checks, then the time order (the order in which the device reports them)
        for h in range(H):
            for j in range(int(r_host_off[h]), int(r_host_off[h + 1])):
                if int(r_flags[j]) & ~(READ_PEEK | READ_FIRST):
                    hit("err_flag")
                    raise RefError(ERR_ARG, "flag")
        for h in range(H):
            for j in range(int(r_host_off[h]), int(r_host_off[h + 1])):
                if int(r_slot[j]) >= self.nsock[h]:
                    hit("err_slot")
                    raise RefError(ERR_ARG, "slot")
                if self.socks[h][int(r_slot[j])].kind == EXTERNAL:
                    hit("err_external_read")
                    raise RefError(ERR_ARG, "EXTERNAL slot")
        for h in range(H):
            for j in range(int(r_host_off[h]) + 1, int(r_host_off[h + 1])):
                if (int(r_time[j]) == int(r_time[j - 1]) and int(r_flags[j]) & READ_FIRST
                        and not int(r_flags[j - 1]) & READ_FIRST):
                    hit("err_contradict")
                    raise RefError(ERR_ARG, "READ_FIRST behind a read without it")
        for h in range(H):
            rows = [i for i in range(int(host_off[h]), int(host_off[h + 1])) if is_delivery[i]]
            if any(int(time[a]) > int(time[b]) for a, b in zip(rows, rows[1:])):
                hit("err_backward_delivery")
                raise RefError(ERR_TIME_BACKWARD, "delivery")
            rr = range(int(r_host_off[h]), int(r_host_off[h + 1]))
            if any(int(r_time[a]) > int(r_time[a + 1]) for a in list(rr)[:-1]):
                hit("err_backward_read")
                raise RefError(ERR_TIME_BACKWARD, "read")
        out_status, out_slot = [SKIPPED] * n, [NO_SLOT] * n
        rs, rg, rt, rp = [0] * nr, [0] * nr, [0] * nr, [0] * nr
        for h in range(H):
            rows = [i for i in range(int(host_off[h]), int(host_off[h + 1])) if is_delivery[i]]
            hit("skipped") if len(rows) < int(host_off[h + 1]) - int(host_off[h]) else None
            di, j, j1 = 0, int(r_host_off[h]), int(r_host_off[h + 1])
            while di < len(rows) or j < j1:
                if j < j1 and (di == len(rows) or read_before(int(r_time[j]), int(r_flags[j]), int(time[rows[di]]))):
                    rs[j], rg[j], rt[j], rp[j] = self.read(h, int(r_slot[j]), int(r_flags[j]))
                    j += 1
                else:
                    i = rows[di]
                    out_status[i], out_slot[i] = self.deliver(h, int(tag[i]), int(time[i]))
                    di += 1
        res = {k: 0 for k in RESULT_KEYS}
        names = ("num_skipped", "num_no_socket", "num_external", "num_peer_mismatch", "num_full", "num_buffered")
        for s in out_status:
            res[names[s]] += 1
        res["num_read"] = sum(rs)
        res["num_would_block"] = nr - sum(rs)
        res["num_buffered_messages"] = sum(len(s.msgs) for hs in self.socks for s in hs)
        return out_status, out_slot, rs, rg, rt, rp, res
