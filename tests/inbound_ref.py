"""A plain-Python restatement of a host's inbound path, written from the reference and independent of
shadow_amd/csrc/inbound_rule.h: deque and integers.

  router/codel_queue.rs:125-319   CoDelQueue
  relay/token_bucket.rs:68-157    TokenBucket
  relay/mod.rs:111-288            Relay (notify, forward task, forward_until_blocked), create_token_bucket
  host.rs:853-858                 a packet event: route_incoming_packet, notify_router_has_packets
  core/work/event.rs:103-110      Packet before Local at equal time

Python integers do not wrap, so the reference's saturating operations are written as min(..., U64).
COUNTERS counts the branches the tests must reach (test_inbound_gpu.py asserts every one nonzero).
"""
import math
from collections import deque

U64 = 2**64 - 1
TARGET = 10_000_000
INTERVAL = 100_000_000
MTU = 1500
REFILL_NS = 1_000_000
TIME_END = 2**62
STORE, DROP = 0, 1

ERR_ARG = 1
ERR_TIME_BACKWARD = 12

BRANCHES = ("bootstrap_forward", "token_block", "block_multi_refill", "arrival_at_wake", "wake_at_window_end",
            "store_to_drop", "drop_in_drop_mode", "control_law_chain", "drop_to_store", "drop_mode_not_due",
            "restart_delta")
COUNTERS = {k: 0 for k in BRANCHES}


def hit(name):
    COUNTERS[name] += 1


class InboundRefError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class TokenBucket:
    def __init__(self, capacity, refill_increment, refill_interval, last_refill):
        assert capacity > 0 and refill_increment > 0 and refill_interval > 0
        self.capacity, self.balance = capacity, capacity
        self.refill_increment, self.refill_interval, self.last_refill = refill_increment, refill_interval, last_refill

    def lazy_refill(self, now):
        span = now - self.last_refill
        assert span >= 0
        if span >= self.refill_interval:
            num_refills = span // self.refill_interval
            num_tokens = min(self.refill_increment * num_refills, U64)
            self.balance = max(0, min(min(self.balance + num_tokens, U64), self.capacity))
            self.last_refill = min(self.last_refill + min(self.refill_interval * num_refills, U64), U64)
            span = now - self.last_refill
        assert span < self.refill_interval
        return self.refill_interval - span

    def conforming_remove(self, decrement, now):
        """(True, balance) or (False, duration until it conforms)."""
        next_refill_span = self.lazy_refill(now)
        if self.balance >= decrement:
            self.balance -= decrement
            return True, self.balance
        required = max(decrement - self.balance, 0)
        refills = required // self.refill_increment + (1 if required % self.refill_increment else 0)
        if refills == 0:
            return False, 0
        if refills == 1:
            return False, next_refill_span
        hit("block_multi_refill")
        return False, min(next_refill_span + min(self.refill_interval * (refills - 1), U64), U64)


def create_token_bucket(bytes_per_second, sim_start):
    refill = max(1, bytes_per_second // 1000)
    return TokenBucket(refill + MTU, refill, REFILL_NS, sim_start)


def control_law(time, count):
    sq = 1.0 if count == 0 else math.sqrt(float(count))
    div = float(INTERVAL) / sq
    fl = math.floor(div)  # f64::round: half away from zero (div > 0; div - fl is exact below 2^52)
    inc = int(fl) + (1 if div - fl >= 0.5 else 0)
    return min(time + inc, U64)


class CoDelQueue:
    """Elements are (enqueue_ts, size, tag); `dropped` receives (element, now) for every drop."""

    def __init__(self, dropped=None):
        self.elements = deque()
        self.total_bytes_stored = 0
        self.mode = STORE
        self.interval_end = None
        self.drop_next = None
        self.current_drop_count = 0
        self.previous_drop_count = 0
        self.dropped = dropped if dropped is not None else (lambda el, now: None)

    def __len__(self):
        return len(self.elements)

    def push(self, size, now, tag=0):
        self.total_bytes_stored += size
        self.elements.append((now, size, tag))

    def _set_mode(self, m):
        if self.mode == DROP and m == STORE:
            hit("drop_to_store")
        self.mode = m

    def pop(self, now):
        item = self.codel_pop(now)
        if item is None:
            self._set_mode(STORE)
            return None
        el, ok_to_drop = item
        if not ok_to_drop:
            self._set_mode(STORE)
            return el
        if self.mode == STORE:
            return self.drop_from_store_mode(now, el)
        return self.drop_from_drop_mode(now, el)

    def drop_from_store_mode(self, now, el):
        hit("store_to_drop")
        self.dropped(el, now)
        nxt = self.codel_pop(now)
        self.mode = DROP
        delta = max(self.current_drop_count - self.previous_drop_count, 0)
        if self.was_dropping_recently(now) and delta > 1:
            hit("restart_delta")
            self.current_drop_count = delta
        else:
            self.current_drop_count = 1
        self.drop_next = control_law(now, self.current_drop_count)
        self.previous_drop_count = self.current_drop_count
        return None if nxt is None else nxt[0]

    def drop_from_drop_mode(self, now, el):
        item = (el, True)
        if not self.should_drop(now):
            hit("drop_mode_not_due")
        while item is not None and self.mode == DROP and self.should_drop(now):
            hit("drop_in_drop_mode")
            self.dropped(item[0], now)
            self.current_drop_count += 1
            item = self.codel_pop(now)
            if item is not None and item[1]:
                hit("control_law_chain")
                self.drop_next = control_law(self.drop_next, self.current_drop_count)
            else:
                self._set_mode(STORE)
        return None if item is None else item[0]

    def codel_pop(self, now):
        if not self.elements:
            self.interval_end = None
            return None
        el = self.elements.popleft()
        self.total_bytes_stored = max(self.total_bytes_stored - el[1], 0)
        assert now >= el[0]
        return el, self.process_standing_delay(now, now - el[0])

    def process_standing_delay(self, now, standing_delay):
        if standing_delay < TARGET or self.total_bytes_stored <= MTU:
            self.interval_end = None
            return False
        if self.interval_end is not None:
            return now >= self.interval_end
        self.interval_end = min(now + INTERVAL, U64)
        return False

    def should_drop(self, now):
        return self.drop_next is not None and now >= self.drop_next

    def was_dropping_recently(self, now):
        if self.drop_next is None:
            return False
        return max(now - self.drop_next, 0) < INTERVAL * 16


class Host:
    """One host's router queue + inbound relay."""

    def __init__(self, bw_down_bits, sim_start, bootstrap_end):
        self.out = []
        self.codel = CoDelQueue(lambda el, now: self.out.append((0, now, el[2])))
        self.bucket = None if bw_down_bits == U64 else create_token_bucket(bw_down_bits // 8, sim_start)
        self.bootstrap_end = bootstrap_end
        self.pending = False
        self.wake = 0
        self.wake_from_block = False
        self.next_packet = None
        self.last_time = sim_start

    def run_forward_task(self, now):
        self.pending = False
        self.last_time = now
        while True:
            el = self.next_packet
            self.next_packet = None
            if el is None:
                el = self.codel.pop(now)
            if el is None:
                return
            if now >= self.bootstrap_end:
                if self.bucket is not None:
                    ok, dur = self.bucket.conforming_remove(el[1], now)
                    if not ok:
                        hit("token_block")
                        self.next_packet = el
                        self.pending, self.wake, self.wake_from_block = True, now + dur, True
                        return
            else:
                hit("bootstrap_forward")
            self.out.append((1, now, el[2]))

    def step(self, until, arrivals):
        """arrivals: [(time, size, tag)] in order; returns [(status, time, tag)] in leaving order."""
        self.out = []
        i, n = 0, len(arrivals)
        while True:
            t = arrivals[i][0] if i < n else None
            if self.pending and self.wake < until and (t is None or t > self.wake):
                self.run_forward_task(self.wake)
            elif t is not None:
                if self.pending and self.wake_from_block and t == self.wake:
                    hit("arrival_at_wake")
                self.codel.push(arrivals[i][1], t, arrivals[i][2])
                self.last_time = max(self.last_time, t)
                if not self.pending:
                    self.pending, self.wake, self.wake_from_block = True, t, False
                i += 1
            else:
                break
        if self.pending and self.wake == until:
            hit("wake_at_window_end")
        return self.out

    def state(self):
        c, b = self.codel, self.bucket
        return dict(balance=b.balance if b else 0, last_refill_ns=b.last_refill if b else None, mode=c.mode,
                    has_interval_end=int(c.interval_end is not None), interval_end_ns=c.interval_end or 0,
                    has_drop_next=int(c.drop_next is not None), drop_next_ns=c.drop_next or 0,
                    current_drop_count=c.current_drop_count, previous_drop_count=c.previous_drop_count,
                    bytes_stored=c.total_bytes_stored, queued=len(c), pending=int(self.pending),
                    wake_ns=self.wake if self.pending else 0, has_cached=int(self.next_packet is not None),
                    cached_tag=self.next_packet[2] if self.next_packet is not None else 0)


class Inbound:
    def __init__(self, bw_down_bits, sim_start, bootstrap_end):
        self.sim_start = sim_start
        self.hosts = [Host(int(b), sim_start, bootstrap_end) for b in bw_down_bits]

    def validate(self, until, time, size, offs):
        H, n = len(self.hosts), len(time)
        if until > TIME_END:
            raise InboundRefError(ERR_ARG, "until")
        if len(offs) != H + 1 or offs[0] != 0 or offs[H] != n or any(offs[h] > offs[h + 1] for h in range(H)):
            raise InboundRefError(ERR_ARG, "offsets")
        if any(t < self.sim_start or t >= TIME_END or t >= until for t in time):
            raise InboundRefError(ERR_ARG, "time")
        for h in range(H):
            b = self.hosts[h].bucket  # (not the reference's: such a packet never conforms, the relay spins)
            if b is not None and any(size[j] > b.capacity for j in range(offs[h], offs[h + 1])):
                raise InboundRefError(ERR_ARG, "size")
        for h in range(H):
            prev = self.hosts[h].last_time
            for j in range(offs[h], offs[h + 1]):
                if time[j] < prev:
                    raise InboundRefError(ERR_TIME_BACKWARD, "backward")
                prev = time[j]

    def step(self, until, time, size, tag, offs):
        """Returns (status, time, tag, host_offsets, result) as lists."""
        time, size, tag, offs = [int(x) for x in time], [int(x) for x in size], [int(x) for x in tag], [int(x) for x in offs]
        self.validate(until, time, size, offs)
        st, tm, tg, oo = [], [], [], [0]
        for h, host in enumerate(self.hosts):
            out = host.step(until, [(time[j], size[j], tag[j]) for j in range(offs[h], offs[h + 1])])
            for s, t, g in out:
                st.append(s)
                tm.append(t)
                tg.append(g)
            oo.append(len(st))
        wakes = [h.wake for h in self.hosts if h.pending]
        res = dict(num_forwarded=sum(st), num_dropped=len(st) - sum(st),
                   num_queued=sum(len(h.codel) + (h.next_packet is not None) for h in self.hosts),
                   min_next_wake_ns=min(wakes) if wakes else U64)
        return st, tm, tg, oo, res

    def host_state(self, h):
        return self.hosts[h].state()


# ---- the golden KATs (tests/golden/inbound_kats.json): operation lists ----------------------------
# ["tb_new", capacity, increment, interval_ns, last_refill_ns]   ["tb_remove", decrement, now]
# ["cq_new"]   ["cq_push", count, now] (mock packets of `size` bytes)   ["cq_pop", now]
# ["cq_psd", now, standing_delay]   ["cq_set_mode", mode]   ["cq_probe", now]   ["law", time, count]
# Every operation yields the same record (kat_record; was_dropping_recently and should_drop are
# evaluated at the operation's `now`); an expectation names the fields it pins.
KAT_FIELDS = ("ret", "value", "len", "mode", "cur", "prev", "has_interval_end", "interval_end", "has_drop_next",
              "bytes", "was_dropping_recently", "should_drop")
KAT_OPS = ("tb_new", "tb_remove", "cq_new", "cq_push", "cq_pop", "cq_psd", "cq_set_mode", "law", "cq_probe")


def kat_record(tb, cq, ret, value, now):
    return dict(ret=int(ret), value=int(value), len=len(cq) if cq is not None else 0, mode=cq.mode if cq is not None else 0,
                cur=cq.current_drop_count if cq is not None else 0, prev=cq.previous_drop_count if cq is not None else 0,
                has_interval_end=int(cq.interval_end is not None) if cq is not None else 0,
                interval_end=(cq.interval_end or 0) if cq is not None else 0,
                has_drop_next=int(cq.drop_next is not None) if cq is not None else 0,
                bytes=cq.total_bytes_stored if cq is not None else (tb.balance if tb else 0),
                was_dropping_recently=int(cq.was_dropping_recently(now)) if cq is not None else 0,
                should_drop=int(cq.should_drop(now)) if cq is not None else 0)


def run_kat(ops, packet_size=1500):
    tb = cq = None
    out = []
    for op in ops:
        name, a = op[0], op[1:]
        ret = value = now = 0
        if name == "tb_new":
            tb, cq = TokenBucket(a[0], a[1], a[2], a[3]), None
        elif name == "tb_remove":
            ok, value = tb.conforming_remove(a[0], a[1])
            ret = int(ok)
        elif name == "cq_new":
            cq, tb = CoDelQueue(), None
        elif name == "cq_push":
            now = a[1]
            for _ in range(a[0]):
                cq.push(packet_size, now)
        elif name == "cq_pop":
            now = a[0]
            ret = int(cq.pop(now) is not None)
        elif name == "cq_psd":
            now = a[0]
            ret = int(cq.process_standing_delay(now, a[1]))
        elif name == "cq_set_mode":
            cq.mode = a[0]
        elif name == "cq_probe":
            now = a[0]
        elif name == "law":
            value = control_law(a[0], a[1]) - a[0]
        else:
            raise ValueError(name)
        out.append(kat_record(tb, cq, ret, value, now))
    return out


def kat_lines(records):
    return [" ".join(str(r[k]) for k in KAT_FIELDS) for r in records]


# ---- scenarios -------------------------------------------------------------------------------
def overload_arrivals(seed, t0, tag0=0):
    """The overload scenario's arrivals for one host: two bursts of 300 packets, sizes from
    {40, 576, 1500}, gaps from {0, 0, 0.5, 1, 3} ms, 1 s of silence between the bursts."""
    import random
    rng = random.Random(seed)
    out, t = [], t0
    for burst in range(2):
        for _ in range(300):
            out.append((t, rng.choice((40, 576, 1500)), tag0 + len(out)))
            t += rng.choice((0, 0, 500_000, 1_000_000, 3_000_000))
        t += 1_000_000_000
    return out
