"""Plain-Python restatement of a round (shadow_amd/csrc/round_rule.h, srg_round_*): the per-host
Xoshiro256++ generator seeded through SplitMix64 (host.rs:122,233), which leaving packets draw
(worker.rs:336-377), where the event id is taken (worker.rs:422 -> event.rs:27: behind the drop
return), and a Round that composes inbound_ref.Inbound, outbound_ref.Outbound, one heapq per host
(event_queue.rs:10-55) and send_packet's arithmetic (worker.rs:374-424).  Python ints throughout;
the f32 subtraction of the reliability goes through numpy.float32."""
import copy
import heapq

import numpy as np

import inbound_ref as IR
import outbound_ref as OR

M64 = 2**64 - 1
U64 = M64
NO_HOST = 0xFFFFFFFF
DROPPED, SENT, LOCAL, AFTER_END, NO_DST = 0, 1, 2, 3, 4
ERR_ARG, ERR_TIME_BACKWARD = 1, 12
MTU = 1500


def rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & M64


class Xoshiro256PlusPlus:
    def __init__(self, words):
        self.s = [int(w) & M64 for w in words]

    @classmethod
    def seed_from_u64(cls, seed):
        x, out = int(seed) & M64, []
        for _ in range(4):  # SplitMix64
            x = (x + 0x9E3779B97F4A7C15) & M64
            z = x
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
            out.append(z ^ (z >> 31))
        return cls(out)

    def next_u64(self):
        s = self.s
        r = (rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = rotl(s[3], 45)
        return r

    def gen_f64(self):  # rand 0.8.5 Standard: 53 bits, exact
        return (self.next_u64() >> 11) * (1.0 / (1 << 53))


def classify(out_status, leave_ns, dst_host, sim_end):
    """-> LOCAL, AFTER_END, NO_DST, or SENT for "draws"."""
    if out_status != 1:
        return LOCAL
    if leave_ns >= sim_end:
        return AFTER_END
    if dst_host == NO_HOST:
        return NO_DST
    return SENT


def dropped(loss, chance, payload, send_ns, bootstrap_end):
    """worker.rs:382: !is_bootstrapping && chance >= reliability && payload_size > 0."""
    reliability = float(np.float32(1) - np.float32(loss))
    return send_ns >= bootstrap_end and chance >= reliability and payload > 0


def draw_host(rng, next_event_id, packets, have_loss, bootstrap_end, sim_end):
    """One host's leaving packets in leaving order: [(out_status, leave_ns, dst_host, loss, payload)]
    -> ([(status, chance or None, event_id or None)], next_event_id)."""
    out = []
    for st, t, dst, loss, payload in packets:
        c = classify(st, t, dst, sim_end)
        if c != SENT:
            out.append((c, None, None))
            continue
        chance = rng.gen_f64()
        if have_loss and dropped(loss, chance, payload, t, bootstrap_end):
            out.append((DROPPED, chance, None))
            continue
        out.append((SENT, chance, next_event_id))
        next_event_id += 1
    return out, next_event_id


class RoundRefError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class Round:
    def __init__(self, host_node, lat, loss, bw_up, bw_down, sockets, qdisc, node_seed, sim_start, bootstrap_end, sim_end):
        self.H = len(host_node)
        self.host_node = [int(x) for x in host_node]
        self.lat, self.loss = lat, loss  # [tn][tn] ints; f32 array or None
        self.boot, self.sim_end = bootstrap_end, sim_end
        self.inb = IR.Inbound(bw_down, sim_start, bootstrap_end)
        self.out = OR.Outbound(bw_up, sockets, qdisc, sim_start, bootstrap_end)
        self.q = [[] for _ in range(self.H)]
        self.last_popped = [0] * self.H
        self.rng = [Xoshiro256PlusPlus.seed_from_u64(s) for s in node_seed]
        self.next_eid = [0] * self.H
        self.dst, self.size, self.payload = [], [], []

    def set_packets(self, dst, size, payload):
        """Lists indexed by tag, kept by reference (the caller appends)."""
        self.dst, self.size, self.payload = dst, size, payload

    def _minima(self):
        wakes = [h.wake for h in self.out.hosts if h.pending]
        iw = [h.wake for h in self.inb.hosts if h.pending]
        m = dict(min_next_event_ns=min((x[0][0] for x in self.q if x), default=U64),
                 min_inbound_wake_ns=min(iw, default=U64), min_outbound_wake_ns=min(wakes, default=U64),
                 num_queued_events=sum(len(x) for x in self.q))
        m["next_start_ns"] = min(m["min_next_event_ns"], m["min_inbound_wake_ns"], m["min_outbound_wake_ns"])
        return m

    def _state(self):
        return (self.inb, self.out, self.q, self.last_popped, self.rng, self.next_eid)

    def _restore(self, saved):
        self.inb, self.out, self.q, self.last_popped, self.rng, self.next_eid = saved

    def receive(self, until):
        saved = copy.deepcopy(self._state())
        try:
            return self._receive(until)
        except Exception:
            self._restore(saved)
            raise

    def _receive(self, until):
        t, g, off = [], [], [0]
        for h in range(self.H):
            while self.q[h] and self.q[h][0][0] < until:  # host.rs:809-818
                e = heapq.heappop(self.q[h])
                self.last_popped[h] = e[0]
                t.append(e[0])
                g.append(e[3])
            off.append(len(t))
        size = [self.size[x] for x in g]
        try:
            st, tm, tg, oo, res = self.inb.step(until, t, size, g, off)
        except IR.InboundRefError as e:
            raise RoundRefError(e.code, str(e))
        d = dict(num_popped=len(t), popped_time=t, popped_tag=g, popped_host_offsets=off, num_leaving=len(st), status=st,
                 time=tm, tag=tg, host_offsets=oo, num_forwarded=res["num_forwarded"], num_dropped=res["num_dropped"],
                 num_queued_inbound=res["num_queued"])
        d.update(self._minima())
        return d

    def send(self, until, time, slot, prio, flags, tag, offs):
        saved = copy.deepcopy(self._state())
        try:
            return self._send(until, time, slot, prio, flags, tag, offs)
        except Exception:
            self._restore(saved)
            raise

    def _send(self, until, time, slot, prio, flags, tag, offs):
        H, n = self.H, len(time)
        flags = [0] * n if flags is None else [int(f) for f in flags]
        tag, offs = [int(x) for x in tag], [int(x) for x in offs]
        if len(offs) != H + 1 or offs[0] != 0 or offs[H] != n or any(offs[h] > offs[h + 1] for h in range(H)):
            raise RoundRefError(ERR_ARG, "offsets")
        if any(g >= len(self.dst) for g in tag):
            raise RoundRefError(ERR_ARG, "tag")
        if any(self.dst[g] >= H and self.dst[g] != NO_HOST for g in tag):
            raise RoundRefError(ERR_ARG, "dst_host")
        if any(f & ~OR.OFFER_BARRIER for f in flags):
            raise RoundRefError(ERR_ARG, "flags")
        size, fl = [], []
        for h in range(H):
            for j in range(offs[h], offs[h + 1]):
                d, s = self.dst[tag[j]], self.size[tag[j]]
                local = d == h
                if not local and d != NO_HOST:
                    b = self.inb.hosts[d].bucket
                    if b is not None and s > b.capacity:
                        raise RoundRefError(ERR_ARG, "size above the destination's bucket")
                size.append(s)
                fl.append(flags[j] | (OR.OFFER_LOCAL if local else 0))
        try:
            o_st, o_tm, o_tg, o_off, o_res = self.out.step(until, time, slot, prio, size, fl, tag, offs)
        except OR.OutboundRefError as e:
            raise RoundRefError(e.code, str(e))
        status, used = [], []
        for h in range(H):
            a = self.host_node[h]
            pk = []
            for j in range(o_off[h], o_off[h + 1]):
                d = self.dst[o_tg[j]]
                ls = float(self.loss[a][self.host_node[d]]) if self.loss is not None and d < H else 0.0
                pk.append((o_st[j], o_tm[j], d, ls, self.payload[o_tg[j]]))
            res, self.next_eid[h] = draw_host(self.rng[h], self.next_eid[h], pk, self.loss is not None, self.boot,
                                              self.sim_end)
            for j, (c, _, eid) in zip(range(o_off[h], o_off[h + 1]), res):
                status.append(c)
                if c != SENT:
                    continue
                d = self.dst[o_tg[j]]
                delay = int(self.lat[a][self.host_node[d]])
                deliver = max(o_tm[j] + delay, until)  # worker.rs:411-414
                if deliver < self.last_popped[d]:  # event_queue.rs:33
                    raise RoundRefError(ERR_TIME_BACKWARD, "push before the last popped event")
                used.append(delay)
                heapq.heappush(self.q[d], (deliver, h, eid, o_tg[j]))
        d = dict(num_leaving=len(status), status=status, time=o_tm, tag=o_tg, host_offsets=o_off,
                 num_sent=status.count(SENT), num_dropped=status.count(DROPPED), num_local=status.count(LOCAL),
                 num_after_end=status.count(AFTER_END), num_no_host=status.count(NO_DST),
                 num_queued_outbound=o_res["num_queued"], min_used_latency_ns=min(used, default=U64))
        d.update(self._minima())
        return d

    def host_rng(self, h):
        return list(self.rng[h].s), self.next_eid[h]

    def set_host_rng(self, h, words, next_event_id):
        self.rng[h] = Xoshiro256PlusPlus(words)
        self.next_eid[h] = int(next_event_id)
