// outbound_rule.h — a host's outbound path, from a socket's offer to Worker::send_packet: the rule
// the outbound step runs on the device (outbound.hip.h), shared with a CPU unit test
// (tests/cpp/outbound_rule_check.cpp, built with g++).  Plain C++, no HIP types.
//
// Reference (src/main/):
//   host/descriptor/socket.c:437-442      a packet of priority 0 enters the control FIFO, any other the data FIFO
//   host/descriptor/socket.c:198-199,466-467   the next packet: the control FIFO's head, else the data FIFO's
//   host.rs:1003-1017                     notify_socket_has_packets: networkinterface_wantsSend, relay_inet_out.notify
//   network_interface.c:344-370           wantsSend: a socket not in the qdisc structure is pushed, one in it is left alone
//   network_interface.c:205-294           the selection step: pop a socket, pull its packet, push it back if it has more
//   network_queuing_disciplines.c:22-160  the round-robin queue; the FIFO heap's comparator (+1 only for pa > pb)
//   utility/priority_queue.c:87-175       entry_smaller, heapify_up, heapify_down, push, pop
//   relay/mod.rs:111-288                  notify / run_forward_task / forward_until_blocked / create_token_bucket
//   relay/token_bucket.rs:68-157          the bucket (inbound_rule.h's inb_lazy_refill / inb_conforming_remove)
//
// Pinned by the reference's own compiled code: the heap (push, pop, both sifts), its comparator and
// the round-robin queue.  oracle/_ref/qdisc_ref is priority_queue.c and network_queuing_disciplines.c
// built from a reference checkout; the scripts it answered are tests/golden/qdisc_reference.json, and
// this header's leaving order on the qdisc_* scenarios equals that program's selection order
// (tests/test_outbound_cpu.py).  Still a restatement, here and in that program's driver: the sockets'
// two FIFOs, wantsSend, the selection loop, the relay and the bucket.
//
// The heap is restated literally.  Its keys are not stored: a compare reads the two sockets' current
// next-packet priority (Q::nprio), so a control packet offered to a socket that already sits in the
// heap changes that socket's key without a re-sift, and `a` is smaller than `b` unless
// prio(a) > prio(b), so equal keys compare as smaller both ways.  heapify_up / heapify_down move one
// entry and compare every other entry against it or against its sibling, which is what the
// reference's chain of swaps does; they are written with the moving entry held aside.
//
// Event order per host.  The offers come in execution order with non-decreasing times.  Before offer
// i at time t is enqueued, every pending forward task with wake < t runs, and one with wake == t runs
// first iff the offer carries OUT_OFFER_BARRIER (in the reference the order of a task and another
// local event of the same nanosecond is by event id, which only the caller knows).  After the last
// offer every task with time < until runs; one at exactly `until` stays pending.
// The task at `now` loops: the cached packet, else the selection step; none -> Idle; at
// now >= bootstrap_end a non-local packet of a limited host removes `size` tokens, and on failure
// the packet is cached and the task is scheduled again at now + duration; else the packet leaves at
// `now` (status 1: Router::push = Worker::send_packet at `now`; status 2: a local packet, pushed back
// into the interface).  A cached packet is never local (only a failed removal caches).
//
// Domain: sim_start <= every time < 2^62 (INB_TIME_END), sizes are u32, until <= 2^62.  In it plain
// u64 arithmetic is what the reference's saturating / checked operations give:
//   * every `now` is an offer time or a wake time below `until`, so now < 2^62;
//   * now - last_refill: last_refill only moves to a refill boundary <= now, and a host's `now`
//     never decreases -- offers are validated against the host's last processed time, a task runs
//     at wake <= the next offer's time, and a blocked task's next wake is strictly later;
//   * lazy_refill's product and sums, compute_conforming_duration: as derived in inbound_rule.h
//     (the same two functions run here, on the same bucket shape: 1 ms interval,
//     max(1, bw_up / 8 / 1000) per refill, capacity refill + 1500 < 2^64, created full);
//   * now + duration: a non-local packet above a limited host's capacity is refused before the
//     step, so a failed removal needs at most capacity / refill + 1 <= 1501 refills: < 2^62 + 2^41;
//   * a host's packet count and every index into its packets are below 2^32 (checked per step);
//   * the heap's (index - 1) / 2 and 2 * index + 1 are on indices below the host's socket count,
//     a u32, held in u32 with 2 * index + 1 formed only for index < 2^31 (checked at creation);
//   * the per-host priority counter (host.rs:714-719) is the caller's: any u64 is a valid key, and
//     equal non-zero keys are ordered as the heap orders them.
#pragma once
#include "inbound_rule.h"

namespace srg {

constexpr int OUT_QDISC_FIFO = 0, OUT_QDISC_ROUND_ROBIN = 1;
constexpr uint8_t OUT_OFFER_LOCAL = 1, OUT_OFFER_BARRIER = 2;
constexpr uint32_t OUT_NIL = 0xffffffffu;

// The resident per-host record (one per host, in HBM on the device).  The qdisc structure's array
// (the heap, or the round-robin ring starting at rr_head) and the sockets' FIFOs live beside it.
struct OutHost {
    uint64_t balance, last_refill;  // TokenBucket
    uint64_t wake, cached_tag;      // relay: Pending's task time, next_packet
    uint64_t last_time;             // the host's last processed event (offer or task)
    uint32_t cached_size;
    uint32_t qlen;     // sockets in the qdisc structure
    uint32_t rr_head;  // round robin: the ring's head position
    uint32_t queued;   // packets in the sockets' FIFOs (the cached one is not)
    uint8_t pending, has_cached, pad[6];
};

SRG_INB_HD inline void out_host_init(OutHost& s, uint64_t refill_increment, uint64_t sim_start_ns) {
    s = OutHost{};
    s.balance = refill_increment ? refill_increment + INB_MTU : 0;
    s.last_refill = sim_start_ns;
    s.last_time = sim_start_ns;
}

// A queue type Q gives the rule its sockets and offers:
//   uint32_t ord_get(uint32_t i); void ord_set(uint32_t i, uint32_t slot)   the qdisc structure's array
//   uint64_t nprio(uint32_t slot)              the socket's current next-packet priority
//   bool has_offer(); uint64_t offer_time(); uint8_t offer_flags()          the next offer not yet enqueued
//   bool push_offer(uint32_t& slot)            append it to its socket; true: the socket was empty
//   bool pull(uint32_t slot, uint32_t& size, uint8_t& flags)   take the socket's next packet; true: it has more
//   void leave(uint8_t status, uint64_t now)   the last pulled packet leaves
//   void cache_last()                          the last pulled packet becomes the relay's cached packet
//   void leave_cached(uint64_t now)            the relay's cached packet leaves (status 1)

// priority_queue.c:87-89 with network_queuing_disciplines.c:82-94
SRG_INB_HD inline bool out_key_smaller(uint64_t pa, uint64_t pb) { return !(pa > pb); }

// priority_queue.c:91-97; the entry `slot` (key pk) moves up from `index`
template <class Q>
SRG_INB_HD inline void out_heapify_up(Q& q, uint32_t index, uint32_t slot, uint64_t pk) {
    while (index > 0) {
        const uint32_t parent = (index - 1) / 2;
        const uint32_t ps = q.ord_get(parent);
        if (!out_key_smaller(pk, q.nprio(ps))) break;
        q.ord_set(index, ps);
        index = parent;
    }
    q.ord_set(index, slot);
}

// priority_queue.c:99-113; the entry `slot` (key pk) moves down from `index` in a heap of `size`
template <class Q>
SRG_INB_HD inline void out_heapify_down(Q& q, uint32_t size, uint32_t index, uint32_t slot, uint64_t pk) {
    for (;;) {
        uint32_t child = 2 * index + 1;
        if (child >= size) break;
        uint32_t cs = q.ord_get(child);
        uint64_t ck = q.nprio(cs);
        if (child + 1 < size) {
            const uint32_t rs = q.ord_get(child + 1);
            const uint64_t rk = q.nprio(rs);
            if (out_key_smaller(rk, ck)) {
                child = child + 1;
                cs = rs;
                ck = rk;
            }
        }
        if (!out_key_smaller(ck, pk)) break;
        q.ord_set(index, cs);
        index = child;
    }
    q.ord_set(index, slot);
}

// priority_queue.c:133-137 / rrsocketqueue_push; cap: the host's socket count (the ring's size)
template <class Q>
SRG_INB_HD inline void out_qdisc_push(OutHost& s, Q& q, int qdisc, uint32_t cap, uint32_t slot) {
    if (qdisc == OUT_QDISC_FIFO) {
        out_heapify_up(q, s.qlen, slot, q.nprio(slot));
    } else {
        uint32_t tail = s.rr_head + s.qlen;  // both below cap <= 2^31
        if (tail >= cap) tail -= cap;
        q.ord_set(tail, slot);
    }
    ++s.qlen;
}

// priority_queue.c:156-163 / rrsocketqueue_pop; s.qlen > 0
template <class Q>
SRG_INB_HD inline uint32_t out_qdisc_pop(OutHost& s, Q& q, int qdisc, uint32_t cap) {
    uint32_t slot;
    if (qdisc == OUT_QDISC_FIFO) {
        slot = q.ord_get(0);
        --s.qlen;  // swap(0, size - 1), shrink, heapify_down(0)
        if (s.qlen > 0) {
            const uint32_t last = q.ord_get(s.qlen);
            out_heapify_down(q, s.qlen, 0, last, q.nprio(last));
        }
    } else {
        slot = q.ord_get(s.rr_head);
        s.rr_head = s.rr_head + 1 == cap ? 0 : s.rr_head + 1;
        --s.qlen;
    }
    return slot;
}

// network_interface.c:205-294: the selection step (a socket in the structure always has a packet)
template <class Q>
SRG_INB_HD inline bool out_interface_pop(OutHost& s, Q& q, int qdisc, uint32_t cap, uint32_t& size, uint8_t& flags) {
    if (s.qlen == 0) return false;
    const uint32_t slot = out_qdisc_pop(s, q, qdisc, cap);
    const bool more = q.pull(slot, size, flags);
    --s.queued;
    if (more) out_qdisc_push(s, q, qdisc, cap, slot);
    return true;
}

// relay/mod.rs:166-273: the forward task at `now`.  inc == 0: no bucket.
template <class Q>
SRG_INB_HD inline void out_run_task(OutHost& s, uint64_t inc, Q& q, int qdisc, uint32_t cap, uint64_t now,
                                    uint64_t bootstrap_end_ns) {
    s.pending = 0;
    s.last_time = now;
    for (;;) {
        uint32_t size = 0;
        uint8_t flags = 0;
        const bool from_cache = s.has_cached != 0;
        if (from_cache) {
            size = s.cached_size;
            s.has_cached = 0;
        } else if (!out_interface_pop(s, q, qdisc, cap, size, flags)) {
            return;  // Idle
        }
        const bool local = (flags & OUT_OFFER_LOCAL) != 0;
        if (now >= bootstrap_end_ns && !local && inc != 0) {
            uint64_t dur = 0;
            if (!inb_conforming_remove(inc + INB_MTU, inc, INB_REFILL_NS, s.balance, s.last_refill, size, now, &dur)) {
                if (!from_cache) q.cache_last();  // (the queue fills in cached_tag)
                s.has_cached = 1;
                s.cached_size = size;
                s.pending = 1;
                s.wake = now + dur;
                return;
            }
        }
        if (from_cache) q.leave_cached(now);
        else q.leave(local ? 2 : 1, now);
    }
}

// host.rs:1003-1017: the next offer enters its socket, the socket the qdisc structure, the relay is notified
template <class Q>
SRG_INB_HD inline void out_offer(OutHost& s, Q& q, int qdisc, uint32_t cap, uint64_t t) {
    uint32_t slot = 0;
    const bool was_empty = q.push_offer(slot);
    ++s.queued;
    if (was_empty) out_qdisc_push(s, q, qdisc, cap, slot);
    if (!s.pending) {  // notify() on Idle: forward_later(ZERO)
        s.pending = 1;
        s.wake = t;
    }
    s.last_time = t > s.last_time ? t : s.last_time;
}

// One host's slice of a step: every offer the queue holds and every task with time < until_ns.
template <class Q>
SRG_INB_HD inline void out_host_step(OutHost& s, uint64_t inc, Q& q, int qdisc, uint32_t cap, uint64_t until_ns,
                                     uint64_t bootstrap_end_ns) {
    while (q.has_offer()) {
        const uint64_t t = q.offer_time();
        const bool barrier = (q.offer_flags() & OUT_OFFER_BARRIER) != 0;
        while (s.pending && (s.wake < t || (s.wake == t && barrier)))
            out_run_task(s, inc, q, qdisc, cap, s.wake, bootstrap_end_ns);
        out_offer(s, q, qdisc, cap, t);
    }
    while (s.pending && s.wake < until_ns) out_run_task(s, inc, q, qdisc, cap, s.wake, bootstrap_end_ns);
}

}  // namespace srg
