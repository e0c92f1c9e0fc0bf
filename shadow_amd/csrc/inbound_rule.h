// inbound_rule.h — a host's inbound path, from the router's queue to the point where the host's
// interface takes over: the rule the inbound step runs on the device (inbound.hip.h), shared with a
// CPU unit test (tests/cpp/inbound_rule_check.cpp, built with g++).  Plain C++, no HIP types.
//
// Reference (src/main/):
//   host.rs:853-858              route_incoming_packet(packet); notify_router_has_packets()
//   router/mod.rs:59-61          -> CoDelQueue::push(packet, now)
//   router/codel_queue.rs:125-319   pop / drop_from_store_mode / drop_from_drop_mode / codel_pop /
//                                process_standing_delay / should_drop / was_dropping_recently /
//                                apply_control_law / push
//   relay/mod.rs:111-273         notify / forward_later / run_forward_task / forward_until_blocked
//   relay/mod.rs:278-288         create_token_bucket: 1 ms interval, max(1, bytes/1000) per refill,
//                                capacity = refill + CONFIG_MTU
//   relay/token_bucket.rs:68-157 conforming_remove_inner / compute_conforming_duration / lazy_refill
//   core/work/event.rs:103-110   at equal time a packet event runs before a local event (the task)
//
// Event order per host.  An arrival at t is pushed with enqueue_ts = t; if the relay is Idle a
// forward task is scheduled at t.  A task at T runs after every arrival with time <= T.  The task
// loops: the cached packet, else CoDel::pop(T); none -> Idle; at T >= bootstrap_end a limited host
// removes `size` tokens, and on failure the packet is cached and the task is scheduled again at
// T + duration; else the packet is forwarded at T.  is_local is never true on this path (the
// router's address is UNSPECIFIED).  Before bootstrap_end the bucket is not touched, not refilled.
//
// Domain: sim_start <= every time < 2^62 (INB_TIME_END), sizes are u32, until <= 2^62.  In it plain
// u64 arithmetic is what the reference's saturating / checked operations give:
//   * every `now` is an arrival time or a wake time below `until`, so now < 2^62;
//   * now - enqueue_ts, now - last_refill, now - drop_next (guarded by now >= drop_next, as
//     saturating_duration_since gives 0 below it): the subtrahend is never the larger one --
//     enqueue_ts <= now because a task runs after the arrivals up to it, last_refill only moves to
//     a refill boundary <= now, and a host's `now` never decreases (validated per step);
//   * now + INTERVAL, drop_next + increment (increment <= 1e8, and the chain only advances while
//     drop_next <= now): below 2^62 + 2e8;
//   * total_bytes_stored: a sum of u32 sizes of fewer than 2^64 / 2^32 stored packets; its
//     saturating_sub subtracts a stored packet's own size;
//   * lazy_refill: refill_increment * num_refills can exceed u64 (num_refills < 2^62 / 1e6), where
//     the reference saturates and then clamps to the capacity.  min(capacity, balance + product) is
//     the exact value either way, so it is computed without forming the product (inb_lazy_refill);
//     last_refill + interval * num_refills <= now;
//   * compute_conforming_duration: at most 2^32 refills of 1 ms on top of a span <= 1 ms: < 2^53;
//     a failed checked_sub means decrement > balance, so at least one refill is required and the
//     duration is >= 1 ns: the next task is strictly later;
//   * capacity = bw / 8 / 1000 + 1500 < 2^64; bw == UINT64_MAX is RateLimit::Unlimited;
//   * Option::unwrap on drop_next (drop_from_drop_mode): Drop mode is only entered by
//     drop_from_store_mode, which sets it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SRG_INB_HD __host__ __device__
#else
#define SRG_INB_HD
#endif
#include <math.h>

namespace srg {

constexpr uint64_t INB_TARGET_NS = 10000000ull;     // codel_queue.rs:23
constexpr uint64_t INB_INTERVAL_NS = 100000000ull;  // codel_queue.rs:28
constexpr uint64_t INB_MTU = 1500;                  // CONFIG_MTU
constexpr uint64_t INB_REFILL_NS = 1000000ull;      // relay/mod.rs:279
constexpr uint64_t INB_TIME_END = 1ull << 62;
constexpr uint32_t INB_STORE = 0, INB_DROP = 1;

// The resident per-host state (one record per host, in HBM on the device).
struct InbHost {
    uint64_t balance, last_refill;  // TokenBucket
    uint64_t interval_end, drop_next;
    uint64_t cur_drops, prev_drops, bytes;  // CoDelQueue
    uint64_t wake, cached_tag;              // relay: Pending's task time, next_packet
    uint64_t last_time;                     // the host's last processed event (arrival or task)
    uint32_t cached_size;
    uint8_t mode, has_interval_end, has_drop_next, pending;
    uint8_t has_cached, pad[7];
};

// relay/mod.rs:280; 0 stands for RateLimit::Unlimited (no bucket)
SRG_INB_HD inline uint64_t inb_refill_increment(uint64_t bw_down_bits) {
    if (bw_down_bits == UINT64_MAX) return 0;
    const uint64_t v = bw_down_bits / 8 / 1000;
    return v ? v : 1;
}

SRG_INB_HD inline void inb_host_init(InbHost& s, uint64_t refill_increment, uint64_t sim_start_ns) {
    s = InbHost{};
    s.balance = refill_increment ? refill_increment + INB_MTU : 0;
    s.last_refill = sim_start_ns;
    s.last_time = sim_start_ns;
}

// token_bucket.rs:127-157; returns the span to the next refill
SRG_INB_HD inline uint64_t inb_lazy_refill(uint64_t capacity, uint64_t inc, uint64_t interval, uint64_t& balance,
                                           uint64_t& last_refill, uint64_t now) {
    uint64_t span = now - last_refill;
    if (span >= interval) {
        const uint64_t num_refills = span / interval;
        const uint64_t room = capacity > balance ? capacity - balance : 0;
        // min(capacity, balance + inc * num_refills) with no product formed (see the domain note)
        if (num_refills > room / inc) balance = capacity;
        else balance += inc * num_refills;
        if (balance > capacity) balance = capacity;  // clamp(0, capacity)
        last_refill += interval * num_refills;
        span = now - last_refill;
    }
    return interval - span;
}

// token_bucket.rs:75-120; true = removed; false = *dur is the conforming duration
SRG_INB_HD inline bool inb_conforming_remove(uint64_t capacity, uint64_t inc, uint64_t interval, uint64_t& balance,
                                             uint64_t& last_refill, uint64_t decrement, uint64_t now, uint64_t* dur) {
    const uint64_t next_span = inb_lazy_refill(capacity, inc, interval, balance, last_refill, now);
    if (balance >= decrement) {
        balance -= decrement;
        return true;
    }
    const uint64_t required = decrement - balance;
    const uint64_t refills = required / inc + (required % inc ? 1 : 0);
    *dur = refills == 0 ? 0 : refills == 1 ? next_span : next_span + interval * (refills - 1);
    return false;
}

// codel_queue.rs:287-300: f64 sqrt, f64 divide, round half away from zero; count 0 as 1
SRG_INB_HD inline uint64_t inb_control_increment(uint64_t count) {
    const double sq = count == 0 ? 1.0 : sqrt((double)count);
    const double div = 100000000.0 / sq;
    return (uint64_t)round(div);
}
SRG_INB_HD inline uint64_t inb_control_law(uint64_t time, uint64_t count) { return time + inb_control_increment(count); }

// codel_queue.rs:233-264 (bytes: total_bytes_stored after the popped packet's were subtracted)
SRG_INB_HD inline bool inb_process_standing_delay(InbHost& s, uint64_t now, uint64_t standing_delay) {
    if (standing_delay < INB_TARGET_NS || s.bytes <= INB_MTU) {
        s.has_interval_end = 0;
        s.interval_end = 0;
        return false;
    }
    if (s.has_interval_end) return now >= s.interval_end;
    s.has_interval_end = 1;
    s.interval_end = now + INB_INTERVAL_NS;
    return false;
}

SRG_INB_HD inline bool inb_should_drop(const InbHost& s, uint64_t now) { return s.has_drop_next && now >= s.drop_next; }

SRG_INB_HD inline bool inb_was_dropping_recently(const InbHost& s, uint64_t now) {
    if (!s.has_drop_next) return false;
    const uint64_t since = now >= s.drop_next ? now - s.drop_next : 0;
    return since < INB_INTERVAL_NS * 16;
}

// A queue type Q gives the rule its packets:
//   bool pop_front(uint64_t& enqueue_ts, uint32_t& size)   false: empty
//   void leave(uint8_t status, uint64_t now)               the last popped packet leaves (0 dropped, 1 forwarded)
//   void leave_cached(uint8_t status, uint64_t now)        the relay's cached packet leaves
//   bool has_arrival(); uint64_t next_arrival_time()       arrivals not yet enqueued
//   void enqueue_upto(uint64_t t, InbHost& s)              push every arrival with time <= t (bytes, last_time)

// codel_queue.rs:205-229
template <class Q>
SRG_INB_HD inline bool inb_codel_pop_item(InbHost& s, Q& q, uint64_t now, bool& ok_to_drop, uint32_t& size) {
    uint64_t ts;
    if (!q.pop_front(ts, size)) {
        s.has_interval_end = 0;
        s.interval_end = 0;
        return false;
    }
    s.bytes -= size;
    ok_to_drop = inb_process_standing_delay(s, now, now - ts);
    return true;
}

// codel_queue.rs:151-171
template <class Q>
SRG_INB_HD inline bool inb_drop_from_store_mode(InbHost& s, Q& q, uint64_t now, uint32_t& size) {
    q.leave(0, now);
    bool ok;
    const bool has = inb_codel_pop_item(s, q, now, ok, size);
    s.mode = INB_DROP;
    const uint64_t delta = s.cur_drops > s.prev_drops ? s.cur_drops - s.prev_drops : 0;
    s.cur_drops = inb_was_dropping_recently(s, now) && delta > 1 ? delta : 1;
    s.drop_next = inb_control_law(now, s.cur_drops);
    s.has_drop_next = 1;
    s.prev_drops = s.cur_drops;
    return has;
}

// codel_queue.rs:173-202
template <class Q>
SRG_INB_HD inline bool inb_drop_from_drop_mode(InbHost& s, Q& q, uint64_t now, uint32_t& size) {
    bool has = true;
    while (has && s.mode == INB_DROP && inb_should_drop(s, now)) {
        q.leave(0, now);
        s.cur_drops += 1;
        bool ok = false;
        has = inb_codel_pop_item(s, q, now, ok, size);
        if (has && ok) s.drop_next = inb_control_law(s.drop_next, s.cur_drops);
        else s.mode = INB_STORE;
    }
    return has;
}

// codel_queue.rs:125-149
template <class Q>
SRG_INB_HD inline bool inb_codel_pop(InbHost& s, Q& q, uint64_t now, uint32_t& size) {
    bool ok = false;
    if (!inb_codel_pop_item(s, q, now, ok, size)) {
        s.mode = INB_STORE;
        return false;
    }
    if (!ok) {
        s.mode = INB_STORE;
        return true;
    }
    return s.mode == INB_STORE ? inb_drop_from_store_mode(s, q, now, size) : inb_drop_from_drop_mode(s, q, now, size);
}

// relay/mod.rs:166-273: the forward task at `now`.  inc == 0: no bucket.
template <class Q>
SRG_INB_HD inline void inb_run_task(InbHost& s, uint64_t inc, Q& q, uint64_t now, uint64_t bootstrap_end_ns) {
    s.pending = 0;
    s.last_time = now;
    for (;;) {
        uint32_t size = 0;
        const bool from_cache = s.has_cached != 0;
        if (from_cache) {
            size = s.cached_size;
            s.has_cached = 0;
        } else if (!inb_codel_pop(s, q, now, size)) {
            return;  // Idle
        }
        if (now >= bootstrap_end_ns && inc != 0) {
            uint64_t dur = 0;
            if (!inb_conforming_remove(inc + INB_MTU, inc, INB_REFILL_NS, s.balance, s.last_refill, size, now, &dur)) {
                s.has_cached = 1;  // (a packet just popped: the queue fills in cached_tag)
                s.cached_size = size;
                s.pending = 1;
                s.wake = now + dur;
                return;
            }
        }
        if (from_cache) q.leave_cached(1, now);
        else q.leave(1, now);
    }
}

// One host's slice of a step: every arrival the queue holds and every task with time < until_ns.
template <class Q>
SRG_INB_HD inline void inb_host_step(InbHost& s, uint64_t inc, Q& q, uint64_t until_ns, uint64_t bootstrap_end_ns) {
    for (;;) {
        if (!s.pending) {
            if (!q.has_arrival()) break;
            s.pending = 1;  // notify() on Idle: forward_later(ZERO)
            s.wake = q.next_arrival_time();
        }
        if (s.wake >= until_ns) {  // the task stays pending; the arrivals (all < until) only enqueue
            q.enqueue_upto(UINT64_MAX, s);
            break;
        }
        q.enqueue_upto(s.wake, s);
        inb_run_task(s, inc, q, s.wake, bootstrap_end_ns);
    }
}

}  // namespace srg
