// round_rule.h — what joins the outbound step to Worker::send_packet inside a round: the per-host
// random generator, which leaving packets draw from it, and the per-host event-id counter.  The rule
// the round kernels run on the device (round.hip.h), shared with a CPU unit test
// (tests/cpp/round_rule_check.cpp, built with g++).  Plain C++, no HIP types.
//
// Reference (src/main/):
//   host/host.rs:122,233      random: Xoshiro256PlusPlus::seed_from_u64(params.node_seed) (rand_xoshiro 0.6.0)
//   host/host.rs:258,690-694  event_id_counter starts at 0; get_new_event_id returns it and adds 1
//   core/worker.rs:336-343    is_completed (current_time >= sim_end_time): return, nothing drawn
//   core/worker.rs:352-368    the destination resolves to no host: PDS_INET_DROPPED, return, nothing drawn
//   core/worker.rs:377        chance = src_host.random_mut().gen::<f64>(): one draw per remaining packet,
//                             during bootstrap and for payload size 0 as well
//   core/worker.rs:382-390    the drop decision (send_rule.h), return
//   core/worker.rs:422, 644-654, core/work/event.rs:18-31
//                             push_packet_to_host -> Event::new_packet -> src_host.get_new_event_id()
//
// The generator, written from its published definition (Blackman & Vigna, xoshiro256++ 1.0):
//   next:  r = rotl(s0 + s3, 23) + s0; t = s1 << 17; s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3; s2 ^= t;
//          s3 = rotl(s3, 45)
//   seed_from_u64: the four words are four consecutive SplitMix64 outputs from x = seed
//          (x += 0x9e3779b97f4a7c15; z = x; z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9;
//           z = (z ^ z >> 27) * 0x94d049bb133111eb; out = z ^ z >> 31)
//   gen::<f64>() (rand 0.8.5, Standard): (next_u64() >> 11) * 2^-53, one step per draw.  The shifted
//          value has 53 bits, so the conversion and the product by a power of two are both exact.
// Every other draw from the same generator (next_u32, fill_bytes per 8 bytes) is whole steps too, so
// a caller folds its host's other draws in by stepping the state words between two calls
// (srg_round_host_rng / srg_round_set_host_rng).
//
// Which packets draw.  A packet that leaves the outbound step with status 2 (local) never reaches
// send_packet.  One with status 1 is, in this order: after the end (leave time >= sim_end_ns: no
// draw, no id), without a host (dst_host == ROUND_NO_HOST: no draw, no id), else it draws exactly
// one chance -- whatever its payload and whether or not the time is before bootstrap_end_ns.
//
// Event ids.  The id is taken where the reference takes it: Event::new_packet runs inside
// push_packet_to_host (worker.rs:422), which is behind the drop return (worker.rs:389).  So a packet
// dropped by loss draws but takes NO id; only a sent packet takes next_event_id[h]++ of its source
// host, in the host's leaving order.  (Dropped packets could take one without changing any pop
// order; they do not, so that the counter equals the reference's for a host that has no local
// events.)
//   Why a counter of packet events alone gives the reference's pop order although get_new_event_id
// is shared with the host's local events (event.rs:41): the queue key is (time, src_host_id,
// src_host_event_id) (event.rs:84-155).  The id is reached only between two events equal in time and
// source host, so ids are only ever compared between events of one source host.  The reference's
// ids of one host's packet events strictly increase in the order of its send_packet calls (the
// counter only grows, local events in between only widen the gaps); this counter strictly increases
// in the same order.  Two strictly increasing assignments over the same sequence order every pair
// alike.  A caller that wants the reference's very values adds its local events' ids through
// srg_round_set_host_rng between two calls.
#pragma once
#include <stdint.h>

#include "send_rule.h"

#if defined(__HIPCC__)
#define SRG_ROUND_HD __host__ __device__
#else
#define SRG_ROUND_HD
#endif

namespace srg {

constexpr uint32_t ROUND_NO_HOST = 0xffffffffu;  // a destination address no host owns
// a leaving packet's status in a round's send half
constexpr uint8_t ROUND_DROPPED = 0;    // drew, dropped by loss (PDS_INET_DROPPED)
constexpr uint8_t ROUND_SENT = 1;       // drew, took an event id, entered the destination's queue
constexpr uint8_t ROUND_LOCAL = 2;      // the outbound step's status 2: never reaches send_packet
constexpr uint8_t ROUND_AFTER_END = 3;  // leave time >= sim_end_ns: no draw, no id
constexpr uint8_t ROUND_NO_DST = 4;     // the destination resolves to no host: no draw, no id

struct RoundRng {
    uint64_t s[4];
};

SRG_ROUND_HD inline uint64_t round_rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }

SRG_ROUND_HD inline uint64_t round_next_u64(RoundRng& g) {
    const uint64_t r = round_rotl(g.s[0] + g.s[3], 23) + g.s[0];
    const uint64_t t = g.s[1] << 17;
    g.s[2] ^= g.s[0];
    g.s[3] ^= g.s[1];
    g.s[1] ^= g.s[2];
    g.s[0] ^= g.s[3];
    g.s[2] ^= t;
    g.s[3] = round_rotl(g.s[3], 45);
    return r;
}

SRG_ROUND_HD inline uint64_t round_splitmix64(uint64_t& x) {
    x += 0x9e3779b97f4a7c15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

SRG_ROUND_HD inline void round_seed_from_u64(RoundRng& g, uint64_t seed) {
    for (int i = 0; i < 4; ++i) g.s[i] = round_splitmix64(seed);
}

// gen::<f64>() from one generator output
SRG_ROUND_HD inline double round_chance(uint64_t r) { return (double)(r >> 11) * (1.0 / 9007199254740992.0); }

// out_status: the outbound step's (1 to the router, 2 local).  ROUND_SENT here means "draws": the
// drop decision comes behind the draw.
SRG_ROUND_HD inline uint8_t round_classify(uint8_t out_status, uint64_t leave_ns, uint32_t dst_host,
                                           uint64_t sim_end_ns) {
    if (out_status != 1) return ROUND_LOCAL;
    if (leave_ns >= sim_end_ns) return ROUND_AFTER_END;
    if (dst_host == ROUND_NO_HOST) return ROUND_NO_DST;
    return ROUND_SENT;
}

// One drawing packet of a host, in leaving order: the draw, the decision, the id.  `loss` is the
// table's packet_loss[src_node, dst_node] (0 without a loss table: nothing is dropped, the draw still
// happens).  Returns ROUND_SENT or ROUND_DROPPED; *event_id is the id a sent packet took.
SRG_ROUND_HD inline uint8_t round_draw_one(RoundRng& g, uint64_t& next_event_id, bool have_loss, float loss,
                                           uint32_t payload, uint64_t leave_ns, uint64_t bootstrap_end_ns,
                                           double* chance, uint64_t* event_id) {
    *chance = round_chance(round_next_u64(g));
    *event_id = next_event_id;
    if (have_loss && dropped(loss, *chance, payload, leave_ns, bootstrap_end_ns)) return ROUND_DROPPED;
    ++next_event_id;
    return ROUND_SENT;
}

}  // namespace srg
