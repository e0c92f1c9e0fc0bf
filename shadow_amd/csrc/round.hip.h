// round.hip.h — the glue of a round on the device (gfx950): what lies between the caller's offers and
// the outbound step, between the outbound step and the send batch (round_rule.h: the per-host
// generator, which packets draw, the event ids), and between the pop and the inbound step.
//
// The caller's packet pool is three arrays indexed by tag (RoundPackets): dst_host, total_size,
// payload_size.  Resident per host, two sets (a send builds the spare set, the host side makes it
// current only when the whole call succeeded): the generator's four words and next_event_id.
//
//   k_round_offers  one thread per offer: tag < num_packets, dst_host < num_hosts or ROUND_NO_HOST, no
//                   flag bit but the barrier, no non-local packet above its DESTINATION's downstream
//                   bucket (so the inbound step can never refuse it later), the offsets; gathers
//                   total_size and derives the local bit (dst_host == the offering host)
//   k_round_count   one wave64 per host over the outbound step's outputs, 64 packets at a time, one
//                   per lane: each packet's class (round_classify) into the status array, the host's
//                   number of drawing packets by ballot
//   (a hipcub scan of the per-host counts: the hosts' first rows in the send batch)
//   k_round_draw    one wave64 per host, four hosts per workgroup, as k_out_step maps them.  The
//                   generator is a dependent chain (about ten integer instructions per draw), so a
//                   host is sequential whatever runs it; the wave makes everything around the chain
//                   parallel and coalesced.  Per 64 packets: the drawing lanes are ranked by ballot,
//                   the chain is stepped popcount times wave-uniform (every lane holds the same
//                   words), and each lane keeps the output whose index is its rank.  The table
//                   gathers, the drop decision and the row's stores are then one per lane; the ids
//                   are next_event_id + the lane's rank among the sent lanes.
//   k_round_sizes   one thread per popped event: total_size[tag] for the inbound step
// State is written with ordinary vector stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inbound_rule.h"
#include "outbound_rule.h"
#include "round_rule.h"

namespace srg {

constexpr uint32_t ROUND_BAD_TAG = 1;      // a tag >= num_packets
constexpr uint32_t ROUND_BAD_DST = 2;      // a dst_host that is neither < num_hosts nor ROUND_NO_HOST
constexpr uint32_t ROUND_BAD_SIZE = 4;     // a non-local packet above its destination's downstream bucket
constexpr uint32_t ROUND_BAD_FLAGS = 8;    // a flag bit other than the barrier
constexpr uint32_t ROUND_BAD_OFFSETS = 16; // host offsets not monotone / not ending at num_offers
constexpr int ROUND_HOSTS_PER_WG = 4;

struct RoundPackets {
    uint64_t n;
    const uint32_t* dst;      // [n] HostId, or ROUND_NO_HOST
    const uint32_t* size;     // [n] packet.total_size()
    const uint32_t* payload;  // [n] packet_getPayloadSize
};

// what a call reads back (one copy)
struct RoundReduce {
    unsigned long long after_end, no_dst;
    uint32_t flags, pad;
};

// the compacted send batch, one row per drawing packet
struct RoundRows {
    uint32_t *src_node, *dst_node, *src_host, *dst_host;
    uint64_t *send_ns, *event_id;
    double* chance;
    uint32_t* payload;
    uint64_t* tag;
};

__global__ void __launch_bounds__(256) k_round_offers(uint64_t n, const uint64_t* __restrict__ tag,
                                                      const uint8_t* __restrict__ flags,
                                                      const uint64_t* __restrict__ host_off, uint32_t num_hosts,
                                                      RoundPackets pk, const uint64_t* __restrict__ down_inc,
                                                      uint32_t* __restrict__ out_size, uint8_t* __restrict__ out_flags,
                                                      RoundReduce* red) {
    uint32_t bad = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    for (size_t h = t0; h <= num_hosts; h += stride) {
        const uint64_t o = host_off[h];
        if (h == 0 && o != 0) bad |= ROUND_BAD_OFFSETS;
        if (h == num_hosts ? o != n : o > host_off[h + 1]) bad |= ROUND_BAD_OFFSETS;
    }
    for (size_t j = t0; j < n; j += stride) {
        const uint8_t fl = flags ? flags[j] : 0;
        if (fl & ~OUT_OFFER_BARRIER) bad |= ROUND_BAD_FLAGS;
        uint32_t size = 0;
        uint8_t f = fl & OUT_OFFER_BARRIER;
        const uint64_t g = tag[j];
        if (g >= pk.n) {
            bad |= ROUND_BAD_TAG;
        } else {
            uint32_t lo = 0, hi = num_hosts;  // the host h with host_off[h] <= j < host_off[h + 1]
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (host_off[mid + 1] <= j) lo = mid + 1;
                else hi = mid;
            }
            const uint32_t dst = pk.dst[g];
            size = pk.size[g];
            if (dst == lo && lo < num_hosts) {
                f |= OUT_OFFER_LOCAL;
            } else if (dst < num_hosts) {
                const uint64_t r = down_inc[dst];
                if (r != 0 && size > r + INB_MTU) bad |= ROUND_BAD_SIZE;
            } else if (dst != ROUND_NO_HOST) {
                bad |= ROUND_BAD_DST;
            }
        }
        out_size[j] = size;
        out_flags[j] = f;
    }
    if (bad) atomicOr(&red->flags, bad);  // invalid input only
}

// o_*: the outbound step's outputs, off[H + 1] its host offsets.  Writes each packet's class over
// o_status and cnt[h] = the host's drawing packets (cnt[num_hosts] = 0, for the scan).
__global__ void __launch_bounds__(64 * ROUND_HOSTS_PER_WG)
    k_round_count(uint8_t* __restrict__ o_status, const uint64_t* __restrict__ o_time,
                  const uint64_t* __restrict__ o_tag, const uint64_t* __restrict__ off, uint32_t num_hosts,
                  RoundPackets pk, uint64_t sim_end, uint64_t* __restrict__ cnt, RoundReduce* red) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t h = (uint64_t)blockIdx.x * ROUND_HOSTS_PER_WG + (threadIdx.x >> 6);
    if (h > num_hosts) return;
    if (h == num_hosts) {
        if (lane == 0) cnt[h] = 0;
        return;
    }
    const uint64_t base = off[h], n = off[h + 1] - base;
    uint64_t draws = 0;
    uint32_t after_end = 0, no_dst = 0, bad = 0;
    for (uint64_t c = 0; c < n; c += 64) {
        const uint64_t i = base + c + lane;
        uint8_t cls = ROUND_LOCAL;
        if (c + lane < n) {
            const uint64_t g = o_tag[i];
            if (g >= pk.n) {
                bad |= ROUND_BAD_TAG;
            } else {
                cls = round_classify(o_status[i], o_time[i], pk.dst[g], sim_end);
                // a destination outside the hosts can only be a pool entry rewritten since its offer
                if (cls == ROUND_SENT && pk.dst[g] >= num_hosts) bad |= ROUND_BAD_DST;
            }
            o_status[i] = cls;
            after_end += cls == ROUND_AFTER_END;
            no_dst += cls == ROUND_NO_DST;
        }
        draws += __popcll(__ballot(cls == ROUND_SENT));
    }
    for (int o = 32; o; o >>= 1) {
        after_end += __shfl_xor(after_end, o, 64);
        no_dst += __shfl_xor(no_dst, o, 64);
    }
    if (lane == 0) {
        cnt[h] = draws;
        if (after_end) atomicAdd(&red->after_end, (unsigned long long)after_end);
        if (no_dst) atomicAdd(&red->no_dst, (unsigned long long)no_dst);
    }
    if (bad) atomicOr(&red->flags, bad);  // a pool changed under the round: invalid input only
}

// status: the classes k_round_count wrote; a drawing packet's becomes ROUND_SENT or ROUND_DROPPED.
// row0[h]: the host's first row.  rng_cur / eid_cur -> rng_new / eid_new for every host.
__global__ void __launch_bounds__(64 * ROUND_HOSTS_PER_WG)
    k_round_draw(uint8_t* __restrict__ status, const uint64_t* __restrict__ o_time, const uint64_t* __restrict__ o_tag,
                 const uint64_t* __restrict__ off, const uint64_t* __restrict__ row0, uint32_t num_hosts,
                 RoundPackets pk, const uint32_t* __restrict__ host_node, const float* __restrict__ loss, uint32_t tn,
                 uint64_t bootstrap_end, const uint64_t* __restrict__ rng_cur, const uint64_t* __restrict__ eid_cur,
                 uint64_t* __restrict__ rng_new, uint64_t* __restrict__ eid_new, RoundRows rows) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t h = (uint64_t)blockIdx.x * ROUND_HOSTS_PER_WG + (threadIdx.x >> 6);
    if (h >= num_hosts) return;
    RoundRng g;
    for (int k = 0; k < 4; ++k) g.s[k] = rng_cur[h * 4 + k];
    uint64_t eid = eid_cur[h], row = row0[h];
    const uint64_t base = off[h], n = off[h + 1] - base;
    const uint32_t a = host_node[h];
    const unsigned long long below = (1ull << lane) - 1;
    for (uint64_t c = 0; c < n; c += 64) {
        const uint64_t i = base + c + lane;
        const bool draws = c + lane < n && status[i] == ROUND_SENT;
        const unsigned long long mask = __ballot(draws);
        const uint32_t k = (uint32_t)__popcll(mask), rank = (uint32_t)__popcll(mask & below);
        uint64_t mine = 0;
        for (uint32_t j = 0; j < k; ++j) {  // the chain: wave-uniform
            const uint64_t r = round_next_u64(g);
            if (rank == j) mine = r;
        }
        bool sent = false;
        uint64_t t = 0, tag = 0;
        uint32_t dst = 0, b = 0, payload = 0;
        double chance = 0.0;
        if (draws) {
            tag = o_tag[i];
            t = o_time[i];
            dst = pk.dst[tag];
            payload = pk.payload[tag];
            b = host_node[dst];
            chance = round_chance(mine);
            sent = !(loss && dropped(loss[(size_t)a * tn + b], chance, payload, t, bootstrap_end));
        }
        const unsigned long long smask = __ballot(sent);
        if (draws) {
            const uint64_t r = row + rank;
            rows.src_node[r] = a;
            rows.dst_node[r] = b;
            rows.src_host[r] = (uint32_t)h;
            rows.dst_host[r] = dst;
            rows.send_ns[r] = t;
            rows.event_id[r] = eid + (uint64_t)__popcll(smask & below);  // (a dropped row's id is never read)
            rows.chance[r] = chance;
            rows.payload[r] = payload;
            rows.tag[r] = tag;
            status[i] = sent ? ROUND_SENT : ROUND_DROPPED;
        }
        eid += (uint64_t)__popcll(smask);
        row += k;
    }
    if (lane == 0) {  // (constant indices only: a lane-indexed g.s[] would move the words out of registers)
        for (int k = 0; k < 4; ++k) rng_new[h * 4 + k] = g.s[k];
        eid_new[h] = eid;
    }
}

__global__ void __launch_bounds__(256) k_round_sizes(uint64_t n, const uint64_t* __restrict__ tag, RoundPackets pk,
                                                     uint32_t* __restrict__ out_size, RoundReduce* red) {
    uint32_t bad = 0;
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) {
        const uint64_t g = tag[j];
        if (g >= pk.n) bad |= ROUND_BAD_TAG;
        out_size[j] = g < pk.n ? pk.size[g] : 0;
    }
    if (bad) atomicOr(&red->flags, bad);  // a pool shrunk under the round: invalid input only
}

__global__ void __launch_bounds__(256) k_round_seed(const uint64_t* __restrict__ seed, uint32_t num_hosts,
                                                    uint64_t* __restrict__ rng, uint64_t* __restrict__ eid) {
    for (size_t h = blockIdx.x * (size_t)blockDim.x + threadIdx.x; h < num_hosts; h += (size_t)gridDim.x * blockDim.x) {
        RoundRng g;
        round_seed_from_u64(g, seed[h]);
        for (int k = 0; k < 4; ++k) rng[h * 4 + k] = g.s[k];
        eid[h] = 0;
    }
}

}  // namespace srg
