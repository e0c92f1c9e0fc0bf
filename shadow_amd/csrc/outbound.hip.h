// outbound.hip.h — the hosts' outbound path on the device (gfx950): the sockets' FIFOs, the
// interface's qdisc structure and relay_inet_out's token bucket (outbound_rule.h) as a per-host
// state machine over the caller's offers.
//
// Resident form, two sets (a step builds the spare set, the host side makes it current only after
// the device flags were read back):
//   OutHost hosts[H]            the bucket, the relay, the qdisc structure's length and ring head
//   per-socket segments [sum of sockets_per_host], a host's slots at seg_off[h]:
//     ord    the heap array (or the round-robin ring) of slots
//     ch ct dh dt   head and tail of the slot's control and data FIFO: indices into the host's packets
//     nprio  the slot's current next-packet priority, so a heap compare is ord -> nprio, not
//            ord -> head -> priority
//   a flat backlog of the packets still in sockets, in arrival order (slot, priority, size, flags,
//   tag; host_off[H + 1]) and `next`, each packet's successor in its FIFO (index in the host's slice)
// A host's packets in a step are one sequence: its backlog, then its offers; a FIFO is a linked list
// through it (the links of a step live in scratch, seeded from the backlog's).
//
//   k_out_validate  one thread per offer: the offsets (monotone, ending at num_offers), the times (in
//                   the domain, < until, non-decreasing inside a host's slice -- the neighbour through
//                   a lane shuffle -- and the slice's first one >= the host's last processed time),
//                   the slot, the flag bits, and no non-local packet above a limited host's capacity
//   k_out_step      one wave64 per host, four hosts per workgroup.  The wave copies the host's
//                   segments and links into the spare set (coalesced), reads the offers in
//                   64-element chunks, one per lane (coalesced), and runs the rule wave-uniform: every
//                   value of the rule is formed through readfirstlane and lives in scalar registers;
//                   the mutable arrays (ord, heads, tails, nprio, links) are read and written by
//                   lane 0 alone, so a load after a store is one thread's program order.  What leaves
//                   is recorded in leaving order (sequence index, time, status) in scratch.
//   (hipcub scans of the per-host leave counts and remainders)
//   k_out_commit    one wave per host: the leaving packets into the caller's outputs; the un-pulled
//                   packets compacted in arrival order into the spare backlog, their links and the
//                   slots' heads and tails renumbered by the same compaction
// A host is sequential: a step costs (events of the busiest host) x (chain latency per event).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "outbound_rule.h"

namespace srg {

constexpr uint32_t OUT_BAD_OFFSETS = 1;    // host offsets not monotone / not ending at num_offers
constexpr uint32_t OUT_BAD_TIME = 2;       // a time outside [sim_start, 2^62) or >= until
constexpr uint32_t OUT_TIME_BACKWARD = 4;  // an offer earlier than its predecessor / the host's last time
constexpr uint32_t OUT_BAD_SIZE = 8;       // a non-local packet larger than a limited host's bucket
constexpr uint32_t OUT_BAD_SLOT = 16;      // a slot >= the host's socket count
constexpr uint32_t OUT_BAD_FLAGS = 32;     // a flag bit other than LOCAL | BARRIER
constexpr int OUT_HOSTS_PER_WG = 4;

struct OutSeg {  // the per-socket segments of one set
    uint32_t *ord, *ch, *ct, *dh, *dt;
    uint64_t* nprio;
};

struct OutBacklog {
    uint32_t* slot;
    uint64_t* prio;
    uint32_t* size;
    uint8_t* flags;
    uint64_t* tag;
    uint32_t* next;
    uint64_t* host_off;  // [H + 1]
};

struct OutOffers {
    uint64_t n;
    const uint64_t* time;
    const uint32_t* slot;
    const uint64_t* prio;
    const uint32_t* size;
    const uint8_t* flags;  // may be null: all 0
    const uint64_t* tag;
    const uint64_t* host_off;  // [H + 1]
};

// what a step reads back (one copy)
struct OutReduce {
    unsigned long long min_wake, sent, local, cached;
    uint32_t flags, pad;
};

// per step scratch; a host's sequence region starts at b0 + a0, its leave region at b0 + a0 + h
struct OutScratch {
    uint32_t* lnk;      // [nseq] FIFO successor
    uint8_t* gone;      // [nseq] pulled in this step (zeroed before the step)
    uint32_t* newidx;   // [nseq] position after the compaction
    uint32_t* o_idx;    // [nseq + H] leaving order: sequence index, OUT_NIL = the previously cached packet
    uint64_t* o_time;   // [nseq + H]
    uint8_t* o_status;  // [nseq + H]
};

__global__ void __launch_bounds__(256) k_out_validate(OutOffers a, const OutHost* __restrict__ hosts,
                                                      const uint64_t* __restrict__ inc,
                                                      const uint64_t* __restrict__ seg_off, uint32_t num_hosts,
                                                      uint64_t sim_start, uint64_t until, OutReduce* red) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t bad = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    // the offsets, one host per thread
    for (size_t h = blockIdx.x * (size_t)blockDim.x + threadIdx.x; h <= num_hosts; h += stride) {
        const uint64_t o = a.host_off[h];
        if (h == 0 && o != 0) bad |= OUT_BAD_OFFSETS;
        if (h == num_hosts ? o != a.n : o > a.host_off[h + 1]) bad |= OUT_BAD_OFFSETS;
    }
    // the offers; whole waves stay in the loop together (the shuffle needs every lane)
    for (size_t j0 = blockIdx.x * (size_t)blockDim.x + (threadIdx.x & ~63u); j0 < a.n; j0 += stride) {
        const size_t j = j0 + lane;
        const bool in_range = j < a.n;
        const uint64_t t = in_range ? a.time[j] : 0;
        uint64_t p = __shfl_up((unsigned long long)t, 1, 64);
        if (lane == 0 && in_range && j > 0) p = a.time[j - 1];
        if (in_range) {
            if (t < sim_start || t >= INB_TIME_END || t >= until) bad |= OUT_BAD_TIME;
            const uint8_t fl = a.flags ? a.flags[j] : 0;
            if (fl & ~(OUT_OFFER_LOCAL | OUT_OFFER_BARRIER)) bad |= OUT_BAD_FLAGS;
            uint32_t lo = 0, hi = num_hosts;  // the host h with host_off[h] <= j < host_off[h + 1]
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.host_off[mid + 1] <= j) lo = mid + 1;
                else hi = mid;
            }
            if (lo < num_hosts) {
                const uint64_t floor_t = a.host_off[lo] == j ? hosts[lo].last_time : p;
                if (t < floor_t) bad |= OUT_TIME_BACKWARD;
                if (a.slot[j] >= seg_off[lo + 1] - seg_off[lo]) bad |= OUT_BAD_SLOT;
                const uint64_t r = inc[lo];
                if (r != 0 && !(fl & OUT_OFFER_LOCAL) && a.size[j] > r + INB_MTU) bad |= OUT_BAD_SIZE;
            }
        }
    }
    if (bad) atomicOr(&red->flags, bad);  // invalid input only
}

// outbound_rule.h's queue over one host's sockets and offers, held by one wave.  Every member but
// the offer chunk (e_*) is wave-uniform.
struct OutWaveQ {
    // the host's sequence: backlog [0, nb), offers [nb, n)
    const uint64_t *b_prio, *a_time, *a_prio;
    const uint32_t *b_size, *a_slot, *a_size;
    const uint8_t *b_flags, *a_flags;
    uint32_t nb, n;
    // the spare set's segments of this host, the step's links and marks
    uint32_t *ord, *ch, *ct, *dh, *dt, *lnk;
    uint64_t* nprio_;
    uint8_t* gone;
    uint32_t *o_idx;
    uint64_t* o_time;
    uint8_t* o_status;
    uint32_t lane;
    uint32_t enq, enq_base;  // the next offer; the chunk held one element per lane
    uint64_t e_t, e_p;
    uint32_t e_slot, e_fl;
    uint32_t last, cached_idx, n_out, n_sent, n_local;

    // uniform memory access: lane 0 alone touches the mutable arrays
    __device__ __forceinline__ uint32_t ld(const uint32_t* p) const {
        uint32_t v = 0;
        if (lane == 0) v = *p;
        return __builtin_amdgcn_readfirstlane(v);
    }
    __device__ __forceinline__ uint64_t ld(const uint64_t* p) const {
        uint32_t lo = 0, hi = 0;
        if (lane == 0) {
            const uint64_t v = *p;
            lo = (uint32_t)v;
            hi = (uint32_t)(v >> 32);
        }
        return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(hi) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane(lo);  // (the builtin returns int)
    }
    __device__ __forceinline__ uint32_t ld(const uint8_t* p) const {
        uint32_t v = 0;
        if (lane == 0) v = *p;
        return __builtin_amdgcn_readfirstlane(v);
    }
    template <class T>
    __device__ __forceinline__ void st(T* p, T v) const {
        if (lane == 0) *p = v;
    }
    __device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t src) const {
        return __builtin_amdgcn_readfirstlane(__shfl(v, (int)src, 64));
    }
    __device__ __forceinline__ uint64_t bcast(uint64_t v, uint32_t src) const {
        return ((uint64_t)bcast((uint32_t)(v >> 32), src) << 32) | bcast((uint32_t)v, src);
    }
    __device__ __forceinline__ uint64_t prio_of(uint32_t i) const { return i < nb ? ld(b_prio + i) : ld(a_prio + (i - nb)); }

    __device__ __forceinline__ void load_chunk() {
        const uint32_t i = enq_base + lane;
        e_t = ~0ull;
        e_p = 0;
        e_slot = e_fl = 0;
        if (i < n) {
            const uint32_t j = i - nb;
            e_t = a_time[j];
            e_p = a_prio[j];
            e_slot = a_slot[j];
            e_fl = a_flags ? a_flags[j] : 0;
        }
    }

    __device__ __forceinline__ uint32_t ord_get(uint32_t i) const { return ld(ord + i); }
    __device__ __forceinline__ void ord_set(uint32_t i, uint32_t slot) const { st(ord + i, slot); }
    __device__ __forceinline__ uint64_t nprio(uint32_t slot) const { return ld(nprio_ + slot); }
    __device__ __forceinline__ bool has_offer() const { return enq < n; }
    __device__ __forceinline__ uint64_t offer_time() const { return bcast(e_t, enq - enq_base); }
    __device__ __forceinline__ uint8_t offer_flags() const { return (uint8_t)bcast(e_fl, enq - enq_base); }
    __device__ __forceinline__ bool push_offer(uint32_t& slot) {
        const uint32_t k = enq - enq_base, idx = enq;
        slot = bcast(e_slot, k);
        const uint64_t p = bcast(e_p, k);
        const uint32_t c = ld(ch + slot), d = ld(dh + slot);
        const bool was_empty = c == OUT_NIL && d == OUT_NIL;
        uint32_t* head = p == 0 ? ch : dh;
        uint32_t* tail = p == 0 ? ct : dt;
        if ((p == 0 ? c : d) == OUT_NIL) st(head + slot, idx);
        else st(lnk + ld(tail + slot), idx);
        st(tail + slot, idx);
        st(lnk + idx, OUT_NIL);
        if (p == 0) st(nprio_ + slot, (uint64_t)0);  // the control FIFO's head is the next packet
        else if (was_empty) st(nprio_ + slot, p);
        ++enq;
        if (enq < n && enq == enq_base + 64) {
            enq_base += 64;
            load_chunk();
        }
        return was_empty;
    }
    __device__ __forceinline__ bool pull(uint32_t slot, uint32_t& size, uint8_t& flags) {
        uint32_t c = ld(ch + slot), d = ld(dh + slot), idx;
        if (c != OUT_NIL) {
            idx = c;
            c = ld(lnk + idx);
            st(ch + slot, c);
            if (c == OUT_NIL) st(ct + slot, OUT_NIL);
        } else {
            idx = d;
            d = ld(lnk + idx);
            st(dh + slot, d);
            if (d == OUT_NIL) st(dt + slot, OUT_NIL);
        }
        if (c != OUT_NIL) st(nprio_ + slot, (uint64_t)0);
        else if (d != OUT_NIL) st(nprio_ + slot, prio_of(d));
        size = idx < nb ? ld(b_size + idx) : ld(a_size + (idx - nb));
        flags = (uint8_t)(idx < nb ? ld(b_flags + idx) : (a_flags ? ld(a_flags + (idx - nb)) : 0u));
        st(gone + idx, (uint8_t)1);
        last = idx;
        return c != OUT_NIL || d != OUT_NIL;
    }
    __device__ __forceinline__ void record(uint32_t idx, uint8_t status, uint64_t now) {
        st(o_idx + n_out, idx);
        st(o_time + n_out, now);
        st(o_status + n_out, status);
        ++n_out;
        if (status == 1) ++n_sent;
        else ++n_local;
    }
    __device__ __forceinline__ void leave(uint8_t status, uint64_t now) { record(last, status, now); }
    __device__ __forceinline__ void cache_last() { cached_idx = last; }
    __device__ __forceinline__ void leave_cached(uint64_t now) {
        record(cached_idx, 1, now);  // OUT_NIL: the packet cached by an earlier step
        cached_idx = OUT_NIL;
    }
};

__device__ __forceinline__ uint64_t out_first_lane(uint64_t v) {
    // (the builtin returns int: without the casts the low half would sign-extend over the high one)
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
}

// the record was loaded from one address by every lane: say so, so that it lives in scalar registers
__device__ __forceinline__ void out_make_uniform(OutHost& s) {
    s.balance = out_first_lane(s.balance);
    s.last_refill = out_first_lane(s.last_refill);
    s.wake = out_first_lane(s.wake);
    s.cached_tag = out_first_lane(s.cached_tag);
    s.last_time = out_first_lane(s.last_time);
    s.cached_size = __builtin_amdgcn_readfirstlane(s.cached_size);
    s.qlen = __builtin_amdgcn_readfirstlane(s.qlen);
    s.rr_head = __builtin_amdgcn_readfirstlane(s.rr_head);
    s.queued = __builtin_amdgcn_readfirstlane(s.queued);
    s.pending = (uint8_t)__builtin_amdgcn_readfirstlane((uint32_t)s.pending);
    s.has_cached = (uint8_t)__builtin_amdgcn_readfirstlane((uint32_t)s.has_cached);
}

__global__ void __launch_bounds__(64 * OUT_HOSTS_PER_WG)
    k_out_step(const OutHost* __restrict__ cur, OutHost* __restrict__ next, const uint64_t* __restrict__ inc,
               const uint64_t* __restrict__ seg_off, OutSeg CS, OutSeg NS, OutBacklog B, OutOffers A, OutScratch X,
               uint32_t num_hosts, int qdisc, uint64_t until, uint64_t bootstrap_end, uint64_t* __restrict__ cnt,
               uint64_t* __restrict__ rem, OutReduce* red) {
    const uint32_t lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t h = blockIdx.x * OUT_HOSTS_PER_WG + w;
    unsigned long long wake = ~0ull;
    uint32_t sent = 0, local = 0, cached = 0;
    if (h < num_hosts) {
        const uint64_t b0 = B.host_off[h], b1 = B.host_off[h + 1], a0 = A.host_off[h], a1 = A.host_off[h + 1];
        const uint64_t s0 = seg_off[h];
        const uint32_t cap = (uint32_t)(seg_off[h + 1] - s0);
        OutWaveQ q;
        q.b_prio = B.prio + b0;
        q.b_size = B.size + b0;
        q.b_flags = B.flags + b0;
        q.a_time = A.time + a0;
        q.a_prio = A.prio + a0;
        q.a_slot = A.slot + a0;
        q.a_size = A.size + a0;
        q.a_flags = A.flags ? A.flags + a0 : nullptr;
        q.nb = (uint32_t)(b1 - b0);
        q.n = q.nb + (uint32_t)(a1 - a0);
        q.ord = NS.ord + s0;
        q.ch = NS.ch + s0;
        q.ct = NS.ct + s0;
        q.dh = NS.dh + s0;
        q.dt = NS.dt + s0;
        q.nprio_ = NS.nprio + s0;
        q.lnk = X.lnk + (b0 + a0);
        q.gone = X.gone + (b0 + a0);
        q.o_idx = X.o_idx + (b0 + a0 + h);
        q.o_time = X.o_time + (b0 + a0 + h);
        q.o_status = X.o_status + (b0 + a0 + h);
        q.lane = lane;
        q.enq = q.enq_base = q.nb;
        q.last = q.cached_idx = OUT_NIL;
        q.n_out = q.n_sent = q.n_local = 0;
        // the host's current segments and links into the spare set and the scratch
        for (uint32_t i = lane; i < cap; i += 64) {
            q.ord[i] = CS.ord[s0 + i];
            q.ch[i] = CS.ch[s0 + i];
            q.ct[i] = CS.ct[s0 + i];
            q.dh[i] = CS.dh[s0 + i];
            q.dt[i] = CS.dt[s0 + i];
            q.nprio_[i] = CS.nprio[s0 + i];
        }
        for (uint32_t i = lane; i < q.nb; i += 64) q.lnk[i] = B.next[b0 + i];
        __threadfence_block();  // lane 0 reads what the other lanes copied
        q.load_chunk();
        OutHost s = cur[h];
        out_make_uniform(s);
        out_host_step(s, inc[h], q, qdisc, cap, until, bootstrap_end);
        if (s.has_cached && q.cached_idx != OUT_NIL)
            s.cached_tag = q.cached_idx < q.nb ? B.tag[b0 + q.cached_idx] : A.tag[a0 + (q.cached_idx - q.nb)];
        if (lane == 0) {
            next[h] = s;
            cnt[h] = q.n_out;
            rem[h] = s.queued;
        }
        if (s.pending) wake = s.wake;
        sent = q.n_sent;
        local = q.n_local;
        cached = s.has_cached;
    } else if (h == num_hosts && lane == 0) {
        cnt[h] = 0;  // the scans' total slots
        rem[h] = 0;
    }
    __shared__ unsigned long long s_wake[OUT_HOSTS_PER_WG];
    __shared__ uint32_t s_cnt[3][OUT_HOSTS_PER_WG];
    if (lane == 0) {
        s_wake[w] = wake;
        s_cnt[0][w] = sent;
        s_cnt[1][w] = local;
        s_cnt[2][w] = cached;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // one same-address atomic per workgroup and value
        unsigned long long f = 0, d = 0, c = 0;
        for (int k = 0; k < OUT_HOSTS_PER_WG; ++k) {
            wake = s_wake[k] < wake ? s_wake[k] : wake;
            f += s_cnt[0][k];
            d += s_cnt[1][k];
            c += s_cnt[2][k];
        }
        if (wake != ~0ull) atomicMin(&red->min_wake, wake);
        if (f) atomicAdd(&red->sent, f);
        if (d) atomicAdd(&red->local, d);
        if (c) atomicAdd(&red->cached, c);
    }
}

// One wave per host: the packets that left, into the caller's arrays at out_off[h]; the packets still
// in sockets, in arrival order, into the spare backlog at NB.host_off[h], with the FIFO links and the
// slots' heads and tails (in NS, written by the step) renumbered.
__global__ void __launch_bounds__(64 * OUT_HOSTS_PER_WG)
    k_out_commit(const OutHost* __restrict__ cur, const uint64_t* __restrict__ seg_off, OutSeg NS, OutBacklog B, OutOffers A,
                 OutScratch X, uint32_t num_hosts, const uint64_t* __restrict__ cnt, const uint64_t* __restrict__ out_off,
                 uint8_t* __restrict__ out_status, uint64_t* __restrict__ out_time, uint64_t* __restrict__ out_tag,
                 OutBacklog NB) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t h = blockIdx.x * OUT_HOSTS_PER_WG + (threadIdx.x >> 6);
    const bool live = h < num_hosts;
    uint64_t b0 = 0, a0 = 0, k0 = 0;
    uint32_t nb = 0, n = 0;
    if (live) {
        b0 = B.host_off[h];
        nb = (uint32_t)(B.host_off[h + 1] - b0);
        a0 = A.host_off[h];
        n = nb + (uint32_t)(A.host_off[h + 1] - a0);
        k0 = NB.host_off[h];
        const uint64_t dst = out_off[h], src = b0 + a0 + h;
        const uint32_t left = (uint32_t)cnt[h];
        for (uint32_t k = lane; k < left; k += 64) {
            const uint32_t i = X.o_idx[src + k];
            out_status[dst + k] = X.o_status[src + k];
            out_time[dst + k] = X.o_time[src + k];
            out_tag[dst + k] = i == OUT_NIL ? cur[h].cached_tag : i < nb ? B.tag[b0 + i] : A.tag[a0 + (i - nb)];
        }
        // the compaction: each remaining packet's new position
        uint32_t base = 0;
        for (uint32_t i0 = 0; i0 < n; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool keep = i < n && !X.gone[b0 + a0 + i];
            const uint64_t mask = __ballot(keep);
            if (keep) X.newidx[b0 + a0 + i] = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
            base += (uint32_t)__popcll(mask);
        }
    }
    __threadfence_block();
    __syncthreads();  // newidx is read across lanes
    if (!live) return;
    const uint32_t* newidx = X.newidx + (b0 + a0);
    for (uint32_t i = lane; i < n; i += 64) {
        if (X.gone[b0 + a0 + i]) continue;
        const uint64_t k = k0 + newidx[i];
        const uint32_t nx = X.lnk[b0 + a0 + i];
        NB.next[k] = nx == OUT_NIL ? OUT_NIL : newidx[nx];
        if (i < nb) {
            NB.slot[k] = B.slot[b0 + i];
            NB.prio[k] = B.prio[b0 + i];
            NB.size[k] = B.size[b0 + i];
            NB.flags[k] = B.flags[b0 + i];
            NB.tag[k] = B.tag[b0 + i];
        } else {
            const uint64_t j = a0 + (i - nb);
            NB.slot[k] = A.slot[j];
            NB.prio[k] = A.prio[j];
            NB.size[k] = A.size[j];
            NB.flags[k] = A.flags ? (uint8_t)(A.flags[j] & OUT_OFFER_LOCAL) : (uint8_t)0;
            NB.tag[k] = A.tag[j];
        }
    }
    const uint64_t s0 = seg_off[h];
    const uint32_t cap = (uint32_t)(seg_off[h + 1] - s0);
    auto renumber = [&](uint32_t* p) {
        if (*p != OUT_NIL) *p = newidx[*p];
    };
    for (uint32_t i = lane; i < cap; i += 64) {
        renumber(NS.ch + s0 + i);
        renumber(NS.ct + s0 + i);
        renumber(NS.dh + s0 + i);
        renumber(NS.dt + s0 + i);
    }
}

// refill increments, the initial records and empty sockets, from the hosts' bandwidths
__global__ void __launch_bounds__(256) k_out_init(const uint64_t* __restrict__ bw, uint32_t num_hosts, uint64_t num_slots,
                                                  uint64_t sim_start, uint64_t* __restrict__ inc, OutHost* __restrict__ a,
                                                  OutHost* __restrict__ b, OutSeg sa, OutSeg sb) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    for (size_t h = t0; h < num_hosts; h += stride) {
        const uint64_t r = inb_refill_increment(bw[h]);
        OutHost s;
        out_host_init(s, r, sim_start);
        inc[h] = r;
        a[h] = s;
        b[h] = s;
    }
    for (size_t i = t0; i < num_slots; i += stride) {
        sa.ord[i] = sb.ord[i] = 0;
        sa.ch[i] = sa.ct[i] = sa.dh[i] = sa.dt[i] = OUT_NIL;
        sb.ch[i] = sb.ct[i] = sb.dh[i] = sb.dt[i] = OUT_NIL;
        sa.nprio[i] = sb.nprio[i] = 0;
    }
}

}  // namespace srg
