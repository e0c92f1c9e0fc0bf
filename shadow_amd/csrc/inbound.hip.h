// inbound.hip.h — the hosts' inbound path on the device (gfx950): the router's CoDel queue and the
// inbound relay's token bucket (inbound_rule.h) as a per-host state machine over the arrays
// srg_event_queues_pop_device writes, plus a packet size.
//
// Resident form: one InbHost record per host (bucket, CoDel, relay, last processed time), the
// refill increment per host (0: unlimited), and a flat backlog of the packets still in the router
// queues (enqueue time, size, tag; host_off[H + 1]).  Two sets: a step builds the spare set, and
// the host side makes it current only after the device flags were read back.
//
//   k_inb_validate  one thread per arrival: the offsets (monotone, ending at num_arrivals), the
//                   times (in the domain, < until, non-decreasing inside a host's slice -- the
//                   neighbour through a lane shuffle, as k_evq_gather -- and the slice's first one
//                   >= the host's last processed time), and no packet above a limited host's
//                   bucket capacity (the balance is clamped to it: the relay would wake for ever)
//   k_inb_step      one wave64 per host, four hosts per workgroup.  A host's input is one FIFO: its
//                   backlog segment, then its arrival slice (every arrival is newer than every
//                   queued packet).  CoDel is FIFO, so what leaves in a step is a prefix of that
//                   sequence, with the previously cached packet in front.  Two cursors over it, the
//                   enqueue frontier and the pop head, each with a 64-element chunk held one
//                   element per lane (loaded coalesced, read out by lane index); the rule itself
//                   runs wave-uniform.  Enqueueing up to a task's time is one ballot and a wave sum
//                   of the sizes; a popped element's (status, leave time) is kept in the lane of
//                   its slot and stored coalesced per chunk into scratch aligned with the sequence.
//   (hipcub scans of the per-host leave counts and remainders)
//   k_inb_commit    one wave per host: the compacting copy into the caller's outputs and of the
//                   un-popped suffix into the spare backlog
// A host is sequential: a step costs (events of the busiest host) x (chain latency per event).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "event_queue.hip.h"
#include "inbound_rule.h"

namespace srg {

constexpr uint32_t INB_BAD_OFFSETS = 1;    // host offsets not monotone / not ending at num_arrivals
constexpr uint32_t INB_BAD_TIME = 2;       // a time outside [sim_start, 2^62) or >= until
constexpr uint32_t INB_TIME_BACKWARD = 4;  // an arrival earlier than its predecessor / the host's last time
constexpr uint32_t INB_BAD_SIZE = 8;       // a packet larger than a limited host's bucket: it would never conform
constexpr int INB_HOSTS_PER_WG = 4;

struct InbBacklog {
    uint64_t* time;
    uint32_t* size;
    uint64_t* tag;
    uint64_t* host_off;  // [H + 1]
};

struct InbArrivals {
    uint64_t n;
    const uint64_t* time;
    const uint32_t* size;
    const uint64_t* tag;
    const uint64_t* host_off;  // [H + 1]
};

// what a step reads back (one copy)
struct InbReduce {
    unsigned long long min_wake, forwarded, dropped, cached;
    uint32_t flags, pad;
};

// per host, what the step left for the commit
struct InbHostOut {
    uint64_t left_seq;    // elements of the host's sequence that left (a prefix)
    uint64_t head;        // popped elements (left_seq, plus one when the last popped is cached)
    uint64_t old_time;    // the previously cached packet's leave time ...
    uint8_t old_left;     // ... when it left in this step
    uint8_t old_status;
    uint8_t pad[6];
};

__global__ void __launch_bounds__(256) k_inb_validate(InbArrivals a, const InbHost* __restrict__ hosts,
                                                      const uint64_t* __restrict__ inc, uint32_t num_hosts,
                                                      uint64_t sim_start, uint64_t until, InbReduce* red) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t bad = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    // the offsets, one host per thread
    for (size_t h = blockIdx.x * (size_t)blockDim.x + threadIdx.x; h <= num_hosts; h += stride) {
        const uint64_t o = a.host_off[h];
        if (h == 0 && o != 0) bad |= INB_BAD_OFFSETS;
        if (h == num_hosts ? o != a.n : o > a.host_off[h + 1]) bad |= INB_BAD_OFFSETS;
    }
    // the times; whole waves stay in the loop together (the shuffle needs every lane)
    for (size_t j0 = blockIdx.x * (size_t)blockDim.x + (threadIdx.x & ~63u); j0 < a.n; j0 += stride) {
        const size_t j = j0 + lane;
        const bool in_range = j < a.n;
        const uint64_t t = in_range ? a.time[j] : 0;
        uint64_t p = __shfl_up((unsigned long long)t, 1, 64);
        if (lane == 0 && in_range && j > 0) p = a.time[j - 1];
        if (in_range) {
            if (t < sim_start || t >= INB_TIME_END || t >= until) bad |= INB_BAD_TIME;
            uint32_t lo = 0, hi = num_hosts;  // the host h with host_off[h] <= j < host_off[h + 1]
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.host_off[mid + 1] <= j) lo = mid + 1;
                else hi = mid;
            }
            if (lo < num_hosts) {
                const uint64_t floor_t = a.host_off[lo] == j ? hosts[lo].last_time : p;
                if (t < floor_t) bad |= INB_TIME_BACKWARD;
                const uint64_t r = inc[lo];
                if (r != 0 && a.size[j] > r + INB_MTU) bad |= INB_BAD_SIZE;
            }
        }
    }
    if (bad) atomicOr(&red->flags, bad);  // invalid input only
}

__device__ __forceinline__ uint64_t inb_wave_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor((unsigned long long)v, off, 64);
    return v;
}

// inbound_rule.h's queue over one host's sequence, held by one wave
struct InbWaveQ {
    const uint64_t *b_time, *a_time;
    const uint32_t *b_size, *a_size;
    uint64_t nb, n;  // backlog elements, all elements
    uint8_t* o_status;
    uint64_t* o_time;
    uint32_t lane;
    uint64_t enq, enq_base, e_t;
    uint32_t e_s;
    uint64_t head, head_base, h_t;
    uint32_t h_s;
    uint8_t my_status;
    uint64_t my_time;
    bool old_cached;
    uint8_t old_left, old_status;
    uint64_t old_time;
    uint32_t n_fwd, n_drop;

    __device__ __forceinline__ void load(uint64_t base, uint64_t& t, uint32_t& s) const {
        const uint64_t i = base + lane;
        t = ~0ull;
        s = 0;
        if (i < nb) {
            t = b_time[i];
            s = b_size[i];
        } else if (i < n) {
            t = a_time[i - nb];
            s = a_size[i - nb];
        }
    }
    __device__ __forceinline__ void flush() const {
        const uint64_t i = head_base + lane;
        if (i < head) {
            o_status[i] = my_status;
            o_time[i] = my_time;
        }
    }
    __device__ __forceinline__ bool pop_front(uint64_t& ts, uint32_t& size) {
        if (head == enq) return false;
        if (head == head_base + 64) {
            flush();
            head_base += 64;
            load(head_base, h_t, h_s);
        }
        const int src = (int)(head - head_base);
        ts = __shfl((unsigned long long)h_t, src, 64);
        size = __shfl(h_s, src, 64);
        ++head;
        return true;
    }
    __device__ __forceinline__ void leave(uint8_t status, uint64_t now) {
        if (lane == (uint32_t)(head - 1 - head_base)) {
            my_status = status;
            my_time = now;
        }
        if (status) ++n_fwd;
        else ++n_drop;
    }
    __device__ __forceinline__ void leave_cached(uint8_t status, uint64_t now) {
        if (!old_cached) return leave(status, now);
        old_cached = false;
        old_left = 1;
        old_status = status;
        old_time = now;
        if (status) ++n_fwd;
        else ++n_drop;
    }
    __device__ __forceinline__ bool has_arrival() const { return enq < n; }
    __device__ __forceinline__ uint64_t next_arrival_time() const {
        return __shfl((unsigned long long)e_t, (int)(enq - enq_base), 64);
    }
    __device__ __forceinline__ void enqueue_upto(uint64_t limit, InbHost& s) {
        while (enq < n) {
            const uint64_t i = enq_base + lane;
            const bool in = i >= enq && i < n && e_t <= limit;
            const uint64_t mask = __ballot(in);
            const uint32_t cnt = (uint32_t)__popcll(mask);
            if (cnt == 0) break;
            s.bytes += inb_wave_sum(in ? (uint64_t)e_s : 0ull);
            const uint64_t last = __shfl((unsigned long long)e_t, (int)(enq + cnt - 1 - enq_base), 64);
            s.last_time = last > s.last_time ? last : s.last_time;
            enq += cnt;
            if (enq < enq_base + 64 || enq >= n) break;
            enq_base += 64;
            load(enq_base, e_t, e_s);
        }
        // (the frontier's chunk always holds element enq when there is one)
        if (enq < n && enq == enq_base + 64) {
            enq_base += 64;
            load(enq_base, e_t, e_s);
        }
    }
};

__global__ void __launch_bounds__(64 * INB_HOSTS_PER_WG)
    k_inb_step(const InbHost* __restrict__ cur, InbHost* __restrict__ next, const uint64_t* __restrict__ inc,
               InbBacklog B, InbArrivals A, uint32_t num_hosts, uint64_t until, uint64_t bootstrap_end,
               uint8_t* __restrict__ scr_status, uint64_t* __restrict__ scr_time, InbHostOut* __restrict__ hout,
               uint64_t* __restrict__ cnt, uint64_t* __restrict__ rem, InbReduce* red) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t h = blockIdx.x * INB_HOSTS_PER_WG + w;
    unsigned long long wake = ~0ull;
    uint32_t fwd = 0, drop = 0, cached = 0;
    if (h < num_hosts) {
        InbHost s = cur[h];
        const uint64_t b0 = B.host_off[h], b1 = B.host_off[h + 1], a0 = A.host_off[h], a1 = A.host_off[h + 1];
        InbWaveQ q;
        q.b_time = B.time + b0;
        q.b_size = B.size + b0;
        q.a_time = A.time + a0;
        q.a_size = A.size + a0;
        q.nb = b1 - b0;
        q.n = q.nb + (a1 - a0);
        q.o_status = scr_status + b0 + a0;
        q.o_time = scr_time + b0 + a0;
        q.lane = lane;
        q.enq = q.enq_base = q.nb;
        q.head = q.head_base = 0;
        q.my_status = 0;
        q.my_time = 0;
        q.old_cached = s.has_cached != 0;
        q.old_left = q.old_status = 0;
        q.old_time = 0;
        q.n_fwd = q.n_drop = 0;
        q.load(q.enq_base, q.e_t, q.e_s);
        q.load(0, q.h_t, q.h_s);
        inb_host_step(s, inc[h], q, until, bootstrap_end);
        q.flush();
        const bool new_cached = s.has_cached && !q.old_cached;
        if (new_cached) {
            const uint64_t i = q.head - 1;
            s.cached_tag = i < q.nb ? B.tag[b0 + i] : A.tag[a0 + (i - q.nb)];
        }
        if (lane == 0) {
            next[h] = s;
            InbHostOut o{};
            o.left_seq = q.head - (new_cached ? 1 : 0);
            o.head = q.head;
            o.old_time = q.old_time;
            o.old_left = q.old_left;
            o.old_status = q.old_status;
            hout[h] = o;
            cnt[h] = o.left_seq + q.old_left;
            rem[h] = q.n - q.head;
        }
        if (s.pending) wake = s.wake;
        fwd = q.n_fwd;
        drop = q.n_drop;
        cached = s.has_cached;
    } else if (h == num_hosts && lane == 0) {
        cnt[h] = 0;  // the scans' total slots
        rem[h] = 0;
    }
    __shared__ unsigned long long s_wake[INB_HOSTS_PER_WG];
    __shared__ uint32_t s_cnt[3][INB_HOSTS_PER_WG];
    if (lane == 0) {
        s_wake[w] = wake;
        s_cnt[0][w] = fwd;
        s_cnt[1][w] = drop;
        s_cnt[2][w] = cached;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // one same-address atomic per workgroup and value
        unsigned long long f = 0, d = 0, c = 0;
        for (int q = 0; q < INB_HOSTS_PER_WG; ++q) {
            wake = s_wake[q] < wake ? s_wake[q] : wake;
            f += s_cnt[0][q];
            d += s_cnt[1][q];
            c += s_cnt[2][q];
        }
        if (wake != ~0ull) atomicMin(&red->min_wake, wake);
        if (f) atomicAdd(&red->forwarded, f);
        if (d) atomicAdd(&red->dropped, d);
        if (c) atomicAdd(&red->cached, c);
    }
}

// One wave per host: the packets that left, into the caller's arrays at out_off[h]; the un-popped
// suffix of the sequence into the spare backlog at nb_off[h].
__global__ void __launch_bounds__(64 * INB_HOSTS_PER_WG)
    k_inb_commit(const InbHost* __restrict__ cur, InbBacklog B, InbArrivals A, uint32_t num_hosts,
                 const uint8_t* __restrict__ scr_status, const uint64_t* __restrict__ scr_time,
                 const InbHostOut* __restrict__ hout, const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out_status,
                 uint64_t* __restrict__ out_time, uint64_t* __restrict__ out_tag, InbBacklog NB) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t h = blockIdx.x * INB_HOSTS_PER_WG + (threadIdx.x >> 6);
    if (h >= num_hosts) return;
    const uint64_t b0 = B.host_off[h], nb = B.host_off[h + 1] - b0, a0 = A.host_off[h], n = nb + (A.host_off[h + 1] - a0);
    const InbHostOut o = hout[h];
    uint64_t dst = out_off[h];
    if (o.old_left) {
        if (lane == 0) {
            out_status[dst] = o.old_status;
            out_time[dst] = o.old_time;
            out_tag[dst] = cur[h].cached_tag;
        }
        ++dst;
    }
    for (uint64_t i = lane; i < o.left_seq; i += 64) {
        out_status[dst + i] = scr_status[b0 + a0 + i];
        out_time[dst + i] = scr_time[b0 + a0 + i];
        out_tag[dst + i] = i < nb ? B.tag[b0 + i] : A.tag[a0 + (i - nb)];
    }
    const uint64_t k0 = NB.host_off[h];
    for (uint64_t i = o.head + lane; i < n; i += 64) {
        const uint64_t k = k0 + (i - o.head);
        if (i < nb) {
            NB.time[k] = B.time[b0 + i];
            NB.size[k] = B.size[b0 + i];
            NB.tag[k] = B.tag[b0 + i];
        } else {
            NB.time[k] = A.time[a0 + (i - nb)];
            NB.size[k] = A.size[a0 + (i - nb)];
            NB.tag[k] = A.tag[a0 + (i - nb)];
        }
    }
}

// refill increments and the initial records, from the hosts' bandwidths
__global__ void __launch_bounds__(256) k_inb_init(const uint64_t* __restrict__ bw, uint32_t num_hosts, uint64_t sim_start,
                                                  uint64_t* __restrict__ inc, InbHost* __restrict__ a, InbHost* __restrict__ b) {
    for (size_t h = blockIdx.x * (size_t)blockDim.x + threadIdx.x; h < num_hosts; h += (size_t)gridDim.x * blockDim.x) {
        const uint64_t r = inb_refill_increment(bw[h]);
        InbHost s;
        inb_host_init(s, r, sim_start);
        inc[h] = r;
        a[h] = s;
        b[h] = s;
    }
}

#ifdef SRG_TEST_HOOKS
// TEST HOOK: the control law's increments as the device computes them
__global__ void __launch_bounds__(256) k_inb_test_law(const uint64_t* __restrict__ counts, uint32_t n,
                                                      uint64_t* __restrict__ out) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = inb_control_increment(counts[i]);
}
#endif

}  // namespace srg
