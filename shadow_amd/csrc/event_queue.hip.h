// event_queue.hip.h — the per-host packet-event queues themselves, resident in HBM across rounds
// (gfx950): a round's sent events are merged in at the barrier, a window's events are popped out.
//
// Reference semantics (packet events only; Local events stay with the host):
//   EventQueue::push        event_queue.rs:28-36   assert!(time >= last_popped_event_time)
//   EventQueue::pop         event_queue.rs:38-49   smallest of (time, src_host_id, src_host_event_id)
//   Host::execute           host.rs:809-818        pops while next_event_time() < until
//   Host::next_event_time   host.rs:866-868        the head of what remains
//   manager's reduction     manager.rs:416-435, 459-464   min over the hosts' heads
//
// Resident form: one flat array of keys (evq_merge.h: three u64 words + the caller's tag, 32 B per
// event, as four parallel arrays) sorted by (dst_host, time, src_host, event_id); host_off[H + 1]
// bounds each host's segment, head[h] is the host's first live event (a pop only moves it: the kept
// backlog is never rewritten), last_popped[h] its last popped time.  Two sets of arrays: a push
// builds the spare set and the caller commits it after the flags were read.
//
// Push = a merge, never a re-sort of the backlog.  O(backlog + batch):
//   k_evq_gather     the batch through `order` into key form; validates index, host, strict key
//                    increase (one neighbour compare, through a lane shuffle) and time >= last_popped
//   k_evq_dead       head - host_off per host, then an exclusive scan (hipcub, on the host side)
//   k_evq_partition  one merge-path binary search per tile boundary over the two global arrays,
//                    and the number of live outputs below the boundary
//   k_evq_merge      one workgroup per tile of EVQ_TILE merged ranks: its A and B slices' keys go
//                    to LDS, each thread searches its own sub-diagonal there and merges EVQ_ITEMS
//                    ranks sequentially; popped (dead) A events are dropped on the way (a tile-local
//                    scan of the live outputs on top of the boundary's live count: compaction costs
//                    nothing extra); results leave through an LDS index stage in output order, so
//                    the global stores are coalesced.  Flags equal live keys (no order).
//   k_evq_finish     host_off and head of the merged array
// Pop.  O(popped log H + H):
//   k_evq_pop_find   per host, binary search of [head, segment end) for the first time >= until
//   (hipcub scan of the counts -> the output offsets; the total is checked against the capacity)
//   k_evq_pop_copy   one thread per popped event
//   k_evq_pop_commit head, last_popped, and the minimum of the new heads
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "events.hip.h"
#include "evq_merge.h"

namespace srg {

// The merge kernel's shape (build-time: -DSRG_EVQ_THREADS / -DSRG_EVQ_ITEMS for an A/B of two builds).
// Measured on the C5 push (10^7 events into 10^8, profiles/event_queues/tile_shapes.txt): 256 x 8
// (49 KB of keys in LDS, two workgroups per CU) 3.53 ms, 512 x 4 2.79 ms, 256 x 4 2.57 ms, 128 x 4
// 2.60 ms, 256 x 2 2.50 ms: the short sequential run and five and more workgroups per CU are what
// counts; below 1024 ranks per tile the differences are inside the spreads.
#ifndef SRG_EVQ_THREADS
#define SRG_EVQ_THREADS 256
#endif
#ifndef SRG_EVQ_ITEMS
#define SRG_EVQ_ITEMS 4
#endif
constexpr int EVQ_THREADS = SRG_EVQ_THREADS;
constexpr int EVQ_ITEMS = SRG_EVQ_ITEMS;
constexpr int EVQ_TILE = EVQ_THREADS * EVQ_ITEMS;  // merged ranks per workgroup: 24 KB of keys in LDS

constexpr uint32_t EVQ_BAD_ORDER = 1;      // order entry / dst_host out of range, or keys not strictly increasing
constexpr uint32_t EVQ_TIME_BACKWARD = 2;  // a pushed event earlier than its host's last popped time
constexpr uint32_t EVQ_EQUAL_KEYS = 4;     // two live events with no relative order

struct EvqSet {
    uint64_t *k0, *k1, *k2, *tag;
};

struct EvqState {
    unsigned long long min_head;
    uint32_t flags;
    uint32_t pad;
};

// three parallel key-word arrays (global or LDS) read as EvqKeys
struct EvqKeys {
    const uint64_t *k0, *k1, *k2;
    __device__ __forceinline__ EvqKey operator()(uint64_t i) const { return EvqKey{k0[i], k1[i], k2[i]}; }
};

struct EvqGatherIn {
    uint64_t num_events, num_order;
    const uint32_t* order;
    const uint32_t* dst_host;
    const uint32_t* src_host;
    const uint64_t* event_id;
    const uint64_t* deliver;
    const uint64_t* tag;  // null: the event's index
    uint32_t num_hosts;
};

__device__ __forceinline__ bool evq_gather_key(const EvqGatherIn& in, uint64_t j, EvqKey& k, uint64_t& idx) {
    const uint32_t i = in.order[j];
    if (i >= in.num_events) return false;
    const uint32_t dst = in.dst_host[i];
    if (dst >= in.num_hosts) return false;
    k = evq_pack(dst, in.deliver[i], in.src_host[i], in.event_id[i]);
    idx = i;
    return true;
}

__global__ void __launch_bounds__(256) k_evq_gather(EvqGatherIn in, EvqSet b, const uint64_t* __restrict__ last_popped,
                                                    EvqState* st) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t bad = 0;
    // whole waves stay in the loop together (the shuffles below need every lane)
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j0 = blockIdx.x * (size_t)blockDim.x + (threadIdx.x & ~63u); j0 < in.num_order; j0 += stride) {
        const size_t j = j0 + lane;
        const bool in_range = j < in.num_order;
        EvqKey k{~0ull, ~0ull, ~0ull};
        uint64_t idx = 0;
        bool ok = in_range && evq_gather_key(in, j, k, idx);
        if (in_range && !ok) bad |= EVQ_BAD_ORDER;
        // the predecessor's key: the lane below, or for lane 0 a gather of its own
        EvqKey p;
        p.w0 = __shfl_up((unsigned long long)k.w0, 1, 64);
        p.w1 = __shfl_up((unsigned long long)k.w1, 1, 64);
        p.w2 = __shfl_up((unsigned long long)k.w2, 1, 64);
        bool pok = __shfl_up((int)ok, 1, 64) != 0;
        if (lane == 0) {
            uint64_t pidx;
            pok = j > 0 && in_range && evq_gather_key(in, j - 1, p, pidx);
        }
        if (ok) {
            if (j > 0 && pok && !evq_less(p, k)) bad |= EVQ_BAD_ORDER;
            if (evq_time(k.w0, k.w1) < last_popped[evq_dst(k.w0)]) bad |= EVQ_TIME_BACKWARD;
            b.k0[j] = k.w0;
            b.k1[j] = k.w1;
            b.k2[j] = k.w2;
            b.tag[j] = in.tag ? in.tag[idx] : idx;
        }
    }
    if (bad) atomicOr(&st->flags, bad);  // invalid input only
}

// dead[h] = popped events still stored in front of host h's segment; dead[H] = 0 (the scan's total slot)
__global__ void __launch_bounds__(256) k_evq_dead(const uint64_t* __restrict__ host_off, const uint64_t* __restrict__ head,
                                                  uint32_t num_hosts, uint64_t* __restrict__ dead) {
    for (size_t h = blockIdx.x * (size_t)blockDim.x + threadIdx.x; h <= num_hosts; h += (size_t)gridDim.x * blockDim.x)
        dead[h] = h < num_hosts ? head[h] - host_off[h] : 0;
}

// boundary i (0 .. ntiles) sits at merged rank min(i * EVQ_TILE, na + nb): part_a[i] = the A events
// below it, part_live[i] = the live outputs below it
__global__ void __launch_bounds__(256) k_evq_partition(EvqSet A, uint64_t na, EvqSet B, uint64_t nb,
                                                       const uint64_t* __restrict__ host_off,
                                                       const uint64_t* __restrict__ head,
                                                       const uint64_t* __restrict__ dead_excl, uint32_t num_hosts,
                                                       uint64_t ntiles, uint64_t* __restrict__ part_a,
                                                       uint64_t* __restrict__ part_live) {
    const EvqKeys fa{A.k0, A.k1, A.k2}, fb{B.k0, B.k1, B.k2};
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i <= ntiles; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t diag = (uint64_t)i * EVQ_TILE;
        if (diag > na + nb) diag = na + nb;
        const uint64_t a = evq_merge_path(fa, na, fb, nb, diag);
        const uint32_t dst = a < na ? evq_dst(A.k0[a]) : 0u;
        part_a[i] = a;
        part_live[i] = diag - evq_dead_before(a, na, dst, host_off, head, dead_excl, num_hosts);
    }
}

// LDS slots: 0 = the A event in front of the tile's A slice (the equal-key check of the tile's
// first B event looks at it), 1 .. na = the A slice, na + 1 .. na + nb = the B slice.
__global__ void __launch_bounds__(EVQ_THREADS) k_evq_merge(EvqSet A, EvqSet B, uint64_t n,
                                                           const uint64_t* __restrict__ part_a,
                                                           const uint64_t* __restrict__ part_live,
                                                           const uint64_t* __restrict__ head, EvqSet out,
                                                           uint64_t n_out, EvqState* st) {
    __shared__ uint64_t s0[EVQ_TILE + 1], s1[EVQ_TILE + 1], s2[EVQ_TILE + 1];
    __shared__ uint32_t sidx[EVQ_TILE];
    __shared__ uint8_t slive[EVQ_TILE + 1];
    __shared__ uint32_t wtot[EVQ_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t d0 = (uint64_t)blockIdx.x * EVQ_TILE;
    const uint64_t d1 = d0 + EVQ_TILE < n ? d0 + EVQ_TILE : n;
    const uint64_t a0 = part_a[blockIdx.x], a1 = part_a[blockIdx.x + 1];
    const uint64_t b0 = d0 - a0, b1 = d1 - a1;
    const uint32_t na = (uint32_t)(a1 - a0), nb = (uint32_t)(b1 - b0), total = na + nb;  // total <= EVQ_TILE
    for (uint32_t j = tid; j <= na; j += EVQ_THREADS) {
        if (j == 0 && a0 == 0) {
            s0[0] = s1[0] = s2[0] = 0;
            slive[0] = 0;
            continue;
        }
        const uint64_t g = a0 - 1 + j;
        const uint64_t w0 = A.k0[g];
        s0[j] = w0;
        s1[j] = A.k1[g];
        s2[j] = A.k2[g];
        slive[j] = g >= head[evq_dst(w0)];
    }
    for (uint32_t j = tid; j < nb; j += EVQ_THREADS) {
        const uint64_t g = b0 + j;
        s0[1 + na + j] = B.k0[g];
        s1[1 + na + j] = B.k1[g];
        s2[1 + na + j] = B.k2[g];
        slive[1 + na + j] = 1;
    }
    __syncthreads();
    const EvqKeys fa{s0 + 1, s1 + 1, s2 + 1}, fb{s0 + 1 + na, s1 + 1 + na, s2 + 1 + na};
    const uint32_t diag = tid * EVQ_ITEMS < total ? tid * EVQ_ITEMS : total;
    uint32_t a = (uint32_t)evq_merge_path(fa, na, fb, nb, diag), b = diag - a;
    uint32_t src[EVQ_ITEMS];
    uint32_t nl = 0;
    bool dup = false;
    EvqKey ka{~0ull, ~0ull, ~0ull}, kb{~0ull, ~0ull, ~0ull};
    if (a < na) ka = fa(a);
    if (b < nb) kb = fb(b);
#pragma unroll
    for (int it = 0; it < EVQ_ITEMS; ++it) {
        src[it] = ~0u;
        if (a + b < total) {
            uint32_t s;
            bool live;
            if (b >= nb || (a < na && !evq_less(kb, ka))) {  // A first on equal keys
                s = 1 + a;
                live = slive[s] != 0;
                ++a;
                if (a < na) ka = fa(a);
            } else {
                s = 1 + na + b;
                live = true;
                // an equal A event was merged right in front of this one: slot a
                if (slive[a] && s0[a] == kb.w0 && s1[a] == kb.w1 && s2[a] == kb.w2) dup = true;
                ++b;
                if (b < nb) kb = fb(b);
            }
            if (live) {
                src[it] = s;
                ++nl;
            }
        }
    }
    // the live outputs' tile-local positions: wave scan, then the waves' totals
    uint32_t incl = nl;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off, 64);
        if ((int)lane >= off) incl += y;
    }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    uint32_t pos = incl - nl, tile_live = 0;
#pragma unroll
    for (uint32_t q = 0; q < EVQ_THREADS / 64; ++q) {
        if (q < w) pos += wtot[q];
        tile_live += wtot[q];
    }
#pragma unroll
    for (int it = 0; it < EVQ_ITEMS; ++it)
        if (src[it] != ~0u) sidx[pos++] = src[it];
    __syncthreads();
    const uint64_t obase = part_live[blockIdx.x];
    for (uint32_t j = tid; j < tile_live; j += EVQ_THREADS) {
        const uint32_t s = sidx[j];
        const uint64_t p = obase + j;
        if (p < n_out) {
            out.k0[p] = s0[s];
            out.k1[p] = s1[s];
            out.k2[p] = s2[s];
            out.tag[p] = s <= na ? A.tag[a0 - 1 + s] : B.tag[b0 + (s - 1 - na)];
        }
    }
    if (dup) atomicOr(&st->flags, EVQ_EQUAL_KEYS);  // an error path only
}

// the merged array's per-host bounds (empty hosts included); every head starts at its segment
__global__ void __launch_bounds__(256) k_evq_finish(const uint64_t* __restrict__ k0, uint64_t n, uint32_t num_hosts,
                                                    uint64_t* __restrict__ host_off, uint64_t* __restrict__ head) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t d = evq_dst(k0[i]);
        if (d >= num_hosts) d = num_hosts - 1;  // (validated at the push: never taken)
        const uint32_t h0 = i ? evq_dst(k0[i - 1]) + 1 : 0;
        for (uint32_t h = h0; h <= d; ++h) host_off[h] = head[h] = i;
        if (i == n - 1) {
            for (uint32_t h = d + 1; h < num_hosts; ++h) host_off[h] = head[h] = n;
            host_off[num_hosts] = n;
        }
    }
}

// one same-address atomic per workgroup, as ev_block_reduce
__device__ __forceinline__ void evq_block_min(unsigned long long m, unsigned long long* dst) {
    m = wave_min(m);
    __shared__ unsigned long long sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (int)(blockDim.x + 63) >> 6;
        for (int q = 1; q < nw; ++q) m = min(m, sm[q]);
        if (m != ~0ull) atomicMin(dst, m);
    }
}

// min over the hosts' heads: the manager's min_next_event_time
__global__ void __launch_bounds__(256) k_evq_min(EvqSet S, const uint64_t* __restrict__ host_off,
                                                 const uint64_t* __restrict__ head, uint32_t num_hosts, EvqState* st) {
    unsigned long long m = ~0ull;
    for (size_t h = blockIdx.x * (size_t)blockDim.x + threadIdx.x; h < num_hosts; h += (size_t)gridDim.x * blockDim.x) {
        const uint64_t p = head[h];
        if (p < host_off[h + 1]) {
            const unsigned long long t = evq_time(S.k0[p], S.k1[p]);
            m = t < m ? t : m;
        }
    }
    evq_block_min(m, &st->min_head);
}

// new_head[h] = the first live event of host h with time >= until; cnt[h] = the events in front of
// it (cnt has num_hosts + 1 entries, the last 0: the scan's total slot)
__global__ void __launch_bounds__(256) k_evq_pop_find(EvqSet S, const uint64_t* __restrict__ host_off,
                                                      const uint64_t* __restrict__ head, uint32_t num_hosts,
                                                      uint64_t until, uint64_t* __restrict__ new_head,
                                                      uint64_t* __restrict__ cnt) {
    const EvqKeys f{S.k0, S.k1, S.k2};
    for (size_t h = blockIdx.x * (size_t)blockDim.x + threadIdx.x; h <= num_hosts; h += (size_t)gridDim.x * blockDim.x) {
        if (h == num_hosts) {
            cnt[h] = 0;
            continue;
        }
        const uint64_t lo = head[h];
        const uint64_t p = evq_lower_bound(f, lo, host_off[h + 1], evq_pack((uint32_t)h, until, 0u, 0ull));
        new_head[h] = p;
        cnt[h] = p - lo;
    }
}

// popped event j belongs to the host h with offs[h] <= j < offs[h + 1]
__global__ void __launch_bounds__(256) k_evq_pop_copy(EvqSet S, const uint64_t* __restrict__ head,
                                                      const uint64_t* __restrict__ offs, uint32_t num_hosts,
                                                      uint64_t total, uint64_t* __restrict__ out_time,
                                                      uint32_t* __restrict__ out_src, uint64_t* __restrict__ out_id,
                                                      uint64_t* __restrict__ out_tag) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < total; j += (size_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = num_hosts;  // the first h in [0, H] with offs[h] > j, minus one
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (offs[mid + 1] <= j) lo = mid + 1;
            else hi = mid;
        }
        const uint64_t p = head[lo] + (j - offs[lo]);
        const uint64_t w0 = S.k0[p], w1 = S.k1[p];
        out_time[j] = evq_time(w0, w1);
        if (out_src) out_src[j] = evq_src(w1);
        if (out_id) out_id[j] = S.k2[p];
        out_tag[j] = S.tag[p];
    }
}

__global__ void __launch_bounds__(256) k_evq_pop_commit(EvqSet S, const uint64_t* __restrict__ host_off,
                                                        uint64_t* __restrict__ head, uint64_t* __restrict__ last_popped,
                                                        const uint64_t* __restrict__ new_head, uint32_t num_hosts,
                                                        EvqState* st) {
    unsigned long long m = ~0ull;
    for (size_t h = blockIdx.x * (size_t)blockDim.x + threadIdx.x; h < num_hosts; h += (size_t)gridDim.x * blockDim.x) {
        const uint64_t p = new_head[h];
        if (p > head[h]) {
            last_popped[h] = evq_time(S.k0[p - 1], S.k1[p - 1]);
            head[h] = p;
        }
        if (p < host_off[h + 1]) {
            const unsigned long long t = evq_time(S.k0[p], S.k1[p]);
            m = t < m ? t : m;
        }
    }
    evq_block_min(m, &st->min_head);
}

}  // namespace srg
