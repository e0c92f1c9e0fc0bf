// evq_merge.h — the key form, the key compare and the merge-path search of the device-resident
// per-host event queues, shared by the kernels (event_queue.hip.h) and a CPU unit test
// (tests/cpp/evq_merge_check.cpp, built with g++).  No HIP types.
//
// A queued packet event is three 64-bit words that compare as plain lexicographic integers in the
// queues' total order (dst_host, time, src_host_id, src_host_event_id) -- Event::partial_cmp,
// event.rs:84-155, with the owning host in front:
//     w0 = dst_host << 32 | time >> 32        w1 = time << 32 | src_host        w2 = event_id
// Every field is recoverable, none is narrowed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SRG_EVQ_HD __host__ __device__
#else
#define SRG_EVQ_HD
#endif

namespace srg {

struct EvqKey {
    uint64_t w0, w1, w2;
};

SRG_EVQ_HD inline EvqKey evq_pack(uint32_t dst_host, uint64_t time, uint32_t src_host, uint64_t event_id) {
    return EvqKey{(uint64_t)dst_host << 32 | time >> 32, time << 32 | src_host, event_id};
}
SRG_EVQ_HD inline uint32_t evq_dst(uint64_t w0) { return (uint32_t)(w0 >> 32); }
SRG_EVQ_HD inline uint64_t evq_time(uint64_t w0, uint64_t w1) { return w0 << 32 | w1 >> 32; }
SRG_EVQ_HD inline uint32_t evq_src(uint64_t w1) { return (uint32_t)w1; }

SRG_EVQ_HD inline bool evq_less(const EvqKey& x, const EvqKey& y) {
    if (x.w0 != y.w0) return x.w0 < y.w0;
    if (x.w1 != y.w1) return x.w1 < y.w1;
    return x.w2 < y.w2;
}
SRG_EVQ_HD inline bool evq_equal(const EvqKey& x, const EvqKey& y) {
    return x.w0 == y.w0 && x.w1 == y.w1 && x.w2 == y.w2;
}

// Merge path: how many of the first `diag` outputs of merge(A, B) come from A, with A first on
// equal keys.  a(i) / b(i) return the EvqKey at index i of sorted sequences of na / nb keys;
// diag <= na + nb.  One binary search over the diagonal.
template <class FA, class FB>
SRG_EVQ_HD inline uint64_t evq_merge_path(const FA& a, uint64_t na, const FB& b, uint64_t nb, uint64_t diag) {
    uint64_t lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (evq_less(b(diag - 1 - mid), a(mid))) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The resident array A keeps each host's popped (dead) events as a prefix of the host's segment:
// host h owns A[host_off[h], host_off[h+1]), of which [host_off[h], head[h]) is dead.
// dead_excl[h] = the dead events of the hosts below h (an exclusive scan of head - host_off,
// num_hosts + 1 entries).  Returns the dead events among A[0, a); dst_of_a = the host of A[a]
// (unused when a == na).
SRG_EVQ_HD inline uint64_t evq_dead_before(uint64_t a, uint64_t na, uint32_t dst_of_a, const uint64_t* host_off,
                                           const uint64_t* head, const uint64_t* dead_excl, uint32_t num_hosts) {
    if (a >= na) return dead_excl[num_hosts];
    const uint64_t upto = a < head[dst_of_a] ? a : head[dst_of_a];
    return dead_excl[dst_of_a] + (upto - host_off[dst_of_a]);
}

// lower bound: the first index in [lo, hi) whose key is not below k
template <class FA>
SRG_EVQ_HD inline uint64_t evq_lower_bound(const FA& a, uint64_t lo, uint64_t hi, const EvqKey& k) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (evq_less(a(mid), k)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace srg
