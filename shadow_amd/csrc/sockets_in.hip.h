// sockets_in.hip.h — interface receive on the device (gfx950): the socket lookup, the UDP receive
// buffers and the tracker's input counters (sockets_in_rule.h) over the arrays the inbound step, the
// round's receive half or the round's send half write, plus a packet table indexed by tag.
//
// Resident form: one SinSocket record per slot (sock_off[H + 1] gives a host's first slot), five
// counters per host, the association table (open addressing, 32-byte entries, load factor <= 1/2:
// a probe is one 128-byte line, which holds four consecutive entries) and a flat message store
// grouped by socket (tag, recv_time, payload; msg_off[S + 1]).  Two sets of everything a step
// changes: a step builds the spare set, and the host side makes it current only after the device
// flags were read back.
//
//   k_sin_lookup    one thread per row: the row's host (binary search of the offsets), the packet's
//                   header by tag, at most two probes, the socket's filter.  Rows that end here get
//                   their status; rows that go on to a buffer get the socket as their sort key.  The
//                   tracker's counters are reduced per (wave, host) segment -- ballot of the lanes on
//                   the leader's host, wave sums, one lane adds -- not per packet.  Also validates
//                   both offset arrays and the tags.
//   (hipcub exclusive sum of the delivery flags)
//   k_sin_compact   the deliveries' times and rows, compacted; the compacted host offsets
//   k_sin_reads     one thread per read: validation, then its place in its host's merged order: the
//                   deliveries before it by binary search (sin_read_before is monotone)
//   k_sin_delivs    one thread per delivery: time order against its predecessor, the reads before it
//                   by binary search
//   (hipcub stable radix sort of the merged operations by socket; k_sin_segments: each socket's run)
//   k_sin_chain     one wave64 per socket, four per workgroup, 64 operations per pass, one per
//                   lane.  A pass is cut into runs of one kind by the ballot of the kinds.  len_bytes
//                   only grows inside a run of deliveries, so the buffered ones are the prefix with
//                   len + (exclusive scan of the payloads) < limit: one wave scan and one ballot.  A
//                   run of reads pops min(popping reads, messages): a read's message is the one at
//                   "popping reads before it".  Before the runs, the whole pass is tried at once on
//                   the assumption that no delivery of it is refused (the count is then a prefix sum
//                   with a running minimum, len_bytes a prefix sum of payloads in and out); the runs
//                   are walked only when that assumption fails.  Everything the control flow depends
//                   on comes from ballots, so the wave never diverges; the state (len, count, popped,
//                   appended) is wave-uniform in scalar registers and no lane-indexed array exists.
//   (hipcub exclusive sum of the new message counts)
//   k_sin_commit    one wave per socket: the surviving old messages and the newly buffered ones into
//                   the spare store
// A socket is sequential only across passes (across runs, in a pass that refuses a delivery): a step
// costs (passes of the busiest socket) x (latency of a pass), a pass being 64 operations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sockets_in_rule.h"

namespace srg {

constexpr uint32_t SIN_BAD_OFFSETS = 1;   // offsets not monotone / not ending at the count
constexpr uint32_t SIN_BAD_TAG = 2;       // a delivery's tag >= num_packets
constexpr uint32_t SIN_BACKWARD = 4;      // a delivery / read earlier than its host's previous one
constexpr uint32_t SIN_BAD_SLOT = 8;      // a read on a slot >= sockets_per_host[h] or on an EXTERNAL slot
constexpr uint32_t SIN_BAD_FLAG = 16;     // an unknown read flag
constexpr uint32_t SIN_CONTRADICT = 32;   // SIN_READ_FIRST behind a read without it at the same time
constexpr int SIN_SOCKS_PER_WG = 4;
constexpr uint32_t SIN_IS_READ = 0x80000000u;

struct SinPackets {
    uint64_t n;
    const uint8_t* protocol;
    const uint32_t* src_ip;
    const uint16_t* src_port;
    const uint16_t* dst_port;
    const uint32_t* total;
    const uint32_t* payload;
};

struct SinRows {
    uint64_t n;
    const uint8_t* status;  // null: every row is a delivery
    const uint64_t* time;
    const uint64_t* tag;
    const uint64_t* host_off;  // [H + 1]
    uint8_t deliver_status;
};

struct SinReads {
    uint64_t n;
    const uint64_t* time;
    const uint32_t* slot;
    const uint8_t* flags;  // null: all 0
    const uint64_t* host_off;  // [H + 1]
};

struct SinMsgs {
    uint64_t* tag;
    uint64_t* time;
    uint32_t* payload;
    uint64_t* off;  // [S + 1]
};

// what a step reads back (one copy)
struct SinReduce {
    unsigned long long status[6];  // rows per SIN_* status
    unsigned long long num_read, num_would_block;
    uint32_t flags, pad;
};

// per socket, what the chain left for the commit
struct SinSockOut {
    uint64_t popped, appended;
};

__device__ __forceinline__ uint64_t sin_wave_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor((unsigned long long)v, off, 64);
    return v;
}

__device__ __forceinline__ uint64_t sin_wave_inclusive(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = __shfl_up((unsigned long long)v, off, 64);
        if (lane >= (uint32_t)off) v += o;
    }
    return v;
}

__device__ __forceinline__ int sin_wave_inclusive_i32(int v, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= (uint32_t)off) v += o;
    }
    return v;
}

__device__ __forceinline__ int sin_wave_running_min(int v, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= (uint32_t)off) v = o < v ? o : v;
    }
    return v;
}

// the segment h with off[h] <= j < off[h + 1]; n segments (h == n: j is past the last offset)
template <class T>
__device__ __forceinline__ uint32_t sin_segment_of(const T* __restrict__ off, uint32_t n, uint64_t j) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid + 1] <= j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256)
    k_sin_lookup(SinRows R, SinReads Q, SinPackets P, const SinEntry* __restrict__ table, uint64_t mask,
                 const SinSocket* __restrict__ socks, const uint64_t* __restrict__ sock_off, uint32_t num_hosts,
                 uint32_t num_socks, uint8_t* __restrict__ out_status, uint32_t* __restrict__ out_slot,
                 uint32_t* __restrict__ act, uint32_t* __restrict__ key, unsigned long long* __restrict__ counters,
                 SinReduce* red) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    uint32_t bad = 0;
    for (size_t h = blockIdx.x * (size_t)blockDim.x + threadIdx.x; h <= num_hosts; h += stride) {
        const uint64_t o = R.host_off[h], r = Q.host_off[h];
        if (h == 0 && (o != 0 || r != 0)) bad |= SIN_BAD_OFFSETS;
        if (h == num_hosts ? o != R.n : o > R.host_off[h + 1]) bad |= SIN_BAD_OFFSETS;
        if (h == num_hosts ? r != Q.n : r > Q.host_off[h + 1]) bad |= SIN_BAD_OFFSETS;
    }
    uint32_t n_status[4] = {0, 0, 0, 0};  // SKIPPED, NO_SOCKET, EXTERNAL, PEER_MISMATCH (wave-uniform counts)
    // whole waves stay in the loop together (the ballots need every lane)
    for (size_t j0 = blockIdx.x * (size_t)blockDim.x + (threadIdx.x & ~63u); j0 < R.n; j0 += stride) {
        const size_t j = j0 + lane;
        const bool in_range = j < R.n;
        uint32_t h = 0, slot = SIN_NO_SLOT, k = num_socks, total = 0, payload = 0;
        uint8_t st = SIN_SKIPPED;
        bool found = false;
        if (in_range) {
            h = sin_segment_of(R.host_off, num_hosts, j);
            const bool deliver = !R.status || R.status[j] == R.deliver_status;
            if (deliver && h < num_hosts) {
                st = SIN_NO_SOCKET;
                const uint64_t g = R.tag[j];
                if (g >= P.n) {
                    bad |= SIN_BAD_TAG;
                } else {
                    const uint32_t sip = P.src_ip[g];
                    const uint16_t sport = P.src_port[g];
                    slot = sin_lookup(table, mask, h, P.protocol[g], P.dst_port[g], sip, sport);
                    if (slot != SIN_NO_SLOT) {
                        found = true;
                        total = P.total[g];
                        payload = P.payload[g];
                        const uint32_t sidx = (uint32_t)(sock_off[h] + slot);
                        st = sin_filter(socks[sidx], sip, sport);
                        if (st == SIN_BUFFERED) k = sidx;  // (the chain writes this row's status)
                    }
                }
            }
            act[j] = st != SIN_SKIPPED;
            key[j] = k;
            out_slot[j] = slot;
            if (st != SIN_BUFFERED) out_status[j] = st;
        }
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) n_status[c] += (uint32_t)__popcll(__ballot(in_range && st == c));
        // the tracker: one reduction per host present in the wave
        uint64_t rem = __ballot(found);
        while (rem) {
            const int leader = __ffsll((unsigned long long)rem) - 1;
            const uint32_t h0 = __shfl(h, leader, 64);
            const bool mine = found && h == h0;
            const uint64_t m = __ballot(mine);
            const bool data = mine && payload > 0, ctl = mine && payload == 0;
            const uint64_t pc = (uint64_t)__popcll(__ballot(ctl)), pd = (uint64_t)__popcll(__ballot(data));
            const uint64_t bch = sin_wave_sum(ctl ? (uint64_t)total : 0ull);
            const uint64_t bdh = sin_wave_sum(data ? (uint64_t)(total - payload) : 0ull);
            const uint64_t bdp = sin_wave_sum(data ? (uint64_t)payload : 0ull);
            if ((int)lane == leader) {
                unsigned long long* c = counters + (size_t)h0 * 5;
                if (pc) atomicAdd(c + 0, pc);
                if (pd) atomicAdd(c + 1, pd);
                if (bch) atomicAdd(c + 2, bch);
                if (bdh) atomicAdd(c + 3, bdh);
                if (bdp) atomicAdd(c + 4, bdp);
            }
            rem &= ~m;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (n_status[c]) atomicAdd(&red->status[c], (unsigned long long)n_status[c]);
    }
    if (bad) atomicOr(&red->flags, bad);  // invalid input only
}

// pos: the exclusive sum of act over [0, n]
__global__ void __launch_bounds__(256)
    k_sin_compact(SinRows R, const uint32_t* __restrict__ act, const uint32_t* __restrict__ pos, uint32_t num_hosts,
                  uint64_t* __restrict__ c_time, uint32_t* __restrict__ c_row, uint32_t* __restrict__ coff) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t h = blockIdx.x * (size_t)blockDim.x + threadIdx.x; h <= num_hosts; h += stride)
        coff[h] = pos[R.host_off[h]];
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < R.n; j += stride)
        if (act[j]) {
            const uint32_t k = pos[j];
            c_time[k] = R.time[j];
            c_row[k] = (uint32_t)j;
        }
}

// A host's merged order is its compacted deliveries and its reads interleaved by sin_read_before;
// the host's merged segment starts at coff[h] + Q.host_off[h].
__global__ void __launch_bounds__(256)
    k_sin_reads(SinReads Q, const SinSocket* __restrict__ socks, const uint64_t* __restrict__ sock_off, uint32_t num_hosts,
                uint32_t num_socks, const uint64_t* __restrict__ c_time, const uint32_t* __restrict__ coff,
                uint32_t* __restrict__ mkey, uint32_t* __restrict__ mval, SinReduce* red) {
    uint32_t bad = 0;
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < Q.n; j += (size_t)gridDim.x * blockDim.x) {
        const uint32_t h = sin_segment_of(Q.host_off, num_hosts, j);
        if (h >= num_hosts) continue;
        const uint64_t t = Q.time[j];
        const uint8_t f = Q.flags ? Q.flags[j] : 0;
        const uint32_t slot = Q.slot[j];
        uint32_t k = num_socks, b = 0;
        if (f & ~(SIN_READ_PEEK | SIN_READ_FIRST)) b |= SIN_BAD_FLAG;
        if (slot >= sock_off[h + 1] - sock_off[h]) {
            b |= SIN_BAD_SLOT;
        } else {
            k = (uint32_t)(sock_off[h] + slot);
            if (socks[k].kind == SIN_EXTERNAL) b |= SIN_BAD_SLOT;
        }
        if (j > Q.host_off[h]) {
            const uint64_t tp = Q.time[j - 1];
            if (t < tp) b |= SIN_BACKWARD;
            if (sin_reads_contradict(tp, Q.flags ? Q.flags[j - 1] : 0, t, f)) b |= SIN_CONTRADICT;
        }
        // the deliveries before this read: the first one it does not run after
        uint32_t lo = coff[h], hi = coff[h + 1];
        const uint32_t d0 = lo;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (!sin_read_before(t, f, c_time[mid])) lo = mid + 1;
            else hi = mid;
        }
        const size_t m = (size_t)d0 + j + (lo - d0);
        mkey[m] = b ? num_socks : k;
        mval[m] = (uint32_t)j | SIN_IS_READ;
        bad |= b;
    }
    if (bad) atomicOr(&red->flags, bad);  // invalid input only
}

__global__ void __launch_bounds__(256)
    k_sin_delivs(const uint32_t* __restrict__ pos, uint64_t num_rows, SinReads Q, uint32_t num_hosts,
                 const uint64_t* __restrict__ c_time, const uint32_t* __restrict__ c_row, const uint32_t* __restrict__ coff,
                 const uint32_t* __restrict__ key, uint32_t* __restrict__ mkey, uint32_t* __restrict__ mval,
                 SinReduce* red) {
    const uint32_t nact = pos[num_rows];
    uint32_t bad = 0;
    for (size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x; k < nact; k += (size_t)gridDim.x * blockDim.x) {
        const uint32_t h = sin_segment_of(coff, num_hosts, k);
        if (h >= num_hosts) continue;
        const uint64_t t = c_time[k];
        if (k > coff[h] && t < c_time[k - 1]) bad |= SIN_BACKWARD;
        // the reads before this delivery: the first one that does not run before it
        uint64_t lo = Q.host_off[h], hi = Q.host_off[h + 1];
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (sin_read_before(Q.time[mid], Q.flags ? Q.flags[mid] : 0, t)) lo = mid + 1;
            else hi = mid;
        }
        const size_t m = k + lo;  // = coff[h] + Q.host_off[h] + (k - coff[h]) + (lo - Q.host_off[h])
        const uint32_t row = c_row[k];
        mkey[m] = key[row];
        mval[m] = row;
    }
    if (bad) atomicOr(&red->flags, bad);  // invalid input only
}

// ops_off[s] = the first sorted operation with key >= s, for s in [0, S + 1]
__global__ void __launch_bounds__(256)
    k_sin_segments(const uint32_t* __restrict__ skey, uint32_t num_ops, uint32_t num_socks, uint32_t* __restrict__ ops_off) {
    for (size_t s = blockIdx.x * (size_t)blockDim.x + threadIdx.x; s <= (size_t)num_socks + 1;
         s += (size_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = num_ops;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (skey[mid] < s) lo = mid + 1;
            else hi = mid;
        }
        ops_off[s] = lo;
    }
}

__global__ void __launch_bounds__(64 * SIN_SOCKS_PER_WG)
    k_sin_chain(const SinSocket* __restrict__ cur, SinSocket* __restrict__ next, SinMsgs M, SinRows R, SinReads Q,
                SinPackets P, uint32_t num_socks, const uint32_t* __restrict__ sval, const uint32_t* __restrict__ ops_off,
                uint32_t* bufl, uint8_t* __restrict__ out_status, uint8_t* __restrict__ r_status,
                uint64_t* __restrict__ r_tag, uint64_t* __restrict__ r_time, uint32_t* __restrict__ r_payload,
                uint64_t* __restrict__ cnt, SinSockOut* __restrict__ sout, SinReduce* red) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t s = blockIdx.x * SIN_SOCKS_PER_WG + w;
    uint32_t n_full = 0, n_buf = 0, n_read = 0, n_wb = 0;
    if (s < num_socks) {
        SinSocket rec = cur[s];
        const uint32_t o0 = ops_off[s], o1 = ops_off[s + 1];
        const uint64_t m0 = M.off[s], nold = rec.count;
        uint64_t popped = 0, appended = 0;
        for (uint32_t base = o0; base < o1; base += 64) {
            const uint32_t e = base + lane;
            const bool in = e < o1;
            const uint32_t v = in ? sval[e] : 0u;
            const bool is_read = in && (v & SIN_IS_READ);
            const uint32_t idx = v & ~SIN_IS_READ;  // a read's index, a delivery's row
            uint8_t f = 0;
            uint32_t pay = 0;
            if (is_read) f = Q.flags ? Q.flags[idx] : 0;
            else if (in) pay = P.payload[R.tag[idx]];
            const uint64_t rmask = __ballot(is_read);
            const uint32_t nin = (uint32_t)__popcll(__ballot(in));
            {
                // The whole pass at once, on the assumption that none of its deliveries is refused.
                // Then the count follows c' = max(c + x, 0) with x = +1 (delivery), -1 (popping read),
                // 0 (peek), whose solution is c + S_i - min(0, c + min_{k<=i} S_k) over the prefix
                // sums S; a read gets a message iff the count before it is positive, the popped
                // messages are the store's next ones in order, and len_bytes before an operation is
                // len + (payloads delivered) - (payloads popped) before it.  The assumption is then
                // checked: every delivery must have found len_bytes < limit.  Otherwise nothing of
                // this block counts and the pass is walked run by run below.
                const bool is_del = in && !is_read;
                const bool popping = is_read && !(f & SIN_READ_PEEK);
                const uint64_t lt = (1ull << lane) - 1;
                const int sum = sin_wave_inclusive_i32(is_del ? 1 : popping ? -1 : 0, lane);
                const int64_t low = (int64_t)rec.count + sin_wave_running_min(sum, lane);
                const int64_t c_after = (int64_t)rec.count + sum - (low < 0 ? low : 0);
                int64_t c_before = __shfl_up((long long)c_after, 1, 64);
                if (lane == 0) c_before = (int64_t)rec.count;
                const bool gets = is_read && c_before > 0;
                const uint64_t smask = __ballot(popping && gets), dmask = __ballot(is_del);
                const uint32_t nd = (uint32_t)__popcll(dmask), ns = (uint32_t)__popcll(smask);
                if (is_del) bufl[o0 + appended + (uint32_t)__popcll(dmask & lt)] = idx;
                if (nd) __threadfence_block();  // the reads below load bufl from other lanes
                uint64_t g = 0, t = 0;
                uint32_t mp = 0;
                if (gets) {
                    const uint64_t q = popped + (uint32_t)__popcll(smask & lt);
                    if (q < nold) {
                        g = M.tag[m0 + q];
                        t = M.time[m0 + q];
                        mp = M.payload[m0 + q];
                    } else {
                        const uint32_t row = __hip_atomic_load(bufl + o0 + (q - nold), __ATOMIC_RELAXED,
                                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                        g = R.tag[row];
                        t = R.time[row];
                        mp = P.payload[g];
                    }
                }
                // (unsigned wrap-around arithmetic: the true value is never negative)
                const uint64_t delta = is_del ? (uint64_t)pay : popping && gets ? 0ull - (uint64_t)mp : 0ull;
                const uint64_t moved = sin_wave_inclusive(delta, lane);
                const bool refused = is_del && !sin_has_space(rec.len, moved - delta, rec.limit);
                if (__ballot(refused) == 0) {
                    if (is_del) out_status[idx] = SIN_BUFFERED;
                    if (is_read) {
                        r_status[idx] = gets ? 1 : 0;
                        r_tag[idx] = g;
                        r_time[idx] = t;
                        r_payload[idx] = mp;
                    }
                    rec.len += __shfl((unsigned long long)moved, 63, 64);
                    rec.count = rec.count + nd - ns;
                    appended += nd;
                    popped += ns;
                    n_buf += nd;
                    const uint32_t ng = (uint32_t)__popcll(__ballot(gets));
                    n_read += ng;
                    n_wb += (uint32_t)__popcll(rmask) - ng;
                    continue;
                }
            }
            uint32_t at = 0;
            while (at < nin) {
                const bool reads = (rmask >> at) & 1;
                const uint64_t inmask = nin == 64 ? ~0ull : ((1ull << nin) - 1);
                const uint64_t other = (reads ? ~rmask : rmask) & inmask & (~0ull << at);
                const uint32_t end = other ? (uint32_t)(__ffsll((unsigned long long)other) - 1) : nin;
                const bool in_run = lane >= at && lane < end;
                if (!reads) {
                    const uint64_t p = in_run ? (uint64_t)pay : 0ull;
                    const uint64_t before = sin_wave_inclusive(p, lane) - p;
                    const bool ok = in_run && sin_has_space(rec.len, before, rec.limit);
                    const uint32_t nb = (uint32_t)__popcll(__ballot(ok));  // (a prefix of the run)
                    if (in_run) out_status[idx] = ok ? SIN_BUFFERED : SIN_FULL;
                    if (ok) bufl[o0 + appended + (lane - at)] = idx;
                    rec.len += sin_wave_sum(ok ? p : 0ull);
                    rec.count += nb;
                    appended += nb;
                    n_buf += nb;
                    n_full += end - at - nb;
                    if (nb) __threadfence_block();  // a later run's reads load bufl from other lanes
                } else {
                    const bool popping = in_run && !(f & SIN_READ_PEEK);
                    const uint64_t pm = __ballot(popping);
                    const uint32_t x = (uint32_t)__popcll(pm & ((1ull << lane) - 1));
                    const bool gets = in_run && (uint64_t)x < rec.count;
                    uint64_t g = 0, t = 0;
                    uint32_t mp = 0;
                    if (gets) {
                        const uint64_t q = popped + x;
                        if (q < nold) {
                            g = M.tag[m0 + q];
                            t = M.time[m0 + q];
                            mp = M.payload[m0 + q];
                        } else {
                            const uint32_t row = __hip_atomic_load(bufl + o0 + (q - nold), __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_WORKGROUP);
                            g = R.tag[row];
                            t = R.time[row];
                            mp = P.payload[g];
                        }
                    }
                    if (in_run) {
                        r_status[idx] = gets ? 1 : 0;
                        r_tag[idx] = g;
                        r_time[idx] = t;
                        r_payload[idx] = mp;
                    }
                    const uint64_t np = (uint64_t)__popcll(pm);
                    const uint64_t npop = np < rec.count ? np : rec.count;
                    rec.len -= sin_wave_sum(popping && gets ? (uint64_t)mp : 0ull);
                    rec.count -= npop;
                    popped += npop;
                    const uint32_t ng = (uint32_t)__popcll(__ballot(gets));
                    n_read += ng;
                    n_wb += end - at - ng;
                }
                at = end;
            }
        }
        if (lane == 0) {
            next[s] = rec;
            cnt[s] = rec.count;
            sout[s] = SinSockOut{popped, appended};
        }
    } else if (s == num_socks && lane == 0) {
        cnt[s] = 0;  // the scan's total slot
    }
    __shared__ uint32_t s_cnt[4][SIN_SOCKS_PER_WG];
    if (lane == 0) {
        s_cnt[0][w] = n_full;
        s_cnt[1][w] = n_buf;
        s_cnt[2][w] = n_read;
        s_cnt[3][w] = n_wb;
    }
    __syncthreads();
    if (threadIdx.x < 4) {  // one same-address atomic per workgroup and value
        unsigned long long a = 0;
        for (int q = 0; q < SIN_SOCKS_PER_WG; ++q) a += s_cnt[threadIdx.x][q];
        unsigned long long* dst = threadIdx.x == 0   ? &red->status[SIN_FULL]
                                  : threadIdx.x == 1 ? &red->status[SIN_BUFFERED]
                                  : threadIdx.x == 2 ? &red->num_read
                                                     : &red->num_would_block;
        if (a) atomicAdd(dst, a);
    }
}

// One wave per socket: message q of the socket's sequence (its old messages, then the ones this
// step buffered) goes to the spare store at new_off[s] + q - popped, for q >= popped.
__global__ void __launch_bounds__(64 * SIN_SOCKS_PER_WG)
    k_sin_commit(const SinSocket* __restrict__ cur, SinMsgs M, SinMsgs N, SinRows R, SinPackets P, uint32_t num_socks,
                 const uint32_t* __restrict__ ops_off, const uint32_t* __restrict__ bufl,
                 const SinSockOut* __restrict__ sout) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * SIN_SOCKS_PER_WG + (threadIdx.x >> 6);
    if (s >= num_socks) return;
    const uint64_t nold = cur[s].count, m0 = M.off[s], k0 = N.off[s];
    const SinSockOut o = sout[s];
    const uint32_t o0 = ops_off[s];
    for (uint64_t q = o.popped + lane; q < nold + o.appended; q += 64) {
        const uint64_t k = k0 + (q - o.popped);
        if (q < nold) {
            N.tag[k] = M.tag[m0 + q];
            N.time[k] = M.time[m0 + q];
            N.payload[k] = M.payload[m0 + q];
        } else {
            const uint32_t row = bufl[o0 + (q - nold)];
            const uint64_t g = R.tag[row];
            N.tag[k] = g;
            N.time[k] = R.time[row];
            N.payload[k] = P.payload[g];
        }
    }
}

struct SinConfig {
    uint64_t limit;
    uint32_t sidx, peer_ip;
    uint16_t peer_port;
    uint8_t kind, has_peer;
    uint32_t pad;
};

// srg_sockets_in_configure: the fields a caller sets; len and count stay
__global__ void __launch_bounds__(256) k_sin_configure(const SinConfig* __restrict__ c, uint64_t n, SinSocket* __restrict__ socks) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        SinSocket& s = socks[c[i].sidx];
        s.limit = c[i].limit;
        s.peer_ip = c[i].peer_ip;
        s.peer_port = c[i].peer_port;
        s.kind = c[i].kind;
        s.has_peer = c[i].has_peer;
    }
}

__global__ void __launch_bounds__(256) k_sin_init(uint32_t num_socks, SinSocket* __restrict__ a) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < num_socks; i += (size_t)gridDim.x * blockDim.x) {
        SinSocket s{};
        s.limit = SIN_DEFAULT_LIMIT;
        a[i] = s;
    }
}

}  // namespace srg
