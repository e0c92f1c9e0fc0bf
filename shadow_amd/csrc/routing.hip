// routing.hip -- MI355X routing-table builder: device pipeline + C ABI (include/shadow_routing.h).
//
// Replaces NetworkGraph::compute_shortest_paths (src/main/network/graph/mod.rs:183-228) and
// NetworkGraph::get_direct_paths (mod.rs:230-252).  compute_device chooses the build:
//   dense (run_dense)    k_edge_scan / k_lat_gcd validate; k_w_key + k_w_split build W; blocked
//                        min-plus Floyd-Warshall (symmetric over line buffers when undirected);
//                        k_certify, k_extract; then k_ess_mask -> tight_v5 -> k_loss_rows, or
//                        tight_scan -> k_loss_round above the sparse-scan threshold
//   sparse (run_sparse)  batched delta-stepping + loss fold (k_sparse_ds), or the lexicographic
//                        Bellman-Ford sweeps (k_sparse_bf) for u64 labels
// Files: env_switches.h (every SRG_* environment switch), host_pool.h (host worker pool), plan.h
// (rank / XCD / scan-group splits), entry_plan.h (the rank row / edge split, the host entry's
// flags) -- all four without HIP; dense.hip.h (run_dense) and sparse_run.hip.h (run_sparse,
// choose_sparse), sections of this translation unit; the device headers (kernels, tight_sparse,
// sparse, sparse_ds, events, event_queue, xchg); routes.hip.h (route tracing and link loads over a
// finished table, rule in route_rule.h) and route_trees.hip.h (whole route trees and loads pushed
// up them, rules in route_tree_rule.h), sections too; stage.hip.h (what the resident stages share:
// scan, grow, read-back, the two sets, create / destroy) and the stages, each with its srg_*
// entry points beside its struct and drivers: events_run.hip.h (the packet-event batch and the
// event queues), inbound_run.hip.h and outbound_run.hip.h (the hosts' inbound and outbound paths:
// kernels in inbound.hip.h / outbound.hip.h, rules in inbound_rule.h / outbound_rule.h),
// round_run.hip.h (a round over the three), sockets_in_run.hip.h (interface receive: kernels in
// sockets_in.hip.h, rule in sockets_in_rule.h); h2d_codec.hip.h (the host entry's plain copy, H2D
// codec and late-loss thread) and host_entry.hip.h (the host entry, stage by stage), the last two
// sections.
// Still here, in order: the validation / W / certify / extract kernels, the context (srg_ctx),
// prelude(), HostSink, the FW schedules (stream_hop, fw_blocked, SymFw, FwOverlap),
// compute_device, direct paths, guard(), device_call(), the rest of extern "C".
// No CPU fallback: every entry point fails loudly (status code) when HIP is unavailable.
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/shadow_routing.h"
#include "internal.h"
#include "env_switches.h"
#include "host_pool.h"
#include "plan.h"
#include "kernels.hip.h"
#include "guards.h"
#include "edge_codec.h"
#include "tight_sparse.hip.h"
#include "comm.h"
#include "sparse.hip.h"
#include "sparse_ds.hip.h"
#include "events.hip.h"
#include "route_rule.h"
#include "route_tree_rule.h"
#include "event_queue.hip.h"
#include "inbound.hip.h"
#include "outbound.hip.h"
#include "round.hip.h"
#include "sockets_in.hip.h"
#include "xchg.hip.h"

#include <hipcub/hipcub.hpp>

using namespace srg;

namespace {

struct Failure {
    int code;
    std::string msg;
};

[[noreturn]] void fail(int code, const std::string& m) { throw Failure{code, m}; }

#define HIP_CHECK(expr)                                                                           \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            if (e_ == hipErrorOutOfMemory)                                                        \
                fail(SRG_ERR_OOM, std::string("device allocation failed: ") + hipGetErrorString(e_)); \
            fail(SRG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
        }                                                                                         \
    } while (0)

void set_err(char* buf, size_t len, const std::string& m) {
    if (buf && len) std::snprintf(buf, len, "%s", m.c_str());
}

// grow-only device buffer; owns its allocation
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void* get(size_t need) {
        if (need <= bytes) return p;
        if (p) HIP_CHECK(hipFree(p));
        p = nullptr;
        bytes = 0;
        HIP_CHECK(hipMalloc(&p, need ? need : 16));
        bytes = need;
        return p;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// an owned hipEvent_t: null until created, destroyed with its owner
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }  // (vectors of events grow)
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    void create() {  // ordering only (no timestamps); a second call keeps the first event
        if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    void create_timed() {
        if (!e) HIP_CHECK(hipEventCreate(&e));
    }
    operator hipEvent_t() const { return e; }
};

struct EdgeStats {
    unsigned long long max_lat;   // max latency over non-self-loop edges
    unsigned long long unit;      // gcd of the non-self-loop latencies (0: none, or all zero)
    uint32_t bad_endpoint;        // an endpoint >= V
    uint32_t lat_overflow;        // a non-self-loop latency == UINT64_MAX (ns conversion overflow)
    unsigned long long min_lat_inv;  // ~(min latency over non-self-loop edges) (0: no such edge)
};

struct Flags {
    uint32_t changed;
    uint32_t inf_in_used_row;
    uint32_t unreachable_used_pair;
    uint32_t bad_node;
    unsigned long long first_bad;  // direct paths: first (i*n+j) with edge count != 1
    uint32_t wrap;                 // k_wrap_edges: a relaxation the reference would run wraps u64
    uint32_t wrap_inf;             // k_wrap_edges: a relaxation from a vertex left at INF (unknown distance)
    uint32_t impossible;           // k_certify: a used off-diagonal key below the smallest edge key (guards.h)
};

constexpr int kThreads = 256;

inline unsigned grid_for(size_t work, size_t cap = 256 * 16) {
    size_t g = (work + kThreads - 1) / kThreads;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// ---------------------------------------------------------------------------------------
__global__ void k_check_nodes(const uint32_t* __restrict__ nodes, uint32_t n, uint32_t V,
                              uint32_t* __restrict__ mark, Flags* flags) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t v = nodes[i];
        if (v >= V) {
            atomicOr(&flags->bad_node, 1u);
            continue;
        }
        if (atomicAdd(&mark[v], 1u) != 0) atomicOr(&flags->bad_node, 2u);
    }
}

// binary gcd (gcd(0, b) = b)
__device__ __forceinline__ unsigned long long gcd64(unsigned long long a, unsigned long long b) {
    if (a == 0) return b;
    if (b == 0) return a;
    const int sh = __builtin_ctzll(a | b);
    a >>= __builtin_ctzll(a);
    do {
        b >>= __builtin_ctzll(b);
        if (a > b) {
            const unsigned long long t = a;
            a = b;
            b = t;
        }
        b -= a;
    } while (b);
    return a << sh;
}

__global__ void k_edge_scan(uint64_t E, const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                            const uint64_t* __restrict__ lat, const float* __restrict__ loss, uint32_t V,
                            uint32_t* __restrict__ selfcnt, uint64_t* __restrict__ self_lat,
                            float* __restrict__ self_loss, EdgeStats* st) {
    unsigned long long mx = 0, mn = 0;  // mn = ~min: a max reduction like mx (0 = no edge yet)
    uint32_t bad = 0, ovf = 0;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < E; e += (size_t)gridDim.x * blockDim.x) {
        const uint32_t s = src[e], t = dst[e];
        if (s >= V || t >= V) {
            bad = 1;
            continue;
        }
        const uint64_t l = lat[e];
        if (s == t) {
            atomicAdd(&selfcnt[s], 1u);
            self_lat[s] = l;      // meaningful only when the count ends at exactly 1
            if (loss) self_loss[s] = loss[e];  // null: the loss arrives later (k_self_loss)
        } else {
            mx = l > mx ? l : mx;
            mn = ~l > mn ? ~l : mn;
            ovf |= (l == UINT64_MAX);
        }
    }
    // wave reduction then one atomic per wave
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long o = __shfl_down(mx, off, 64);
        mx = o > mx ? o : mx;
        o = __shfl_down(mn, off, 64);
        mn = o > mn ? o : mn;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&st->max_lat, mx);
    if ((threadIdx.x & 63) == 0 && mn) atomicMax(&st->min_lat_inv, mn);
    if (bad) atomicOr(&st->bad_endpoint, 1u);
    if (ovf) atomicOr(&st->lat_overflow, 1u);
}

// The latency unit (compute_device: keys = latency / unit) = gcd of the non-self-loop latencies,
// in a pass of its own: each wave folds 256-edge chunks and publishes its gcd, and every wave stops
// once the published unit is 1 -- on nanosecond-random latencies after the first round of chunks
// (~1 M edges), on unit-granular ones after the whole list.  (Folded into k_edge_scan, the gcd
// tripled that kernel: 298 -> 884 us on C3.)
__global__ void __launch_bounds__(256) k_lat_gcd(uint64_t E, const uint32_t* __restrict__ src,
                                                 const uint32_t* __restrict__ dst, const uint64_t* __restrict__ lat,
                                                 unsigned long long* unit) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
    const size_t nch = (E + 255) / 256;
    for (size_t ch = wave; ch < nch; ch += nwaves) {
        if (__hip_atomic_load(unit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1ull) return;  // whole wave
        unsigned long long un = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t e = ch * 256 + (size_t)j * 64 + lane;
            if (e < E && src[e] != dst[e]) un = gcd64(un, lat[e]);
        }
        for (int off = 32; off > 0; off >>= 1) un = gcd64(un, __shfl_down(un, off, 64));
        if (lane == 0 && un) {
            // gcd has no atomic: compare-and-swap until the stored unit divides this wave's
            unsigned long long cur = __hip_atomic_load(unit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (;;) {
                const unsigned long long nu = gcd64(cur, un);
                if (nu == cur) break;
                const unsigned long long prev = atomicCAS(unit, cur, nu);
                if (prev == cur) break;
                cur = prev;
            }
        }
    }
}

// the self-loops' loss, when the edge losses arrive after k_edge_scan (host entry, late loss)
__global__ void k_self_loss(uint64_t E, const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                            const float* __restrict__ loss, uint32_t V, float* __restrict__ self_loss) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < E; e += (size_t)gridDim.x * blockDim.x) {
        const uint32_t s = src[e];
        if (s == dst[e] && s < V) self_loss[s] = loss[e];
    }
}

template <class K>
__global__ void k_fill(K* __restrict__ p, size_t count, K v) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        p[i] = v;
}

// latency -> key: latency / unit, where the unit (the gcd of all non-self-loop latencies) divides
// every path sum, so keys compare and add exactly as the latencies do; outputs are key * unit
template <class K>
__device__ __forceinline__ K to_key(uint64_t l, uint64_t unit) {
    if (unit != 1) l /= unit;
    if constexpr (sizeof(K) == 4) return l >= KeyOps<K>::INF ? KeyOps<K>::INF : (uint32_t)l;
    else return (K)l;
}

template <class K>
__global__ void k_w_lat(uint64_t E, const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                        const uint64_t* __restrict__ lat, uint64_t unit, int directed, K* __restrict__ W, size_t ld) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < E; e += (size_t)gridDim.x * blockDim.x) {
        const uint32_t s = src[e], t = dst[e];
        if (s == t) continue;  // self-loops never shorten a path; kept for the diagonal only
        const K l = to_key<K>(lat[e], unit);
        atomicMin(&W[(size_t)s * ld + t], l);
        if (!directed) atomicMin(&W[(size_t)t * ld + s], l);
    }
}

template <class K>
__global__ void k_w_loss(uint64_t E, const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                         const uint64_t* __restrict__ lat, uint64_t unit, const float* __restrict__ loss, int directed,
                         const K* __restrict__ W, uint32_t* __restrict__ WL, size_t ld) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < E; e += (size_t)gridDim.x * blockDim.x) {
        const uint32_t s = src[e], t = dst[e];
        if (s == t) continue;
        const K l = to_key<K>(lat[e], unit);
        // -0.0 compares equal to 0.0 (partial_cmp) and folds identically: normalise it
        const uint32_t bits = __float_as_uint(loss[e] + 0.0f);
        if (W[(size_t)s * ld + t] == l) atomicMin(&WL[(size_t)s * ld + t], bits);
        if (!directed && W[(size_t)t * ld + s] == l) atomicMin(&WL[(size_t)t * ld + s], bits);
    }
}

// u32 keys: one pass over the edges with a packed lexicographic key
//   KW[s][t] = min over parallel edges of (latency << 32 | loss bits)    (mod.rs:305-313)
// (loss in [0,1] is non-negative, so its f32 bit order is its numeric order).
// (V: endpoints past it are skipped -- the FW beside the H2D builds W before the edge checks run)
__global__ void k_w_key(uint64_t E, const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                        const uint64_t* __restrict__ lat, uint64_t unit, const float* __restrict__ loss,
                        unsigned long long* __restrict__ KW, size_t ld, uint32_t V = 0xFFFFFFFFu) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < E; e += (size_t)gridDim.x * blockDim.x) {
        const uint32_t s = src[e], t = dst[e];
        if (s == t || s >= V || t >= V) continue;  // self-loops never shorten a path; kept for the diagonal only
        // null loss: latency only (WL is then built by k_w_loss once the losses have arrived)
        const uint64_t l = unit != 1 ? lat[e] / unit : lat[e];  // < 2^32-1: the u32 path's precondition
        const unsigned long long k = ((unsigned long long)l << 32) | (loss ? __float_as_uint(loss[e] + 0.0f) : 0u);
        atomicMin(&KW[(size_t)s * ld + t], k);
    }
}

// 64x64 tiles: (undirected) KW = min(KW, KW^T), then split into W (latency), WL (loss bits)
// and D (= W with a zero diagonal).  grid = (nb64, nb64) over the upper triangle incl. diagonal
// blocks when undirected (each block pair handled once), all blocks when directed.
// WL_ONLY: only WL is written (late loss: W and D were split from latency-only keys before FW)
// (bi0: first 64-block row of the launch -- the FW beside the H2D splits a block-row at a time)
template <bool WL_ONLY = false>
__global__ void __launch_bounds__(256) k_w_split(const unsigned long long* __restrict__ KW, size_t ld, int directed,
                                                 uint32_t* __restrict__ W, uint32_t* __restrict__ WL,
                                                 uint32_t* __restrict__ D, uint32_t bi0 = 0) {
    __shared__ unsigned long long tb[64][65];
    const uint32_t bi = bi0 + blockIdx.y, bj = blockIdx.x;
    if (!directed && bj < bi) return;
    const uint32_t tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    if (!directed) {
        for (uint32_t r = ty; r < 64; r += 4) tb[r][tx] = KW[(size_t)(bj * 64 + r) * ld + bi * 64 + tx];  // (bj, bi)
        __syncthreads();
    }
    for (uint32_t r = ty; r < 64; r += 4) {
        const size_t i = bi * 64 + r, j = bj * 64 + tx;
        unsigned long long k = KW[i * ld + j];
        if (!directed) k = min(k, tb[tx][r]);
        const uint32_t w = min((uint32_t)(k >> 32), KeyOps<uint32_t>::INF);  // no edge / >= INF -> INF
        WL[i * ld + j] = (uint32_t)k;
        if (!WL_ONLY) {
            W[i * ld + j] = w;
            D[i * ld + j] = i == j ? 0u : w;
        }
        if (!directed && bi != bj) tb[tx][r] = k;  // the mirrored element, written below
    }
    if (!directed && bi != bj) {
        __syncthreads();
        for (uint32_t r = ty; r < 64; r += 4) {
            const size_t i = bj * 64 + r, j = bi * 64 + tx;
            const unsigned long long k = tb[r][tx];
            const uint32_t w = min((uint32_t)(k >> 32), KeyOps<uint32_t>::INF);
            WL[i * ld + j] = (uint32_t)k;
            if (!WL_ONLY) {
                W[i * ld + j] = w;
                D[i * ld + j] = w;
            }
        }
    }
}

template <class K>
__global__ void k_init_d(const K* __restrict__ W, K* __restrict__ D, size_t ld) {
    const size_t total = ld * ld;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / ld, c = i - r * ld;
        D[i] = (r == c) ? (K)0 : W[i];
    }
}

// INF in a used (row, column) pair (u32 certification).  Only used columns can change an
// output: a stored key <= INF plus an edge w > 0 never falsely equals a finite D[s][t], so an
// unreachable UNUSED vertex leaves the u32 result exact.
// Row kernels over (used row x used column) arrays: one workgroup per row (grid = rows), the
// threads striding over the columns -- no 64-bit division per element (the grid-stride form with
// i / ncols ran 10x below HBM rate: 0.6 ms per C3 pass).
// Also the impossible-result guard (guards.h): a used off-diagonal key below the smallest edge key
// (0 included) cannot be a path length -- a fault inside the builder, never returned as OK.
template <class K>
__global__ void __launch_bounds__(256) k_certify(const K* __restrict__ D, size_t ld, const uint32_t* __restrict__ rows,
                                                 uint32_t nrows, const uint32_t* __restrict__ cols, uint32_t ncols,
                                                 K min_key, Flags* flags) {
    const uint32_t s = rows[blockIdx.x];
    const K* Dr = D + (size_t)s * ld;
    uint32_t hit = 0, bad = 0;
    constexpr uint32_t U = 8;  // independent loads in flight per thread (the gather is latency-bound)
    for (uint32_t j0 = threadIdx.x; j0 < ncols; j0 += blockDim.x * U) {
        uint32_t cc[U];
        K d[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t j = j0 + u * blockDim.x;
            cc[u] = cols[j < ncols ? j : 0];
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) d[u] = Dr[cc[u]];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const bool in = j0 + u * blockDim.x < ncols;
            hit |= in & (d[u] == KeyOps<K>::INF);
            bad |= in & impossible_key<K>(d[u], min_key, cc[u] == s);
        }
    }
    if (__ballot(hit) && (threadIdx.x & 63) == 0) atomicOr(&flags->inf_in_used_row, 1u);
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&flags->impossible, 1u);
}

template <class K>
__global__ void k_loss_round(const uint32_t* __restrict__ PRED, const K* __restrict__ D, const K* __restrict__ W,
                             const uint32_t* __restrict__ WL, const uint32_t* __restrict__ nodes, uint32_t n,
                             uint32_t V, size_t ld, const float* __restrict__ Lin, float* __restrict__ Lout,
                             Flags* flags) {
    const size_t total = (size_t)n * V;
    uint32_t changed = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / V, t = i - r * V;
        const uint32_t s = nodes[r];
        const uint32_t p = PRED[r * ld + t];
        const float* Lrow = Lin + r * ld;
        float v;
        if (t == s) {
            v = 0.0f;  // Dijkstra start score PathProperties::default() (mod.rs:297)
        } else if (p == PRED_NONE) {
            v = 1.0f;  // unreachable: never read by a reachable vertex
        } else if (p != PRED_MULTI) {
            const float pl = __uint_as_float(WL[(size_t)p * ld + t]);
            v = fold_loss(Lrow[p], __fsub_rn(1.0f, pl));
        } else {
            // several latency-tight predecessors: Dijkstra keeps the smallest loss
            const K dst_st = D[(size_t)s * ld + t];
            const K* Ds = D + (size_t)s * ld;
            v = 1.0f;
            for (uint32_t u = 0; u < V; ++u) {
                if (KeyOps<K>::add(Ds[u], W[(size_t)u * ld + t]) != dst_st) continue;
                const float pl = __uint_as_float(WL[(size_t)u * ld + t]);
                const float c = fold_loss(Lrow[u], __fsub_rn(1.0f, pl));
                v = c < v ? c : v;
            }
        }
        Lout[r * ld + t] = v;
        changed |= (v != Lrow[t]);
    }
    if (changed) atomicOr(&flags->changed, 1u);
}

// Wrap check (graphs whose max edge latency x V reaches 2^64 ns only).  The reference
// sums u64 latencies with wrapping arithmetic (mod.rs:327, release build): its Dijkstra from s
// relaxes every edge (u, t) of a visited u towards a not-yet-visited t, i.e. with D[s][t] >= D[s][u]
// (ties either way), and a sum D[s][u] + w >= 2^64 ns wraps and corrupts its result.  This kernel
// flags such a relaxation for the local source rows (grid = (edge blocks, rows)): D is in latency
// units (outputs are D * unit), w in ns.  A relaxation from a vertex whose key is INF can only be
// judged when INF means unreachable; `inf_known` = 0 flags it instead (the caller reruns on wider
// keys or reports the range).
template <class K>
__global__ void __launch_bounds__(256) k_wrap_edges(uint64_t E, const uint32_t* __restrict__ src,
                                                    const uint32_t* __restrict__ dst, const uint64_t* __restrict__ lat,
                                                    int directed, const K* __restrict__ D, size_t ld,
                                                    const uint32_t* __restrict__ rows, uint64_t unit, int inf_known,
                                                    Flags* flags) {
    const K* Ds = D + (size_t)rows[blockIdx.y] * ld;
    uint32_t wrap = 0, winf = 0;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < E; e += (size_t)gridDim.x * blockDim.x) {
        const uint32_t s = src[e], t = dst[e];
        if (s == t) continue;
        const uint64_t w = lat[e];
        for (int dir = 0; dir < (directed ? 1 : 2); ++dir) {
            const uint32_t u = dir ? t : s, v = dir ? s : t;
            const K du = Ds[u], dv = Ds[v];
            if (du == KeyOps<K>::INF) {
                winf |= !inf_known;  // unknown distance: the relaxation may or may not wrap
                continue;
            }
            if (dv < du) continue;  // v was visited before u: Dijkstra skips the edge
            const unsigned __int128 sum = (unsigned __int128)du * unit + w;
            wrap |= (uint32_t)(sum >> 64) != 0;
        }
    }
    if (__ballot(wrap) && (threadIdx.x & 63) == 0) atomicOr(&flags->wrap, 1u);
    if (__ballot(winf) && (threadIdx.x & 63) == 0) atomicOr(&flags->wrap_inf, 1u);
}

// (stride 2: the packed {u, 1 - loss} PRED rows of tight_v5<true>, marker in the first word)
__global__ void __launch_bounds__(256) k_count_multi(const uint32_t* __restrict__ PRED, uint32_t n, uint32_t V,
                                                     size_t ld, unsigned long long* out, uint32_t stride = 1) {
    const uint32_t* row = PRED + (size_t)blockIdx.x * ld * stride;
    unsigned long long c = 0;
    for (uint32_t t = threadIdx.x; t < V; t += blockDim.x) c += row[(size_t)t * stride] == PRED_MULTI;
    if (c) atomicAdd(out, c);
}

// Used x used outputs for the local source rows: row a (source snodes[a]) goes to output row
// rowpos[a]; columns are the full `cols` (= nodes) list.  L == nullptr: out_loss was already
// written by k_loss_rows.
template <class K>
__global__ void __launch_bounds__(256) k_extract(const K* __restrict__ D, const float* __restrict__ L, size_t ld,
                                                 const uint32_t* __restrict__ snodes, uint32_t nloc,
                                                 const uint32_t* __restrict__ cols, uint32_t ncols,
                                                 const uint32_t* __restrict__ rowpos,
                                                 const uint64_t* __restrict__ self_lat, const float* __restrict__ self_loss,
                                                 uint64_t* __restrict__ out_lat, float* __restrict__ out_loss, Flags* flags,
                                                 int mode, uint64_t unit, uint32_t* __restrict__ out_key = nullptr,
                                                 uint64_t* __restrict__ out_diag = nullptr) {
    // out_key (RoutingInfo's key table, srg_internal_compute_table): latencies as u32 keys instead of
    // ns (0xFFFFFFFF on the diagonal, whose raw self-loop latency goes to out_diag)
    // mode bit 0: latency (+ unreachable check), bit 1: loss from L; one workgroup per local row a,
    // U columns per thread in flight (the gathers are latency-bound)
    const uint32_t a = blockIdx.x;
    const uint32_t s = snodes[a], p = rowpos[a];
    const K* Ds = D + (size_t)s * ld;
    const float* La = L ? L + (size_t)a * ld : nullptr;
    uint64_t* ol = out_lat + (size_t)p * ncols;
    uint32_t* ok = out_key ? out_key + (size_t)p * ncols : nullptr;
    float* os = out_loss + (size_t)p * ncols;
    uint32_t unreach = 0;
    constexpr uint32_t U = 4;
    for (uint32_t b0 = threadIdx.x; b0 < ncols; b0 += blockDim.x * U) {
        uint32_t tt[U];
        K d[U];
        float l[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t b = b0 + u * blockDim.x;
            tt[u] = cols[b < ncols ? b : 0];
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            if (mode & 1) d[u] = Ds[tt[u]];
            if (mode & 2) l[u] = La[tt[u]];
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t b = b0 + u * blockDim.x;
            if (b >= ncols) break;
            if (p == b) {
                // raw self-loop weight, no 1-(1-p) rounding (mod.rs:211-217)
                if (mode & 1) {
                    if (ok) {
                        ok[b] = 0xFFFFFFFFu;
                        out_diag[p] = self_lat[s];
                    } else {
                        ol[b] = self_lat[s];
                    }
                }
                if (mode & 2) os[b] = self_loss[s];
            } else {
                if (mode & 1) {
                    unreach |= d[u] == KeyOps<K>::INF;
                    if (ok) ok[b] = (uint32_t)d[u];
                    else ol[b] = (uint64_t)d[u] * unit;
                }
                if (mode & 2) os[b] = l[u];
            }
        }
    }
    if (__ballot(unreach) && (threadIdx.x & 63) == 0) atomicOr(&flags->unreachable_used_pair, 1u);
}

// k_extract's latency pass when every vertex is used in vertex order (nodes[j] == j, the GML
// complete graphs): a row copy of D at 16 B per lane (the per-column index gathers of k_extract
// ran at ~1.25 TB/s), the diagonal patched in the register before the store.  ncols % 4 == 0.
template <class K>
__global__ void __launch_bounds__(256) k_extract_ident(const K* __restrict__ D, size_t ld, const uint32_t* __restrict__ snodes,
                                                       uint32_t ncols, const uint64_t* __restrict__ self_lat,
                                                       uint64_t* __restrict__ out_lat, Flags* flags, uint64_t unit,
                                                       uint32_t* __restrict__ out_key, uint64_t* __restrict__ out_diag) {
    const uint32_t s = snodes[blockIdx.x];  // (= its output row: identity)
    const K* Ds = D + (size_t)s * ld;
    uint32_t unreach = 0;
    for (uint32_t b = threadIdx.x * 4; b < ncols; b += blockDim.x * 4) {
        K d[4];
        if constexpr (sizeof(K) == 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(Ds + b);
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
            const ulonglong2 v0 = *reinterpret_cast<const ulonglong2*>(Ds + b);
            const ulonglong2 v1 = *reinterpret_cast<const ulonglong2*>(Ds + b + 2);
            d[0] = v0.x, d[1] = v0.y, d[2] = v1.x, d[3] = v1.y;
        }
        uint64_t o[4];
        uint32_t k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool diag = b + u == s;
            unreach |= !diag && d[u] == KeyOps<K>::INF;
            k[u] = diag ? 0xFFFFFFFFu : (uint32_t)d[u];
            o[u] = diag ? self_lat[s] : (uint64_t)d[u] * unit;  // raw self-loop weight (mod.rs:211-217)
        }
        if (out_key) {
            *reinterpret_cast<uint4*>(out_key + (size_t)s * ncols + b) = make_uint4(k[0], k[1], k[2], k[3]);
            if (b <= s && s < b + 4) out_diag[s] = self_lat[s];
        } else {
            uint64_t* ol = out_lat + (size_t)s * ncols + b;
            *reinterpret_cast<ulonglong2*>(ol) = make_ulonglong2(o[0], o[1]);
            *reinterpret_cast<ulonglong2*>(ol + 2) = make_ulonglong2(o[2], o[3]);
        }
    }
    if (__ballot(unreach) && (threadIdx.x & 63) == 0) atomicOr(&flags->unreachable_used_pair, 1u);
}

// min over a u64 array (RoutingInfo::get_smallest_latency_ns, mod.rs:474-476: all n^2 entries,
// diagonal included)
__global__ void k_min_u64(const uint64_t* __restrict__ a, size_t count, unsigned long long* out) {
    unsigned long long m = ~0ull;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        m = a[i] < m ? a[i] : m;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(m, off, 64);
        m = o < m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m != ~0ull) atomicMin(out, m);
}

// min over a key table (the diagonal's 0xFFFFFFFF excluded by being the maximum)
__global__ void k_min_u32(const uint32_t* __restrict__ a, size_t count, unsigned long long* out) {
    uint32_t m = 0xFFFFFFFFu;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        m = a[i] < m ? a[i] : m;
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_down(m, off, 64);
        m = o < m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m != 0xFFFFFFFFu) atomicMin(out, (unsigned long long)m);
}

__global__ void k_positions(const uint32_t* __restrict__ nodes, uint32_t n, int32_t* __restrict__ pos) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        pos[nodes[i]] = (int32_t)i;
}

__global__ void k_direct(uint64_t E, const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                         const uint64_t* __restrict__ lat, const float* __restrict__ loss, int directed,
                         const int32_t* __restrict__ pos, uint32_t n, uint32_t* __restrict__ cnt,
                         uint64_t* __restrict__ out_lat, float* __restrict__ out_loss) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < E; e += (size_t)gridDim.x * blockDim.x) {
        const int32_t ps = pos[src[e]], pt = pos[dst[e]];
        if (ps < 0 || pt < 0) continue;
        size_t k = (size_t)ps * n + pt;
        if (atomicAdd(&cnt[k], 1u) == 0) {
            out_lat[k] = lat[e];
            out_loss[k] = loss[e];
        }
        if (!directed && ps != pt) {
            k = (size_t)pt * n + ps;
            if (atomicAdd(&cnt[k], 1u) == 0) {
                out_lat[k] = lat[e];
                out_loss[k] = loss[e];
            }
        }
    }
}

__global__ void k_direct_check(const uint32_t* __restrict__ cnt, uint32_t n, Flags* flags) {
    const size_t total = (size_t)n * n;
    unsigned long long first = ~0ull;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        if (cnt[i] != 1 && i < first) first = i;
    if (first != ~0ull) atomicMin(&flags->first_bad, first);
}

// ---------------------------------------------------------------------------------------
double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

// The HSA agents of a HIP device (matched by PCI domain / bus / device), for SDMA copies.
struct SdmaAgents {
    bool ok = false;
    hsa_agent_t gpu{}, cpu{};
    uint32_t engine = 0;  // hsa_amd_sdma_engine_id_t bit of the engine used for D2H
    void init(int device) {
        if (hsa_init() != HSA_STATUS_SUCCESS) return;
        int bus = -1, dev = -1, dom = -1;
        if (hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, device) != hipSuccess ||
            hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, device) != hipSuccess ||
            hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, device) != hipSuccess)
            return;
        struct Q {
            int bus, dev, dom;
            hsa_agent_t gpu{}, cpu{};
            bool found = false, have_cpu = false;
        } q{bus, dev, dom};
        hsa_iterate_agents(
            [](hsa_agent_t a, void* p) -> hsa_status_t {
                Q& q = *static_cast<Q*>(p);
                hsa_device_type_t t;
                if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
                if (t == HSA_DEVICE_TYPE_CPU && !q.have_cpu) {
                    q.cpu = a;
                    q.have_cpu = true;
                } else if (t == HSA_DEVICE_TYPE_GPU && !q.found) {
                    uint32_t bdf = 0, dom = 0;
                    if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) == HSA_STATUS_SUCCESS &&
                        hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom) == HSA_STATUS_SUCCESS &&
                        (int)(bdf >> 8) == q.bus && (int)((bdf >> 3) & 31) == q.dev && (int)dom == q.dom) {
                        q.gpu = a;
                        q.found = true;
                    }
                }
                return HSA_STATUS_SUCCESS;
            },
            &q);
        if (!q.found || !q.have_cpu) return;
        uint32_t mask = 0;
        if (hsa_amd_memory_copy_engine_status(q.cpu, q.gpu, &mask) != HSA_STATUS_SUCCESS || !mask) return;
        gpu = q.gpu;
        cpu = q.cpu;
        engine = mask & (~mask + 1);  // lowest available engine
        ok = true;
    }
};

// Pinned-table pool (srg_internal_table_get / _put): the host tables a RoutingInfo owns
// (routing_info.cpp) come from their context's pool and go back to it when the RoutingInfo is
// freed, still page-locked.  The first build into a table pays the prefault + hipHostRegister
// (on the host entry's helper thread, beside the H2D and FW, as for any caller's table); a later
// build into a recycled table pays neither (the 1.2 GB C3 pair: ~12 ms cold, measured r04).
// A table can outlive its context: it holds the pool by reference count, and a closed pool frees
// what comes back.
struct TablePool;
struct srg_table {
    std::shared_ptr<TablePool> pool;
    void* p = nullptr;         // 2 MB aligned (transparent huge pages)
    size_t cap = 0;            // its bytes (a multiple of 2 MB)
    void* view = nullptr;      // its device view once registered
    bool registered = false;
};
struct TablePool {
    std::mutex mu;
    std::vector<srg_table*> idle;
    size_t idle_bytes = 0;
    // idle bytes kept (SRG_OPT_TABLE_POOL_BYTES); by default no byte cap but only the most recently
    // freed pair (a RoutingInfo's latency + loss tables): page-locked memory the OS cannot reclaim
    // stays bounded by one table set per context
    size_t limit = ~(size_t)0;
    size_t max_idle = 2;  // idle tables kept (0 = no count cap once a byte cap is set)
    bool open = true;
    static void destroy(srg_table* t);
    void trim_locked(size_t keep) {  // the oldest idle tables first
        while ((idle_bytes > keep || (max_idle && idle.size() > max_idle)) && !idle.empty()) {
            srg_table* t = idle.front();
            idle.erase(idle.begin());
            idle_bytes -= t->cap;
            destroy(t);
        }
    }
    void close() {
        std::lock_guard<std::mutex> lk(mu);
        open = false;
        trim_locked(0);
    }
};
void TablePool::destroy(srg_table* t) {
    if (t->registered) (void)hipHostUnregister(t->p);
    if (t->p) munmap(t->p, t->cap);
    delete t;
}

struct srg_ctx {
    int device = 0;
    double sparse_threshold = 0.35;  // essential-edge density above which the dense scan is used
    bool profiling = false;
    bool gather_output = true;       // multi-rank: every rank ends with all n x n outputs
    int algorithm = SRG_ALGO_AUTO;   // dense FW / sparse batched Bellman-Ford
    bool sparse_locality = true;     // sparse: batch sources in BFS order
    int sparse_delta_div = 1;        // sparse: bucket width = max edge latency / this (0 = plain BF)
    bool sparse_global_bitmaps = false;  // sparse: force the vertex bitmaps into global memory
    int fw_tile = 0;                 // 0 = auto, 64 or 128
    bool fw_symmetric = true;        // undirected + one rank: FW over the tiles I <= J only (SRG_OPT_FW_SYMMETRIC)
    int d2h_mode = 1;                // host entry D2H: 1 = SDMA engine, 0 = hipMemcpyAsync (SRG_OPT_D2H_MODE)
    DevBuf b_DST2;                   // low words of the u64-key DST (the scan input)
    SdmaAgents sdma;
    int h2d_codec = 1;               // host entry: narrowed edge list over PCIe (SRG_OPT_H2D_CODEC)
    HostPool* pool = nullptr;        // its host workers
    void* h_ring = nullptr;          // its page-locked staging ring (hipHostMalloc)
    size_t h_ring_bytes = 0;
    Event ev_ring[3];
    DevBuf b_n16s, b_n16d, b_n32l;   // narrowed edge arrays on the device
    DevBuf b_exc;                    // sequential-pair codec: a chunk's exceptions (index, src, dst)
    std::vector<std::vector<uint32_t>> codec_ex;  // its per-worker exception lists
    std::vector<uint32_t> slice_exc;    // the slice's exceptions (global index, src, dst), all chunks
    DevBuf b_xexc;                      // edge-sharded exchange: every rank's exceptions, counts
    int late_loss = 1;               // host entry: edge losses shipped beside FW (SRG_OPT_LATE_LOSS)
    hipStream_t loss_stream = nullptr;  // = d2h_stream (see srg_create)
    Event ev_ledges, ev_lin, ev_ldone, ev_wlate;
    void* h_lring = nullptr;         // pinned ring of the late loss H2D
    Event ev_lring[3];
    int edge_shard = -1;             // host entry, multi-rank: ship 1/N of the edges, allgatherv the rest (SRG_OPT_EDGE_SHARD)
    const uint32_t* sim_edges = nullptr;  // simulated rank: the edge list whose other slices are resident
    size_t sim_E = 0;
    int scan_groups = 0;             // host entry: v5 scan launches interleaved with the loss rows (0 = auto: 3, mirrored scan 4) (SRG_OPT_SCAN_GROUPS)
    int loss_chunks = 0;             // k_loss_rows launches (0 = auto: 8 when the host entry ships rows early, else 1) (SRG_OPT_LOSS_CHUNKS)
    srg::Comm* comm = nullptr;       // null = single GPU
    // srg_multi: the caller's output arrays are page-locked once for every rank (portable); the
    // host entry then waits for that registration (returns the arrays' device views, false if it
    // failed) instead of registering them itself
    std::function<bool(void** views, double* ms)> ext_reg;
    std::vector<Event> prof_events;  // timed pairs around the profiled launches (SRG_OPT_PROFILING)
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;   // FW lookahead: phase 1/2 of the next pivot block
    hipStream_t comm_stream = nullptr;  // pivot-panel broadcasts (multi-rank)
    hipStream_t d2h_stream = nullptr;   // host entry: output rows to the caller while kernels run
    Event ev_a, ev_b, ev_c, ev_d, ev_e;
    std::mutex mu;
    DevBuf b_src, b_dst, b_lat, b_loss, b_nodes, b_olat, b_oloss;  // host-entry staging
    DevBuf b_W, b_WL, b_D, b_PRED, b_PRED2, b_L0, b_L1, b_mark, b_selfcnt, b_selflat, b_selfloss;
    DevBuf b_stats, b_flags, b_multi, b_pos, b_cnt;
    // sparse tight scan
    DevBuf b_ecnt, b_eoff, b_indeg, b_cscoff, b_cscfill, b_entkey, b_entw, b_entb, b_grpe, b_cscent, b_DST,
        b_scantmp, b_ess, b_rlen;
    // multi-rank: local sources, their output rows, exchange staging
    DevBuf b_lnodes, b_lpos, b_red, b_outoff, b_outdst;
    DevBuf b_cflags, b_tiles, b_tslot;  // symmetric FW: closure barrier words, own tiles, packed slots
    uint32_t* fw_timeout = nullptr;     // symmetric FW: raised by a closure grid barrier that timed out
    unsigned char* hbox = nullptr;      // page-locked mailbox for small device -> host readbacks (rb_async)
    uint32_t* sig[2] = {nullptr, nullptr};  // stream_hop signals (HSA signal memory), their last values
    uint32_t sig_val[2] = {0, 0};
    bool hop_values = false;            // this build's hops use the signals (stream_hop)
    unsigned long long hop_bound_ticks = 200000000ull;  // a value hop's wait bound (100 MHz ticks; SymFw::begin)
    Event ev_fwreset;                   // SymFw::begin: the chain stream after the reset of the FW sync words
    Event ev_dst;                       // the scan's DST columns built (on the aux stream, beside the entry fill)
    int fw_line_split = 0;              // symmetric FW: line sub-tiles per dimension (0 = auto) (SRG_OPT_FW_LINE_SPLIT)
    int fw_step = -1;                   // symmetric FW's line exchange between ranks (SRG_OPT_FW_STEP, chain_xmode)
    DevBuf b_xlb, b_xflags;             // line buffers (kept lines / the exchange's three), peers' arrival flags
    uint32_t xepoch = 0;                // device-side exchange: this build's flag value (agreed in share_ptrs)
    std::vector<Event> ev_ov;           // FW beside the H2D: one "chunk landed" event per chunk
    uint32_t* kout_key = nullptr;       // this call's RoutingInfo key table on the device (key mode), and
    uint64_t* kout_diag = nullptr;      // its diagonal (raw self-loop latencies per position)
    DevBuf b_odiag;
    int fw_overlap = 1;                 // host entry: FW starts while the edge list arrives (SRG_OPT_FW_OVERLAP)
    int fw_xcd_order = 1;               // symmetric FW bulk: tiles dealt to the XCDs in Z-order runs (SRG_OPT_FW_XCD_ORDER)
    int scan_mirror = 1;                // undirected one-rank builds: scan the pairs (tile >= source block), mirror the rest (SRG_OPT_SCAN_MIRROR)
    int scan_mirrored = 0;              // the last build: 0 = every pair scanned, 1 = mirrored, 2 = mirrored, then rescanned (SRG_OPT_SCAN_MIRRORED)
    int loss_kind = 0;                  // the last dense build's loss pass, SRG_LOSS_* (SRG_OPT_LOSS_KIND)
    int scan_mirror_cap = 0;            // the mirror worklist's capacity in pairs per launch (0 = 1 / 1024 of the rows' pairs) (SRG_OPT_SCAN_MIRROR_CAP)
    DevBuf b_tri;                       // the triangular scan launches' block lists
    int test_fault = 0;                 // TEST HOOK (SRG_OPT_TEST_FAULT): 1 = zero D after FW, 2 = stale FW sync words
    std::shared_ptr<TablePool> tpool = std::make_shared<TablePool>();  // RoutingInfo's pinned tables
    double ms_create_runtime = 0, ms_create_lib = 0;  // srg_create: HIP runtime / device init vs the library's own
    // packet-event batches (events.hip.h): key / index ping-pong buffers, tile histograms
    DevBuf b_ek0, b_ek1, b_eh0, b_eh1, b_ei0, b_ei1, b_ehist, b_eoffs, b_ered;
    // routes (routes.hip.h): in-edge lists (route trees build theirs here too), walk state, hop counts / offsets,
    // query order, nonzero pairs
    DevBuf b_rt_off, b_rt_cur, b_rt_ce, b_rt_cu, b_rt_cl, b_rt_cp, b_rt_self, b_rt_state, b_rt_hops, b_rt_offs, b_rt_idx, b_rt_perm,
        b_rt_keys, b_rt_tmp, b_rt_pairs, b_rt_nsel;
    // route trees (route_trees.hip.h): a batch's predecessors, hops, doubling / subtree scratch, deepest level per
    // row, the rows with a nonzero count
    DevBuf b_rtt_pe, b_rtt_pv, b_rtt_hops, b_rtt_scr, b_rtt_rowmax, b_rtt_rownnz, b_rtt_active, b_rtt_nsel;
    int route_tree_rows = 0;            // source rows per batch of the route-tree calls, 0 = by budget (SRG_OPT_ROUTE_TREE_ROWS)
    // Teardown.  The body releases what depends on order; the DevBuf and Event members free
    // themselves afterwards (members are destroyed after the body), so device buffers go last.
    // Every path that deletes a context has set its device on the calling thread first:
    // srg_destroy (also srg_multi's teardown, rank by rank) and srg_create's failure path.
    //   1. comm, before the streams its collectives were queued on
    //   2. the hop signals, the late-loss ring, the mailbox
    //   3. the streams (loss_stream is d2h_stream: destroyed once)
    //   4. the host pool (joins its workers), then the codec's pinned ring they wrote
    //   5. the pinned-table pool is closed; tables still held by a RoutingInfo free themselves
    ~srg_ctx() {
        delete comm;
        for (uint32_t* p : sig)
            if (p) (void)hipFree(p);
        if (h_lring) (void)hipHostFree(h_lring);
        if (hbox) (void)hipHostFree(hbox);
        for (hipStream_t s : {aux_stream, comm_stream, d2h_stream, stream})
            if (s) (void)hipStreamDestroy(s);
        delete pool;
        if (h_ring) (void)hipHostFree(h_ring);
        tpool->close();
    }
};

namespace {

// Host entry with SRG_OPT_LATE_LOSS: the edge losses cross PCIe on their own stream after the
// endpoints and latencies, while the W build and FW (which need no loss) run.  Every reader of
// `DevGraph::loss` first calls loss_arrive() on its stream.
struct LateLoss {
    hipStream_t ls = nullptr;   // c.loss_stream
    std::thread th;             // queues the chunked H2D of the losses (pinned ring) on c.loss_stream
    hipEvent_t ev_in = nullptr;  // recorded by `th` after the last loss chunk
    hipEvent_t ev_done = nullptr;  // the losses and the self-loop losses are on the device
    bool joined = false, applied = false;
    std::string err;
    // edge-sharded host entry: each rank shipped only its slice's losses; they are exchanged when
    // first read (loss_arrive, at the same point on every rank): allgatherv with these segments
    srg::Comm* comm = nullptr;
    std::vector<size_t> offs, lens;
    void join() {
        if (!joined) {
            if (th.joinable()) th.join();
            joined = true;
        }
        if (!err.empty()) fail(SRG_ERR_HIP, "loss H2D: " + err);
    }
    ~LateLoss() {  // no DMA into the ring or the device losses may outlive the call
        if (th.joinable()) th.join();
        if (ls) (void)hipStreamSynchronize(ls);
    }
};

struct DevGraph {
    uint32_t V;
    int directed;
    uint64_t E;
    const uint32_t* src;
    const uint32_t* dst;
    const uint64_t* lat;
    const float* loss;
    const uint32_t* ids_dev;    // may be null
    const uint32_t* ids_host;   // may be null (host entry)
    LateLoss* late = nullptr;   // non-null: `loss` is still in flight (loss_arrive before reading it)
};

// Make `s` wait until g.loss (and the self-loop losses) are on the device.
void loss_arrive(const DevGraph& g, float* self_loss, hipStream_t s) {
    LateLoss* L = g.late;
    if (!L) return;
    L->join();  // every loss chunk is queued and ev_in recorded
    if (!L->applied) {
        HIP_CHECK(hipStreamWaitEvent(s, L->ev_in, 0));
        if (L->comm) L->comm->allgatherv(const_cast<float*>(g.loss), L->offs.data(), L->lens.data(), s);
        if (g.E) k_self_loss<<<grid_for(g.E), kThreads, 0, s>>>(g.E, g.src, g.dst, g.loss, g.V, self_loss);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(L->ev_done, s));
        L->applied = true;
    } else {
        HIP_CHECK(hipStreamWaitEvent(s, L->ev_done, 0));
    }
}

uint32_t node_gml_id(const DevGraph& g, uint32_t v, hipStream_t st) {
    if (g.ids_host) return g.ids_host[v];
    if (!g.ids_dev) return v;
    uint32_t id = v;
    HIP_CHECK(hipMemcpyAsync(&id, g.ids_dev + v, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return id;
}

// at least n timed events in c.prof_events (SRG_OPT_PROFILING)
void ensure_prof_events(srg_ctx& c, size_t n) {
    while (c.prof_events.size() < n) {
        c.prof_events.emplace_back();
        c.prof_events.back().create_timed();
    }
}

template <class F>
void set_lds(F func, size_t bytes) {
    static_assert(sizeof(F) > 0, "");
    if (bytes > 65536)
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(func),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

// Small device -> host readbacks (flags, counters) through the context's page-locked mailbox:
// one asynchronous DMA each, read after the stream's next synchronisation.  Into pageable host
// memory the runtime stages such a copy synchronously (~20 us per call on top of the sync;
// C1 paid a dozen of them per build).  64-byte slots, kMailSlots of them.
constexpr int kMailSlots = 64;
template <class T>
void rb_async(srg_ctx& c, int slot, const T* dev, hipStream_t st) {
    static_assert(sizeof(T) <= 64, "mailbox slot");
    HIP_CHECK(hipMemcpyAsync(c.hbox + 64 * slot, dev, sizeof(T), hipMemcpyDeviceToHost, st));
}
template <class T>
T rb_get(const srg_ctx& c, int slot) {
    T v;
    std::memcpy(&v, c.hbox + 64 * slot, sizeof(T));
    return v;
}
enum MailSlot { MS_EDGESTATS, MS_FLAGS, MS_TIMEOUT, MS_REDUCE, MS_TAIL0, MS_TAIL1, MS_NMULTI, MS_CHANGED, MS_MIN, MS_REDUCE2, MS_MIRROR };

// Common validation: nodes in range & unique, edge endpoints, self-loop counts, latency range.
struct Prelude {
    EdgeStats es;
    uint32_t* selfcnt;
    uint64_t* selflat;
    float* selfloss;
    Flags* flags;
    std::vector<uint32_t> nodes_h;  // host copy of `nodes` (partitioning, error text)
    bool ident = false;             // nodes == 0, 1, ..., V - 1 (k_extract_ident)
    bool range_risk = false;         // max_key * (V-1) >= 2^62: an INF used pair on the u64 keys may be a
                                     // path >= 2^62 units (SRG_ERR_LATENCY_RANGE), not an unreachable one
    bool wrap_risk = false;          // max_lat * V >= 2^64 ns: a relaxation of the reference may wrap u64
                                     // (checked after FW by k_wrap_edges; the sparse path is not taken)
    uint64_t unit = 1;               // latency unit in ns: keys = latency / unit (compute_device)
    unsigned long long max_key = 0;  // max_lat / unit
};

Prelude prelude(srg_ctx& c, const DevGraph& g, const uint32_t* nodes, uint32_t n, hipStream_t st,
                bool check_selfloops) {
    Prelude P{};
    const uint32_t V = g.V;
    uint32_t* mark = (uint32_t*)c.b_mark.get((size_t)V * 4);
    P.selfcnt = (uint32_t*)c.b_selfcnt.get((size_t)V * 4);
    P.selflat = (uint64_t*)c.b_selflat.get((size_t)V * 8);
    P.selfloss = (float*)c.b_selfloss.get((size_t)V * 4);
    EdgeStats* es = (EdgeStats*)c.b_stats.get(sizeof(EdgeStats));
    P.flags = (Flags*)c.b_flags.get(sizeof(Flags));
    HIP_CHECK(hipMemsetAsync(mark, 0, (size_t)V * 4, st));
    HIP_CHECK(hipMemsetAsync(P.selfcnt, 0, (size_t)V * 4, st));
    HIP_CHECK(hipMemsetAsync(es, 0, sizeof(EdgeStats), st));
    HIP_CHECK(hipMemsetAsync(P.flags, 0, sizeof(Flags), st));
    if (n) k_check_nodes<<<grid_for(n), kThreads, 0, st>>>(nodes, n, V, mark, P.flags);
    if (g.E) {
        k_edge_scan<<<grid_for(g.E), kThreads, 0, st>>>(g.E, g.src, g.dst, g.lat, g.late ? nullptr : g.loss, V, P.selfcnt,
                                                       P.selflat, P.selfloss, es);
        k_lat_gcd<<<grid_for(g.E / 4, 1024), kThreads, 0, st>>>(g.E, g.src, g.dst, g.lat, &es->unit);
    }
    HIP_CHECK(hipGetLastError());
    Flags fl;
    P.nodes_h.resize(n);
    rb_async(c, MS_EDGESTATS, es, st);
    rb_async(c, MS_FLAGS, P.flags, st);
    if (n) HIP_CHECK(hipMemcpyAsync(P.nodes_h.data(), nodes, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    P.es = rb_get<EdgeStats>(c, MS_EDGESTATS);
    fl = rb_get<Flags>(c, MS_FLAGS);
    P.ident = n == V;
    for (uint32_t i = 0; i < n && P.ident; ++i) P.ident = P.nodes_h[i] == i;
    if (P.es.bad_endpoint) fail(SRG_ERR_ARG, "edge endpoint out of range (>= num_vertices)");
    if (fl.bad_node & 1) fail(SRG_ERR_ARG, "node index out of range (>= num_vertices)");
    if (fl.bad_node & 2) fail(SRG_ERR_ARG, "duplicate node index in `nodes`");
    if (check_selfloops) {
        if (P.es.lat_overflow)
            fail(SRG_ERR_LATENCY_RANGE, "The resulting value is outside of the bounds [0, 18446744073709551615]");
        // there must be a single self-loop for each node (mod.rs:215-216), in `nodes` order
        std::vector<uint32_t> cnt(V);
        HIP_CHECK(hipMemcpyAsync(cnt.data(), P.selfcnt, (size_t)V * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t v = P.nodes_h[i];
            if (cnt[v] == 1) continue;
            const uint32_t id = node_gml_id(g, v, st);
            if (cnt[v] == 0)
                fail(SRG_ERR_NO_EDGE, "No edge connecting node " + std::to_string(id) + " to " + std::to_string(id));
            fail(SRG_ERR_MULTI_EDGE,
                 "More than one edge connecting node " + std::to_string(id) + " to " + std::to_string(id));
        }
    }
    return P;
}

struct Timer {
    hipStream_t st;
    std::chrono::steady_clock::time_point t0;
    explicit Timer(hipStream_t s) : st(s) { t0 = std::chrono::steady_clock::now(); }
    double lap() {
        HIP_CHECK(hipStreamSynchronize(st));
        double m = ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        return m;
    }
};

// Host entry output sink: the caller's n x n host arrays.  Finished output rows are copied
// while later kernels run (latency rows right after FW, loss rows per chunk of k_loss_rows),
// so the 1.2 GB C3 table mostly leaves during the scan and loss pass.  The caller's (pageable)
// buffers are page-locked by a helper thread that runs concurrently with the H2D copy and FW;
// until `ready()` confirms it, nothing is sent early and the host entry copies everything at
// the end instead.
// Copy engines (SRG_OPT_D2H_MODE): 1 (default) = an SDMA engine (hsa_amd_memory_async_copy_on_engine),
// issued by a helper thread once the producing kernels' event has completed -- measured to leave
// the overlapped kernels at full speed, where hipMemcpyAsync into registered memory (0) runs as a
// full-chip blit kernel that held k_ess_mask 0.26 -> 12.7 ms and each k_loss_rows chunk
// 0.48 -> 2.2 ms (profiles/r02c/).
struct HostSink {
    uint64_t* lat = nullptr;
    float* loss = nullptr;
    void* lat_view = nullptr;   // device views of the mapped host arrays (SDMA destinations)
    void* loss_view = nullptr;
    int mode = 1;
    const SdmaAgents* sdma = nullptr;
    int device = 0;
    size_t n = 0;
    hipStream_t cs = nullptr;
    hipEvent_t ev = nullptr;
    std::function<bool()> ready;
    bool checked = false, registered = false;
    bool lat_sent = false, loss_sent = false;
    uint64_t early_bytes = 0;
    // SDMA worker
    struct Job {
        hipEvent_t ev;
        void* dst;
        const void* src;
        size_t bytes;
    };
    std::thread worker;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Job> jobs;
    bool closing = false;
    std::string err;
    std::vector<hsa_signal_t> sigs;
    std::vector<hipEvent_t> evs;
    // latency rows as the build's u32 keys (widen = true: host entry, dense u32 build, one rank):
    // half the bytes of u64 ns over PCIe; a helper thread ships them through the context's pinned
    // ring (3 slots) on the SDMA engine and the host pool widens each slot (key x unit) into the u64
    // table while the next slots cross
    bool widen = false;
    HostPool* pool = nullptr;
    unsigned char* ring = nullptr;
    size_t ring_slot = 0;
    std::thread kthread;
    std::string kerr;
    double ms_widen = 0;
    uint64_t key_unit = 1;  // the keys' latency unit (set by the build that wrote them)
    void send_keys(hipStream_t st, const uint32_t* dkey, size_t row0, size_t rows, uint64_t unit) {
        if (!rows || !n) return;
        hipEvent_t e;
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        evs.push_back(e);
        HIP_CHECK(hipEventRecord(e, st));
        kthread = std::thread([this, e, dkey, row0, rows, unit]() { key_worker(e, dkey, row0, rows, unit); });
        early_bytes += rows * n * 4;
    }
    void key_worker(hipEvent_t ev, const uint32_t* dkey, size_t row0, size_t rows, uint64_t unit) {
        (void)hipSetDevice(device);
        if (hipEventSynchronize(ev) != hipSuccess) {
            kerr = "hipEventSynchronize failed before the key D2H";
            return;
        }
        const auto t0 = std::chrono::steady_clock::now();
        constexpr int NS = 3;
        const size_t rpc = std::max<size_t>(1, ring_slot / (n * 4));  // rows per chunk
        const size_t nch = (rows + rpc - 1) / rpc;
        hsa_signal_t sg[NS];
        int made = 0;
        for (; made < NS; ++made)
            if (hsa_signal_create(0, 0, nullptr, &sg[made]) != HSA_STATUS_SUCCESS) break;
        if (made < NS) {
            for (int i = 0; i < made; ++i) hsa_signal_destroy(sg[i]);
            kerr = "hsa_signal_create failed";
            return;
        }
        auto issue = [&](size_t ci) {
            const size_t r = ci * rpc, cnt = std::min(rpc, rows - r);
            hsa_signal_store_relaxed(sg[ci % NS], 1);
            if (hsa_amd_memory_async_copy_on_engine(ring + (ci % NS) * ring_slot, sdma->cpu, dkey + (row0 + r) * n, sdma->gpu,
                                                    cnt * n * 4, 0, nullptr, sg[ci % NS],
                                                    (hsa_amd_sdma_engine_id_t)sdma->engine, true) != HSA_STATUS_SUCCESS) {
                kerr = "hsa_amd_memory_async_copy_on_engine failed (keys)";
                hsa_signal_store_relaxed(sg[ci % NS], 0);
                return false;
            }
            return true;
        };
        bool ok = true;
        for (size_t ci = 0; ci < std::min<size_t>(NS, nch) && ok; ++ci) ok = issue(ci);
        for (size_t ci = 0; ci < nch && ok; ++ci) {
            hsa_signal_wait_scacquire(sg[ci % NS], HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
            const size_t r = ci * rpc, cnt = std::min(rpc, rows - r);
            const uint32_t* kb = reinterpret_cast<const uint32_t*>(ring + (ci % NS) * ring_slot);
            uint64_t* ob = lat + (row0 + r) * n;
            const size_t tot = cnt * n;
            pool->run([&](int w, int nw) {  // (the diagonal's 0xFFFFFFFF is patched by the caller)
                const size_t a = tot * w / nw, z = tot * (w + 1) / nw;
                if (unit == 1)
                    for (size_t i = a; i < z; ++i) ob[i] = kb[i];
                else
                    for (size_t i = a; i < z; ++i) ob[i] = (uint64_t)kb[i] * unit;
            });
            if (ci + NS < nch) ok = issue(ci + NS);
        }
        // drain: no copy may still target the ring when the call returns
        for (int i = 0; i < NS; ++i) {
            hsa_signal_wait_scacquire(sg[i], HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
            hsa_signal_destroy(sg[i]);
        }
        ms_widen = ms_since(t0);
    }
    bool ok() {
        if (!checked) {
            registered = ready && ready();
            checked = true;
        }
        return registered;
    }
    void work() {
        (void)hipSetDevice(device);
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return closing || !jobs.empty(); });
                if (jobs.empty()) return;
                j = jobs.front();
                jobs.pop_front();
            }
            if (!err.empty()) continue;
            if (hipEventSynchronize(j.ev) != hipSuccess) {
                err = "hipEventSynchronize failed before a D2H copy";
                continue;
            }
            hsa_signal_t sg;
            if (hsa_signal_create(1, 0, nullptr, &sg) != HSA_STATUS_SUCCESS) {
                err = "hsa_signal_create failed";
                continue;
            }
            sigs.push_back(sg);
            if (hsa_amd_memory_async_copy_on_engine(j.dst, sdma->cpu, j.src, sdma->gpu, j.bytes, 0, nullptr, sg,
                                                    (hsa_amd_sdma_engine_id_t)sdma->engine, true) != HSA_STATUS_SUCCESS)
                err = "hsa_amd_memory_async_copy_on_engine failed";
        }
    }
    // rows [row0, row0 + rows) of a row-major n-column device array, after the work queued on st
    void send_rows(hipStream_t st, const void* dev, void* host, size_t row0, size_t rows, size_t elem) {
        const size_t off = row0 * n * elem, bytes = rows * n * elem;
        if (!bytes) return;
        const unsigned char* src = (const unsigned char*)dev + off;
        void* view = host == (void*)lat ? lat_view : host == (void*)loss ? loss_view : nullptr;
        if (mode == 1 && sdma && sdma->ok) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            evs.push_back(e);
            HIP_CHECK(hipEventRecord(e, st));
            {
                std::lock_guard<std::mutex> lk(mu);
                jobs.push_back(Job{e, (unsigned char*)(view ? view : host) + off, src, bytes});
            }
            if (!worker.joinable()) worker = std::thread([this] { work(); });
            cv.notify_one();
            early_bytes += bytes;
            return;
        }
        HIP_CHECK(hipEventRecord(ev, st));
        HIP_CHECK(hipStreamWaitEvent(cs, ev, 0));
        HIP_CHECK(hipMemcpyAsync((unsigned char*)host + off, src, bytes, hipMemcpyDeviceToHost, cs));
        early_bytes += bytes;
    }
    // wait for every copy; throws on a failed one
    void finish() {
        drain();
        if (!kerr.empty()) fail(SRG_ERR_HIP, "key D2H: " + kerr);
        HIP_CHECK(hipStreamSynchronize(cs));
        if (!err.empty()) fail(SRG_ERR_HIP, "D2H copy: " + err);
    }
    ~HostSink() { drain(); }  // an exception unwound past finish(): drain before the buffers go away

   private:
    // both helper threads joined, every SDMA copy complete, the per-copy signals and events gone
    void drain() {
        if (kthread.joinable()) kthread.join();
        if (worker.joinable()) {
            {
                std::lock_guard<std::mutex> lk(mu);
                closing = true;
            }
            cv.notify_one();
            worker.join();
        }
        for (hsa_signal_t sg : sigs) {
            hsa_signal_wait_scacquire(sg, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
            hsa_signal_destroy(sg);
        }
        sigs.clear();
        for (hipEvent_t e : evs) (void)hipEventDestroy(e);
        evs.clear();
    }
};

// The caller's output arrays are page-locked for the SDMA copies; a fresh array (the Rust
// binding's vec![0u64; n*n] is lazily zeroed memory) is faulted in by that registration, 4 KB at
// a time.  Advising transparent huge pages first (the boxes run THP in "madvise" mode) lets the
// not-yet-touched part of the range fault in 2 MB pages: ~600 faults for the 1.2 GB C3 table
// instead of ~300 000.  Advisory only: pages already present stay as they are.
void advise_huge(void* p, size_t bytes) {
    const uintptr_t a = ((uintptr_t)p + ((size_t)2 << 20) - 1) & ~(uintptr_t)(((size_t)2 << 20) - 1);
    const uintptr_t e = ((uintptr_t)p + bytes) & ~(uintptr_t)(((size_t)2 << 20) - 1);
    if (e > a) (void)madvise((void*)a, e - a, MADV_HUGEPAGE);
}

// Fault a fresh output range in from several threads before it is page-locked: hipHostRegister
// faults the never-touched pages in one thread (49-58 ms for the 1.2 GB C3 table even in 2 MB
// pages, exposed after FW on a fresh table); each thread writes one byte per page of its slice (the
// table is an output: its contents are overwritten anyway).
void prefault(void* p, size_t bytes, int nthreads) {
    if (!p || bytes < ((size_t)64 << 20)) return;
    const size_t pg = 4096, per = (bytes / nthreads + pg - 1) / pg * pg;
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t) {
        const size_t a = (size_t)t * per, e = std::min(bytes, a + per);
        if (a >= e) break;
        th.emplace_back([=]() {
            volatile unsigned char* b = (volatile unsigned char*)p;
            for (size_t o = a; o < e; o += pg) b[o] = 0;
        });
    }
    for (auto& x : th) x.join();
}

// Contexts per device in this process (srg_create / srg_destroy): the FW's cross-stream hops
// use stream memory operations only when a context is alone on its device (stream_hop).
std::mutex g_dev_mu;
std::map<int, int> g_dev_ctx;

// `to` waits until `from` has reached this point.  hipStreamWriteValue32 + hipStreamWaitValue32 on
// HSA signal memory cost 5 us per hop against 11 us for hipEventRecord + hipStreamWaitEvent
// (tools/xq_probe.hip; 1-3 ms of FW at N = 2..8).  The wait is a polling kernel the
// runtime knows nothing about, so it is safe only while every wait is queued behind the write it
// waits for: true for one context -- ONE host thread enqueues both halves of every hop, the write
// first (fw_line_sym: the calling thread; FwOverlap: its FW thread, which issues every launch on
// the FW and chain streams, the submitting thread only the H2D stream), and streams sharing a
// hardware queue keep that order -- not for several contexts on one device (in-process rank
// groups: two waits could each block the queue holding the other's write), nor under a profiler
// that serialises dispatches (rocprofv3 --pmc hung on it): those use events (and
// SRG_STREAM_HOPS=events forces them).
// The value form is a pair of one-wave kernels of our own instead of hipStreamWriteValue32 /
// hipStreamWaitValue32 (the same mechanism: the runtime's wait is a polling blit kernel too), so
// that the wait is bounded: past its bound it raises the FW timeout word and returns, and the host
// reports SRG_ERR_HIP after FW instead of hanging on a mis-ordered enqueue.
// The wait also returns as soon as the timeout word is set (a closure barrier gave up: nothing
// after it is valid).  That word and the closure barrier words are reset per build on the FW
// stream; SymFw::begin orders the chain stream after that reset with an EVENT.  Without it (rounds
// 3-4) a chain-stream wait could run before the reset, read the previous occupant's value of the
// word (a recycled allocation: nonzero), return at once, and the reset then erased the evidence:
// the chain ran ahead of line 0 and the build returned an all-zero table with rc = 0, or a closure
// counted arrivals into words the reset then zeroed (the barrier timeouts) -- DESIGN.md §5.
__global__ void k_hop_set(uint32_t* sig, uint32_t v) {
    if (threadIdx.x == 0) __hip_atomic_store(sig, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void k_hop_wait(const uint32_t* sig, uint32_t v, uint32_t* timeout, unsigned long long bound_ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();  // 100 MHz
    while (__hip_atomic_load(sig, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - v > 0x7FFFFFFFu) {  // sig < v (mod 2^32)
        if (__hip_atomic_load(timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;  // keep the raiser's code
        if (wall_clock64() - t0 > bound_ticks) {
            uint32_t zero = 0;  // 2 = a hop timed out, unless something else was first
            __hip_atomic_compare_exchange_strong(timeout, &zero, 2u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

void stream_hop(srg_ctx& c, int i, hipStream_t from, hipStream_t to, hipEvent_t ev) {
    if (c.hop_values && c.sig[i] && c.fw_timeout) {
        const uint32_t v = ++c.sig_val[i];
        k_hop_set<<<1, 64, 0, from>>>(c.sig[i], v);
        k_hop_wait<<<1, 64, 0, to>>>(c.sig[i], v, c.fw_timeout, c.hop_bound_ticks);
        HIP_CHECK(hipGetLastError());
        return;
    }
    HIP_CHECK(hipEventRecord(ev, from));
    HIP_CHECK(hipStreamWaitEvent(to, ev, 0));
}

// FW lookahead chain kernels raise their wave priority (s_setprio 3) beside the bulk tiles: C3 FW
// 24.1 -> 23.5 ms (profiles/r02/prio; the option that turned it off was A/B only and is gone)
constexpr int kChainPrio = 1;

#ifndef SRG_FW_KC
#define SRG_FW_KC 32
#endif
constexpr int KC = SRG_FW_KC;

// tiles of one min-plus product launch: rows [ra, rb) minus {rx...}, cols [ca, cb) minus {cx...}
struct Rect {
    TileSet ts;
    int nr, nc;
};

inline Rect make_rect(int ra, int rb, std::initializer_list<int> rx, int ca, int cb, std::initializer_list<int> cx) {
    auto norm = [](int a, int b, std::initializer_list<int> x, int& x0, int& x1) {
        std::vector<int> v;
        for (int e : x)
            if (e >= a && e < b && std::find(v.begin(), v.end(), e) == v.end()) v.push_back(e);
        std::sort(v.begin(), v.end());
        x0 = v.size() > 0 ? v[0] : -1;
        x1 = v.size() > 1 ? v[1] : -1;
        return std::max(0, b - a - (int)v.size());
    };
    Rect r;
    r.nr = norm(ra, rb, rx, r.ts.rx0, r.ts.rx1);
    r.nc = norm(ca, cb, cx, r.ts.cx0, r.ts.cx1);
    r.ts.r0 = ra;
    r.ts.c0 = ca;
    return r;
}

// split-K factor for a short launch of `tiles` workgroups (critical-path launches only)
template <int T, int KCV>
int split_for(int tiles, bool enable) {
    if (!enable) return 1;
    constexpr int maxs = T / KCV;
    int sp = 1;
    while (sp < maxs && tiles * sp * 2 <= 512) sp *= 2;
    return sp;
}

template <int PK>
constexpr int kc_for() { return PK ? pk_kc<PK>() : KC; }

template <class K, int T, int PK>
void fw_tiles(K* D, size_t ld, int kb, int ra, int rb, std::initializer_list<int> rx, int ca, int cb,
              std::initializer_list<int> cx, size_t lds, hipStream_t s, bool split = false) {
    const Rect r = make_rect(ra, rb, rx, ca, cb, cx);
    if (r.nr <= 0 || r.nc <= 0) return;
    const int sp = split_for<T, kc_for<PK>()>(r.nr * r.nc, split);
    fw_product<K, T, kc_for<PK>(), PK><<<dim3(r.nc, r.nr, sp), 256, lds, s>>>(D, ld, kb, r.ts);
}

template <class K, int T, int PK>
void fw_tiles_pair(K* D, size_t ld, int kb, const Rect& a, const Rect& b, size_t lds, hipStream_t s,
                   bool split = false) {
    const int na = std::max(0, a.nr) * std::max(0, a.nc), nb = std::max(0, b.nr) * std::max(0, b.nc);
    if (na + nb == 0) return;
    const int sp = split_for<T, kc_for<PK>()>(na + nb, split);
    fw_product_pair<K, T, kc_for<PK>(), PK><<<dim3(na + nb, 1, sp), 256, lds, s>>>(D, ld, kb, a.ts, na, std::max(1, a.nc),
                                                                        b.ts, std::max(1, b.nc));
}

// Blocked Floyd-Warshall over the rank's row blocks with a one-block lookahead:
//   pivot kb+1's owner updates row kb+1 (w.r.t. kb) first, closes pivot kb+1 and its row
//   panel on the auxiliary stream, and broadcasts the panel (T x Vp keys, in place) while
//   every rank finishes the remaining tiles of kb; then each rank updates its own column
//   panel of kb+1.  Single GPU: the same schedule with the broadcast elided.
template <class K, int T, int PK>
void fw_blocked(srg_ctx& c, const Plan& pl, K* D, size_t Vp, hipStream_t st, uint64_t& prof_relax, int& prof_n) {
    const int nb = pl.nb;
    constexpr int KCV = kc_for<PK>();
    // double-buffered LDS image: A^T + B (add + min3 tiles) or the k-pair image (packed tiles)
    const size_t lds = PK ? pk_lds_bytes<T, KCV>() : (size_t)4 * KCV * (T + 16 / (int)sizeof(K)) * sizeof(K);
    set_lds(fw_product<K, T, KCV, PK>, lds);
    set_lds(fw_product_pair<K, T, KCV, PK>, lds);
    const bool multi = c.comm && c.comm->nranks > 1;
    const bool prof = c.profiling && nb > 2;
    if (prof) {
        ensure_prof_events(c, (size_t)2 * nb);
    }
    hipStream_t aux = c.aux_stream, cs = c.comm_stream;
    const size_t panel_bytes = (size_t)T * Vp * sizeof(K);
    auto panel = [&](int b) { return (void*)(D + (size_t)b * T * Vp); };
    const int r0 = pl.rb0, r1 = pl.rb1;
    // pivot 0
    if (pl.own(0)) {
        fw_phase1<K, T><<<1, 512, 0, st>>>(D, Vp, 0, kChainPrio);
        fw_tiles<K, T, PK>(D, Vp, 0, 0, 1, {}, 0, nb, {0}, lds, st, pl.G > 1);
    }
    if (multi) {
        HIP_CHECK(hipEventRecord(c.ev_c, st));
        HIP_CHECK(hipStreamWaitEvent(cs, c.ev_c, 0));
        c.comm->bcast(panel(0), panel_bytes, pl.owner(0), cs);
        HIP_CHECK(hipEventRecord(c.ev_c, cs));
        HIP_CHECK(hipStreamWaitEvent(st, c.ev_c, 0));
    }
    fw_tiles<K, T, PK>(D, Vp, 0, r0, r1, {0}, 0, 1, {}, lds, st);
    for (int kb = 0; kb < nb; ++kb) {
        if (kb + 1 >= nb) {
            fw_tiles<K, T, PK>(D, Vp, kb, r0, r1, {kb}, 0, nb, {kb}, lds, st);
            break;
        }
        const int k1 = kb + 1;
        // critical chain on the (high-priority) aux stream, concurrent with the bulk tiles of kb
        // on st: row k1 + own column k1 (w.r.t. kb) in one launch -> close pivot k1 -> its row +
        // column panels.  The chain's tiles are disjoint from the bulk's; both only read panel kb.
        const bool sk = pl.G > 1;  // split-K the chain's short launches when the rest is short too
        HIP_CHECK(hipEventRecord(c.ev_a, st));  // st: bulk of kb-1 (row k1 w.r.t. kb-1) done
        HIP_CHECK(hipStreamWaitEvent(aux, c.ev_a, 0));
        const Rect rowr = pl.own(k1) ? make_rect(k1, k1 + 1, {}, 0, nb, {kb}) : Rect{TileSet{0, -1, -1, 0, -1, -1}, 0, 0};
        fw_tiles_pair<K, T, PK>(D, Vp, kb, rowr, make_rect(r0, r1, {kb, k1}, k1, k1 + 1, {}), lds, aux, sk);
        const Rect colp = make_rect(r0, r1, {k1}, k1, k1 + 1, {});  // own column panel of k1
        if (pl.own(k1)) {
            fw_phase1<K, T><<<1, 512, 0, aux>>>(D, Vp, k1, kChainPrio);
            // the column panel of k1 rewrites tile (kb, k1) of panel kb: its broadcast (still the
            // last one recorded in ev_c) must have left first
            if (multi) HIP_CHECK(hipStreamWaitEvent(aux, c.ev_c, 0));
            fw_tiles_pair<K, T, PK>(D, Vp, k1, make_rect(k1, k1 + 1, {}, 0, nb, {k1}), colp, lds, aux, sk);
        }
        if (multi) {
            HIP_CHECK(hipEventRecord(c.ev_b, aux));
            HIP_CHECK(hipStreamWaitEvent(cs, c.ev_b, 0));
            c.comm->bcast(panel(k1), panel_bytes, pl.owner(k1), cs);
            HIP_CHECK(hipEventRecord(c.ev_c, cs));
            if (!pl.own(k1)) {  // the pivot tile arrives in the panel
                HIP_CHECK(hipStreamWaitEvent(aux, c.ev_c, 0));
                fw_tiles_pair<K, T, PK>(D, Vp, k1, Rect{TileSet{0, -1, -1, 0, -1, -1}, 0, 0}, colp, lds, aux, sk);
            }
        }
        HIP_CHECK(hipEventRecord(c.ev_d, aux));
        // the remaining tiles of kb (the dominant kernel), overlapped with the above
        const int nr = (r1 - r0) - (pl.own(kb) ? 1 : 0) - (pl.own(k1) ? 1 : 0);
        const bool timed = prof && nr > 0 && nb > 2;
        if (timed) HIP_CHECK(hipEventRecord(c.prof_events[2 * prof_n], st));
        fw_tiles<K, T, PK>(D, Vp, kb, r0, r1, {kb, k1}, 0, nb, {kb, k1}, lds, st);
        if (timed) {
            HIP_CHECK(hipEventRecord(c.prof_events[2 * prof_n + 1], st));
            prof_relax += (uint64_t)nr * (nb - 2) * T * T * T;
            ++prof_n;
        }
        HIP_CHECK(hipStreamWaitEvent(st, c.ev_d, 0));
        // receivers need panel k1 before their next updates; its owner only before it rewrites a
        // tile of it (the column panel of k2 on aux, which waits above), so the owner's chain of
        // k2 overlaps the broadcast of k1
        if (multi && !pl.own(k1)) HIP_CHECK(hipStreamWaitEvent(st, c.ev_c, 0));
    }
}

// low 32 bits of u64 keys (the u64 path's scan input, tight_v5 with inf_check = 0)
__global__ void k_low_words(const uint64_t* __restrict__ x, size_t n, uint32_t* __restrict__ lo) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        lo[i] = (uint32_t)x[i];
}

// Symmetric blocked FW over line buffers (undirected graph, u32 pair-packed tiles, one or
// several ranks; kernels.hip.h fw_core_lb / LineMap).  Tile (I, J) belongs to rank (I + J) mod G.
// Per pivot kb, with k1 = kb + 1:
//   chain (aux stream, raised priority), after this rank's bulk of kb - 1:
//     1. line k1 w.r.t. kb over the rank's own tiles of line k1 -> D and the line buffer LB(k1)
//     2. (ranks > 1) allgatherv of LB(k1): one contiguous segment per rank (owner-major slots)
//     3. close the pivot tile (k1, k1) inside LB(k1): eight squaring launches of 64 workgroups
//        (every rank, redundantly)
//     4. line k1 w.r.t. k1 over all of LB(k1), own tiles written back to D (every rank)
//   bulk (main stream): the rank's stored tiles off lines kb and k1 through LB(kb).
// Line 0 needs no exchange (every rank starts from the same D).  The chain of k1 overlaps the
// bulk of kb; LB(k1) is written only after the bulk of kb - 1, the last reader of its buffer.
// At the end the lower triangle is mirrored (one rank) or the ranks' tiles are all-gathered and
// unpacked with the mirror, so that every rank holds the whole D.  shadow_amd/dist.py line_fw
// restates this schedule in numpy (tests/test_dist_cpu.py runs it on gloo ranks).
template <class K, int T>
void fw_sym_finish(srg_ctx& c, const Plan& pl, K* D, size_t Vp, hipStream_t st, const std::vector<int>& own_h,
                   const std::vector<int>& slot_h, const std::vector<int>& first, double& ms_xchg);

// this rank's stored tiles (triangle indices, row-major; uploaded to c.b_tiles), and for the final
// exchange every tile's slot in the packed buffer (owner-major, each owner's tiles in triangle order)
inline void sym_tiles(srg_ctx& c, const Plan& pl, hipStream_t st, std::vector<int>& own_h, std::vector<int>& slot_h,
                      std::vector<int>& first, std::vector<int>& bulk_off) {
    const int nb = pl.nb, G = pl.G, g = pl.g;
    const int ntri = nb * (nb + 1) / 2;
    own_h.clear();
    slot_h.assign(ntri, 0);
    first.assign(G + 1, 0);
    for (int t = 0, I = 0; I < nb; ++I)
        for (int J = I; J < nb; ++J, ++t) {
            const int r = (I + J) % G;
            if (r == g) own_h.push_back(t);
            ++first[r + 1];
        }
    for (int r = 0; r < G; ++r) first[r + 1] += first[r];
    std::vector<int> fill(first.begin(), first.end() - 1);
    for (int t = 0, I = 0; I < nb; ++I)
        for (int J = I; J < nb; ++J, ++t) slot_h[t] = fill[(I + J) % G]++;
    // the bulk's launch order after own_h in the same buffer: one list for every pivot
    // (xcd_tile_order), or own_h itself (bulk_off empty)
    std::vector<int> bulk;
    bulk_off.clear();
    if (c.fw_xcd_order) xcd_tile_order(own_h, nb, bulk, bulk_off);
    int* tiles = (int*)c.b_tiles.get(std::max<size_t>(own_h.size() + bulk.size(), 1) * 4);
    if (!own_h.empty()) {
        HIP_CHECK(hipMemcpyAsync(tiles, own_h.data(), own_h.size() * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(tiles + own_h.size(), bulk.data(), bulk.size() * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));  // (host vectors)
    }
}

// The schedule as a stepper: begin() builds line 0, pivot(kb, maxI) enqueues the chain of kb + 1 and
// the bulk of kb (tiles of block-rows <= maxI), end() mirrors or exchanges.  fw_line_sym runs it
// straight through; the host entry's FW beside the H2D (FwOverlap) runs pivots as block-rows of the
// edge list land, with every line kept (keep_lines) for the late tiles' catch-up.
int chain_xmode(const srg_ctx& c);

template <class K, int T>
struct SymFw {
    static constexpr int KCS = 16;
    static constexpr size_t TT = (size_t)T * T;
    srg_ctx& c;
    const Plan& pl;
    K* D;
    size_t Vp;
    hipStream_t st;
    int nb, G, g, split = 1, bulk_split = 1, ntile = 0, prio = kChainPrio;
    bool multi = false, prof = false, keep_lines = false;
    LineMap lm{1, 1};
    size_t lds_bulk = 0;
    uint32_t* cflags = nullptr;
    const int* tiles = nullptr;   // own stored tiles (triangle order), then the bulk's launch order
    std::vector<int> own_h, slot_h, first;
    std::vector<int> bulk_off;    // SRG_OPT_FW_XCD_ORDER: pivot kb's launch list at tiles + ntile + bulk_off[kb]
    K* lbuf[3] = {nullptr, nullptr, nullptr};
    K* lball = nullptr;  // keep_lines: line p at lball + p * nb * TT
    int xmode = 0;       // chain_xmode: how LB(k1) is exchanged
    std::vector<void*> plb;       // xmode 2: every rank's line-buffer block, arrival words
    std::vector<uint32_t*> pfl;
    uint32_t* myflags = nullptr;
    bool sys = false;
    uint64_t* prof_relax = nullptr;
    int* prof_n = nullptr;

    SymFw(srg_ctx& c_, const Plan& pl_, K* D_, size_t Vp_, hipStream_t st_) : c(c_), pl(pl_), D(D_), Vp(Vp_), st(st_) {
        nb = pl.nb;
        G = pl.G;
        g = pl.g;
        multi = c.comm && c.comm->nranks > 1;
        lm = LineMap{nb, G};
        xmode = chain_xmode(c);
    }
    // two line buffers round-robin; three with a device-side exchange (a peer may store LB(k1) while
    // this rank's bulk of kb - 1 still reads LB(kb - 1), never earlier: the peer's chain of k1 ran
    // after its exchange of kb, which waited for this rank's line kb, i.e. this rank's bulk of kb - 2)
    K* lb(int p) const { return keep_lines ? lball + (size_t)p * nb * TT : lbuf[xmode ? p % 3 : p & 1]; }
    void line(const K* lbL, int L, K* lbK, int K1, int mode, int ntiles, hipStream_t s) const {
        if (!ntiles) return;
        if (split == 4)
            fw_line_lb<K, T, 4><<<dim3(ntiles, 16), 256, lb_lds<K, T / 4, line_kc<4>()>(), s>>>(D, Vp, lbL, L, lbK, K1, mode, lm, g, prio);
        else if (split == 2)
            fw_line_lb<K, T, 2><<<dim3(ntiles, 4), 256, lb_lds<K, T / 2, line_kc<2>()>(), s>>>(D, Vp, lbL, L, lbK, K1, mode, lm, g, prio);
        else
            fw_line_lb<K, T, 1><<<dim3(ntiles, 1), 256, lb_lds<K, T, line_kc<1>()>(), s>>>(D, Vp, lbL, L, lbK, K1, mode, lm, g, prio);
    }
    void close_pivot(K* lbk, int k, hipStream_t s) const {
        fw_close_sq<K, T><<<dim3(T / 16, T / 16), 256, 0, s>>>(lbk + (size_t)lm.slot(k, k) * TT, cflags + 16 * k, c.fw_timeout,
                                                             prio);
    }
    void begin(uint64_t& relax, int& n) {
        prof_relax = &relax;
        prof_n = &n;
        {
            const bool events = srg_env::stream_hops_events();
            std::lock_guard<std::mutex> lk(g_dev_mu);
            c.hop_values = g_dev_ctx[c.device] == 1 && !events;
        }
        lds_bulk = lb_lds<K, T, KCS>();
        set_lds(fw_bulk_lb<K, T, KCS>, lds_bulk);
        // The chain's line launches.  A large bulk (C3 on one rank: ~nb^2/2 = 3 160 tiles, four rounds
        // of the chip's 768 slots) hides the chain, so the lines take whole tiles (the fewest CU slots
        // taken from the bulk).  A bulk below ~2 rounds (several ranks, or a small graph) leaves the
        // chain as the critical path: sub-tiles, S^2 x the workgroups at a fraction of the latency
        // (SRG_OPT_FW_LINE_SPLIT; FW at sim 2:0 / 4:0 / 8:0 with whole tiles, quadrants, 32 x 32:
        // 17.9 / 15.1 / 15.6, 14.9 / 12.2 / 12.1, 11.0 / 7.7 / 7.2 ms, profiles/r03c/, r03k/; one rank,
        // C2 (nb = 32) 3.6 / 2.8 / 2.6 ms, C1 (nb = 8) 0.79 / 0.48 / 0.47 ms, profiles/r03x/).  The
        // pivot closure is one launch of 64 workgroups either way (fw_close_sq; eight squaring launches
        // took 45-117 us per pivot, the one-workgroup FW closure 159 us beside the bulk: r03b/).
        const int bulk_tiles = nb * (nb + 1) / 2 / G;
        // (C2, nb = 32, 528 tiles: quadrant lines, host entry 7.16-7.27 vs 7.39-8.76 ms with 32 x 32,
        // profiles/r06/c2/)
        split = c.fw_line_split ? c.fw_line_split : bulk_tiles >= 2048 ? 1 : bulk_tiles >= 512 ? 2 : 4;
        // a bulk below one round of the slots (3 per CU) runs as quadrants (fw_bulk_lb_q): sim 8:0
        // bulk launch 59.5 -> 48.6 us, FW 6.24-6.28 -> 6.02-6.04 ms (profiles/r05/chain/)
        // (one rank too: C2, nb = 32, 528 tiles; SRG_FW_BULK_Q = 0 / 1 forces it off / on for A/B)
        const int bq = srg_env::fw_bulk_q();
        if (sizeof(K) == 4 && T == 128 && bq != 0) {
            int cus = 256;
            HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device));
            if (bulk_tiles < 3 * cus || bq == 1) {
                bulk_split = 2;
                set_lds(fw_bulk_lb_q<K, T, 32>, lb_lds<K, T / 2, 32>());
            }
        }
        set_lds(fw_line_lb<K, T, 1>, lb_lds<K, T, line_kc<1>()>());
        set_lds(fw_line_lb<K, T, 2>, lb_lds<K, T / 2, line_kc<2>()>());
        set_lds(fw_line_lb<K, T, 4>, lb_lds<K, T / 4, line_kc<4>()>());
        prof = c.profiling && nb > 2;
        if (prof) {
            ensure_prof_events(c, (size_t)2 * nb);
        }
        if (keep_lines) lball = (K*)c.b_xlb.get((size_t)nb * nb * TT * sizeof(K));
        else if (xmode) {  // one block of three (the peers' stores address it by offset)
            K* x = (K*)c.b_xlb.get(3 * (size_t)nb * TT * sizeof(K));
            for (int i = 0; i < 3; ++i) lbuf[i] = x + (size_t)i * nb * TT;
        } else {
            lbuf[0] = (K*)c.b_L0.get(nb * TT * sizeof(K));
            lbuf[1] = (K*)c.b_L1.get(nb * TT * sizeof(K));
        }
        if (xmode == 2) {  // every rank's block and arrival words (a host rendezvous per build)
            const size_t fb = (size_t)nb * G * 4;
            if (c.b_xflags.bytes < fb) {
                c.b_xflags.get(fb);
                HIP_CHECK(hipMemsetAsync(c.b_xflags.p, 0, fb, st));
            }
            myflags = (uint32_t*)c.b_xflags.p;
            HIP_CHECK(hipStreamSynchronize(st));  // zeroed words before any peer may raise one
            plb.assign(G, nullptr);
            pfl.assign(G, nullptr);
            // the flag value of this build: every rank proposes its next one and all take the largest,
            // so a rank that skipped or repeated a build cannot leave the others waiting for a stale
            // value
            uint32_t ep = c.xepoch + 1 ? c.xepoch + 1 : 1;
            c.comm->share_ptrs(lbuf[0], myflags, plb.data(), pfl.data(), &sys, &ep);
            c.xepoch = ep;
        }
        // closure barrier words: 16 per pivot (arrival counter, changed flag per step), then the
        // timeout word; zeroed per build (a multiple of 16 bytes from the allocation's start)
        cflags = (uint32_t*)c.b_cflags.get(((size_t)nb * 16 + 4) * 4);
        c.fw_timeout = cflags + (size_t)nb * 16;
#ifdef SRG_TEST_HOOKS
        if (c.test_fault == 2) {
            // TEST HOOK: the state of a recycled allocation -- nonzero sync words, zero line buffers --
            // in place before this build's reset (the value-hop race of rounds 3-4, stream_hop)
            HIP_CHECK(hipMemsetAsync(cflags, 0xA5, ((size_t)nb * 16 + 4) * 4, c.aux_stream));
            if (keep_lines) HIP_CHECK(hipMemsetAsync(lball, 0, (size_t)nb * nb * TT * sizeof(K), c.aux_stream));
            HIP_CHECK(hipStreamSynchronize(c.aux_stream));
        }
#endif
        HIP_CHECK(hipMemsetAsync(cflags, 0, ((size_t)nb * 16 + 4) * 4, st));
        // the chain stream's kernels (hop waits, closures, the exchange) read and count in these
        // words: the chain stream waits for their reset by an EVENT (a value hop's wait kernel would
        // read the very word being reset; see stream_hop)
        HIP_CHECK(hipEventRecord(c.ev_fwreset, st));
        HIP_CHECK(hipStreamWaitEvent(c.aux_stream, c.ev_fwreset, 0));
        // a value hop's wait bound: 2 s, or 20 x an estimate of the longest legitimate wait (one
        // bulk launch of this rank at ~30 T relaxations/s) when that is longer
        {
            const double relax = (double)nb * (nb + 1) / 2 / G * (double)T * T * T;
            const double ticks = 20.0 * relax / 30e12 * 1e8;
            c.hop_bound_ticks = std::max<unsigned long long>(200000000ull, (unsigned long long)std::min(ticks, 1e12));
        }
        sym_tiles(c, pl, st, own_h, slot_h, first, bulk_off);
        ntile = (int)own_h.size();
        tiles = (const int*)c.b_tiles.p;
        // line 0: every rank holds the same initial D
        k_pack_line<K, T><<<nb, 256, 0, st>>>(D, Vp, lb(0), 0, lm);
        close_pivot(lb(0), 0, st);
        line(lb(0), 0, lb(0), 0, 1, nb, st);  // (with nb == 1 this only copies the closed pivot tile back to D)
        HIP_CHECK(hipGetLastError());
    }
    // the chain of k1 = kb + 1 (aux stream) and the bulk of kb over block-rows <= maxI (main stream)
    void pivot(int kb, int maxI) {
        const int k1 = kb + 1;
        hipStream_t aux = c.aux_stream;
        K* lbk = lb(kb);
        if (k1 < nb) {
            K* lbn = lb(k1);
            stream_hop(c, 0, st, aux, c.ev_a);  // st: bulk of kb - 1 done
            line(lbk, kb, lbn, k1, 0, lm.count(g, k1), aux);
            if (multi && xmode) {
                exchange(lbn, k1, aux);
            } else if (multi) {  // on the chain's own stream: no cross-queue hop around it
                std::vector<size_t> offs(G), lens(G);
                for (int r = 0; r < G; ++r) {
                    offs[r] = (size_t)lm.base(r, k1) * TT * sizeof(K);
                    lens[r] = (size_t)lm.count(r, k1) * TT * sizeof(K);
                }
                c.comm->allgatherv(lbn, offs.data(), lens.data(), aux);
            }
            close_pivot(lbn, k1, aux);
            line(lbn, k1, lbn, k1, 1, nb, aux);
            HIP_CHECK(hipGetLastError());
        }
        // the remaining tiles of kb (the dominant kernel), overlapped with the chain of k1
        const bool timed = prof && ntile > 0 && k1 < nb && maxI >= nb - 1;
        if (timed) HIP_CHECK(hipEventRecord(c.prof_events[2 * *prof_n], st));
        auto bulk = [&](int nl, const int* list) {
            if (bulk_split == 2)
                fw_bulk_lb_q<K, T, 32><<<dim3(nl, 4), 256, lb_lds<K, T / 2, 32>(), st>>>(D, Vp, lbk, kb, kb, k1 < nb ? k1 : -1,
                                                                                         lm, list, maxI);
            else
                fw_bulk_lb<K, T, KCS><<<nl, 256, lds_bulk, st>>>(D, Vp, lbk, kb, kb, k1 < nb ? k1 : -1, lm, list, maxI);
        };
        if (!bulk_off.empty() && maxI >= nb - 1) {  // (beside the H2D, with rows still missing: triangle order,
                                                    // which spreads the missing rows' idle slots over the XCDs)
            const int nl = bulk_off[kb + 1] - bulk_off[kb];
            if (nl > 0) bulk(nl, tiles + ntile + bulk_off[kb]);
        } else if (ntile > 0) {
            bulk(ntile, tiles);
        }
        HIP_CHECK(hipGetLastError());
        if (timed) {
            int64_t m = 0;  // relaxations of this launch: own tiles off lines kb and k1
            for (int t : own_h) {
                int I, J;
                tri_tile_h(nb, t, I, J);
                if (I != kb && I != k1 && J != kb && J != k1) ++m;
            }
            HIP_CHECK(hipEventRecord(c.prof_events[2 * *prof_n + 1], st));
            *prof_relax += (uint64_t)m * T * T * T;
            ++*prof_n;
        }
        if (k1 < nb) stream_hop(c, 1, aux, st, c.ev_d);  // the chain of k1 (LB(k1) final) before the bulk of k1
    }
    // device-side exchange of LB(k1) on the chain's stream (k_line_xchg)
    void exchange(K* lbn, int k1, hipStream_t s) {
        XchgArgs<K> a{};
        a.k1 = k1;
        a.G = G;
        a.g = g;
        a.sys = sys ? 1 : 0;
        a.xmode = xmode;
        a.epoch = c.xepoch;
        a.timeout = c.fw_timeout;
        a.myflags = myflags;
        a.cnt = cflags + 16 * k1 + 13;  // a free word of the pivot's group (the closure uses 0..8)
        a.off = (size_t)lm.base(g, k1) * TT;
        a.seg = lbn + a.off;
        a.n8 = (size_t)lm.count(g, k1) * TT * sizeof(K) / 8;
        int grid = 1;
        if (xmode == 1) {
            size_t mx = 0;  // the largest segment a peer sends this rank
            for (int r = 0; r < G; ++r)
                if (r != g) mx = std::max(mx, (size_t)lm.count(r, k1) * TT * sizeof(K));
            a.model_ns = (uint32_t)c.comm->model_xchg_ns(mx);
        } else {
            const size_t blk = (size_t)lbn - (size_t)lbuf[0];  // LB(k1)'s offset inside the block
            for (int r = 0; r < G && r < kMaxPeers; ++r)
                if (r != g) {
                    a.peer_lb[r] = (K*)((unsigned char*)plb[r] + blk);
                    a.peer_flags[r] = pfl[r];
                }
            grid = (int)std::max<size_t>(1, std::min<size_t>(64, (a.n8 + 255) / 256));
        }
        k_line_xchg<K><<<grid, 256, 0, s>>>(a);
        HIP_CHECK(hipGetLastError());
    }
    void end(double& ms_xchg) {
        HIP_CHECK(hipGetLastError());
        fw_sym_finish<K, T>(c, pl, D, Vp, st, own_h, slot_h, first, ms_xchg);
    }
};

template <class K, int T>
void fw_line_sym(srg_ctx& c, const Plan& pl, K* D, size_t Vp, hipStream_t st, uint64_t& prof_relax,
                 int& prof_n, double& ms_xchg) {
    SymFw<K, T> f(c, pl, D, Vp, st);
    f.begin(prof_relax, prof_n);
    for (int kb = 0; kb < f.nb; ++kb) f.pivot(kb, f.nb);
    f.end(ms_xchg);
}

// End of the symmetric FW: mirror the lower triangle (one rank), or every rank ends with the whole D:
// pack the own tiles, all-gather, unpack with the mirror.
template <class K, int T>
void fw_sym_finish(srg_ctx& c, const Plan& pl, K* D, size_t Vp, hipStream_t st, const std::vector<int>& own_h,
                   const std::vector<int>& slot_h, const std::vector<int>& first, double& ms_xchg) {
    const int nb = pl.nb, G = pl.G, g = pl.g;
    constexpr size_t TT = (size_t)T * T;
    const bool multi = c.comm && c.comm->nranks > 1;
    const int ntri = nb * (nb + 1) / 2, ntile = (int)own_h.size();
    const int* tiles = (const int*)c.b_tiles.p;
    hipStream_t cs = c.comm_stream;
    if (!multi) {
        const unsigned nb64 = (unsigned)(Vp / 64);
        k_sym_mirror<K><<<dim3(nb64, nb64), 256, 0, st>>>(D, Vp);
        return;
    }
    HIP_CHECK(hipStreamSynchronize(st));  // (FW done: the exchange is timed on its own)
    auto t0x = std::chrono::steady_clock::now();
    K* Pk = (K*)c.b_PRED.get((size_t)ntri * TT * sizeof(K));
    int* slot = (int*)c.b_tslot.get((size_t)ntri * 4);
    HIP_CHECK(hipMemcpyAsync(slot, slot_h.data(), (size_t)ntri * 4, hipMemcpyHostToDevice, st));
    if (ntile) k_pack_tiles<K, T><<<ntile, 256, 0, st>>>(D, Vp, nb, tiles, (size_t)first[g], Pk);
    std::vector<size_t> offs(G), lens(G);
    for (int r = 0; r < G; ++r) {
        offs[r] = (size_t)first[r] * TT * sizeof(K);
        lens[r] = (size_t)(first[r + 1] - first[r]) * TT * sizeof(K);
    }
    HIP_CHECK(hipEventRecord(c.ev_b, st));
    HIP_CHECK(hipStreamWaitEvent(cs, c.ev_b, 0));
    c.comm->allgatherv(Pk, offs.data(), lens.data(), cs);
    HIP_CHECK(hipEventRecord(c.ev_c, cs));
    HIP_CHECK(hipStreamWaitEvent(st, c.ev_c, 0));
    k_unpack_tiles<K, T><<<ntri, 256, 0, st>>>(Pk, slot, nb, D, Vp);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));
    ms_xchg += ms_since(t0x);
}

// General FW, several ranks: every rank ends with the whole D (row blocks all-gathered)
template <class K>
void gather_rows(srg_ctx& c, const Plan& pl, K* D, size_t Vp, int T, hipStream_t st, double& ms_xchg) {
    HIP_CHECK(hipStreamSynchronize(st));  // (FW done: the exchange is timed on its own)
    auto t0x = std::chrono::steady_clock::now();
    std::vector<size_t> offs(pl.G), lens(pl.G);
    for (int r = 0; r < pl.G; ++r) {
        const size_t a = std::min<size_t>(Vp, (size_t)pl.blk_lo[r] * T), b = std::min<size_t>(Vp, (size_t)pl.blk_lo[r + 1] * T);
        offs[r] = a * Vp * sizeof(K);
        lens[r] = (b - a) * Vp * sizeof(K);
    }
    HIP_CHECK(hipEventRecord(c.ev_b, st));
    HIP_CHECK(hipStreamWaitEvent(c.comm_stream, c.ev_b, 0));
    c.comm->allgatherv(D, offs.data(), lens.data(), c.comm_stream);
    HIP_CHECK(hipEventRecord(c.ev_c, c.comm_stream));
    HIP_CHECK(hipStreamWaitEvent(st, c.ev_c, 0));
    HIP_CHECK(hipStreamSynchronize(st));
    ms_xchg += ms_since(t0x);
}

// The chain's exchange of LB(k1) (xchg.hip.h): 0 = the communicator's allgather on the chain's
// stream, 1 = a simulated rank's modelled device-side exchange, 2 = stores into the peers' line
// buffers + arrival words (k_line_xchg).  Auto (SRG_OPT_FW_STEP = -1): the modelled exchange for
// simulated ranks, else the collective; 2 asks for the stores between in-process ranks.  The stores
// stay opt-in until they have run between distinct devices (only ranks sharing one GPU
// have exercised them; such ranks then need a hardware queue each for their chain streams).
int chain_xmode(const srg_ctx& c) {
    const bool multi = c.comm && c.comm->nranks > 1;
    if (!multi || c.fw_step == 0 || c.comm->nranks > kMaxPeers) return 0;
    const int dx = c.comm->device_exchange();
    if (dx == 1) return 1;
    if (dx == 2 && c.fw_step == 2) return 2;
    return 0;
}

// the symmetric FW over line buffers applies: undirected, u32 pair-packed 128-tiles or u64 64-tiles
template <class K, int T>
bool sym_fw_for(const srg_ctx& c, const DevGraph& g) {
    return ((sizeof(K) == 4 && T == 128) || (sizeof(K) == 8 && T == 64)) && c.fw_symmetric &&
           !g.directed;
}

// The host entry's FW beside the H2D (one rank, undirected graph, symmetric FW on u32
// keys counted in ns).  A GML complete graph lists its edges by source row, each (s, d) with s <= d;
// then block-row I of W (rows [128 I, 128 (I + 1))) is complete once the chunk holding the last edge
// of its rows has landed, and block-row I is all that line I and the rows' tiles need.  Per chunk:
// the chunk's latency-only keys into KW (k_w_key, on the H2D stream); per newly complete block-row:
// its tiles split from KW into W / D (k_w_split) and caught up on the pivots whose bulks already ran
// without them (fw_catchup, from the kept final lines); then every pivot whose line is complete is
// enqueued (SymFw::pivot, bulk over the complete block-rows only).  FW thus starts while the list
// is still arriving instead of after it (C3: the H2D is ~8 ms, host-bound on the codec's encoding).
// Speculative: the keys are nanoseconds (latency unit 1) -- exact whatever the unit -- and the edge
// checks run after the H2D as before (a failed check or certification discards this FW).  Any chunk
// that is not sequential-pair, or an edge (s, d) with s > d or a source row going backwards,
// abandons the overlap (ok = false): the build then runs from the landed edge list as usual.
// The FW's launches are issued by a thread of its own (enq): from the codec's submitting thread,
// ~80 pivots x ~6 launches and waits delayed the chunk submissions, H2D 8-9 -> 11-13 ms at C3
// (profiles/r04/c3_overlap_ab.txt).  The submitting thread records one event per landed chunk and
// queues (rows complete, event); the FW thread waits on the event in its stream and enqueues.
struct FwOverlap {
    static constexpr int T = 128;
    static constexpr size_t TT = (size_t)T * T;
    srg_ctx* c = nullptr;
    hipStream_t st = nullptr;   // FW (c.stream)
    hipStream_t hs = nullptr;   // H2D chunks (c.comm_stream)
    uint32_t V = 0;
    size_t Vp = 0;
    int nb = 0;
    Plan pl;
    std::unique_ptr<SymFw<uint32_t, T>> fw;
    uint32_t *W = nullptr, *WL = nullptr, *D = nullptr;
    unsigned long long* KW = nullptr;
    int A = -1, next = 0;       // block-rows complete; pivots enqueued (FW thread)
    int splitA = -1;            // block-rows split from KW on the H2D stream (submitting thread)
    std::atomic<bool> ok{false};
    bool on = false, begun = false, ended = false;
    // the FW thread and its queue of (block-rows complete, chunk event)
    std::thread enq;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::pair<int, hipEvent_t>> q;
    bool closing = false;
    std::exception_ptr err;
    size_t nev = 0;  // chunk events used this call
    static constexpr int catchup_wgs = 768;  // catch-up launch size target (128 / 256 / 1536 measured slower)
    uint32_t prev_src = 0;
    uint64_t prof_relax = 0;
    int prof_n = 0;
    double ms_xchg = 0;
    // SRG_DEBUG_OVERLAP: timing events (H2D start, each chunk's keys landed, each pivot's bulk done)
    bool dbg = false;
    hipEvent_t e0 = nullptr;
    std::vector<hipEvent_t> ce, pe;
    std::vector<int> ca;  // block-rows complete after each chunk
    hipEvent_t tev(hipStream_t s) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        HIP_CHECK(hipEventRecord(e, s));
        return e;
    }
    // after the FW: when each chunk landed and how far the FW had got by then (debug only: syncs)
    void report() {
        if (!dbg || !e0) return;
        HIP_CHECK(hipStreamSynchronize(st));
        auto ms = [&](hipEvent_t e) {
            float m = 0;
            HIP_CHECK(hipEventElapsedTime(&m, e0, e));
            return m;
        };
        std::vector<float> pt(pe.size());
        for (size_t i = 0; i < pe.size(); ++i) pt[i] = ms(pe[i]);
        for (size_t i = 0; i < ce.size(); ++i) {
            const float t = ms(ce[i]);
            int done = 0;
            for (float x : pt) done += x <= t;
            std::fprintf(stderr, "fw-overlap: chunk %2zu landed %6.2f ms, block-rows %3d, pivots done %3d\n", i, t, ca[i], done);
        }
        if (!pt.empty()) std::fprintf(stderr, "fw-overlap: last pivot done %.2f ms\n", pt.back());
        {  // a few entries of each buffer (debug)
            uint32_t w = 0, d = 0, l[4] = {0, 0, 0, 0};
            unsigned long long kw = 0;
            HIP_CHECK(hipMemcpy(&w, W + 1, 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(&d, D + 1, 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(&kw, KW + 1, 8, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(l, fw->lball + 1, 16, hipMemcpyDeviceToHost));
            std::fprintf(stderr, "fw-overlap: W[0][1] %u D[0][1] %u KW[0][1] %llx LB0 %u %u %u %u\n", w, d, kw, l[0], l[1],
                         l[2], l[3]);
        }
        for (hipEvent_t e : ce) HIP_CHECK(hipEventDestroy(e));
        for (hipEvent_t e : pe) HIP_CHECK(hipEventDestroy(e));
        HIP_CHECK(hipEventDestroy(e0));
        ce.clear();
        pe.clear();
        ca.clear();
        e0 = nullptr;
    }

    void init(srg_ctx& cc, uint32_t V_, const std::vector<uint32_t>& nodes_h) {
        c = &cc;
        st = cc.stream;
        hs = cc.comm_stream;
        V = V_;
        Vp = ((size_t)V + T - 1) / T * T;
        nb = (int)(Vp / T);
        pl = make_plan(1, 0, V, T, nodes_h);
        const size_t VV = Vp * Vp;
        W = (uint32_t*)cc.b_W.get(VV * 4);
        WL = (uint32_t*)cc.b_WL.get(VV * 4);
        D = (uint32_t*)cc.b_D.get(VV * 4);
        KW = (unsigned long long*)cc.b_PRED.get(VV * 8);
        HIP_CHECK(hipMemsetAsync(KW, 0xFF, VV * 8, hs));
        fw.reset(new SymFw<uint32_t, T>(cc, pl, D, Vp, st));
        fw->keep_lines = true;
        on = true;
        ok = true;
        dbg = srg_env::debug_overlap();
        if (dbg) e0 = tev(hs);
        enq = std::thread([this]() { run(); });
    }
    void run() {  // the FW thread: wait on each landed chunk in the FW stream, enqueue what it completes
        try {
            HIP_CHECK(hipSetDevice(c->device));
            for (;;) {
                std::pair<int, hipEvent_t> it;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&]() { return closing || !q.empty(); });
                    if (q.empty()) return;
                    it = q.front();
                    q.pop_front();
                }
                if (!ok) continue;
                HIP_CHECK(hipStreamWaitEvent(st, it.second, 0));
                advance(it.first);
            }
        } catch (...) {
            err = std::current_exception();
            ok = false;
        }
    }
    // every queued chunk enqueued (or dropped); rethrows the FW thread's error
    void finish() {
        if (!enq.joinable()) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            closing = true;
        }
        cv.notify_one();
        enq.join();
        if (err) std::rethrow_exception(err);
    }
    ~FwOverlap() {
        if (enq.joinable()) {
            {
                std::lock_guard<std::mutex> lk(mu);
                closing = true;
                ok = false;
            }
            cv.notify_one();
            enq.join();
        }
    }
    // a chunk's edges [e0, e0 + ne) are on the device (in hs order); exc = its exceptions (global
    // index, src, dst) when sequential-pair, null otherwise
    void chunk(const DevGraph& dg, size_t e0, size_t ne, const uint32_t* exc, size_t nexc, bool last) {
        if (!ok) return;
        bool good = exc != nullptr;
        for (size_t k = 0; good && k < nexc; ++k) {
            const uint32_t s = exc[3 * k + 1], d = exc[3 * k + 2];
            // a self-loop whose next edge is an exception too opens no row (W ignores it): any
            // position, e.g. a block of self-loops ahead of the rows
            const bool next_exc = k + 1 < nexc ? exc[3 * (k + 1)] == exc[3 * k] + 1 : exc[3 * k] + 1 == e0 + ne;
            if (s == d && next_exc) continue;
            good = s >= prev_src && s <= d;
            prev_src = s;
        }
        if (!good) {
            ok = false;
            return;
        }
        k_w_key<<<grid_for(ne), kThreads, 0, hs>>>(ne, dg.src + e0, dg.dst + e0, dg.lat + e0, 1, nullptr, KW, Vp, V);
        HIP_CHECK(hipGetLastError());
        // rows below the chunk's last source row are complete (all of them after the last chunk):
        // their tiles are split from KW here, on the H2D stream (beside FW: k_w_split writes the
        // upper tiles of its block-row, which FW does not touch before the row is complete, and
        // lower-triangle entries FW never reads)
        const int newA = last ? nb - 1 : std::min(nb - 1, (int)(prev_src / T) - 1);
        for (int I = splitA + 1; I <= newA; ++I)
            k_w_split<false><<<dim3((unsigned)(Vp / 64), 2), 256, 0, hs>>>(KW, Vp, 0, W, WL, D, (uint32_t)(2 * I));
        splitA = std::max(splitA, newA);
        HIP_CHECK(hipGetLastError());
        // one event per chunk (the FW thread may not have waited on the previous one yet)
        if (nev == c->ev_ov.size()) {
            c->ev_ov.emplace_back();
            c->ev_ov.back().create();
        }
        hipEvent_t ev = c->ev_ov[nev++];
        HIP_CHECK(hipEventRecord(ev, hs));
        if (dbg) {
            ce.push_back(tev(hs));
            ca.push_back(newA + 1);
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            q.emplace_back(newA, ev);
        }
        cv.notify_one();
    }
    void advance(int newA) {
        for (int I = A + 1; I <= newA; ++I)
            if (I > splitA)  // (only after the H2D: the submitting thread splits every landed row)
                k_w_split<false><<<dim3((unsigned)(Vp / 64), 2), 256, 0, st>>>(KW, Vp, 0, W, WL, D, (uint32_t)(2 * I));
        if (next > 0 && newA > A) {
            // the newly complete block-rows (A, newA] catch up in ONE launch over all their tiles,
            // each workgroup a K = 128 pg product over a group of the pivots run so far.  The
            // group count minimises waves x (pg + merge): a grid just past the 768 slots (3 per CU)
            // ran a second, nearly empty wave of full-length workgroups -- rounding ceil(768 /
            // tiles) groups up did that in most C3 launches (816-918 workgroups).  Host entry
            // 47.7-48.1 vs 48.1-50.1 ms in alternating runs (profiles/r05/catchup/)
            int tiles = 0;
            for (int I = A + 1; I <= newA; ++I) tiles += nb - I;
            int pg = next;
            double best = 1e300;
            for (int g = 1; g <= next; ++g) {
                const int p = (next + g - 1) / g, gg = (next + p - 1) / p;
                const double waves = std::ceil((double)tiles * gg / catchup_wgs);
                const double cost = waves * (p + 0.25);  // (0.25: C load + atomicMin merge, in pivots)
                if (cost < best - 1e-9) best = cost, pg = p;
            }
            set_lds(fw_catchup<T>, lb_lds<uint32_t, T, 16>());
            fw_catchup<T><<<dim3(tiles, (next + pg - 1) / pg), 256, lb_lds<uint32_t, T, 16>(), st>>>(
                D, Vp, fw->lball, (size_t)nb * TT, A + 1, nb, next, pg);
        }
        HIP_CHECK(hipGetLastError());
        A = std::max(A, newA);
        if (A < 0) return;
        if (!begun) {
            fw->begin(prof_relax, prof_n);
            begun = true;
        }
        while (next < nb && (next + 1 < nb ? A >= next + 1 : A >= nb - 1)) {
            fw->pivot(next, A);
            if (dbg) pe.push_back(tev(st));
            ++next;
        }
        if (next == nb && !ended) {
            fw->end(ms_xchg);
            ended = true;
        }
    }
};

#include "dense.hip.h"
#include "sparse_run.hip.h"
#include "routes.hip.h"
#include "route_trees.hip.h"

void compute_device(srg_ctx& c, const DevGraph& g, const uint32_t* nodes, uint32_t n, uint64_t* out_lat,
                    float* out_loss, hipStream_t st, srg_stats* stats, HostSink* sink = nullptr,
                    FwOverlap* ov = nullptr) {
    HIP_CHECK(hipStreamSynchronize(c.aux_stream));  // nothing of an aborted call still writes WL / PRED
    HIP_CHECK(hipStreamSynchronize(c.comm_stream));  // ... or the essential-entry counts
    c.scan_mirrored = 0;
    c.loss_kind = SRG_LOSS_NONE;
    if (g.V == 0) {
        if (n) fail(SRG_ERR_ARG, "nodes given for an empty graph");
        return;
    }
    // with the FW already queued beside the H2D the edge checks go on the (idle) H2D stream: on st
    // they would wait behind the whole FW before the host could read them
    const bool ov_fw = ov && ov->on && ov->ok && ov->begun;
    Prelude P = prelude(c, g, nodes, n, ov_fw ? c.comm_stream : st, true);
    if (n == 0) return;
    // u64 keys hold path sums below INF = 2^62 (a sum of two keys never wraps); a graph whose
    // worst-case path could reach 2^62 still runs, and only a used pair left at INF is an error:
    // SRG_ERR_LATENCY_RANGE then, since it may be a path the reference would wrap (mod.rs:327)
    // latency unit: every non-self-loop latency is a multiple of their gcd, hence so is every path
    // sum; keys count units (a ms-granular graph fits u32 keys up to 2^31-1 ms of path), outputs
    // are key * unit -- exact.  SRG_LATENCY_UNIT=1 keeps nanosecond keys (tests, A/B).
    const uint64_t unit = (P.es.unit > 1 && !srg_env::latency_unit_ns()) ? P.es.unit : 1;
    P.unit = unit;
    // the FW that ran beside the H2D counted nanoseconds (exact for any unit; its certification
    // decides as usual, a failure reruns on the u64 keys)
    const bool pre = ov && ov->on && ov->ok && ov->ended && P.es.max_lat < 0xFFFFFFFFull;
    if (pre) P.unit = 1;
    P.max_key = P.es.max_lat / P.unit;
    if (stats) stats->latency_unit_ns = P.unit;
    const unsigned __int128 bound = (unsigned __int128)P.max_key * (g.V > 1 ? g.V - 1 : 1);
    P.range_risk = bound >= ((unsigned __int128)1 << 62);
    // every shortest path is at most max_lat * (V - 1) ns and every relaxation the reference runs
    // at most max_lat * V: below 2^64 nothing wraps, and outputs D * unit fit u64
    P.wrap_risk = (unsigned __int128)P.es.max_lat * g.V >= ((unsigned __int128)1 << 64);
    const int G = c.comm ? c.comm->nranks : 1, rk = c.comm ? c.comm->rank : 0;
    if (choose_sparse(c, g) && !P.wrap_risk) {
        // u32 latency keys first; a graph whose arcs or used paths pass 2^32-1 units takes the
        // wide (u64-key) labels: exact, since max_lat * V < 2^64 (no wrap risk) bounds every sum
        loss_arrive(g, P.selfloss, st);
        if (P.max_key < 0xFFFFFFFFull && run_sparse(c, g, nodes, n, out_lat, out_loss, st, P, stats)) return;
        run_sparse(c, g, nodes, n, out_lat, out_loss, st, P, stats, true);
        return;
    }
    if (pre) {
        if (run_dense<uint32_t, FwOverlap::T>(c, g, ov->pl, nodes, n, out_lat, out_loss, st, P, stats, sink, ov)) {
            if (stats) stats->fw_overlap_kept = 1;
            return;
        }
        // the overlapped FW counted nanoseconds and failed its certification: the latencies' gcd unit
        // may still fit u32 keys -- the normal u32 build before the u64 one
        P.unit = unit;
        P.max_key = P.es.max_lat / P.unit;
        if (stats) stats->latency_unit_ns = P.unit;
        P.range_risk = (unsigned __int128)P.max_key * (g.V > 1 ? g.V - 1 : 1) >= ((unsigned __int128)1 << 62);
    }
    if ((!pre || P.unit > 1) && P.max_key < 0xFFFFFFFFull) {
        // FW tile: 128 (more work per launch) on one GPU; the multi-rank schedule is bound by
        // the per-pivot chain (close pivot -> panels), whose latency scales with T^3
        const int tile = c.fw_tile ? c.fw_tile : 128;
        if (tile == 64) {
            Plan pl = make_plan(G, rk, g.V, 64, P.nodes_h);
            if (run_dense<uint32_t, 64>(c, g, pl, nodes, n, out_lat, out_loss, st, P, stats, sink)) return;
        } else {
            Plan pl = make_plan(G, rk, g.V, 128, P.nodes_h);
            if (run_dense<uint32_t, 128>(c, g, pl, nodes, n, out_lat, out_loss, st, P, stats, sink)) return;
        }
    }
    Plan pl = make_plan(G, rk, g.V, 64, P.nodes_h);
    run_dense<uint64_t, 64>(c, g, pl, nodes, n, out_lat, out_loss, st, P, stats, sink);
}

void direct_device(srg_ctx& c, const DevGraph& g, const uint32_t* nodes, uint32_t n, uint64_t* out_lat,
                   float* out_loss, hipStream_t st) {
    Prelude P = prelude(c, g, nodes, n, st, false);
    loss_arrive(g, P.selfloss, st);
    if (n == 0) return;
    int32_t* pos = (int32_t*)c.b_pos.get((size_t)g.V * 4);
    uint32_t* cnt = (uint32_t*)c.b_cnt.get((size_t)n * n * 4);
    HIP_CHECK(hipMemsetAsync(pos, 0xFF, (size_t)g.V * 4, st));
    HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)n * n * 4, st));
    HIP_CHECK(hipMemsetAsync(&P.flags->first_bad, 0xFF, 8, st));
    k_positions<<<grid_for(n), kThreads, 0, st>>>(nodes, n, pos);
    if (g.E)
        k_direct<<<grid_for(g.E), kThreads, 0, st>>>(g.E, g.src, g.dst, g.lat, g.loss, g.directed, pos, n, cnt,
                                                     out_lat, out_loss);
    k_direct_check<<<grid_for((size_t)n * n), kThreads, 0, st>>>(cnt, n, P.flags);
    HIP_CHECK(hipGetLastError());
    Flags fl;
    HIP_CHECK(hipMemcpyAsync(&fl, P.flags, sizeof(Flags), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (fl.first_bad != ~0ull) {
        const size_t k = fl.first_bad;
        uint32_t cv = 0, a = 0, b = 0;
        HIP_CHECK(hipMemcpy(&cv, cnt + k, 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&a, nodes + k / n, 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&b, nodes + k % n, 4, hipMemcpyDeviceToHost));
        const std::string ia = std::to_string(node_gml_id(g, a, st)), ib = std::to_string(node_gml_id(g, b, st));
        if (cv == 0) fail(SRG_ERR_NO_EDGE, "No edge connecting node " + ia + " to " + ib);
        fail(SRG_ERR_MULTI_EDGE, "More than one edge connecting node " + ia + " to " + ib);
    }
    // get_direct_paths converts every used edge to ns with unwrap (mod.rs:240, 336)
    if (P.es.lat_overflow || P.es.max_lat == UINT64_MAX) {
        // only an error when an overflowing edge is among the outputs
        std::vector<uint64_t> lat((size_t)n * n);
        HIP_CHECK(hipMemcpy(lat.data(), out_lat, lat.size() * 8, hipMemcpyDeviceToHost));
        for (uint64_t v : lat)
            if (v == UINT64_MAX)
                fail(SRG_ERR_LATENCY_RANGE, "The resulting value is outside of the bounds [0, 18446744073709551615]");
    }
}

int guard(char* errbuf, size_t errlen, const std::function<void()>& body) {
    try {
        body();
        if (errbuf && errlen) errbuf[0] = 0;
        return SRG_OK;
    } catch (const Failure& f) {
        set_err(errbuf, errlen, f.msg);
        return f.code;
    } catch (const srg::CommError& e) {
        set_err(errbuf, errlen, std::string("collective: ") + e.what());
        return SRG_ERR_RCCL;
    } catch (const std::bad_alloc&) {
        set_err(errbuf, errlen, "out of host memory");
        return SRG_ERR_OOM;
    } catch (const std::exception& e) {
        set_err(errbuf, errlen, std::string("internal error: ") + e.what());
        return SRG_ERR_INTERNAL;
    } catch (...) {
        set_err(errbuf, errlen, "internal error");
        return SRG_ERR_INTERNAL;
    }
}

// A device call of the C ABI, after its null checks: under ctx->mu, on the context's device,
// body(st) with the caller's stream or the context's.  *ms_total (when given) is the wall time from
// here to the return, of a failed call too.  The stream is not synchronised here: every body does
// that itself on each path that queued work.
template <class F>
int device_call(srg_ctx* ctx, void* hip_stream, double* ms_total, char* errbuf, size_t errlen, F&& body) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto t0 = std::chrono::steady_clock::now();
    const int rc = guard(errbuf, errlen, [&]() {
        HIP_CHECK(hipSetDevice(ctx->device));
        body(hip_stream ? (hipStream_t)hip_stream : ctx->stream);
    });
    if (ms_total) *ms_total = ms_since(t0);
    return rc;
}

#include "stage.hip.h"
#include "events_run.hip.h"
#include "inbound_run.hip.h"
#include "outbound_run.hip.h"
#include "round_run.hip.h"
#include "sockets_in_run.hip.h"
#include "h2d_codec.hip.h"

#include "host_entry.hip.h"
}  // namespace

extern "C" {

__global__ void k_warm(uint32_t* p) {
    if (threadIdx.x == 0 && blockIdx.x == 0) p[0] = 0;
}

// srg_create's warm-up (SRG_CREATE_WARM=0 skips it, for A/B): what the first host-entry call would
// otherwise pay on the routing path -- the code object's load on the device (the first launch), each
// stream's first dispatch, the codec worker pool, the page-locked H2D rings (96 + 24 MB), the first
// copy of each kind (H2D and D2H by the runtime, D2H on the SDMA engine).  Shadow creates its context
// before parsing the GML, so this runs off the routing path.
void warm_context(srg_ctx& c) {
    ensure_pool(c);
    ensure_rings(c);
    uint32_t* d = (uint32_t*)c.b_red.get(128);
    const hipStream_t ss[4] = {c.stream, c.aux_stream, c.comm_stream, c.d2h_stream};
    for (hipStream_t s : ss) k_warm<<<1, 64, 0, s>>>(d);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(d, c.h_ring, 64, hipMemcpyHostToDevice, c.comm_stream));
    HIP_CHECK(hipMemcpyAsync(c.h_lring, d + 16, 64, hipMemcpyDeviceToHost, c.d2h_stream));
    for (hipStream_t s : ss) HIP_CHECK(hipStreamSynchronize(s));
    if (c.sdma.ok) {
        hsa_signal_t sg;
        if (hsa_signal_create(1, 0, nullptr, &sg) == HSA_STATUS_SUCCESS) {
            if (hsa_amd_memory_async_copy_on_engine(c.h_ring, c.sdma.cpu, d, c.sdma.gpu, 64, 0, nullptr, sg,
                                                    (hsa_amd_sdma_engine_id_t)c.sdma.engine, true) == HSA_STATUS_SUCCESS)
                hsa_signal_wait_scacquire(sg, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
            hsa_signal_destroy(sg);
        }
    }
}

int srg_create(srg_ctx** out, int device, char* errbuf, size_t errlen) {
    if (!out) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    *out = nullptr;
    srg_ctx* c = nullptr;
    int rc = guard(errbuf, errlen, [&]() {
        // SRG_DEBUG_CREATE: where srg_create's time goes (the cold call Shadow pays once)
        const bool dbg = srg_env::debug_create();
        auto tc = std::chrono::steady_clock::now();
        auto lap = [&](const char* what) {
            if (dbg) std::fprintf(stderr, "srg_create: %-28s %7.2f ms\n", what, ms_since(tc));
            tc = std::chrono::steady_clock::now();
        };
        const auto tcreate = std::chrono::steady_clock::now();
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        lap("hipGetDeviceCount");
        if (e != hipSuccess || count == 0)
            fail(SRG_ERR_HIP, std::string("no HIP device available (") + hipGetErrorString(e) +
                                  "); the routing builder has no CPU fallback");
        if (device < 0 || device >= count) fail(SRG_ERR_ARG, "device index out of range");
        c = new srg_ctx();
        c->device = device;
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipFree(nullptr));  // (the device's runtime context, if this process has none yet)
        lap("hipSetDevice");
        // the first stream is where the runtime initialises the device for this process (80-145 ms
        // on the boxes, the next streams ~5 ms each; creating the four from four threads at once took
        // as long, profiles/r05/create/): counted as the runtime's part
        HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        lap("stream main");
        c->ms_create_runtime = ms_since(tcreate);
        const auto tlib = std::chrono::steady_clock::now();
        // the FW lookahead chain (pivot close, row/col panels) is latency-critical: its workgroups
        // should be dispatched ahead of the bulk phase-3 tiles
        int prio_lo = 0, prio_hi = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        HIP_CHECK(hipStreamCreateWithPriority(&c->aux_stream, hipStreamNonBlocking, prio_hi));
        HIP_CHECK(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
        HIP_CHECK(hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking));
        lap("streams aux, comm, d2h");
        HIP_CHECK(hipHostMalloc((void**)&c->hbox, 64 * kMailSlots, hipHostMallocDefault));
        lap("mailbox");
        c->sdma.init(device);  // SDMA engine for the host entry's early D2H (else hipMemcpyAsync)
        lap("sdma agents");
        // the late-loss H2D and WL build share the D2H stream (idle until FW ends): a fifth
        // stream would share a hardware queue (GPU_MAX_HW_QUEUES = 4) with the main stream and
        // serialise the W build and FW behind the loss DMAs (measured: build 1.0 -> 3.6 ms)
        c->loss_stream = c->d2h_stream;
        for (Event* e : {&c->ev_a, &c->ev_b, &c->ev_c, &c->ev_d, &c->ev_e, &c->ev_ledges, &c->ev_wlate, &c->ev_fwreset,
                         &c->ev_dst})
            e->create();
        int wv = 0;
        if (hipDeviceGetAttribute(&wv, hipDeviceAttributeCanUseStreamWaitValue, device) == hipSuccess && wv) {
            for (uint32_t*& p : c->sig) HIP_CHECK(hipExtMallocWithFlags((void**)&p, 8, hipMallocSignalMemory));
            HIP_CHECK(hipStreamWriteValue32(c->stream, c->sig[0], 0, 0));
            HIP_CHECK(hipStreamWriteValue32(c->stream, c->sig[1], 0, 0));
            HIP_CHECK(hipStreamSynchronize(c->stream));
        }
        lap("events, signals");
        if (!srg_env::create_warm_off()) {
            warm_context(*c);
            lap("warm-up (module, rings, copies)");
        }
        c->ms_create_lib = ms_since(tlib);
        std::lock_guard<std::mutex> lk(g_dev_mu);
        ++g_dev_ctx[device];
    });
    if (rc != SRG_OK) {
        delete c;
        return rc;
    }
    *out = c;
    return SRG_OK;
}

int srg_set_option(srg_ctx* ctx, int option, double value) {
    if (!ctx) return SRG_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    switch (option) {
        case SRG_OPT_PROFILING:
            ctx->profiling = value != 0.0;
            return SRG_OK;
        case SRG_OPT_SPARSE_THRESHOLD:
            if (!(value >= 0.0)) return SRG_ERR_ARG;
            ctx->sparse_threshold = value;
            return SRG_OK;
        case SRG_OPT_GATHER_OUTPUT:
            ctx->gather_output = value != 0.0;
            return SRG_OK;
        case SRG_OPT_SIMULATE_RANK: {
            // value = nranks * 1000 + rank; 0 detaches
            const int v = (int)value;
            delete ctx->comm;
            ctx->comm = nullptr;
            ctx->sim_edges = nullptr;
            if (v > 0) {
                const int nr = v / 1000, rk = v % 1000;
                if (nr < 1 || rk >= nr) return SRG_ERR_ARG;
                ctx->comm = srg::null_create(nr, rk);
            }
            return SRG_OK;
        }
        case SRG_OPT_FW_TILE:
            if (value != 0 && value != 64 && value != 128) return SRG_ERR_ARG;
            ctx->fw_tile = (int)value;
            return SRG_OK;
        case SRG_OPT_SPARSE_LOCALITY:
            ctx->sparse_locality = value != 0.0;
            return SRG_OK;
        case SRG_OPT_SPARSE_DELTA_DIV:
            if (!(value >= 0.0 && value <= 1e6)) return SRG_ERR_ARG;
            ctx->sparse_delta_div = (int)value;
            return SRG_OK;
        case SRG_OPT_SPARSE_GLOBAL_BITMAPS:
            ctx->sparse_global_bitmaps = value != 0.0;
            return SRG_OK;
        case SRG_OPT_FW_SYMMETRIC:
            ctx->fw_symmetric = value != 0.0;
            return SRG_OK;
        case SRG_OPT_LATE_LOSS:
            if (value != 0 && value != 1) return SRG_ERR_ARG;
            ctx->late_loss = (int)value;
            return SRG_OK;
        case SRG_OPT_EDGE_SHARD:
            if (value != 0 && value != 1 && value != -1) return SRG_ERR_ARG;
            ctx->edge_shard = (int)value;
            return SRG_OK;
        case SRG_OPT_H2D_CODEC:
            if (value != 0 && value != 1) return SRG_ERR_ARG;
            ctx->h2d_codec = (int)value;
            return SRG_OK;
        case SRG_OPT_SCAN_GROUPS:
            if (value < 0 || value > 1024) return SRG_ERR_ARG;
            ctx->scan_groups = (int)value;
            return SRG_OK;
        case SRG_OPT_LOSS_CHUNKS:
            if (value < 0 || value > 1024) return SRG_ERR_ARG;
            ctx->loss_chunks = (int)value;
            return SRG_OK;
        case SRG_OPT_D2H_MODE:
            if (value != 0 && value != 1) return SRG_ERR_ARG;
            ctx->d2h_mode = (int)value;
            return SRG_OK;
        case SRG_OPT_FW_LINE_SPLIT:
            if (value != 0 && value != 1 && value != 2 && value != 4) return SRG_ERR_ARG;
            ctx->fw_line_split = (int)value;
            return SRG_OK;
        case SRG_OPT_FW_STEP:
            // (1, the fused one-launch-per-pivot FW, was removed in round 5: DESIGN.md §7)
            if (value != 0 && value != 2 && value != -1) return SRG_ERR_ARG;
            ctx->fw_step = (int)value;
            return SRG_OK;
        case SRG_OPT_FW_OVERLAP:
            if (value != 0 && value != 1) return SRG_ERR_ARG;
            ctx->fw_overlap = (int)value;
            return SRG_OK;
        case SRG_OPT_TEST_FAULT:
            // test hooks exist only in the test build (libshadow_routing_testhooks.so, -DSRG_TEST_HOOKS);
            // the product library accepts 0 (off) and refuses the rest
            if (value != 0 && value != 1 && value != 2) return SRG_ERR_ARG;
#ifndef SRG_TEST_HOOKS
            if (value != 0) return SRG_ERR_ARG;
#endif
            ctx->test_fault = (int)value;
            return SRG_OK;
        case SRG_OPT_FW_XCD_ORDER:
            if (value != 0 && value != 1) return SRG_ERR_ARG;
            ctx->fw_xcd_order = (int)value;
            return SRG_OK;
        case SRG_OPT_SCAN_MIRROR:
            if (value != 0 && value != 1) return SRG_ERR_ARG;
            ctx->scan_mirror = (int)value;
            return SRG_OK;
        case SRG_OPT_SCAN_MIRROR_CAP:
            if (!(value >= 0 && value <= 1073741824.0)) return SRG_ERR_ARG;
            ctx->scan_mirror_cap = (int)value;
            return SRG_OK;
        case SRG_OPT_ROUTE_TREE_ROWS:
            if (!(value >= 0 && value <= 1073741824.0)) return SRG_ERR_ARG;
            ctx->route_tree_rows = (int)value;
            return SRG_OK;
        case SRG_OPT_TABLE_POOL_BYTES: {
            if (!(value >= 0.0 && value <= 1e15)) return SRG_ERR_ARG;
            std::lock_guard<std::mutex> pl(ctx->tpool->mu);
            ctx->tpool->limit = (size_t)value;
            ctx->tpool->max_idle = 0;  // an explicit byte cap replaces the one-pair default
            ctx->tpool->trim_locked(ctx->tpool->limit);
            return SRG_OK;
        }
        case SRG_OPT_ALGORITHM:
            if (value != SRG_ALGO_AUTO && value != SRG_ALGO_DENSE && value != SRG_ALGO_SPARSE) return SRG_ERR_ARG;
            ctx->algorithm = (int)value;
            return SRG_OK;
        default:
            return SRG_ERR_ARG;
    }
}

int srg_get_option(srg_ctx* ctx, int option, double* value) {
    if (!ctx || !value) return SRG_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    switch (option) {
        case SRG_OPT_PROFILING: *value = ctx->profiling; break;
        case SRG_OPT_SPARSE_THRESHOLD: *value = ctx->sparse_threshold; break;
        case SRG_OPT_GATHER_OUTPUT: *value = ctx->gather_output; break;
        case SRG_OPT_ALGORITHM: *value = ctx->algorithm; break;
        case SRG_OPT_SPARSE_LOCALITY: *value = ctx->sparse_locality; break;
        case SRG_OPT_FW_TILE: *value = ctx->fw_tile; break;
        case SRG_OPT_SPARSE_DELTA_DIV: *value = ctx->sparse_delta_div; break;
        case SRG_OPT_SPARSE_GLOBAL_BITMAPS: *value = ctx->sparse_global_bitmaps; break;
        case SRG_OPT_FW_SYMMETRIC: *value = ctx->fw_symmetric; break;
        case SRG_OPT_D2H_MODE: *value = ctx->d2h_mode; break;
        case SRG_OPT_LOSS_CHUNKS: *value = ctx->loss_chunks; break;
        case SRG_OPT_SCAN_GROUPS: *value = ctx->scan_groups; break;
        case SRG_OPT_H2D_CODEC: *value = ctx->h2d_codec; break;
        case SRG_OPT_EDGE_SHARD: *value = ctx->edge_shard; break;
        case SRG_OPT_LATE_LOSS: *value = ctx->late_loss; break;
        case SRG_OPT_FW_LINE_SPLIT: *value = ctx->fw_line_split; break;
        case SRG_OPT_FW_STEP: *value = ctx->fw_step; break;
        case SRG_OPT_FW_OVERLAP: *value = ctx->fw_overlap; break;
        case SRG_OPT_TEST_FAULT: *value = ctx->test_fault; break;
        case SRG_OPT_TABLE_POOL_BYTES: {
            std::lock_guard<std::mutex> pl(ctx->tpool->mu);
            *value = (double)ctx->tpool->limit;
            break;
        }
        case SRG_OPT_TABLE_POOL_IDLE_BYTES: {
            std::lock_guard<std::mutex> pl(ctx->tpool->mu);
            *value = (double)ctx->tpool->idle_bytes;
            break;
        }
        case SRG_OPT_CREATE_MS_RUNTIME: *value = ctx->ms_create_runtime; break;
        case SRG_OPT_FW_XCD_ORDER: *value = ctx->fw_xcd_order; break;
        case SRG_OPT_CREATE_MS_LIBRARY: *value = ctx->ms_create_lib; break;
        case SRG_OPT_SCAN_MIRROR: *value = ctx->scan_mirror; break;
        case SRG_OPT_SCAN_MIRRORED: *value = ctx->scan_mirrored; break;
        case SRG_OPT_SCAN_MIRROR_CAP: *value = ctx->scan_mirror_cap; break;
        case SRG_OPT_LOSS_KIND: *value = ctx->loss_kind; break;
        case SRG_OPT_ROUTE_TREE_ROWS: *value = ctx->route_tree_rows; break;
        default: return SRG_ERR_ARG;
    }
    return SRG_OK;
}

void srg_destroy(srg_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    {
        std::lock_guard<std::mutex> lk(g_dev_mu);
        --g_dev_ctx[ctx->device];
    }
    delete ctx;
}

int srg_internal_compute_table(srg_ctx* ctx, const srg_edge_list* graph, const uint32_t* nodes, uint32_t num_nodes,
                               int shortest, uint64_t* out_lat, uint32_t* out_key, uint64_t* out_diag, float* out_loss,
                               uint64_t* unit_ns, srg_table* tab_lat, srg_table* tab_loss, srg_stats* stats,
                               char* errbuf, size_t errlen) {
    srg_stats local{};
    srg_stats* st = stats ? stats : &local;
    srg_table* tabs[2] = {tab_lat, tab_loss};
    const int rc = host_entry(ctx, graph, nodes, num_nodes, out_key ? nullptr : out_lat, out_loss, st, errbuf, errlen,
                              !shortest, out_key, out_diag, tabs);
    if (unit_ns) *unit_ns = out_key && st->latency_unit_ns ? st->latency_unit_ns : 1;
    return rc;
}

uint32_t srg_internal_scan_group_cut_tri(uint32_t q, uint32_t ng, uint32_t nblocks) {
    return scan_group_cut_tri(q, ng, nblocks);
}

void srg_internal_loss_limits(uint32_t out[4]) {
    out[0] = LM_T;
    out[1] = LM_E;
    out[2] = MIRROR_STEPS;
    out[3] = LOSS_ROWS_MAX_V;
}

srg_table* srg_internal_table_get(srg_ctx* ctx, size_t bytes, void** host) {
    if (!ctx || !host) return nullptr;
    *host = nullptr;
    constexpr size_t HP = (size_t)2 << 20;
    const size_t cap = (std::max<size_t>(bytes, 1) + HP - 1) / HP * HP;
    TablePool& P = *ctx->tpool;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        size_t best = SIZE_MAX;
        for (size_t i = 0; i < P.idle.size(); ++i)  // the smallest idle table that holds it (and < 2x)
            if (P.idle[i]->cap >= cap && P.idle[i]->cap <= 2 * cap && (best == SIZE_MAX || P.idle[i]->cap < P.idle[best]->cap))
                best = i;
        if (best != SIZE_MAX) {
            srg_table* t = P.idle[best];
            P.idle.erase(P.idle.begin() + best);
            P.idle_bytes -= t->cap;
            *host = t->p;
            return t;
        }
    }
    // a fresh mapping, 2 MB aligned; its pages are faulted in and locked by the first build into
    // it (host_entry's registration thread, beside the H2D and FW)
    void* m = mmap(nullptr, cap + HP, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (m == MAP_FAILED) return nullptr;
    const uintptr_t a = ((uintptr_t)m + HP - 1) / HP * HP;
    if (a > (uintptr_t)m) munmap(m, a - (uintptr_t)m);
    if ((uintptr_t)m + cap + HP > a + cap) munmap((void*)(a + cap), (uintptr_t)m + cap + HP - (a + cap));
    srg_table* t = new (std::nothrow) srg_table();
    if (!t) {
        munmap((void*)a, cap);
        return nullptr;
    }
    t->pool = ctx->tpool;
    t->p = (void*)a;
    t->cap = cap;
    *host = t->p;
    return t;
}

void srg_internal_table_put(srg_table* t) {
    if (!t) return;
    std::shared_ptr<TablePool> P = t->pool;  // (keeps the pool alive past this table)
    std::lock_guard<std::mutex> lk(P->mu);
    if (P->open && t->cap <= P->limit) {
        P->idle.push_back(t);
        P->idle_bytes += t->cap;
        P->trim_locked(P->limit);
    } else {
        TablePool::destroy(t);
    }
}

int srg_compute_shortest_paths(srg_ctx* ctx, const srg_edge_list* graph, const uint32_t* nodes, uint32_t num_nodes,
                               uint64_t* out_latency_ns, float* out_packet_loss, srg_stats* stats, char* errbuf,
                               size_t errlen) {
    return host_entry(ctx, graph, nodes, num_nodes, out_latency_ns, out_packet_loss, stats, errbuf, errlen, false);
}

int srg_get_direct_paths(srg_ctx* ctx, const srg_edge_list* graph, const uint32_t* nodes, uint32_t num_nodes,
                         uint64_t* out_latency_ns, float* out_packet_loss, srg_stats* stats, char* errbuf,
                         size_t errlen) {
    return host_entry(ctx, graph, nodes, num_nodes, out_latency_ns, out_packet_loss, stats, errbuf, errlen, true);
}

int srg_compute_shortest_paths_device(srg_ctx* ctx, const srg_edge_list* g, const uint32_t* nodes_dev,
                                      uint32_t num_nodes, uint64_t* out_lat_dev, float* out_loss_dev,
                                      void* hip_stream, srg_stats* stats, char* errbuf, size_t errlen) {
    if (!ctx || !g || (num_nodes && (!nodes_dev || !out_lat_dev || !out_loss_dev))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return guard(errbuf, errlen, [&]() {
        auto t0 = std::chrono::steady_clock::now();
        if (stats) std::memset(stats, 0, sizeof(*stats));
        HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
        DevGraph dg{g->num_vertices, (int)g->directed, g->num_edges, g->src, g->dst, g->latency_ns,
                    g->packet_loss, g->node_ids, nullptr};
        compute_device(*ctx, dg, nodes_dev, num_nodes, out_lat_dev, out_loss_dev, st, stats);
        HIP_CHECK(hipStreamSynchronize(st));
        if (stats) stats->ms_total = ms_since(t0);
    });
}

int srg_comm_unique_id(unsigned char id[SRG_UNIQUE_ID_BYTES], char* errbuf, size_t errlen) {
    if (!id) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return guard(errbuf, errlen, [&]() {
        const std::string e = srg::rccl_unique_id(id);
        if (!e.empty()) fail(SRG_ERR_RCCL, e);
    });
}

int srg_comm_init(srg_ctx* ctx, int nranks, int rank, const unsigned char id[SRG_UNIQUE_ID_BYTES], char* errbuf,
                  size_t errlen) {
    if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) {
        set_err(errbuf, errlen, "bad argument");
        return SRG_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return guard(errbuf, errlen, [&]() {
        srg::Comm* cm = nullptr;
        const std::string e = srg::rccl_create(nranks, rank, id, ctx->device, &cm);
        if (!e.empty()) fail(SRG_ERR_RCCL, e);
        delete ctx->comm;
        ctx->comm = cm;
    });
}

int srg_local_group_create(int nranks, srg_local_group** out) {
    if (!out || nranks < 1) return SRG_ERR_ARG;
    *out = reinterpret_cast<srg_local_group*>(srg::local_group_create(nranks));
    return SRG_OK;
}

void srg_local_group_release(srg_local_group* g) { srg::local_group_release(reinterpret_cast<srg::LocalGroup*>(g)); }

int srg_comm_init_local(srg_ctx* ctx, srg_local_group* g, int rank, char* errbuf, size_t errlen) {
    if (!ctx || !g) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return guard(errbuf, errlen, [&]() {
        srg::Comm* cm = nullptr;
        const std::string e = srg::local_create(reinterpret_cast<srg::LocalGroup*>(g), rank, ctx->device, &cm);
        if (!e.empty()) fail(SRG_ERR_ARG, e);
        delete ctx->comm;
        ctx->comm = cm;
    });
}

int srg_comm_size(srg_ctx* ctx, int* nranks, int* rank) {
    if (!ctx || !nranks || !rank) return SRG_ERR_ARG;
    *nranks = ctx->comm ? ctx->comm->nranks : 1;
    *rank = ctx->comm ? ctx->comm->rank : 0;
    return SRG_OK;
}

// ---- one call site, several GPUs of this process (srg_multi) ----------------------------------
// Shadow builds its RoutingInfo once, in one process (sim_config.rs:137-141 -> manager.rs:301-324).
// srg_multi drives N GPUs from that one call: one context per device attached to an in-process
// group (collectives = pull kernels over xGMI), one worker thread per rank, and the caller's two
// host arrays page-locked once (portable) while the ranks ship their edges and run FW.  Every rank
// runs the SPMD build with the output exchange off and ships its own sources' rows over its own
// PCIe link straight into the caller's arrays, so the call returns with the whole table there.
struct srg_multi {
    std::vector<srg_ctx*> ranks;
    std::vector<int> devices;
    srg::LocalGroup* group = nullptr;
    std::mutex mu;
    ~srg_multi() {
        for (srg_ctx* c : ranks) srg_destroy(c);
        if (group) srg::local_group_release(group);
    }
};

int srg_multi_create(srg_multi** out, const int* devices, int num_devices, char* errbuf, size_t errlen) {
    if (!out || !devices || num_devices < 1) {
        set_err(errbuf, errlen, "bad argument");
        return SRG_ERR_ARG;
    }
    *out = nullptr;
    auto* m = new srg_multi();
    m->devices.assign(devices, devices + num_devices);
    m->group = srg::local_group_create(num_devices);
    for (int r = 0; r < num_devices; ++r) {
        srg_ctx* c = nullptr;
        int rc = srg_create(&c, devices[r], errbuf, errlen);
        if (rc == SRG_OK) {
            m->ranks.push_back(c);
            if (num_devices > 1) rc = srg_comm_init_local(c, reinterpret_cast<srg_local_group*>(m->group), r, errbuf, errlen);
        }
        if (rc != SRG_OK) {
            delete m;
            return rc;
        }
    }
    *out = m;
    return SRG_OK;
}

void srg_multi_destroy(srg_multi* m) { delete m; }

int srg_multi_size(const srg_multi* m) { return m ? (int)m->ranks.size() : 0; }

int srg_multi_set_option(srg_multi* m, int option, double value) {
    if (!m) return SRG_ERR_ARG;
    if (option == SRG_OPT_GATHER_OUTPUT || option == SRG_OPT_SIMULATE_RANK) return SRG_ERR_ARG;  // fixed by srg_multi
    // all or nothing: the ranks must keep one option set (a split FW tile or line split would run
    // mismatched multi-rank schedules), so a rank that rejects the value rolls the others back
    std::vector<double> old(m->ranks.size(), 0.0);
    for (size_t r = 0; r < m->ranks.size(); ++r)
        if (srg_get_option(m->ranks[r], option, &old[r]) != SRG_OK) return SRG_ERR_ARG;
    for (size_t r = 0; r < m->ranks.size(); ++r) {
        const int rc = srg_set_option(m->ranks[r], option, value);
        if (rc != SRG_OK) {
            for (size_t q = 0; q < r; ++q) (void)srg_set_option(m->ranks[q], option, old[q]);
            return rc;
        }
    }
    return SRG_OK;
}

int srg_multi_compute_shortest_paths(srg_multi* m, const srg_edge_list* graph, const uint32_t* nodes,
                                     uint32_t num_nodes, uint64_t* out_latency_ns, float* out_packet_loss,
                                     srg_stats* stats, char* errbuf, size_t errlen) {
    if (!m || !graph || (num_nodes && (!nodes || !out_latency_ns || !out_packet_loss))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(m->mu);
    const int G = (int)m->ranks.size();
    if (G == 1) return srg_compute_shortest_paths(m->ranks[0], graph, nodes, num_nodes, out_latency_ns, out_packet_loss,
                                                  stats, errbuf, errlen);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t nn = (size_t)num_nodes * num_nodes;
    // one registration of the caller's arrays for every rank, beside the ranks' H2D and FW
    struct Reg {
        std::mutex mu;
        std::thread th;
        bool done = false, ok = false;
        double ms = 0;
        void* p[2] = {nullptr, nullptr};
        size_t b[2] = {0, 0};
        bool wait() {
            std::lock_guard<std::mutex> l(mu);
            if (!done) {
                if (th.joinable()) th.join();
                done = true;
            }
            return ok;
        }
    } reg;
    reg.p[0] = out_latency_ns;
    reg.b[0] = nn * 8;
    reg.p[1] = out_packet_loss;
    reg.b[1] = nn * 4;
    const bool big = nn * 12 >= ((size_t)64 << 20);
    if (big) {
        const int dev0 = m->devices[0];
        reg.th = std::thread([&reg, dev0]() {
            const auto ts = std::chrono::steady_clock::now();
            if (hipSetDevice(dev0) != hipSuccess) return;
            const unsigned fl = hipHostRegisterPortable | hipHostRegisterMapped;
            advise_huge(reg.p[0], reg.b[0]);
            advise_huge(reg.p[1], reg.b[1]);
            if (hipHostRegister(reg.p[0], reg.b[0], fl) != hipSuccess) return;
            if (hipHostRegister(reg.p[1], reg.b[1], fl) != hipSuccess) {
                (void)hipHostUnregister(reg.p[0]);
                return;
            }
            reg.ms = ms_since(ts);
            reg.ok = true;
        });
    }
    std::vector<int> rc(G, SRG_OK);
    std::vector<std::string> msg(G);
    std::vector<srg_stats> st(G);
    std::vector<std::thread> th;
    for (int r = 0; r < G; ++r) {
        srg_ctx* c = m->ranks[r];
        c->gather_output = false;
        if (big)
            c->ext_reg = [&reg](void** views, double* ms) {
                if (!reg.wait()) return false;
                for (int i = 0; i < 2; ++i)
                    if (hipHostGetDevicePointer(&views[i], reg.p[i], 0) != hipSuccess) views[i] = nullptr;
                *ms = reg.ms;
                return true;
            };
        th.emplace_back([&, r, c]() {
            char eb[1024];
            rc[r] = srg_compute_shortest_paths(c, graph, nodes, num_nodes, out_latency_ns, out_packet_loss, &st[r], eb,
                                               sizeof(eb));
            msg[r] = eb;
            if (rc[r] != SRG_OK) srg::local_group_abort(m->group);  // release peers waiting in a collective
        });
    }
    for (auto& t : th) t.join();
    for (srg_ctx* c : m->ranks) c->ext_reg = nullptr;
    srg::local_group_reset(m->group);
    if (big && reg.wait()) {  // every rank's copies into the arrays are complete (their sinks finished)
        (void)hipHostUnregister(reg.p[0]);
        (void)hipHostUnregister(reg.p[1]);
    }
    // the first rank that failed for its own reason (the others report the abort)
    int first = -1;
    for (int r = 0; r < G && first < 0; ++r)
        if (rc[r] != SRG_OK && rc[r] != SRG_ERR_RCCL) first = r;
    for (int r = 0; r < G && first < 0; ++r)
        if (rc[r] != SRG_OK) first = r;
    if (first >= 0) {
        set_err(errbuf, errlen, msg[first]);
        return rc[first];
    }
    if (stats) {
        // wall times: the slowest rank; counts: summed; minimum latency: over every rank's rows
        *stats = st[0];
        stats->local_sources = 0;
        stats->d2h_overlapped_bytes = 0;
        stats->prof_launches = 0;
        stats->prof_kernel_ms = 0;
        stats->prof_relaxations = 0;
        stats->relaxations = 0;
        stats->multi_pred_pairs = 0;
        for (const srg_stats& x : st) {
            for (double srg_stats::*f : {&srg_stats::ms_h2d, &srg_stats::ms_build, &srg_stats::ms_fw, &srg_stats::ms_scan,
                                          &srg_stats::ms_loss, &srg_stats::ms_extract, &srg_stats::ms_d2h,
                                          &srg_stats::ms_exchange, &srg_stats::ms_host_register})
                stats->*f = std::max(stats->*f, x.*f);
            stats->loss_rounds = std::max(stats->loss_rounds, x.loss_rounds);
            stats->local_sources += x.local_sources;
            stats->d2h_overlapped_bytes += x.d2h_overlapped_bytes;
            stats->prof_launches += x.prof_launches;
            stats->prof_kernel_ms += x.prof_kernel_ms;
            stats->prof_relaxations += x.prof_relaxations;
            stats->relaxations += x.relaxations;
            stats->multi_pred_pairs += x.multi_pred_pairs;
            stats->min_latency_ns = std::min(stats->min_latency_ns, x.min_latency_ns);
        }
        stats->rank = 0;
        stats->nranks = G;
        stats->ms_total = ms_since(t0);
    }
    if (errbuf && errlen) errbuf[0] = 0;
    return SRG_OK;
}

int srg_multi_get_direct_paths(srg_multi* m, const srg_edge_list* graph, const uint32_t* nodes, uint32_t num_nodes,
                               uint64_t* out_latency_ns, float* out_packet_loss, srg_stats* stats, char* errbuf,
                               size_t errlen) {
    if (!m) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(m->mu);
    // rank 0 alone: its context must not wait for peers in a collective
    srg_ctx* c = m->ranks[0];
    srg::Comm* cm = nullptr;
    {
        std::lock_guard<std::mutex> l2(c->mu);
        std::swap(cm, c->comm);
    }
    const int rc = srg_get_direct_paths(c, graph, nodes, num_nodes, out_latency_ns, out_packet_loss, stats, errbuf, errlen);
    {
        std::lock_guard<std::mutex> l2(c->mu);
        std::swap(cm, c->comm);
    }
    return rc;
}

int srg_order_packet_events_device(srg_ctx* ctx, const srg_event_batch* b, const uint64_t* table, uint32_t table_n,
                                   uint64_t* out_deliver, uint32_t* out_order, uint64_t* out_host_off,
                                   void* hip_stream, srg_event_result* res, char* errbuf, size_t errlen) {
    if (!ctx || !b || !out_host_off ||
        (b->num_events && (!table || !out_deliver || !out_order || !b->src_node || !b->dst_node || !b->src_host ||
                           !b->dst_host || !b->send_time_ns || !b->src_event_id))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        EvIn in{b->num_events, b->src_node, b->dst_node, b->src_host, b->dst_host, b->send_time_ns,
                b->src_event_id, table, table_n, b->num_hosts, b->round_end_ns};
        event_batch_device<false>(*ctx, in, EvSendIn{}, nullptr, out_deliver, out_order, out_host_off, nullptr, st, res);
    });
}

int srg_send_packets_device(srg_ctx* ctx, const srg_send_batch* sb, const srg_path_table_dev* t, uint8_t* out_status,
                            uint64_t* out_deliver, uint32_t* out_order, uint64_t* out_host_off, uint64_t* packet_counts,
                            void* hip_stream, srg_send_result* res, char* errbuf, size_t errlen) {
    if (!ctx || !sb || !t || !out_host_off) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    const srg_event_batch* b = &sb->ev;
    if (b->num_events && (!out_status || !out_deliver || !out_order || !b->src_node || !b->dst_node || !b->src_host ||
                          !b->dst_host || !b->send_time_ns || !b->src_event_id)) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    if (!t->latency_ns == !t->latency_key) {
        set_err(errbuf, errlen, "path table: exactly one of latency_ns and latency_key must be given");
        return SRG_ERR_ARG;
    }
    if (t->latency_key && (!t->diag_ns || t->unit_ns < 1)) {
        set_err(errbuf, errlen, "path table: latency_key needs diag_ns and unit_ns >= 1");
        return SRG_ERR_ARG;
    }
    if (t->packet_loss && b->num_events && (!sb->chance || !sb->payload_size)) {
        set_err(errbuf, errlen, "send batch: chance and payload_size are required with a packet_loss table");
        return SRG_ERR_ARG;
    }
    return device_call(ctx, hip_stream, res ? &res->ev.ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        EvIn in{b->num_events, b->src_node, b->dst_node, b->src_host, b->dst_host, b->send_time_ns,
                b->src_event_id, nullptr, t->n, b->num_hosts, b->round_end_ns};
        EvSendIn sx{{t->latency_ns, t->latency_key, t->diag_ns, t->unit_ns, t->n}, t->packet_loss, sb->chance,
                    sb->payload_size, sb->bootstrap_end_ns};
        if (res) res->num_sent = res->num_dropped = 0;
        const uint64_t sent = event_batch_device<true>(*ctx, in, sx, out_status, out_deliver, out_order, out_host_off,
                                                       (unsigned long long*)packet_counts, st, res ? &res->ev : nullptr);
        if (res) {
            res->num_sent = sent;
            res->num_dropped = b->num_events - sent;
        }
    });
}

int srg_trace_routes_device(srg_ctx* ctx, const srg_edge_list* g, const srg_path_table_dev* t, const uint32_t* src,
                            const uint32_t* dst, uint64_t num_pairs, uint64_t hop_capacity, uint64_t* out_off,
                            uint32_t* out_edge, uint32_t* out_vertex, void* hip_stream, srg_route_result* res,
                            char* errbuf, size_t errlen) {
    if (!ctx || !g || !t || (num_pairs && (!src || !dst)) || (hop_capacity && (!out_off || !out_edge))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        trace_routes_device(*ctx, g, t, src, dst, num_pairs, hop_capacity, out_off, out_edge, out_vertex, st, res);
    });
}

int srg_link_loads_device(srg_ctx* ctx, const srg_edge_list* g, const srg_path_table_dev* t, const uint64_t* counts,
                          uint64_t* edge_packets, void* hip_stream, srg_route_result* res, char* errbuf,
                          size_t errlen) {
    if (!ctx || !g || !t || (g->num_vertices && !counts) || (g->num_edges && !edge_packets)) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        link_loads_device(*ctx, g, t, counts, edge_packets, st, res);
    });
}

int srg_route_trees_device(srg_ctx* ctx, const srg_edge_list* g, const srg_path_table_dev* t, const uint32_t* sources,
                           uint32_t num_sources, uint32_t* out_pred_edge, uint32_t* out_pred_vertex, uint32_t* out_hops,
                           uint32_t* out_first_edge, void* hip_stream, srg_route_result* res, char* errbuf,
                           size_t errlen) {
    if (!ctx || !g || !t || (num_sources && !out_pred_edge)) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        route_trees_device(*ctx, g, t, sources, num_sources, out_pred_edge, out_pred_vertex, out_hops, out_first_edge,
                           st, res);
    });
}

int srg_link_loads_trees_device(srg_ctx* ctx, const srg_edge_list* g, const srg_path_table_dev* t,
                                const uint64_t* counts, uint64_t* edge_packets, void* hip_stream, srg_route_result* res,
                                char* errbuf, size_t errlen) {
    if (!ctx || !g || !t || (g->num_vertices && !counts) || (g->num_edges && !edge_packets)) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        link_loads_trees_device(*ctx, g, t, counts, edge_packets, st, res);
    });
}

int srg_next_window(uint64_t min_next_event_ns, uint64_t runahead_ns, uint64_t end_time_ns, uint64_t* window_start_ns,
                    uint64_t* window_end_ns) {
    if (!runahead_ns || !window_start_ns || !window_end_ns) return -SRG_ERR_ARG;  // assert_ne!(runahead, ZERO)
    const uint64_t start = min_next_event_ns;
    uint64_t end = start > UINT64_MAX - runahead_ns ? UINT64_MAX : start + runahead_ns;  // checked_add, else MAX
    end = end < end_time_ns ? end : end_time_ns;
    if (!(start < end)) return 0;
    *window_start_ns = start;
    *window_end_ns = end;
    return 1;
}

const char* srg_version(void) { return "shadow_amd routing 0.3 (gfx950, dense FW u32/u64 + tight-DAG loss, RCCL row-block FW, sparse BF, event batches)"; }

}  // extern "C"
