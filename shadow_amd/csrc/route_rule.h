// route_rule.h — the rule that reads a route back from a finished shortest-path table, shared by
// the walk kernels (routes.hip.h) and a CPU unit test (tests/cpp/route_rule_check.cpp, built with
// g++ -ffp-contract=off).
//
// A Dijkstra label is label(u) + edge (PathProperties::add, mod.rs:321-331): the latency adds, the
// loss is the f32 left fold 1 - (1 - L) * (1 - p), each operation rounded.  So for every s != t a
// finished table holds a vertex u and an in-edge e = (u, t) with
//     D[s][u] + lat(e) == D[s][t]   and   bits(fold(L[s][u], loss(e))) == bits(L[s][t]),
// where the source's own label is (0, +0.0f) (PathProperties::default(), mod.rs:297), NOT the
// table's diagonal: the diagonal holds the raw self-loop weight (mod.rs:210-217).  Latencies are
// >= 1, so D[s][.] falls strictly along the walk back from t and the walk ends at s.
//
// Tie rule (the contract that makes the route unique):
//   in-edges of cur = the edges (u, cur), u != cur; on an undirected graph an edge stored as
//   (cur, u) counts too; self-loops are never candidates; among the in-edges that satisfy both
//   equalities the one with the smallest edge index (position in srg_edge_list) is the route's.
// The choice is a min over the matching indices, so it cannot depend on the order in which any
// adjacency list was filled.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "send_rule.h"  // srg::PathLatency, srg::path_latency: the table fetch in either form

#if defined(__HIPCC__)
#define SRG_ROUTE_HD __host__ __device__
#else
#define SRG_ROUTE_HD
#endif

namespace srg {

constexpr uint32_t ROUTE_NO_EDGE = 0xFFFFFFFFu;  // "no candidate": larger than every edge index

SRG_ROUTE_HD inline uint32_t f32_bits(float f) {
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    return b;
}

// PathProperties::add on the loss with an edge's raw loss p: fold_loss(path_loss, 1 - p) of
// kernels.hip.h, i.e. its three roundings (1 - path_loss, the product, 1 - product) behind the
// rounded 1 - p its callers hand it.  No FMA: the device side names every rounding, the host side
// is compiled with -ffp-contract=off.
SRG_ROUTE_HD inline float fold(float path_loss, float edge_loss) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float b = __fsub_rn(1.0f, edge_loss);
    const float x = __fsub_rn(1.0f, path_loss);
    return __fsub_rn(1.0f, __fmul_rn(x, b));
#else
    const float b = 1.0f - edge_loss;
    const float x = 1.0f - path_loss;
    const float y = x * b;
    return 1.0f - y;
#endif
}

// the label of u in the row of source s
struct RouteLabel {
    uint64_t lat;
    float loss;
};

// The source's label is (0, +0.0f) whatever the diagonal holds; every other vertex's is its table
// entry (loss: the row-major n x n table the latencies come with).
SRG_ROUTE_HD inline RouteLabel route_label(const PathLatency& t, const float* loss, uint32_t s, uint32_t u) {
    if (u == s) return RouteLabel{0, 0.0f};
    return RouteLabel{path_latency(t, s, u), loss[(size_t)s * t.n + u]};
}

// Is edge (src, dst) an in-edge of cur?  Sets u to its other endpoint.
SRG_ROUTE_HD inline bool route_in_edge(uint32_t src, uint32_t dst, bool directed, uint32_t cur, uint32_t* u) {
    if (src == dst) return false;  // a self-loop never lies on a route between two vertices
    if (dst == cur) {
        *u = src;
        return true;
    }
    if (!directed && src == cur) {
        *u = dst;
        return true;
    }
    return false;
}

// The predecessor predicate: does the label `lu` of u plus an edge (lat, loss) give exactly the
// entry (d_cur, bits l_cur) of cur?  The latency test subtracts (d_cur >= lat first), so it cannot
// wrap where lu.lat + lat would.
SRG_ROUTE_HD inline bool route_explains(uint64_t d_cur, uint32_t l_cur_bits, const RouteLabel& lu, uint64_t lat,
                                        float loss) {
    return d_cur >= lat && d_cur - lat == lu.lat && f32_bits(fold(lu.loss, loss)) == l_cur_bits;
}

// The tie rule: of two candidates (ROUTE_NO_EDGE = none) the smaller edge index.
SRG_ROUTE_HD inline uint32_t route_better(uint32_t a, uint32_t b) { return a < b ? a : b; }

// One step of the walk over a plain edge list (the CPU restatement; the kernel evaluates the same
// functions over the in-edge list of cur): the route's edge into cur in the row of s, or
// ROUTE_NO_EDGE when no in-edge explains the entry.  *u = the vertex the walk steps to.
SRG_ROUTE_HD inline uint32_t route_step(uint64_t num_edges, const uint32_t* src, const uint32_t* dst,
                                        const uint64_t* lat, const float* loss, bool directed, const PathLatency& t,
                                        const float* table_loss, uint32_t s, uint32_t cur, uint32_t* u) {
    const RouteLabel lc = route_label(t, table_loss, s, cur);
    const uint32_t lc_bits = f32_bits(lc.loss);
    uint32_t best = ROUTE_NO_EDGE;
    for (uint64_t e = 0; e < num_edges && e < ROUTE_NO_EDGE; ++e) {
        uint32_t v;
        if (!route_in_edge(src[e], dst[e], directed, cur, &v)) continue;
        if (!route_explains(lc.lat, lc_bits, route_label(t, table_loss, s, v), lat[e], loss[e])) continue;
        const uint32_t b = route_better(best, (uint32_t)e);
        if (b != best) *u = v;
        best = b;
    }
    return best;
}

// The diagonal: the route s -> s is one hop over the self-loop of s (mod.rs:210-217), the smallest
// index when the list holds several.
SRG_ROUTE_HD inline uint32_t route_self_edge(uint64_t num_edges, const uint32_t* src, const uint32_t* dst, uint32_t s) {
    for (uint64_t e = 0; e < num_edges && e < ROUTE_NO_EDGE; ++e)
        if (src[e] == s && dst[e] == s) return (uint32_t)e;
    return ROUTE_NO_EDGE;
}

}  // namespace srg
