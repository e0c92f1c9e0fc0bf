// route_tree_rule.h — the two small rules behind the route trees, shared by the kernels of
// route_trees.hip.h and a CPU unit test (tests/cpp/route_tree_check.cpp, built with g++).
//
// The routes of one source s form a tree (route_rule.h's tie rule makes every route unique, and the
// route to t through u ends with the route to u): pred_vertex[t] is t's parent.
//
// 1. Pointer doubling.  Every vertex holds a jump (up, d): `up` is an ancestor of t, `d` the number
//    of tree edges between them.  The jumps stop one level below the source:
//        up[t] = t, d = 0   for t == s, for a child of s, and for a vertex without a predecessor,
//        up[t] = pred_vertex[t], d = 1   otherwise.
//    A round replaces every jump by itself followed by the jump of its end, reading the jumps of
//    the round before: (up, d) <- (up[up], d + d[up]).  The end of a fixpoint's jump is itself with
//    d = 0, so a jump that has arrived stays; after ceil(log2(depth)) rounds nothing moves.  Then
//        hops(t) = d + 1   (the edge from s into the child is not among the d),
//        first edge of the route = pred_edge[up[t]].
//    A fixpoint that is not a child of s is an unexplained vertex (or s itself): every vertex whose
//    jump ends there has no route.
// 2. The saturating push.  Packet counts go up the tree: sub[parent] += sub[t], load[edge] +=
//    sub[t], every sum min(a + b, 2^64 - 1).  All terms are non-negative, so the saturated sums
//    give min(true sum, 2^64 - 1) in any order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SRG_TREE_HD __host__ __device__
#else
#define SRG_TREE_HD
#endif

namespace srg {

constexpr uint32_t ROUTE_TREE_NONE = 0xFFFFFFFFu;  // no edge / no vertex (SRG_ROUTE_NONE)

struct TreeJump {
    uint32_t up;  // the ancestor the jump ends at
    uint32_t d;   // tree edges between the vertex and `up`
};

SRG_TREE_HD inline TreeJump tree_jump_init(uint32_t t, uint32_t s, uint32_t pred_vertex) {
    if (t == s || pred_vertex == s || pred_vertex == ROUTE_TREE_NONE) return TreeJump{t, 0u};
    return TreeJump{pred_vertex, 1u};
}

// one round for one vertex: `me` and `at_up` (the jump of me.up) are both of the round before
SRG_TREE_HD inline TreeJump tree_jump_step(TreeJump me, TreeJump at_up) { return TreeJump{at_up.up, me.d + at_up.d}; }

SRG_TREE_HD inline bool tree_jump_moved(TreeJump before, TreeJump after) { return before.up != after.up; }

// after the last round: does the jump of a vertex t != s end at a child of s?  (`root_pred_vertex`
// is pred_vertex[jump.up].)  Otherwise t has no route.
SRG_TREE_HD inline bool tree_root_reaches(TreeJump j, uint32_t s, uint32_t root_pred_vertex) {
    return j.up != s && root_pred_vertex == s;
}

SRG_TREE_HD inline uint32_t tree_hops(TreeJump j) { return j.d + 1u; }

SRG_TREE_HD inline uint64_t tree_sat_add(uint64_t a, uint64_t b) {
    const uint64_t r = a + b;
    return r < a ? ~(uint64_t)0 : r;
}

}  // namespace srg
