// CPU check of shadow_amd/csrc/route_tree_rule.h (the same header the kernels of
// route_trees.hip.h include): the doubling step, its fixpoints, the hops = d + 1 convention and the
// saturating push, on hand-written trees.  Built with g++.  Prints "ok" and exits 0, or names the
// first failing case.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../shadow_amd/csrc/route_tree_rule.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
            ++failures;                                                 \
        }                                                               \
    } while (0)

using namespace srg;

// the rounds as the kernel runs them: every vertex reads the jumps of the round before (double
// buffer), until a round moves nothing.  Returns the rounds in which something moved.
static int run(uint32_t s, const std::vector<uint32_t>& pv, std::vector<TreeJump>& j) {
    const uint32_t V = (uint32_t)pv.size();
    j.resize(V);
    for (uint32_t t = 0; t < V; ++t) j[t] = tree_jump_init(t, s, pv[t]);
    int rounds = 0;
    for (;;) {
        std::vector<TreeJump> nx(V);
        bool moved = false;
        for (uint32_t t = 0; t < V; ++t) {
            nx[t] = tree_jump_step(j[t], j[j[t].up]);
            moved = moved || tree_jump_moved(j[t], nx[t]);
        }
        j = nx;
        if (!moved) return rounds;
        ++rounds;
        if (rounds > 64) return rounds;
    }
}

int main() {
    const uint32_t NONE = ROUTE_TREE_NONE;
    std::vector<TreeJump> j;

    // a chain of 9 from source 0: 0 - 1 - ... - 8.  Depth 8 below the source, 7 below its child:
    // ceil(log2 7) = 3 moving rounds, never 8
    {
        std::vector<uint32_t> pv(9);
        pv[0] = NONE;
        for (uint32_t t = 1; t < 9; ++t) pv[t] = t - 1;
        const int rounds = run(0, pv, j);
        CHECK(rounds <= 4);
        CHECK(rounds == 3);
        for (uint32_t t = 1; t < 9; ++t) {
            CHECK(j[t].up == 1);                 // every jump ends at the child of the source
            CHECK(tree_hops(j[t]) == t);         // hops = d + 1
            CHECK(tree_root_reaches(j[t], 0, pv[j[t].up]));
        }
        CHECK(j[0].up == 0 && j[0].d == 0);      // the source is a fixpoint
        CHECK(!tree_root_reaches(j[0], 0, pv[0]));
    }
    // the same chain from a source in the middle: two branches, the first edge differs by side
    {
        std::vector<uint32_t> pv = {1, 2, 3, 4, NONE, 4, 5, 6, 7};  // source 4
        const int rounds = run(4, pv, j);
        CHECK(rounds == 2);  // depth 3 below each child
        for (uint32_t t = 0; t < 4; ++t) CHECK(j[t].up == 3 && tree_hops(j[t]) == 4 - t);
        for (uint32_t t = 5; t < 9; ++t) CHECK(j[t].up == 5 && tree_hops(j[t]) == t - 4);
    }
    // a star: every vertex a child of the source; nothing moves at all
    {
        std::vector<uint32_t> pv = {2, 2, NONE, 2, 2, 2};
        CHECK(run(2, pv, j) == 0);
        for (uint32_t t = 0; t < 6; ++t) {
            CHECK(j[t].up == t && j[t].d == 0);
            if (t != 2) CHECK(tree_hops(j[t]) == 1 && tree_root_reaches(j[t], 2, pv[t]));
        }
    }
    // a fixpoint that is not a child of the source: vertex 3 has no predecessor, 4 and 5 hang
    // under it.  Their jumps end at 3, which does not reach the source; 1 and 2 are unaffected.
    {
        std::vector<uint32_t> pv = {NONE, 0, 1, NONE, 3, 4};
        run(0, pv, j);
        CHECK(j[3].up == 3 && j[4].up == 3 && j[5].up == 3);
        for (uint32_t t = 3; t < 6; ++t) CHECK(!tree_root_reaches(j[t], 0, pv[j[t].up]));
        CHECK(tree_root_reaches(j[1], 0, pv[j[1].up]) && tree_hops(j[1]) == 1);
        CHECK(tree_root_reaches(j[2], 0, pv[j[2].up]) && tree_hops(j[2]) == 2 && j[2].up == 1);
    }
    // the saturating push
    {
        const uint64_t M = ~(uint64_t)0;
        CHECK(tree_sat_add(0, 0) == 0);
        CHECK(tree_sat_add(M - 1, 1) == M);
        CHECK(tree_sat_add(M - 1, 5) == M);
        CHECK(tree_sat_add(M, 1) == M);
        CHECK(tree_sat_add(M, M) == M);
        CHECK(tree_sat_add(1ull << 63, 1ull << 63) == M);
        CHECK(tree_sat_add(7, 9) == 16);
        // order does not matter once a partial sum saturates: min(sum, 2^64 - 1) either way
        CHECK(tree_sat_add(tree_sat_add(M - 1, 5), 3) == tree_sat_add(M - 1, tree_sat_add(5, 3)));
    }
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
