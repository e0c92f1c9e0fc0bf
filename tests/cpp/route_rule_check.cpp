// CPU check of shadow_amd/csrc/route_rule.h (the same header the walk kernels of routes.hip.h
// include): the fold, the source label, the predecessor predicate, the in-edge orientation, the tie
// rule and the table fetch, on hand-written cases.  Built with g++ -ffp-contract=off.  Prints "ok"
// and exits 0, or names the first failing case.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../shadow_amd/csrc/route_rule.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
            ++failures;                                                 \
        }                                                               \
    } while (0)

int main() {
    using namespace srg;

    // the fold: 1 - (1 - L) * (1 - p), each operation rounded in f32
    CHECK(f32_bits(fold(0.0f, 0.0f)) == f32_bits(0.0f));  // +0, not -0
    CHECK(fold(0.0f, 1.0f) == 1.0f);
    CHECK(fold(1.0f, 0.25f) == 1.0f);
    CHECK(fold(0.5f, 0.5f) == 0.75f);
    {
        // the three roundings against a double evaluation rounded once: they differ for this input,
        // and the header gives the f32 chain
        volatile float a = 0.1f, p = 0.2f;
        volatile float x = 1.0f - a, b = 1.0f - p;
        volatile float y = x * b;
        volatile float want = 1.0f - y;
        CHECK(f32_bits(fold(0.1f, 0.2f)) == f32_bits(want));
    }
    // a loss whose fold from the source label differs from the raw edge loss in the last bits:
    // 1 - p rounds, so 1 - (1 - p) != p
    const float p_odd = 0.1f;
    CHECK(f32_bits(fold(0.0f, p_odd)) != f32_bits(p_odd));
    CHECK(std::fabs(fold(0.0f, p_odd) - p_odd) < 1e-7f);

    // a 3-vertex table, u64 form.  Diagonal = raw self-loop weights (nonzero), NOT the source label.
    //   edges: 0: (0,0) self-loop  1: (0,1) lat 5 loss p_odd  2: (1,2) lat 7 loss 0.25
    //          3: (1,1) self-loop  4: (2,2) self-loop
    const uint32_t src[] = {0, 0, 1, 1, 2}, dst[] = {0, 1, 2, 1, 2};
    const uint64_t elat[] = {99, 5, 7, 98, 97};
    const float eloss[] = {0.5f, p_odd, 0.25f, 0.5f, 0.5f};
    const float l01 = fold(0.0f, p_odd), l02 = fold(l01, 0.25f);
    const float l10 = l01, l12 = fold(0.0f, 0.25f), l20 = fold(l12, p_odd);
    const uint64_t lat[9] = {99, 5, 12, 5, 98, 7, 12, 7, 97};
    const float loss[9] = {0.5f, l01, l02, l10, 0.5f, l12, l20, l12, 0.5f};
    const PathLatency T{lat, nullptr, nullptr, 1, 3};

    // the source label is (0, +0) against the nonzero diagonal
    CHECK(route_label(T, loss, 0, 0).lat == 0 && f32_bits(route_label(T, loss, 0, 0).loss) == 0);
    CHECK(route_label(T, loss, 1, 1).lat == 0);
    CHECK(route_label(T, loss, 0, 1).lat == 5 && route_label(T, loss, 0, 1).loss == l01);
    CHECK(path_latency(T, 0, 0) == 99);

    // predicate: edge 1 explains (0 -> 1) from the source label; with the diagonal as the label
    // (99, 0.5) it would not; the raw loss in the table would not either (fold(0, p) != p)
    CHECK(route_explains(5, f32_bits(l01), route_label(T, loss, 0, 0), 5, p_odd));
    CHECK(!route_explains(5, f32_bits(l01), RouteLabel{99, 0.5f}, 5, p_odd));
    CHECK(!route_explains(5, f32_bits(p_odd), route_label(T, loss, 0, 0), 5, p_odd));
    // one latency unit off, one loss bit off
    CHECK(!route_explains(6, f32_bits(l01), route_label(T, loss, 0, 0), 5, p_odd));
    CHECK(!route_explains(5, f32_bits(l01) ^ 1u, route_label(T, loss, 0, 0), 5, p_odd));

    // in-edge orientation: undirected counts an edge stored either way, directed only (u, cur);
    // a self-loop is never an in-edge
    uint32_t u = 77;
    CHECK(route_in_edge(0, 1, false, 1, &u) && u == 0);
    CHECK(route_in_edge(0, 1, false, 0, &u) && u == 1);
    CHECK(route_in_edge(0, 1, true, 1, &u) && u == 0);
    CHECK(!route_in_edge(0, 1, true, 0, &u));
    CHECK(!route_in_edge(1, 1, false, 1, &u));
    CHECK(!route_in_edge(1, 1, true, 1, &u));
    CHECK(!route_in_edge(0, 1, false, 2, &u));

    // whole steps over the undirected list: 0 -> 2 walks back over edge 2 to 1, then edge 1 to 0;
    // 2 -> 0 uses the same edges stored in the other orientation
    CHECK(route_step(5, src, dst, elat, eloss, false, T, loss, 0, 2, &u) == 2 && u == 1);
    CHECK(route_step(5, src, dst, elat, eloss, false, T, loss, 0, 1, &u) == 1 && u == 0);
    CHECK(route_step(5, src, dst, elat, eloss, false, T, loss, 2, 0, &u) == 1 && u == 1);
    CHECK(route_step(5, src, dst, elat, eloss, false, T, loss, 2, 1, &u) == 2 && u == 2);
    // directed: the same list has no edge into 0
    CHECK(route_step(5, src, dst, elat, eloss, true, T, loss, 2, 0, &u) == ROUTE_NO_EDGE);
    // a self-loop whose weight happens to fit is still ignored: vertex 1's entry in row 0 set to
    // what its self-loop (lat 98) would give from itself
    {
        uint64_t lat2[9];
        float loss2[9];
        for (int i = 0; i < 9; ++i) lat2[i] = lat[i], loss2[i] = loss[i];
        const uint32_t s2[] = {1, 0}, d2[] = {1, 1};  // 0: self-loop (1,1) lat 0-sum fit, 1: (0,1)
        const uint64_t w2[] = {0, 5};
        const float p2[] = {0.0f, p_odd};
        const PathLatency T2{lat2, nullptr, nullptr, 1, 3};
        // the self-loop (lat 0, loss 0) satisfies both equalities trivially from 1's own label
        CHECK(route_explains(5, f32_bits(l01), route_label(T2, loss2, 0, 1), 0, 0.0f));
        CHECK(route_step(2, s2, d2, w2, p2, false, T2, loss2, 0, 1, &u) == 1 && u == 0);
    }
    // the diagonal route: the smallest self-loop index
    CHECK(route_self_edge(5, src, dst, 0) == 0 && route_self_edge(5, src, dst, 1) == 3);
    {
        const uint32_t s3[] = {0, 2, 2}, d3[] = {1, 2, 2};
        CHECK(route_self_edge(3, s3, d3, 2) == 1);
        CHECK(route_self_edge(3, s3, d3, 0) == ROUTE_NO_EDGE);
    }

    // tie rule: two bit-equal candidates (parallel edges), the lower edge index wins -- wherever
    // it stands in the list
    {
        const uint32_t s4[] = {0, 0, 0}, d4[] = {1, 1, 1};
        const uint64_t w4[] = {6, 5, 5};  // edge 0 does not fit, 1 and 2 both do
        const float p4[] = {p_odd, p_odd, p_odd};
        CHECK(route_step(3, s4, d4, w4, p4, false, T, loss, 0, 1, &u) == 1 && u == 0);
        const uint32_t s5[] = {1, 0, 0}, d5[] = {0, 1, 1};  // the winner stored as (cur, u)
        const uint64_t w5[] = {5, 5, 6};
        CHECK(route_step(3, s5, d5, w5, p4, false, T, loss, 0, 1, &u) == 0 && u == 0);
        CHECK(route_better(ROUTE_NO_EDGE, 7) == 7 && route_better(7, 3) == 3 && route_better(3, 7) == 3);
        CHECK(route_better(ROUTE_NO_EDGE, ROUTE_NO_EDGE) == ROUTE_NO_EDGE);
    }

    // the key-form table fetch: latency = key * unit off the diagonal, diag on it; same routes
    {
        const uint32_t key[9] = {0xFFFFFFFFu, 5, 12, 5, 0xFFFFFFFFu, 7, 12, 7, 0xFFFFFFFFu};
        const uint64_t diag[3] = {99000, 98000, 97000};
        const PathLatency K{nullptr, key, diag, 1000, 3};
        const uint64_t klat[] = {99000, 5000, 7000, 98000, 97000};
        CHECK(route_label(K, loss, 0, 2).lat == 12000);
        CHECK(route_label(K, loss, 0, 0).lat == 0);  // not diag
        CHECK(path_latency(K, 0, 0) == 99000);
        CHECK(route_step(5, src, dst, klat, eloss, false, K, loss, 0, 2, &u) == 2 && u == 1);
        CHECK(route_step(5, src, dst, klat, eloss, false, K, loss, 0, 1, &u) == 1 && u == 0);
    }

    // no overflow in the latency compare at D near 2^64: lu.lat + lat would wrap to a small number
    {
        const uint64_t big = UINT64_MAX - 2;
        CHECK(route_explains(big, 0, RouteLabel{big - 10, 0.0f}, 10, 0.0f));
        CHECK((uint64_t)(big + 7) == 4);                                // the sum wraps to 4 ...
        CHECK(!route_explains(4, 0, RouteLabel{big, 0.0f}, 7, 0.0f));   // ... and 4 is still refused: 4 < 7
        CHECK(!route_explains(big, 0, RouteLabel{5, 0.0f}, UINT64_MAX, 0.0f));  // d_cur < lat
        CHECK(route_explains(UINT64_MAX, 0, RouteLabel{0, 0.0f}, UINT64_MAX, 0.0f));
    }

    if (failures) return 1;
    std::puts("ok");
    return 0;
}
