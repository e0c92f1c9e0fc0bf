// CPU check of the distribution plan (shadow_amd/csrc/plan.h): make_plan, tri_tile_h,
// xcd_tile_order and scan_group_cut.  Prints one JSON object; tests/test_plan_cpu.py compares the
// splits with shadow_amd.dist and asserts the flags.  Built plain and with
// -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "../../shadow_amd/csrc/plan.h"

static int g_fail = 0;

#define CHECK(cond, ...)                           \
    do {                                           \
        if (!(cond)) {                             \
            if (g_fail++ < 10) {                   \
                std::fprintf(stderr, __VA_ARGS__); \
                std::fprintf(stderr, "\n");        \
            }                                      \
        }                                          \
    } while (0)

static void print_list(const char* key, const std::vector<int>& v) {
    std::printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", v[i]);
    std::printf("]");
}

// the node list of a case: n entries below V, not in order
static std::vector<uint32_t> node_list(uint32_t n, uint32_t V) {
    std::vector<uint32_t> v(n);
    for (uint32_t i = 0; i < n; ++i) v[i] = (uint32_t)(((uint64_t)i * 7919u + 3u) % V);
    return v;
}

static void check_make_plan() {
    std::printf("\"make_plan\": [");
    bool first = true;
    for (int G = 1; G <= 8; ++G)
        for (int g = 0; g < G; ++g)
            for (uint32_t V : {1u, 63u, 64u, 65u, 1000u, 10000u})
                for (int T : {64, 128}) {
                    std::set<uint32_t> ns{0u, 1u, 7u, V};
                    for (uint32_t n : ns) {
                        const std::vector<uint32_t> nodes = node_list(n, V);
                        const Plan p = make_plan(G, g, V, T, nodes);
                        // lnodes / lpos: the slice [p0, p1) of the list and its positions
                        bool slice_ok = p.p0 <= p.p1 && p.p1 <= n && p.lnodes.size() == p.p1 - p.p0 &&
                                        p.lpos.size() == p.lnodes.size();
                        for (uint32_t q = p.p0; slice_ok && q < p.p1; ++q)
                            slice_ok = p.lnodes[q - p.p0] == nodes[q] && p.lpos[q - p.p0] == q;
                        // owner(b) is the rank whose own(b) holds, for every block
                        bool owner_ok = (int)p.blk_lo.size() == G + 1;
                        for (int b = 0; owner_ok && b < p.nb; ++b) {
                            const int r = p.owner(b);
                            owner_ok = r >= 0 && r < G && p.blk_lo[r] <= b && b < p.blk_lo[r + 1] && (r == g) == p.own(b);
                        }
                        std::printf("%s\n{\"G\": %d, \"g\": %d, \"V\": %u, \"T\": %d, \"n\": %u, \"nb\": %d, \"rb0\": %d, "
                                    "\"rb1\": %d, \"p0\": %u, \"p1\": %u, \"slice_ok\": %s, \"owner_ok\": %s, ",
                                    first ? "" : ",", G, g, V, T, n, p.nb, p.rb0, p.rb1, p.p0, p.p1,
                                    slice_ok ? "true" : "false", owner_ok ? "true" : "false");
                        print_list("blk_lo", p.blk_lo);
                        std::printf("}");
                        first = false;
                    }
                }
    std::printf("]");
}

static const int kNb[] = {1, 2, 3, 9, 32, 79};

// tri_tile_h inverts the row-major index of the triangle I <= J
static void check_tri_tile() {
    for (int nb : kNb) {
        int t = 0;
        for (int I = 0; I < nb; ++I)
            for (int J = I; J < nb; ++J, ++t) {
                int i = -1, j = -1;
                tri_tile_h(nb, t, i, j);
                CHECK(i == I && j == J, "tri_tile_h(%d, %d) = (%d, %d), expected (%d, %d)", nb, t, i, j, I, J);
            }
    }
}

static void check_xcd_order() {
    for (int nb : kNb)
        for (int G : {1, 2, 8})
            for (int g = 0; g < G; ++g) {
                std::vector<int> own;  // the rank's tiles, triangle order
                for (int t = 0, I = 0; I < nb; ++I)
                    for (int J = I; J < nb; ++J, ++t)
                        if ((I + J) % G == g) own.push_back(t);
                std::vector<int> out, off;
                xcd_tile_order(own, nb, out, off);
                CHECK((int)off.size() == nb + 1 && off[0] == 0 && off[nb] == (int)out.size(), "nb=%d G=%d g=%d: off", nb, G, g);
                if ((int)off.size() != nb + 1) continue;
                for (int kb = 0; kb < nb; ++kb) {
                    const int a = off[kb], z = off[kb + 1], k1 = kb + 1;
                    CHECK(a <= z && z <= (int)out.size() && (z - a) % 8 == 0, "nb=%d G=%d g=%d kb=%d: slice [%d, %d)", nb, G, g,
                          kb, a, z);
                    if (!(a <= z && z <= (int)out.size() && (z - a) % 8 == 0)) continue;
                    // expected: the own tiles off lines kb and kb + 1, sorted along the Z-order curve
                    std::vector<std::pair<uint32_t, int>> want;
                    for (int t : own) {
                        int I, J;
                        tri_tile_h(nb, t, I, J);
                        if (I != kb && J != kb && I != k1 && J != k1) want.push_back({morton2((uint32_t)I, (uint32_t)J), t});
                    }
                    std::sort(want.begin(), want.end());
                    // each column x (positions = x mod 8): real entries first, then only -1; the
                    // columns' real entries, x = 0..7 in turn, are consecutive runs of `want`
                    size_t next = 0;
                    for (int x = 0; x < 8; ++x) {
                        bool ended = false;
                        for (int i = a + x; i < z; i += 8) {
                            if (out[i] < 0) {
                                CHECK(out[i] == -1, "nb=%d G=%d kb=%d: entry %d", nb, G, kb, out[i]);
                                ended = true;
                                continue;
                            }
                            CHECK(!ended, "nb=%d G=%d g=%d kb=%d: a tile after a -1 in column %d", nb, G, g, kb, x);
                            CHECK(next < want.size() && want[next].second == out[i],
                                  "nb=%d G=%d g=%d kb=%d: column %d holds tile %d out of Z-order", nb, G, g, kb, x, out[i]);
                            ++next;
                        }
                    }
                    CHECK(next == want.size(), "nb=%d G=%d g=%d kb=%d: %zu of %zu tiles listed", nb, G, g, kb, next, want.size());
                }
            }
}

static void check_scan_cut() {
    for (uint32_t nblocks : {1u, 7u, 8u, 9u, 20u, 79u, 200u}) {
        const std::set<uint32_t> ngs{1u, 2u, 3u, 4u, std::min(8u, nblocks)};
        for (uint32_t ng : ngs) {
            CHECK(scan_group_cut(0, ng, nblocks) == 0, "cut(0) of %u blocks in %u groups", nblocks, ng);
            CHECK(scan_group_cut(ng, ng, nblocks) == nblocks, "cut(ng) of %u blocks in %u groups", nblocks, ng);
            for (uint32_t q = 0; q < ng; ++q) {
                const uint32_t c0 = scan_group_cut(q, ng, nblocks), c1 = scan_group_cut(q + 1, ng, nblocks);
                CHECK(c0 <= c1, "%u blocks, %u groups: cut(%u) = %u > cut(%u) = %u", nblocks, ng, q, c0, q + 1, c1);
                if (q > 0) CHECK(c0 % 8 == 0 || c0 == nblocks, "%u blocks, %u groups: cut(%u) = %u", nblocks, ng, q, c0);
            }
        }
    }
    // C3: 79 source blocks in three groups of 40 / 32 / 7
    const uint32_t want[4] = {0, 40, 72, 79};
    for (uint32_t q = 0; q < 4; ++q)
        CHECK(scan_group_cut(q, 3, 79) == want[q], "79 blocks in 3 groups: cut(%u) = %u", q, scan_group_cut(q, 3, 79));
}

int main() {
    std::printf("{");
    check_make_plan();
    check_tri_tile();
    check_xcd_order();
    check_scan_cut();
    std::printf(",\n\"failed_checks\": %d}\n", g_fail);
    return g_fail ? 1 : 0;
}
