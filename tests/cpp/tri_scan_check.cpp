// CPU check of the triangular scan's host functions (shadow_amd/csrc/plan.h): tri_scan_blocks
// (the block list of a tight_v5 launch that scans only the pairs target tile b >= source block c)
// and scan_group_cut_tri (the scan groups of that launch order).  Prints one JSON object;
// tests/test_tri_scan_cpu.py asserts it.  Built plain and with -fsanitize=address,undefined.
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

static const uint32_t kBlocks[] = {1, 2, 7, 8, 9, 16, 17, 20, 79, 200};

// the workgroups tight_v5 runs for the list of one launch over [c0, c1): (slot & 3) picks the tile
// of the 4-tile group, (slot >> 2) & 7 the source block of the 8-block group
static void run_launch(const std::vector<uint32_t>& list, uint32_t c0, uint32_t c1, uint32_t nb,
                       std::vector<int>& cover, std::vector<char>& in_block) {
    CHECK(list.size() % 8 == 0, "list of [%u, %u) of %u: %zu entries", c0, c1, nb, list.size());
    bool pad = false;
    for (uint32_t d : list) {
        if (d == TRI_PAD) {
            pad = true;
            continue;
        }
        CHECK(!pad, "[%u, %u) of %u: a block after the padding", c0, c1, nb);
        const uint32_t tb = d & 0xFFFFu, sg = d >> 16;
        bool any = false;
        for (uint32_t slot = 0; slot < 32; ++slot) {
            const uint32_t b = tb * 4 + (slot & 3), c = c0 + sg * 8 + ((slot >> 2) & 7);
            if (c >= c1 || b >= nb) continue;
            in_block[(size_t)c * nb + b] = 1;
            if (b < c) continue;
            ++cover[(size_t)c * nb + b];
            any = true;
        }
        CHECK(any, "[%u, %u) of %u: block (%u, %u) holds no pair of the triangle", c0, c1, nb, tb, sg);
    }
}

static void check_blocks() {
    for (uint32_t nb : kBlocks)
        for (uint32_t ng : {1u, 2u, 3u, 4u}) {
            std::vector<int> cover((size_t)nb * nb, 0);
            std::vector<char> in_block((size_t)nb * nb, 0);
            std::vector<uint32_t> all;
            size_t listed = 0;
            for (uint32_t q = 0; q < ng; ++q) {
                const uint32_t c0 = scan_group_cut_tri(q, ng, nb), c1 = scan_group_cut_tri(q + 1, ng, nb);
                const size_t base = all.size();
                tri_scan_blocks(c0, c1, nb, all);  // appended, as run_dense builds the lists
                const std::vector<uint32_t> list(all.begin() + base, all.end());
                CHECK((c1 > c0) == !list.empty(), "%u blocks, group [%u, %u): %zu entries", nb, c0, c1, list.size());
                run_launch(list, c0, c1, nb, cover, in_block);
                for (uint32_t d : list) listed += d != TRI_PAD;
            }
            size_t full = 0;
            for (uint32_t c = 0; c < nb; ++c)
                for (uint32_t b = 0; b < nb; ++b) {
                    const int got = cover[(size_t)c * nb + b];
                    CHECK(got == (b >= c ? 1 : 0), "%u blocks, %u groups: pair (c %u, b %u) run %d times", nb, ng, c, b, got);
                }
            for (uint32_t q = 0; q < ng; ++q) {
                const uint32_t c0 = scan_group_cut_tri(q, ng, nb), c1 = scan_group_cut_tri(q + 1, ng, nb);
                if (c1 > c0) full += (size_t)((nb + 3) / 4) * ((c1 - c0 + 7) / 8);
            }
            CHECK(listed <= full, "%u blocks, %u groups: %zu blocks listed, the full launch has %zu", nb, ng, listed, full);
            // (run_launch: no listed block lies wholly under the diagonal, so from 16 blocks on,
            // where such blocks exist, the list is shorter than the full launch)
            if (nb >= 16 && ng == 1) CHECK(listed < full, "%u blocks: %zu of %zu blocks listed", nb, listed, full);
        }
    // any launch bounds (not only the cut function's): pairs covered once, c0 on a multiple of 8
    for (uint32_t nb : kBlocks)
        for (uint32_t c0 = 0; c0 < nb; c0 += 8)
            for (uint32_t c1 : {c0 + 1, c0 + 8, c0 + 13, nb}) {
                if (c1 > nb || c1 <= c0) continue;
                std::vector<int> cover((size_t)nb * nb, 0);
                std::vector<char> in_block((size_t)nb * nb, 0);
                std::vector<uint32_t> list;
                tri_scan_blocks(c0, c1, nb, list);
                run_launch(list, c0, c1, nb, cover, in_block);
                for (uint32_t c = 0; c < nb; ++c)
                    for (uint32_t b = 0; b < nb; ++b)
                        CHECK(cover[(size_t)c * nb + b] == (c >= c0 && c < c1 && b >= c ? 1 : 0),
                              "%u blocks, launch [%u, %u): pair (c %u, b %u) run %d times", nb, c0, c1, c, b,
                              cover[(size_t)c * nb + b]);
            }
}

static void check_cut() {
    for (uint32_t nb : kBlocks) {
        const std::set<uint32_t> ngs{1u, 2u, 3u, 4u, std::min(8u, nb)};
        for (uint32_t ng : ngs) {
            CHECK(scan_group_cut_tri(0, ng, nb) == 0, "cut(0) of %u blocks in %u groups", nb, ng);
            CHECK(scan_group_cut_tri(ng, ng, nb) == nb, "cut(ng) of %u blocks in %u groups", nb, ng);
            for (uint32_t q = 0; q < ng; ++q) {
                const uint32_t c0 = scan_group_cut_tri(q, ng, nb), c1 = scan_group_cut_tri(q + 1, ng, nb);
                CHECK(c0 <= c1 && c1 <= nb, "%u blocks, %u groups: cut(%u) = %u, cut(%u) = %u", nb, ng, q, c0, q + 1, c1);
                if (q > 0) CHECK(c0 % 8 == 0 || c0 == nb, "%u blocks, %u groups: cut(%u) = %u", nb, ng, q, c0);
            }
        }
        // three groups: the last one is the last partial 8 blocks whenever the others are not empty
        const uint32_t a = scan_group_cut_tri(1, 3, nb), z = scan_group_cut_tri(2, 3, nb);
        if (nb > 8) CHECK(z == (nb - 1) / 8 * 8 && nb - z <= 8, "%u blocks: last cut %u", nb, z);
        // ... and the first two split the work before it evenly, to within the 8-block rounding
        if (z >= 16) {
            const double w = (double)tri_scan_work(z, nb), w0 = (double)tri_scan_work(a, nb);
            const double slack = 4.0 * nb;  // half of 8 blocks, each at most nb tiles
            CHECK(a > 0 && a < z, "%u blocks: cuts %u, %u", nb, a, z);
            CHECK(w0 >= w / 2 - slack && w0 <= w / 2 + slack, "%u blocks: first group's work %.0f of %.0f", nb, w0, w);
        }
    }
    // three non-empty groups first at 17 blocks
    for (uint32_t nb = 1; nb <= 17; ++nb) {
        const uint32_t a = scan_group_cut_tri(1, 3, nb), z = scan_group_cut_tri(2, 3, nb);
        CHECK((a > 0 && z > a && nb > z) == (nb == 17), "%u blocks: cuts %u, %u", nb, a, z);
    }
    // C3: 79 source blocks, 24 / 48 / 7 (work 1620 / 1512 / 28 tile launches)
    const uint32_t want[4] = {0, 24, 72, 79};
    for (uint32_t q = 0; q < 4; ++q)
        CHECK(scan_group_cut_tri(q, 3, 79) == want[q], "79 blocks in 3 groups: cut(%u) = %u", q, scan_group_cut_tri(q, 3, 79));
    // ... and in four groups the blocks after the first group split by rows: 24 / 24 / 24 / 7
    const uint32_t want4[5] = {0, 24, 48, 72, 79};
    for (uint32_t q = 0; q < 5; ++q)
        CHECK(scan_group_cut_tri(q, 4, 79) == want4[q], "79 blocks in 4 groups: cut(%u) = %u", q, scan_group_cut_tri(q, 4, 79));
}

int main() {
    check_blocks();
    check_cut();
    std::printf("{\"failed_checks\": %d}\n", g_fail);
    return g_fail ? 1 : 0;
}
