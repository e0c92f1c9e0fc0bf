// CPU check of the host entry's plan (shadow_amd/csrc/entry_plan.h): rank_rows, slice_tables,
// offered_form and the flags of make_entry_plan.  Prints one JSON object; tests/test_entry_plan_cpu.py
// compares the rank_rows results with shadow_amd.dist.source_split and asserts that no check inside
// the program failed.  Built plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <set>
#include <vector>

#include "../../shadow_amd/csrc/plan.h"  // (includes entry_plan.h; make_plan is compared with rank_rows)

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

// the ranges tile [0, n) in order without a gap, and are make_plan's [p0, p1)
static void check_rank_rows() {
    std::printf("\"rank_rows\": [");
    bool first = true;
    for (int G = 1; G <= 8; ++G) {
        const std::set<uint64_t> ns{0u, 1u, 7u, (uint64_t)G - 1, (uint64_t)G, 10000u};
        for (uint64_t n : ns) {
            size_t at = 0;
            for (int r = 0; r < G; ++r) {
                const Range o = rank_rows(n, r, G);
                CHECK(o.lo == at && o.hi >= o.lo && o.hi <= n, "rank_rows(%llu, %d, %d) = [%zu, %zu) after %zu",
                      (unsigned long long)n, r, G, o.lo, o.hi, at);
                CHECK(o.size() == o.hi - o.lo, "Range::size");
                at = o.hi;
                const Plan p = make_plan(G, r, 64, 64, std::vector<uint32_t>((size_t)n, 0u));
                CHECK(p.p0 == o.lo && p.p1 == o.hi, "make_plan(G=%d, g=%d, n=%llu): [%u, %u) != rank_rows [%zu, %zu)", G,
                      r, (unsigned long long)n, p.p0, p.p1, o.lo, o.hi);
                std::printf("%s\n{\"G\": %d, \"r\": %d, \"n\": %llu, \"lo\": %zu, \"hi\": %zu}", first ? "" : ",", G, r,
                            (unsigned long long)n, o.lo, o.hi);
                first = false;
            }
            CHECK(at == n, "rank_rows(%llu, ., %d) ends at %zu", (unsigned long long)n, G, at);
        }
    }
    std::printf("]");
}

// offsets cumulative from 0, lengths summing to E * elem, each segment the rank's slice; in 64
// bits throughout (E = 3e9: E * r and E * elem both pass 2^32; arithmetic only, nothing allocated)
static void check_slice_tables() {
    for (int G = 1; G <= 8; ++G) {
        const std::set<uint64_t> Es{0u, 1u, (uint64_t)G - 1, ((uint64_t)1 << 20) * G + 1, 3000000000ull};
        for (uint64_t E : Es)
            for (size_t elem : {(size_t)2, (size_t)4, (size_t)8, (size_t)12}) {
                std::vector<size_t> offs{99}, lens;  // (whatever they held is replaced)
                slice_tables(E, G, elem, offs, lens);
                CHECK(offs.size() == (size_t)G && lens.size() == (size_t)G, "slice_tables(G=%d): sizes", G);
                if (offs.size() != (size_t)G || lens.size() != (size_t)G) continue;
                unsigned __int128 at = 0;
                for (int q = 0; q < G; ++q) {
                    CHECK(offs[q] == at, "E=%llu G=%d elem=%zu: offs[%d] = %zu", (unsigned long long)E, G, elem, q, offs[q]);
                    const unsigned __int128 lo = (unsigned __int128)E * q / G, hi = (unsigned __int128)E * (q + 1) / G;
                    CHECK(offs[q] == lo * elem && lens[q] == (hi - lo) * elem, "E=%llu G=%d elem=%zu: segment %d = (%zu, %zu)",
                          (unsigned long long)E, G, elem, q, offs[q], lens[q]);
                    CHECK(lens[q] % elem == 0, "E=%llu G=%d elem=%zu: lens[%d] = %zu", (unsigned long long)E, G, elem, q, lens[q]);
                    at += lens[q];
                }
                CHECK(at == (unsigned __int128)E * elem, "E=%llu G=%d elem=%zu: the lengths do not sum to E * elem",
                      (unsigned long long)E, G, elem);
            }
    }
}

// 0 = sequential-pair, 1 = u16 narrowing, 2 = plain: a rank that is not coded offers plain whatever
// the other two say; a coded one its narrowest
static void check_offered_form() {
    for (int coded = 0; coded < 2; ++coded)
        for (int seq = 0; seq < 2; ++seq)
            for (int narrow = 0; narrow < 2; ++narrow) {
                const uint32_t want = !coded ? 2u : seq ? 0u : narrow ? 1u : 2u;
                const uint32_t got = offered_form(coded != 0, seq != 0, narrow != 0);
                CHECK(got == want, "offered_form(%d, %d, %d) = %u, expected %u", coded, seq, narrow, got, want);
            }
    CHECK(offered_form(true, true, true) == 0 && offered_form(true, true, false) == 0, "coded, all_seq");
    CHECK(offered_form(true, false, true) == 1 && offered_form(true, false, false) == 2, "coded, not all_seq");
    CHECK(offered_form(false, true, true) == 2 && offered_form(false, true, false) == 2 &&
              offered_form(false, false, true) == 2 && offered_form(false, false, false) == 2,
          "not coded");
}

static void check_flags() {
    // early: a table (12 B per pair) of at least 64 MB, shortest paths only
    const size_t mb64 = (size_t)64 << 20;
    CHECK(!ships_early(false, mb64 - 1) && ships_early(false, mb64) && ships_early(false, mb64 + 1), "early at 64 MB");
    CHECK(!ships_early(true, mb64 - 1) && !ships_early(true, mb64) && !ships_early(true, mb64 + 1), "early, direct");
    // n = 2364: n^2 * 12 = 67061952 < 2^26 = 67108864 <= 67118700 = 2365^2 * 12
    CHECK(!make_entry_plan(false, 2364, 0, 1, 0, true, -1).early && make_entry_plan(false, 2365, 0, 1, 0, true, -1).early &&
              !make_entry_plan(true, 2365, 0, 1, 0, true, -1).early,
          "make_entry_plan: early");
    // n * n in 64 bits (n = 2^17: n^2 * 12 passes 2^32)
    CHECK(make_entry_plan(false, (uint64_t)1 << 17, 0, 1, 0, true, -1).early, "make_entry_plan: early, n = 2^17");
    // rows_part: shortest paths of a group of several ranks without the output exchange
    const uint64_t n = 1000, E = 12345;
    for (int direct = 0; direct < 2; ++direct)
        for (int G : {1, 2, 3, 8})
            for (int gather = 0; gather < 2; ++gather)
                for (int shard_opt : {-1, 0, 1})
                    for (int r = 0; r < G; ++r) {
                        const EntryPlan p = make_entry_plan(direct != 0, n, E, G, r, gather != 0, shard_opt);
                        const bool part = !direct && G > 1 && !gather;
                        const bool shard = G > 1 && (shard_opt == 1 || (shard_opt < 0 && G >= 4));
                        CHECK(p.nr == G && p.rk == r, "make_entry_plan: ranks");
                        CHECK(p.rows_part == part, "rows_part(direct=%d, G=%d, gather=%d) = %d", direct, G, gather, (int)p.rows_part);
                        CHECK(p.shard == shard, "shard(G=%d, option %d) = %d", G, shard_opt, (int)p.shard);
                        const Range rows = part ? rank_rows(n, r, G) : Range{0, (size_t)n};
                        const Range edges = shard ? rank_rows(E, r, G) : Range{0, (size_t)E};
                        CHECK(p.rows.lo == rows.lo && p.rows.hi == rows.hi, "rows(direct=%d, G=%d, r=%d, gather=%d) = [%zu, %zu)",
                              direct, G, r, gather, p.rows.lo, p.rows.hi);
                        CHECK(p.edges.lo == edges.lo && p.edges.hi == edges.hi, "edges(G=%d, r=%d, option %d) = [%zu, %zu)", G, r,
                              shard_opt, p.edges.lo, p.edges.hi);
                    }
    // no used node: every rank owns the empty range
    const EntryPlan z = make_entry_plan(false, 0, 0, 3, 1, false, 1);
    CHECK(z.rows.lo == 0 && z.rows.hi == 0 && z.edges.lo == 0 && z.edges.hi == 0 && !z.early, "n = 0, E = 0");
}

int main() {
    std::printf("{");
    check_rank_rows();
    check_slice_tables();
    check_offered_form();
    check_flags();
    std::printf(",\n\"failed_checks\": %d}\n", g_fail);
    return g_fail ? 1 : 0;
}
