// entry_plan.h -- the decisions of a host-entry call that are pure functions of its arguments and
// options: which output rows and which edges a rank owns, and the call's flags.
// Plain C++: no HIP include, so tests/cpp/entry_plan_check.cpp compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

struct Range {  // [lo, hi)
    size_t lo, hi;
    size_t size() const { return hi - lo; }
};

// Rank r of G owns the items [n r / G, n (r+1) / G) of n: the source rows of a build (make_plan,
// run_sparse, the host entry's registration, device tables and D2H tail) and the edges a sharded
// rank ships.  The only place this split is written (shadow_amd.dist.source_split is its Python
// twin); a function of (n, G) only, so every rank agrees on every rank's range.
inline Range rank_rows(uint64_t n, uint64_t r, uint64_t G) { return {(size_t)(n * r / G), (size_t)(n * (r + 1) / G)}; }

// the allgatherv segments of an array of `count` items of `elem` bytes split by rank_rows (edges,
// or the rows of a table): byte offset and length per rank
inline void slice_tables(uint64_t count, int G, size_t elem, std::vector<size_t>& offs, std::vector<size_t>& lens) {
    offs.resize(G);
    lens.resize(G);
    for (int q = 0; q < G; ++q) {
        const Range s = rank_rows(count, q, G);
        offs[q] = s.lo * elem;
        lens[q] = s.size() * elem;
    }
}

// early rows: a table of at least 64 MB is page-locked and its finished rows leave the device while
// later kernels run; smaller tables are copied at the end
inline bool ships_early(bool direct, size_t table_bytes) { return !direct && table_bytes >= ((size_t)64 << 20); }

// the narrowest form of its slice a sharded rank offers the exchange: 0 = sequential-pair, 1 = u16
// narrowing, 2 = plain (the ranks settle on the maximum)
inline uint32_t offered_form(bool coded, bool all_seq, bool all_narrow) {
    return !coded ? 2u : all_seq ? 0u : all_narrow ? 1u : 2u;
}

struct EntryPlan {
    int nr = 1, rk = 0;      // ranks of the group, this rank
    bool early = false;      // ships_early of the n x n table at 12 B per pair
    bool rows_part = false;  // a rank that fills only its own rows of a table the ranks share (SRG_OPT_GATHER_OUTPUT 0)
    bool shard = false;      // this rank ships only its slice of the edges (SRG_OPT_EDGE_SHARD: 1, or < 0 from 4 ranks)
    Range rows{0, 0};        // the output rows this rank fills: rank_rows when rows_part, else all n
    Range edges{0, 0};       // the edges this rank ships over PCIe: rank_rows of E when shard, else all E
};

inline EntryPlan make_entry_plan(bool direct, uint64_t n, uint64_t E, int nranks, int rank, bool gather_output,
                                 int edge_shard) {
    EntryPlan p;
    p.nr = nranks;
    p.rk = rank;
    p.early = ships_early(direct, (size_t)(n * n) * 12);
    p.rows_part = !direct && nranks > 1 && !gather_output;
    p.shard = nranks > 1 && (edge_shard == 1 || (edge_shard < 0 && nranks >= 4));
    p.rows = p.rows_part ? rank_rows(n, rank, nranks) : Range{0, (size_t)n};
    p.edges = p.shard ? rank_rows(E, rank, nranks) : Range{0, (size_t)E};
    return p;
}

}  // namespace
