// plan.h -- which rank and which XCD runs what: the distribution plan, the symmetric FW's
// per-XCD tile order, and the scan-group cut of run_dense.
// Plain C++: no HIP include, so tests/cpp/plan_check.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "entry_plan.h"

namespace {

// ---- distribution plan --------------------------------------------------
// G ranks.  FW ownership: the general FW gives rank r the whole rows of the row blocks
// [blk_lo[r], blk_lo[r+1]); the symmetric FW gives it the stored tiles (I, J) with
// (I + J) mod G == r (fw_line_sym).  After FW every rank holds the whole D.  Sources: rank r
// routes the used nodes at positions [p0, p1) = [n r / G, n (r+1) / G) of `nodes`, so its output
// rows are one contiguous range whatever the node order.
struct Plan {
    int G = 1, g = 0, nb = 0, rb0 = 0, rb1 = 0;
    std::vector<int> blk_lo;               // [G+1] first row block per rank (general FW)
    uint32_t p0 = 0, p1 = 0;               // own sources = nodes[p0 .. p1)
    std::vector<uint32_t> lnodes, lpos;    // own sources (vertex) and their output rows (p0 ..)
    int owner(int b) const { return (int)(std::upper_bound(blk_lo.begin(), blk_lo.end(), b) - blk_lo.begin()) - 1; }
    bool own(int b) const { return b >= rb0 && b < rb1; }
};

inline void tri_tile_h(int nb, int idx, int& I, int& J) {  // kernels.hip.h tri_tile, on the host
    int i = 0;
    while (i + 1 < nb && (i + 1) * nb - (i + 1) * i / 2 <= idx) ++i;
    I = i;
    J = i + (idx - (i * nb - i * (i - 1) / 2));
}

inline Plan make_plan(int G, int g, uint32_t V, int T, const std::vector<uint32_t>& nodes_h) {
    Plan p;
    p.G = G;
    p.g = g;
    p.nb = (int)(((size_t)V + T - 1) / T);
    p.blk_lo.resize(G + 1);
    for (int r = 0; r <= G; ++r) p.blk_lo[r] = (int)((int64_t)r * p.nb / G);
    p.blk_lo[G] = p.nb;
    p.rb0 = p.blk_lo[g];
    p.rb1 = p.blk_lo[g + 1];
    const Range own = rank_rows(nodes_h.size(), g, G);
    p.p0 = (uint32_t)own.lo;
    p.p1 = (uint32_t)own.hi;
    for (uint32_t q = p.p0; q < p.p1; ++q) {
        p.lnodes.push_back(nodes_h[q]);
        p.lpos.push_back(q);
    }
    return p;
}

// The bulk's launch order (SRG_OPT_FW_XCD_ORDER): workgroup b runs on XCD b % 8 (round-robin
// dispatch), and row-major order deals consecutive tiles of a block-row -- which share their row
// operand LB[I] -- to 8 different XCDs, so every XCD's L2 fetches nearly every line-buffer tile of
// the pivot.  Here the tiles are sorted along a Z-order (Morton) curve of (I, J) and cut into 8
// contiguous runs, XCD x taking run x: each XCD works on a compact block of the triangle and reads
// only that block's rows and columns of LB.  Slots past a short run hold -1 (skipped).  One list per
// pivot kb without the tiles of lines kb and kb + 1 (the chain's), so the 8 runs stay equal: with
// those tiles returning early inside one list, the XCDs whose blocks hold line kb idled (measured
// 4 % slower than triangle order).
inline uint32_t morton2(uint32_t a, uint32_t b) {
    uint32_t z = 0;
    for (int i = 0; i < 16; ++i) z |= ((a >> i) & 1u) << (2 * i + 1) | ((b >> i) & 1u) << (2 * i);
    return z;
}
inline void xcd_tile_order(const std::vector<int>& own, int nb, std::vector<int>& out, std::vector<int>& off) {
    struct Z {
        uint32_t key;
        int t, I, J;
        bool operator<(const Z& o) const { return key < o.key; }
    };
    std::vector<Z> z(own.size());
    for (size_t i = 0; i < own.size(); ++i) {
        int I, J;
        tri_tile_h(nb, own[i], I, J);
        z[i] = {morton2((uint32_t)I, (uint32_t)J), own[i], I, J};
    }
    std::sort(z.begin(), z.end());
    out.clear();
    off.assign(nb + 1, 0);
    std::vector<int> run;
    for (int kb = 0; kb < nb; ++kb) {
        const int k1 = kb + 1;
        run.clear();
        for (const Z& q : z)
            if (q.I != kb && q.J != kb && q.I != k1 && q.J != k1) run.push_back(q.t);
        const size_t per = (run.size() + 7) / 8, base = out.size();
        out.resize(base + per * 8, -1);
        for (size_t i = 0; i < run.size(); ++i) out[base + (i % per) * 8 + i / per] = run[i];
        off[kb + 1] = (int)out.size();
    }
}

// run_dense's scan groups (host entry): group q of ng scans the source blocks
// [scan_group_cut(q), scan_group_cut(q + 1)) of nblocks.  Bounds on multiples of 8 blocks: every
// XCD gets the same number of blocks per launch (20 blocks = 3/3/3/3/2/2/2/2 ran 33 % long).
// Three groups: half, then all but the last partial 8 blocks, so the loss rows left to ship after
// the last fold are few (C3 40 / 32 / 7 blocks: exposed D2H 1.8 -> 0.8 ms, scan + tail -0.6 ms vs
// thirds, profiles/r02i/scan_cuts.txt)
inline uint32_t scan_group_cut(uint32_t q, uint32_t ng, uint32_t nblocks) {
    if (q == 0) return 0u;
    if (q == ng) return nblocks;
    const uint32_t half = std::min(nblocks, (nblocks / 2 + 4) / 8 * 8), last = (nblocks - 1) / 8 * 8;
    if (ng == 3 && half > 0 && last > half) return q == 1 ? half : last;
    return std::min(nblocks, (nblocks * q / ng + 4) / 8 * 8);
}

// ---- triangular scan (undirected one-rank builds: SRG_OPT_SCAN_MIRROR) ----
// tight_v5 then scans only the (source block c, target tile b) pairs with b >= c; the pairs below
// the diagonal are derived from them (k_pred_mirror).  Its launch unit stays the block of 4 target
// tiles x 8 source blocks that one XCD holds at once (the workgroups of a block share record
// streams and staged rows), so a launch over the source blocks [c0, c1) lists the blocks that touch
// the triangle: descriptor = (index of the 4-tile group) | (index of the 8-source-block group,
// counted from c0) << 16, source groups outermost as in the full launch.  Workgroups of a listed
// block that lie under the diagonal return at once.  The list is padded to a multiple of 8 with
// TRI_PAD: the blocks are dealt to the 8 XCDs in turn.
constexpr uint32_t TRI_PAD = 0xFFFFFFFFu;
inline void tri_scan_blocks(uint32_t c0, uint32_t c1, uint32_t ntiles, std::vector<uint32_t>& out) {
    const size_t base = out.size();
    if (ntiles && c1 > c0)
        for (uint32_t sg = 0; c0 + 8 * sg < c1; ++sg)
            for (uint32_t tb = 0; 4 * tb < ntiles; ++tb)
                if (std::min(4 * tb + 3, ntiles - 1) >= c0 + 8 * sg) out.push_back(tb | sg << 16);
    while ((out.size() - base) % 8) out.push_back(TRI_PAD);
}

// scan-group cut for the triangular scan: source block c scans nblocks - c target tiles, so the
// work of the blocks [0, c) is tri_scan_work(c).  As scan_group_cut, bounds lie on multiples of 8
// blocks (each XCD the same number of source blocks per launch) and the last group is the last
// partial 8 blocks (few loss rows left to ship after the last fold).  Of the blocks before it the
// first group takes half the triangular work (the latency rows hold the link while it scans: C3 24
// of 72 blocks); further groups split the rest evenly by rows -- their scan is cheap, their loss
// rows are what the link waits for.  Each cut rounded to the nearest multiple of 8.
inline uint64_t tri_scan_work(uint32_t c, uint32_t nblocks) { return (uint64_t)c * nblocks - (uint64_t)c * (c ? c - 1 : 0) / 2; }
inline uint32_t scan_group_cut_tri(uint32_t q, uint32_t ng, uint32_t nblocks) {
    if (q == 0) return 0u;
    if (q >= ng) return nblocks;
    const uint32_t last = nblocks ? (nblocks - 1) / 8 * 8 : 0u;
    const bool tail = ng >= 3 && last > 0;       // the last group = the blocks [last, nblocks)
    const uint32_t end = tail ? last : nblocks;  // the blocks the other groups split
    const uint32_t parts = tail ? ng - 1 : ng;
    if (q >= parts) return end;
    const uint64_t want = tri_scan_work(end, nblocks) / 2;
    uint32_t c = 0;
    while (c < end && tri_scan_work(c, nblocks) < want) ++c;
    const uint32_t half = std::min(end, (c + 4) / 8 * 8);
    if (q == 1) return half;
    return std::min(end, half + ((end - half) * (q - 1) / (parts - 1) + 4) / 8 * 8);
}

}  // namespace
