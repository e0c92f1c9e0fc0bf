// route_trees.hip.h -- the route tree of whole source rows, and link loads pushed up those trees
// (srg_route_trees_device, srg_link_loads_trees_device).  A section of routing.hip's translation
// unit, included there after routes.hip.h; not a header to include elsewhere.  From routes.hip.h it
// takes the in-edge list builder with its essential filter (route_prepare(essential), k_rt_csc<.,
// true>, the lists' workspace b_rt_*), RouteIn, RouteState (below_q is set only here),
// route_read_state, rt_sat_add, route_check_table and route_fail_pass0.
//
// For one source s the routes of route_rule.h to all targets form a tree: the tie rule makes every
// route unique, and the route to t through u ends with the route to u.  So one predecessor per
// (s, t) is the whole answer, where routes.hip.h walks every pair back to s on its own.
//
//   1. Essential in-edge lists (k_rt_csc<., true>): the CSC of routes.hip.h, but an arc u -> t is kept
//      only when lat(e) == D[u][t].  A route edge (u, t) is itself a shortest path u -> t: a match has
//      D[s][u] + lat == D[s][t] <= D[s][u] + D[u][t], so lat <= D[u][t], and D[u][t] <= lat because
//      the edge is a path.  On a shortest-path table the filter therefore removes no candidate of
//      any row, and the tie rule's minimum is unchanged.  The filter reads the entries (u, t) of
//      EVERY row an edge starts from, requested or not: it trusts them.  lat(e) < D[u][t] proves
//      the table is not this graph's and is flagged.
//   2. Predecessors (k_rtt_pred): every (row, t) of a batch evaluates route_explains / route_better
//      over t's essential list with a group of G lanes (G = 16: four targets per wave; 64: a wave
//      per target, kept where the lists average 64 entries or more: C3 255 ms against 274 ms),
//      items ordered by row so that consecutive waves share D[s], L[s].
//   3. Hops and first edges (k_rtt_double): pointer doubling per row (route_tree_rule.h), one
//      workgroup per row, the jumps double-buffered in LDS when 2 * 8 * V bytes fit 64 KiB
//      (V <= 4096: no opt-in, two workgroups per CU), in a global scratch row otherwise.
//   4. Loads (k_rtt_push): per row, counts pushed from the deepest level up, one workgroup per row
//      looping over the levels with a barrier between them; level l is complete once level l + 1
//      is done.  A chain has V - 1 levels of V entries each: correct, and slow.
//
// Rows are processed in batches sized by a workspace budget (kRttBudget) or SRG_OPT_ROUTE_TREE_ROWS.
// The workspace is the context's: the lists in b_rt_* (every call rebuilds them under the context's
// lock, so the pairwise calls and these share one set), the trees' own buffers in b_rtt_*; freed by
// srg_destroy.

constexpr size_t kRttBudget = (size_t)4 << 30;  // workspace bytes a batch of rows may take
constexpr uint32_t kRttLdsJumpV = 4096;          // doubling: 16 * V bytes of LDS up to this V
constexpr uint32_t kRttLdsSubV = 8192;           // push: 8 * V bytes of LDS up to this V

// The predecessor of every (row, t) of a batch.  G lanes per target; pe / pv are the batch's rows
// ([rows * V], pv may be null).  The source's column and an unexplained entry get ROUTE_TREE_NONE;
// flag_bad: an unexplained entry is recorded in st->bad_q as (row0 + row) * V + t.
template <int G>
__global__ void __launch_bounds__(256) k_rtt_pred(RouteIn in, const uint32_t* __restrict__ sources, uint32_t row0,
                                                  uint32_t rows, uint32_t* __restrict__ pe, uint32_t* __restrict__ pv,
                                                  int flag_bad, RouteState* st) {
    constexpr uint32_t TPB = 256 / G;  // targets per workgroup step
    const uint32_t V = in.V;
    const uint32_t gl = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    const uint64_t tiles = (V + TPB - 1) / TPB, items = (uint64_t)rows * tiles;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {  // (it, row, s are workgroup-uniform)
        const uint32_t row = (uint32_t)(it / tiles);
        const uint32_t t = (uint32_t)(it - (uint64_t)row * tiles) * TPB + grp;
        const uint32_t s = sources ? sources[row0 + row] : row0 + row;
        if (s >= V) {
            if (threadIdx.x == 0) atomicOr(&st->bad_arg, 1u);
            continue;
        }
        const bool live = t < V && t != s;
        unsigned long long best = ~0ull;  // (edge index << 32) | u: the min is the tie rule's edge with its u
        if (live) {
            const uint64_t d_cur = path_latency(in.tab, s, t);
            const uint32_t l_cur = f32_bits(in.L[(size_t)s * V + t]);
            const uint32_t b = in.off[t], en = in.off[t + 1];
            for (uint32_t k = b + gl; k < en; k += G) {
                // The latency half of route_explains first, on the entry's endpoint and latency alone: it
                // is necessary, and few entries pass it, so the loss gather, the entry's loss and edge
                // index and the fold are left to those (the gathers are what this kernel is made of).
                const uint64_t w = in.cl[k];
                if (w > d_cur) continue;
                const uint32_t u = in.cu[k];
                if (d_cur - w != (u == s ? 0ull : path_latency(in.tab, s, u))) continue;
                const uint32_t e = in.ce[k];
                const RouteLabel lu = route_label(in.tab, in.L, s, u);
                if (route_explains(d_cur, l_cur, lu, w, in.cp[k]) && route_better((uint32_t)(best >> 32), e) == e)
                    best = ((unsigned long long)e << 32) | u;
            }
        }
        for (int off = G / 2; off; off >>= 1) {  // (xor below G stays inside the group)
            const unsigned long long o = __shfl_xor(best, off, 64);
            best = o < best ? o : best;
        }
        if (gl == 0 && t < V) {
            const size_t k = (size_t)row * V + t;
            const bool none = best == ~0ull;
            pe[k] = none ? ROUTE_TREE_NONE : (uint32_t)(best >> 32);
            if (pv) pv[k] = none ? ROUTE_TREE_NONE : (uint32_t)best;
            if (none && live && flag_bad) atomicMin(&st->bad_q, (unsigned long long)(row0 + row) * V + t);
        }
    }
}

extern __shared__ __align__(16) unsigned char rtt_smem[];

// Pointer doubling of one row per workgroup (route_tree_rule.h).  pe / pv: the batch's rows.
// Writes hops / first (either may be null) and, with st, the statistics:
//   counts == null (trees): over every t != s;
//   counts != null (loads): over the nonzero pairs of the row only, which are also the only ones
//   that have to reach s (bad_q, s * V + t) or own a self-loop (noedge_q); rowmax[row] = the
//   deepest nonzero pair, the push's first level.
template <bool LDS>
__global__ void __launch_bounds__(256) k_rtt_double(uint32_t V, const uint32_t* __restrict__ sources, uint32_t row0,
                                                    const uint32_t* __restrict__ pe, const uint32_t* __restrict__ pv,
                                                    unsigned long long* __restrict__ scratch,
                                                    uint32_t* __restrict__ hops, uint32_t* __restrict__ first,
                                                    const unsigned long long* __restrict__ counts,
                                                    const uint32_t* __restrict__ selfedge, uint32_t* __restrict__ rowmax,
                                                    RouteState* st) {
    const uint32_t row = blockIdx.x;
    const uint32_t s = sources ? sources[row0 + row] : row0 + row;
    if (s >= V) return;  // (k_rtt_pred flagged it; workgroup-uniform)
    TreeJump* a = LDS ? (TreeJump*)rtt_smem : (TreeJump*)(scratch + (size_t)row * 2 * V);
    TreeJump* b = a + V;
    const uint32_t* rpe = pe + (size_t)row * V;
    const uint32_t* rpv = pv + (size_t)row * V;
    for (uint32_t t = threadIdx.x; t < V; t += blockDim.x) a[t] = tree_jump_init(t, s, rpv[t]);
    __syncthreads();
    // D[s][.] falls strictly along the predecessors, so they hold no cycle and ceil(log2 V) rounds
    // suffice; the cap only bounds the loop
    for (int round = 0; round < 32; ++round) {
        int moved = 0;
        for (uint32_t t = threadIdx.x; t < V; t += blockDim.x) {
            const TreeJump me = a[t];
            const TreeJump nx = tree_jump_step(me, a[me.up]);
            moved |= tree_jump_moved(me, nx);
            b[t] = nx;
        }
        TreeJump* sw = a;
        a = b;
        b = sw;
        if (!__syncthreads_or(moved)) break;  // (the barrier also orders this round's writes before the next reads)
    }
    unsigned long long tot = 0, bad = ~0ull, noedge = ~0ull;
    uint32_t hmax = 0;
    for (uint32_t t = threadIdx.x; t < V; t += blockDim.x) {
        const TreeJump j = a[t];
        const uint32_t h = t == s ? 0u : tree_hops(j);
        if (hops) hops[(size_t)row * V + t] = h;
        if (first) first[(size_t)row * V + t] = t == s ? ROUTE_TREE_NONE : rpe[j.up];
        if (!counts) {
            tot += h;
            hmax = max(hmax, h);
        } else if (counts[(size_t)s * V + t] != 0) {
            if (t == s) {
                if (selfedge[s] == ROUTE_NO_EDGE) noedge = (unsigned long long)s * V + s;
                tot += 1;
                hmax = max(hmax, 1u);
            } else if (!tree_root_reaches(j, s, rpv[j.up])) {
                bad = min(bad, (unsigned long long)s * V + t);
            } else {
                tot += h;
                hmax = max(hmax, h);
            }
        }
    }
    for (int off = 32; off; off >>= 1) {
        tot += __shfl_xor(tot, off, 64);
        hmax = max(hmax, (uint32_t)__shfl_xor(hmax, off, 64));
        bad = min(bad, (unsigned long long)__shfl_xor(bad, off, 64));
        noedge = min(noedge, (unsigned long long)__shfl_xor(noedge, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (rowmax && hmax) atomicMax(&rowmax[row], hmax);
        if (st) {
            if (tot) atomicAdd(&st->total, tot);
            if (hmax) atomicMax(&st->max_hops, hmax);
            if (bad != ~0ull) atomicMin(&st->bad_q, bad);
            if (noedge != ~0ull) atomicMin(&st->noedge_q, noedge);
        }
    }
}

// nonzero entries per row of the counts table, and their total
__global__ void __launch_bounds__(256) k_rtt_row_nnz(const unsigned long long* __restrict__ counts, uint32_t V,
                                                     uint32_t* __restrict__ rownnz, unsigned long long* total) {
    for (uint32_t s = blockIdx.x; s < V; s += gridDim.x) {
        uint32_t c = 0;
        for (uint32_t t = threadIdx.x; t < V; t += blockDim.x) c += counts[(size_t)s * V + t] != 0;
        for (int off = 32; off; off >>= 1) c += __shfl_xor(c, off, 64);
        if ((threadIdx.x & 63) == 0 && c) {
            atomicAdd(&rownnz[s], c);
            atomicAdd(total, (unsigned long long)c);
        }
    }
}

struct RttRowActive {
    const uint32_t* n;
    __host__ __device__ bool operator()(uint32_t s) const { return n[s] != 0; }
};

// The push of one validated row per workgroup: sub[t] = the row's count of t, then level by level
// from the deepest, sub[t] goes to the edge into t and to t's parent (saturating, rt_sat_add's
// scheme on both).  Only vertices with a nonzero subtree are touched, and those are explained.
template <bool LDS>
__global__ void __launch_bounds__(256) k_rtt_push(uint32_t V, const uint32_t* __restrict__ sources, uint32_t row0,
                                                  const uint32_t* __restrict__ pe, const uint32_t* __restrict__ pv,
                                                  const uint32_t* __restrict__ hops, const uint32_t* __restrict__ rowmax,
                                                  unsigned long long* __restrict__ scratch,
                                                  const unsigned long long* __restrict__ counts,
                                                  const uint32_t* __restrict__ selfedge, uint64_t E,
                                                  unsigned long long* __restrict__ loads) {
    const uint32_t row = blockIdx.x;
    const uint32_t s = sources[row0 + row];
    unsigned long long* sub = LDS ? (unsigned long long*)rtt_smem : scratch + (size_t)row * 2 * V;
    const uint32_t* rpe = pe + (size_t)row * V;
    const uint32_t* rpv = pv + (size_t)row * V;
    const uint32_t* rh = hops + (size_t)row * V;
    for (uint32_t t = threadIdx.x; t < V; t += blockDim.x) {
        const unsigned long long c = counts[(size_t)s * V + t];
        sub[t] = t == s ? 0ull : c;
        if (t == s && c) {
            const uint32_t e = selfedge[s];
            if (e < E) rt_sat_add(&loads[e], c);  // (validated: the self-loop exists)
        }
    }
    __syncthreads();
    for (uint32_t lvl = rowmax[row]; lvl >= 1; --lvl) {
        for (uint32_t t = threadIdx.x; t < V; t += blockDim.x) {
            if (rh[t] != lvl) continue;
            const unsigned long long c = sub[t];
            const uint32_t e = rpe[t];
            if (c == 0 || e >= E) continue;  // (a nonzero subtree is explained: e is an edge)
            rt_sat_add(&loads[e], c);
            if (lvl > 1) rt_sat_add(&sub[rpv[t]], c);
        }
        __syncthreads();
    }
}

// ---- host side --------------------------------------------------------------------------------
// rows per batch: the option, or what the budget allows of rows that take `row_bytes` each
uint32_t rtt_batch_rows(const srg_ctx& c, uint32_t rows, size_t row_bytes) {
    uint64_t r = c.route_tree_rows > 0 ? (uint64_t)c.route_tree_rows : kRttBudget / std::max<size_t>(row_bytes, 1);
    r = std::min<uint64_t>(r, 0x40000000ull);  // (one workgroup per row: the grid's x dimension)
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(r, 1), rows);
}

// G: a wave per target where the essential lists average a wave's width or more (V targets, off[V]
// arcs), 16 lanes per target below that; SRG_ROUTE_TREE_GROUP forces either.
void rtt_launch_pred(const RouteIn& in, uint32_t arcs, const uint32_t* sources, uint32_t row0, uint32_t rows,
                     uint32_t* pe, uint32_t* pv, int flag_bad, RouteState* sd, hipStream_t st) {
    const uint32_t V = in.V;
    const int forced = srg_env::route_tree_group();
    const bool wave = forced ? forced == 64 : arcs / V >= 64;
    if (wave) {
        const uint64_t items = (uint64_t)rows * ((V + 3) / 4);
        k_rtt_pred<64><<<(unsigned)std::min<uint64_t>(items, 1u << 20), kThreads, 0, st>>>(in, sources, row0, rows, pe, pv,
                                                                                          flag_bad, sd);
    } else {
        const uint64_t items = (uint64_t)rows * ((V + 15) / 16);
        k_rtt_pred<16><<<(unsigned)std::min<uint64_t>(items, 1u << 20), kThreads, 0, st>>>(in, sources, row0, rows, pe, pv,
                                                                                          flag_bad, sd);
    }
    HIP_CHECK(hipGetLastError());
}

void rtt_launch_double(bool lds, uint32_t V, const uint32_t* sources, uint32_t row0, uint32_t rows, const uint32_t* pe,
                       const uint32_t* pv, unsigned long long* scratch, uint32_t* hops, uint32_t* first,
                       const unsigned long long* counts, const uint32_t* self, uint32_t* rowmax, RouteState* sd,
                       hipStream_t st) {
    if (lds)
        k_rtt_double<true><<<rows, kThreads, (size_t)V * 16, st>>>(V, sources, row0, pe, pv, nullptr, hops, first, counts,
                                                                  self, rowmax, sd);
    else
        k_rtt_double<false><<<rows, kThreads, 0, st>>>(V, sources, row0, pe, pv, scratch, hops, first, counts, self,
                                                      rowmax, sd);
    HIP_CHECK(hipGetLastError());
}

void route_trees_device(srg_ctx& c, const srg_edge_list* g, const srg_path_table_dev* t, const uint32_t* sources,
                        uint32_t ns, uint32_t* out_pe, uint32_t* out_pv, uint32_t* out_hops, uint32_t* out_first,
                        hipStream_t st, srg_route_result* res) {
    if (res) *res = srg_route_result{0, 0, UINT64_MAX, 0, 0, 0.0};
    route_check_table(g, t);
    const uint32_t V = g->num_vertices;
    if (ns == 0) return;
    if (!out_pe) fail(SRG_ERR_ARG, "null argument");
    if (V == 0 || (!sources && ns > V)) fail(SRG_ERR_ARG, "source index out of range (>= n)");
    if (res) res->num_pairs = (uint64_t)ns * (V - 1);
    const RoutePrep prep = route_prepare(c, g, t, true, st);
    const RouteIn& in = prep.in;
    RouteState* sd = prep.state_dev;
    const uint32_t arcs = prep.arcs;
    const unsigned long long below = prep.counted.below_q;
    if (below != ~0ull) {
        if (res) res->bad_pair = below;
        fail(SRG_ERR_ROUTE, "an edge from node index " + std::to_string(below / V) + " to " + std::to_string(below % V) +
                                " is shorter than the table entry of that pair (entry " + std::to_string(below) +
                                "): the table is not a shortest-path table of this graph");
    }
    const bool lds = V <= srg_env::route_tree_lds_max_v(kRttLdsJumpV);
    const size_t row_bytes = (size_t)V * ((out_pv ? 0 : 4) + (lds ? 0 : 16));
    const uint32_t R = rtt_batch_rows(c, ns, row_bytes);
    uint32_t* ws_pv = out_pv ? nullptr : (uint32_t*)c.b_rtt_pv.get((size_t)R * V * 4);
    unsigned long long* scr = lds ? nullptr : (unsigned long long*)c.b_rtt_scr.get((size_t)R * V * 16);
    for (uint32_t r0 = 0; r0 < ns; r0 += R) {
        const uint32_t rows = std::min(R, ns - r0);
        const size_t o = (size_t)r0 * V;
        uint32_t* pv = out_pv ? out_pv + o : ws_pv;
        rtt_launch_pred(in, arcs, sources, r0, rows, out_pe + o, pv, 1, sd, st);
        rtt_launch_double(lds, V, sources, r0, rows, out_pe + o, pv, scr, out_hops ? out_hops + o : nullptr,
                          out_first ? out_first + o : nullptr, nullptr, in.selfedge, nullptr, sd, st);
    }
    const RouteState s = route_read_state(sd, st);
    if (s.bad_arg) fail(SRG_ERR_ARG, "source index out of range (>= n)");
    if (s.bad_q != ~0ull) {
        const uint64_t i = s.bad_q / V;
        uint32_t src = (uint32_t)i;
        if (sources) {
            HIP_CHECK(hipMemcpyAsync(&src, sources + i, 4, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        if (res) res->bad_pair = s.bad_q;
        fail(SRG_ERR_ROUTE, "no in-edge explains the table entry of the path from node index " + std::to_string(src) +
                                " to " + std::to_string(s.bad_q % V) + " (row entry " + std::to_string(s.bad_q) +
                                "): the table is not a shortest-path table of this graph");
    }
    if (res) {
        res->total_hops = s.total;
        res->max_hops = s.max_hops;
    }
}

void link_loads_trees_device(srg_ctx& c, const srg_edge_list* g, const srg_path_table_dev* t, const uint64_t* counts,
                             uint64_t* loads, hipStream_t st, srg_route_result* res) {
    if (res) *res = srg_route_result{0, 0, UINT64_MAX, 0, 0, 0.0};
    route_check_table(g, t);
    const uint32_t V = g->num_vertices;
    if (V == 0) return;
    const unsigned long long* cnt = (const unsigned long long*)counts;
    // the rows that hold a nonzero count, in order
    uint32_t* rownnz = (uint32_t*)c.b_rtt_rownnz.get((size_t)V * 4);
    uint32_t* active = (uint32_t*)c.b_rtt_active.get((size_t)V * 4);
    unsigned long long* nsel = (unsigned long long*)c.b_rtt_nsel.get(16);
    HIP_CHECK(hipMemsetAsync(rownnz, 0, (size_t)V * 4, st));
    HIP_CHECK(hipMemsetAsync(nsel, 0, 16, st));
    k_rtt_row_nnz<<<std::min<uint32_t>(V, 1u << 16), kThreads, 0, st>>>(cnt, V, rownnz, nsel);
    HIP_CHECK(hipGetLastError());
    hipcub::CountingInputIterator<uint32_t> first(0u);
    uint32_t* nact_dev = (uint32_t*)(nsel + 1);
    size_t sb = 0;
    HIP_CHECK(hipcub::DeviceSelect::If(nullptr, sb, first, active, nact_dev, (int)V, RttRowActive{rownnz}, st));
    void* stmp = c.b_rt_tmp.get(sb);
    HIP_CHECK(hipcub::DeviceSelect::If(stmp, sb, first, active, nact_dev, (int)V, RttRowActive{rownnz}, st));
    unsigned long long head[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(head, nsel, 16, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long nnz = head[0];
    const uint32_t A = (uint32_t)head[1];
    if (res) res->num_pairs = nnz;
    if (nnz == 0) return;

    // (the push's global sub rows live in the doubling scratch: lds_sub wherever lds_jump)
    const bool lds_jump = V <= srg_env::route_tree_lds_max_v(kRttLdsJumpV);
    const bool lds_sub = lds_jump || V <= srg_env::route_tree_lds_max_v(kRttLdsSubV);
    const size_t row_bytes = (size_t)V * (12 + (lds_jump ? 0 : 16)) + 4;
    const uint32_t R = rtt_batch_rows(c, A, row_bytes);
    const bool keep = R >= A;  // one batch: the validated predecessors and hops stay for the commit
    uint32_t* pe = (uint32_t*)c.b_rtt_pe.get((size_t)R * V * 4);
    uint32_t* pv = (uint32_t*)c.b_rtt_pv.get((size_t)R * V * 4);
    uint32_t* hops = (uint32_t*)c.b_rtt_hops.get((size_t)R * V * 4);
    uint32_t* rowmax = (uint32_t*)c.b_rtt_rowmax.get((size_t)R * 4);
    unsigned long long* scr = lds_jump ? nullptr : (unsigned long long*)c.b_rtt_scr.get((size_t)R * V * 16);
    auto trees = [&](const RoutePrep& p, uint32_t r0, uint32_t rows, RouteState* sd) {
        const RouteIn& in = p.in;
        HIP_CHECK(hipMemsetAsync(rowmax, 0, (size_t)rows * 4, st));
        rtt_launch_pred(in, p.arcs, active, r0, rows, pe, pv, 0, sd, st);
        rtt_launch_double(lds_jump, V, active, r0, rows, pe, pv, scr, hops, nullptr, cnt, in.selfedge, rowmax, sd, st);
    };
    // The essential lists first.  Where they cannot stand for the full lists -- an edge below its
    // entry, or a nonzero pair they leave unexplained -- the full lists decide, so that this call
    // fails exactly where the pairwise walk does.
    for (int filter = 1; filter >= 0; --filter) {
        const RoutePrep prep = route_prepare(c, g, t, filter != 0, st);
        const RouteIn& in = prep.in;
        RouteState* sd = prep.state_dev;
        if (filter && prep.counted.below_q != ~0ull) continue;
        // validate every batch, then commit
        for (uint32_t r0 = 0; r0 < A; r0 += R) trees(prep, r0, std::min(R, A - r0), sd);
        const RouteState s = route_read_state(sd, st);
        if (filter && s.bad_q != ~0ull) continue;
        if (s.noedge_q != ~0ull || s.bad_q != ~0ull) {
            const uint64_t q = std::min(s.noedge_q, s.bad_q);
            route_fail_pass0(s, g, (uint32_t)(q / V), s.bad_q / V, s.bad_q % V, "pair", st, res);
        }
        if (res) {
            res->total_hops = s.total;
            res->max_hops = s.max_hops;
        }
        for (uint32_t r0 = 0; r0 < A; r0 += R) {
            const uint32_t rows = std::min(R, A - r0);
            if (!keep) trees(prep, r0, rows, nullptr);
            if (lds_sub)
                k_rtt_push<true><<<rows, kThreads, (size_t)V * 8, st>>>(V, active, r0, pe, pv, hops, rowmax, nullptr, cnt,
                                                                       in.selfedge, g->num_edges,
                                                                       (unsigned long long*)loads);
            else
                k_rtt_push<false><<<rows, kThreads, 0, st>>>(V, active, r0, pe, pv, hops, rowmax, scr, cnt, in.selfedge,
                                                            g->num_edges, (unsigned long long*)loads);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipStreamSynchronize(st));
        return;
    }
}
