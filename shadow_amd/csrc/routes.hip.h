// routes.hip.h -- the routes a finished table's paths take, and per-edge packet loads
// (srg_trace_routes_device, srg_link_loads_device).  A section of routing.hip's translation unit,
// included there after sparse_run.hip.h (it uses srg_ctx, DevBuf, DevGraph, fail, grid_for from the
// text above it); not a header to include elsewhere.
//
// The reference keeps no routes (petgraph's dijkstra returns scores only, mod.rs:190-208).  They are
// read back from the table alone with the rule of route_rule.h: walk from t towards s, at each
// vertex `cur` pick the in-edge (u, cur) with D[s][u] + lat == D[s][cur] and
// bits(fold(L[s][u], loss)) == bits(L[s][cur]), smallest edge index among the matches.  Nothing of
// the build is used (no PRED buffer), so a table of the dense or the sparse build, in u64 or key
// form, from one rank or many, is walked the same way.
//
// In-edge lists (CSC) are built PER CALL from graph_dev: count, exclusive scan, fill; both
// orientations of an undirected edge, self-loops left out.  Not cached: a cache keyed by the edge
// arrays' pointers and counts cannot see an edge list rewritten in place (or a freed allocation
// handed out again at the same address), and a stale list would name wrong edges silently.  The
// fill order is whatever the atomics give; the walk min-reduces the edge index over all matches,
// so it does not matter.  The workspace is the context's (b_rt_*), freed by srg_destroy.
// route_trees.hip.h builds its lists here too: route_prepare(essential = true) keeps only the arcs
// with lat(e) == D[u][t] (k_rt_csc<., true>) and reports an arc below its entry in
// RouteState::below_q; the pairwise calls below never ask for that and never set below_q.
//
// The walk: one wave64 per query pair; the lanes stride the in-edge list of `cur` in chunks of 64,
// each gathers D[s][u], L[s][u], reads the entry's lat(e), loss(e) and evaluates the rule; a wave
// min over the edge index picks the edge, a ballot finds the lane that holds it and the wave steps
// to its u.  Pass 0
// counts the hops per pair (and validates: nothing is committed before every pair is explained),
// a scan turns the counts into offsets, pass 1 walks again and writes each route in s -> t order
// (pass 2, loads: adds the pair's count to every edge of its route).  D[s][.] falls strictly along
// the walk (latencies >= 1, checked), so it ends; a hop cap of V turns anything else into an error.

struct RouteState {
    unsigned long long bad_q;     // first query no in-edge explains (loads: s * n + t; trees: row * n + t); ~0 = none
    unsigned long long noedge_q;  // first diagonal query whose vertex has no self-loop; ~0 = none
    unsigned long long below_q;   // essential lists: smallest u * n + t of an arc with lat(e) < D[u][t]; ~0 = none
    unsigned long long total;     // sum of route lengths
    uint32_t max_hops;
    uint32_t bad_arg;             // a query (trees: source) index >= n
    uint32_t bad_edge;            // bit 0: an endpoint >= V; bit 1: a non-self-loop edge of latency 0
    uint32_t pad;
};
constexpr RouteState kRouteStateInit{~0ull, ~0ull, ~0ull, 0ull, 0u, 0u, 0u, 0u};

struct RouteIn {
    const uint32_t* off;       // [V + 1] in-edge list bounds
    const uint32_t* ce;        // [arcs] edge index
    const uint32_t* cu;        // [arcs] the edge's other endpoint
    const uint64_t* cl;        // [arcs] the edge's latency and loss, copied beside it: a list is read in
    const float* cp;           //        sequence, where lat[e] / loss[e] would be one cache line per entry
    const uint32_t* selfedge;  // [V] smallest self-loop edge index, ROUTE_NO_EDGE = none
    PathLatency tab;
    const float* L;            // [V x V] table loss
    uint32_t V;
};

// ctr[key] += 1 for every active lane of the wave, one atomic per run of equal keys in consecutive
// lanes (a GML edge list is ordered by source: 64 same-address atomics otherwise serialise at the
// memory side).  Returns the lane's slot: the counter's old value plus its rank in the run.  Every
// lane of the wave calls it.
__device__ __forceinline__ uint32_t rt_run_add(uint32_t* __restrict__ ctr, uint32_t key, bool active) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t k = active ? key : 0xFFFFFFFFu;  // (keys are vertex indices < V <= 2^32 - 1)
    const uint32_t prev = __shfl_up(k, 1, 64);
    const bool head = lane == 0 || prev != k;
    const unsigned long long hm = __ballot(head);
    const int hl = 63 - __clzll((long long)(hm & (~0ull >> (63 - lane))));  // my run's first lane
    const unsigned long long above = hl == 63 ? 0ull : hm & (~0ull << (hl + 1));
    const int end = above ? __ffsll((long long)above) - 1 : 64;
    uint32_t base = 0;
    if (head && active) base = atomicAdd(&ctr[key], (uint32_t)(end - hl));
    base = __shfl(base, hl, 64);
    return base + (lane - (uint32_t)hl);
}

// The in-edges as route_in_edge (route_rule.h) defines them: an edge (s, t), s != t, is an in-edge
// of t from s and, undirected, of s from t.
// FILL = false: in-degrees into ctr, the smallest self-loop index per vertex, the edge checks.
// FILL = true: ctr holds the list starts; every arc takes a slot.  (Run only after the checks of
// the first pass passed: every endpoint is < V and the slots are the counted ones.)
// ESSENTIAL (route_trees.hip.h): an arc u -> t is kept only when lat(e) == D[u][t], each orientation
// of an undirected edge tested on its own (the same predicate in both passes, so the same counts);
// the first pass flags lat(e) < D[u][t] in below_q.  ESSENTIAL = false reads no table entry.
template <bool FILL, bool ESSENTIAL>
__global__ void __launch_bounds__(256) k_rt_csc(uint64_t E, const uint32_t* __restrict__ src,
                                                const uint32_t* __restrict__ dst, const uint64_t* __restrict__ lat,
                                                const float* __restrict__ loss, int directed, uint32_t V,
                                                uint32_t* __restrict__ ctr, uint32_t* __restrict__ ce,
                                                uint32_t* __restrict__ cu, uint64_t* __restrict__ cl, float* __restrict__ cp,
                                                uint32_t* __restrict__ selfedge, RouteState* st, PathLatency tab) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    uint32_t bad = 0;
    unsigned long long below = ~0ull;
    // whole waves stay in the loop together (rt_run_add needs every lane)
    for (size_t e0 = blockIdx.x * (size_t)blockDim.x + (threadIdx.x & ~63u); e0 < E; e0 += stride) {
        const size_t e = e0 + lane;
        const bool in = e < E;
        const uint32_t s = in ? src[e] : 0u, t = in ? dst[e] : 0u;
        const bool ok = in && s < V && t < V;
        const bool arc = ok && s != t;
        const uint64_t w = arc ? lat[e] : 0;
        const float pl = FILL && arc ? loss[e] : 0.0f;
        if (!FILL) {
            if (in && !ok) bad |= 1u;
            if (arc && w == 0) bad |= 2u;
            if (ok && s == t) atomicMin(&selfedge[s], (uint32_t)e);
        }
        bool keep = arc;
        if (ESSENTIAL && arc) {
            const uint64_t d = path_latency(tab, s, t);
            keep = w == d;
            if (!FILL && w < d) below = min(below, (unsigned long long)s * V + t);
        }
        uint32_t p = rt_run_add(ctr, t, keep);
        if (FILL && keep) {
            ce[p] = (uint32_t)e;
            cu[p] = s;
            cl[p] = w;
            cp[p] = pl;
        }
        if (!directed) {
            keep = arc;
            if (ESSENTIAL && arc) {
                const uint64_t d = path_latency(tab, t, s);
                keep = w == d;
                if (!FILL && w < d) below = min(below, (unsigned long long)t * V + s);
            }
            p = rt_run_add(ctr, s, keep);
            if (FILL && keep) {
                ce[p] = (uint32_t)e;
                cu[p] = t;
                cl[p] = w;
                cp[p] = pl;
            }
        }
    }
    if (!FILL) {
        if (bad) atomicOr(&st->bad_edge, bad);
        if (ESSENTIAL && below != ~0ull) atomicMin(&st->below_q, below);
    }
}

__global__ void k_rt_iota(uint32_t* __restrict__ p, uint64_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        p[i] = (uint32_t)i;
}

__global__ void k_rt_count_nonzero(const unsigned long long* __restrict__ a, size_t count, unsigned long long* out) {
    unsigned long long c = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        c += a[i] != 0;
    for (int off = 32; off; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

struct RtNonZero {
    const unsigned long long* c;
    __host__ __device__ bool operator()(unsigned long long i) const { return c[i] != 0; }
};

// saturating 64-bit add, the scheme of k_ev_counts (events.hip.h): an add whose returned old value
// shows a wrap is followed by an atomic max to all-ones
__device__ __forceinline__ void rt_sat_add(unsigned long long* p, unsigned long long c) {
    const unsigned long long old = atomicAdd(p, c);
    if (old + c < old) atomicMax(p, ~0ull);
}

// MODE 0: count the hops of every query into hops[q] (when given) and the state; flag what cannot
//         be walked.  Writes no output.
// MODE 1: write each route's edges (and arrival vertices) in s -> t order at offs[q].
// MODE 2: add counts[q] to loads[e] for every edge of the route.
// Queries: pairs[i] = s * V + t (loads; q = the pair), else (qs[q], qt[q]) with q = perm[i] (the
// queries ordered by source: the rows D[s], L[s] are what consecutive waves share) or q = i.
template <int MODE>
__global__ void __launch_bounds__(256) k_rt_walk(RouteIn in, uint64_t nq, const uint32_t* __restrict__ qs,
                                                 const uint32_t* __restrict__ qt, const uint32_t* __restrict__ perm,
                                                 const unsigned long long* __restrict__ pairs,
                                                 unsigned long long* __restrict__ hops,
                                                 const unsigned long long* __restrict__ offs,
                                                 uint32_t* __restrict__ out_edge, uint32_t* __restrict__ out_vertex,
                                                 const unsigned long long* __restrict__ counts,
                                                 unsigned long long* __restrict__ loads, RouteState* st) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t V = in.V;
    unsigned long long tot = 0;
    uint32_t hmax = 0;
    for (uint64_t i = wave; i < nq; i += nwaves) {  // (i, q, s, t are wave-uniform)
        unsigned long long q;
        uint32_t s, t;
        if (pairs) {
            q = pairs[i];
            s = (uint32_t)(q / V);
            t = (uint32_t)(q - (unsigned long long)s * V);
        } else {
            q = perm ? perm[i] : i;
            s = qs[q];
            t = qt[q];
        }
        if (s >= V || t >= V) {
            if (MODE == 0 && lane == 0) atomicOr(&st->bad_arg, 1u);
            continue;
        }
        const unsigned long long H = MODE == 1 ? hops[q] : 0ull, base = MODE == 1 ? offs[q] : 0ull;
        const unsigned long long cnt = MODE == 2 ? counts[q] : 0ull;
        uint32_t h = 0;
        bool okq = true;
        if (s == t) {
            // the route s -> s is the self-loop of s (mod.rs:210-217)
            const uint32_t e = in.selfedge[s];
            if (e == ROUTE_NO_EDGE) {
                if (MODE == 0 && lane == 0) atomicMin(&st->noedge_q, q);
                continue;
            }
            if (lane == 0) {
                if (MODE == 1 && H == 1) {
                    out_edge[base] = e;
                    if (out_vertex) out_vertex[base] = s;
                }
                if (MODE == 2) rt_sat_add(&loads[e], cnt);
            }
            h = 1;
        } else {
            uint32_t cur = t;
            while (cur != s) {
                if (h >= V) {  // cannot happen while D falls strictly; never a spin
                    okq = false;
                    break;
                }
                const uint64_t d_cur = path_latency(in.tab, s, cur);
                const uint32_t l_cur = f32_bits(in.L[(size_t)s * V + cur]);
                uint32_t best = ROUTE_NO_EDGE, best_u = 0;
                const uint32_t b = in.off[cur], en = in.off[cur + 1];
                for (uint32_t k = b + lane; k < en; k += 64) {
                    const uint32_t e = in.ce[k], u = in.cu[k];
                    const RouteLabel lu = route_label(in.tab, in.L, s, u);
                    if (route_explains(d_cur, l_cur, lu, in.cl[k], in.cp[k]) && route_better(best, e) != best) {
                        best = e;
                        best_u = u;
                    }
                }
                uint32_t m = best;
                for (int off = 32; off; off >>= 1) m = route_better(m, __shfl_xor(m, off, 64));
                if (m == ROUTE_NO_EDGE) {
                    okq = false;
                    break;
                }
                // an edge is in cur's list once: exactly one lane holds it
                const int owner = __ffsll((long long)__ballot(best == m)) - 1;
                const uint32_t u = __shfl(best_u, owner, 64);
                if (lane == 0) {
                    if (MODE == 1 && h < H) {
                        const unsigned long long pos = base + (H - 1 - h);  // walked t -> s, stored s -> t
                        out_edge[pos] = m;
                        if (out_vertex) out_vertex[pos] = cur;
                    }
                    if (MODE == 2) rt_sat_add(&loads[m], cnt);
                }
                cur = u;
                ++h;
            }
        }
        if (!okq) {
            if (MODE == 0 && lane == 0) atomicMin(&st->bad_q, q);
            continue;
        }
        if (MODE == 0) {
            if (hops && lane == 0) hops[q] = h;
            tot += h;
            hmax = h > hmax ? h : hmax;
        }
    }
    if (MODE == 0 && lane == 0) {
        if (tot) atomicAdd(&st->total, tot);
        if (hmax) atomicMax(&st->max_hops, hmax);
    }
}

// ---- host side --------------------------------------------------------------------------------
void route_check_table(const srg_edge_list* g, const srg_path_table_dev* t) {
    if (t->n != g->num_vertices)
        fail(SRG_ERR_ARG, "path table: n must equal num_vertices (the table of every vertex in NodeIndex order)");
    if (!t->latency_ns == !t->latency_key)
        fail(SRG_ERR_ARG, "path table: exactly one of latency_ns and latency_key must be given");
    if (t->latency_key && (!t->diag_ns || t->unit_ns < 1))
        fail(SRG_ERR_ARG, "path table: latency_key needs diag_ns and unit_ns >= 1");
    if (!t->packet_loss) fail(SRG_ERR_ARG, "path table: packet_loss is required");
    if (g->num_edges && (!g->src || !g->dst || !g->latency_ns || !g->packet_loss)) fail(SRG_ERR_ARG, "null argument");
    if (g->num_edges >= 0xFFFFFFFFull || g->num_edges * (g->directed ? 1 : 2) >= 0xFFFFFFFFull)
        fail(SRG_ERR_ARG, "graph too large for u32 edge indices (arcs >= 2^32 - 1)");
}

// The edge checks and the in-edge lists of this call's graph (V >= 1), the essential ones when
// `essential`.  Synchronises once, after the counting pass; returns with the lists queued on st.
struct RoutePrep {
    RouteIn in;
    RouteState* state_dev;  // the call's RouteState (reset before the counting pass)
    RouteState counted;     // its value after the counting pass: bad_edge (checked here), below_q
    uint32_t arcs;
};

template <bool FILL>
void route_launch_csc(bool essential, const srg_edge_list* g, const PathLatency& tab, uint32_t* ctr, uint32_t* ce,
                      uint32_t* cu, uint64_t* cl, float* cp, uint32_t* self, RouteState* sd, hipStream_t st) {
    const uint64_t E = g->num_edges;
    if (essential)
        k_rt_csc<FILL, true><<<grid_for(E, 2048), kThreads, 0, st>>>(E, g->src, g->dst, g->latency_ns, g->packet_loss,
                                                                    (int)g->directed, g->num_vertices, ctr, ce, cu, cl, cp,
                                                                    self, sd, tab);
    else
        k_rt_csc<FILL, false><<<grid_for(E, 2048), kThreads, 0, st>>>(E, g->src, g->dst, g->latency_ns, g->packet_loss,
                                                                     (int)g->directed, g->num_vertices, ctr, ce, cu, cl, cp,
                                                                     self, sd, tab);
    HIP_CHECK(hipGetLastError());
}

RoutePrep route_prepare(srg_ctx& c, const srg_edge_list* g, const srg_path_table_dev* t, bool essential,
                        hipStream_t st) {
    const uint32_t V = g->num_vertices;
    const uint64_t E = g->num_edges;
    const PathLatency tab{t->latency_ns, t->latency_key, t->diag_ns, t->unit_ns, t->n};
    uint32_t* off = (uint32_t*)c.b_rt_off.get(((size_t)V + 1) * 4);
    uint32_t* cur = (uint32_t*)c.b_rt_cur.get(((size_t)V + 1) * 4);
    uint32_t* self = (uint32_t*)c.b_rt_self.get((size_t)V * 4);
    RouteState* sd = (RouteState*)c.b_rt_state.get(sizeof(RouteState));
    HIP_CHECK(hipMemcpyAsync(sd, &kRouteStateInit, sizeof(RouteState), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(cur, 0, ((size_t)V + 1) * 4, st));
    HIP_CHECK(hipMemsetAsync(self, 0xFF, (size_t)V * 4, st));
    if (E) route_launch_csc<false>(essential, g, tab, cur, nullptr, nullptr, nullptr, nullptr, self, sd, st);
    size_t tb = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cur, off, (int)(V + 1), st));
    void* tmp = c.b_rt_tmp.get(tb);
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cur, off, (int)(V + 1), st));
    RoutePrep p{};
    HIP_CHECK(hipMemcpyAsync(&p.counted, sd, sizeof(RouteState), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&p.arcs, off + V, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (p.counted.bad_edge & 1) fail(SRG_ERR_ARG, "edge endpoint out of range (>= num_vertices)");
    if (p.counted.bad_edge & 2)
        fail(SRG_ERR_ARG, "an edge between two vertices has latency 0 (the walk's termination rests on latencies >= 1)");
    uint32_t* ce = (uint32_t*)c.b_rt_ce.get((size_t)p.arcs * 4);
    uint32_t* cu = (uint32_t*)c.b_rt_cu.get((size_t)p.arcs * 4);
    uint64_t* cl = (uint64_t*)c.b_rt_cl.get((size_t)p.arcs * 8);
    float* cp = (float*)c.b_rt_cp.get((size_t)p.arcs * 4);
    if (p.arcs) {
        HIP_CHECK(hipMemcpyAsync(cur, off, ((size_t)V + 1) * 4, hipMemcpyDeviceToDevice, st));
        route_launch_csc<true>(essential, g, tab, cur, ce, cu, cl, cp, self, sd, st);
    }
    p.in = RouteIn{off, ce, cu, cl, cp, self, tab, t->packet_loss, V};
    p.state_dev = sd;
    return p;
}

RouteState route_read_state(RouteState* sd, hipStream_t st) {
    RouteState s;
    HIP_CHECK(hipMemcpyAsync(&s, sd, sizeof(RouteState), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return s;
}

unsigned route_walk_grid(uint64_t nq) {  // 4 waves (queries) per workgroup, at most 8 workgroups per CU
    const uint64_t g = (nq + 3) / 4;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(g, 1), 2048);
}

// what pass 0 refused, in query order: the first of a missing self-loop and an unexplained pair
void route_fail_pass0(const RouteState& s, const srg_edge_list* g, uint32_t ne_vertex, uint64_t bs, uint64_t bt,
                      const char* what, hipStream_t st, srg_route_result* res) {
    if (s.noedge_q < s.bad_q) {
        const DevGraph dg{g->num_vertices, (int)g->directed, g->num_edges, g->src, g->dst, g->latency_ns,
                          g->packet_loss, g->node_ids, nullptr};
        const std::string id = std::to_string(node_gml_id(dg, ne_vertex, st));
        fail(SRG_ERR_NO_EDGE, "No edge connecting node " + id + " to " + id);
    }
    if (res) res->bad_pair = s.bad_q;
    fail(SRG_ERR_ROUTE, "no in-edge explains the table entry of the path from node index " + std::to_string(bs) +
                            " to " + std::to_string(bt) + " (" + what + " " + std::to_string(s.bad_q) +
                            "): the table is not a shortest-path table of this graph");
}

void trace_routes_device(srg_ctx& c, const srg_edge_list* g, const srg_path_table_dev* t, const uint32_t* qs,
                         const uint32_t* qt, uint64_t nq, uint64_t cap, uint64_t* out_off, uint32_t* out_edge,
                         uint32_t* out_vertex, hipStream_t st, srg_route_result* res) {
    if (res) *res = srg_route_result{nq, 0, UINT64_MAX, 0, 0, 0.0};
    route_check_table(g, t);
    if (nq >= 0x7FFFFFFFull) fail(SRG_ERR_ARG, "too many query pairs (>= 2^31 - 1)");
    const uint32_t V = g->num_vertices;
    unsigned long long* hops = (unsigned long long*)c.b_rt_hops.get((nq + 1) * 8);
    unsigned long long* offs = (unsigned long long*)c.b_rt_offs.get((nq + 1) * 8);
    HIP_CHECK(hipMemsetAsync(hops, 0, (nq + 1) * 8, st));
    if (V == 0 && nq) fail(SRG_ERR_ARG, "query index out of range (>= n)");
    RouteState s = kRouteStateInit;
    RouteIn in{};
    RouteState* sd = nullptr;
    const uint32_t* perm = nullptr;
    if (nq) {
        const RoutePrep prep = route_prepare(c, g, t, false, st);
        in = prep.in;
        sd = prep.state_dev;
        if (nq > 1) {
            // the queries in source order (stable: equal sources keep the caller's order)
            uint32_t* idx = (uint32_t*)c.b_rt_idx.get(nq * 4);
            uint32_t* pm = (uint32_t*)c.b_rt_perm.get(nq * 4);
            uint32_t* keys = (uint32_t*)c.b_rt_keys.get(nq * 4);
            k_rt_iota<<<grid_for(nq), kThreads, 0, st>>>(idx, nq);
            HIP_CHECK(hipGetLastError());
            size_t sb = 0;
            HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sb, qs, keys, idx, pm, (int)nq, 0, 32, st));
            void* stmp = c.b_rt_tmp.get(sb);
            HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(stmp, sb, qs, keys, idx, pm, (int)nq, 0, 32, st));
            perm = pm;
        }
        k_rt_walk<0><<<route_walk_grid(nq), kThreads, 0, st>>>(in, nq, qs, qt, perm, nullptr, hops, nullptr, nullptr,
                                                              nullptr, nullptr, nullptr, sd);
        HIP_CHECK(hipGetLastError());
    }
    size_t tb = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, hops, offs, (int)(nq + 1), st));
    void* tmp = c.b_rt_tmp.get(tb);
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, hops, offs, (int)(nq + 1), st));
    if (nq) s = route_read_state(sd, st);
    if (s.bad_arg) fail(SRG_ERR_ARG, "query index out of range (>= n)");
    if (s.noedge_q != ~0ull || s.bad_q != ~0ull) {
        const uint64_t q = std::min(s.noedge_q, s.bad_q);
        uint32_t a = 0, b = 0;
        HIP_CHECK(hipMemcpyAsync(&a, qs + q, 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(&b, qt + q, 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        route_fail_pass0(s, g, a, a, b, "query", st, res);
    }
    if (res) {
        res->total_hops = s.total;
        res->max_hops = s.max_hops;
    }
    if (s.total > cap)
        fail(SRG_ERR_ARG, "hop_capacity too small: " + std::to_string(s.total) + " hops needed");
    if (s.total) {
        k_rt_walk<1><<<route_walk_grid(nq), kThreads, 0, st>>>(in, nq, qs, qt, perm, nullptr, hops, offs, out_edge,
                                                              out_vertex, nullptr, nullptr, sd);
        HIP_CHECK(hipGetLastError());
    }
    if (out_off) HIP_CHECK(hipMemcpyAsync(out_off, offs, (nq + 1) * 8, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

void link_loads_device(srg_ctx& c, const srg_edge_list* g, const srg_path_table_dev* t, const uint64_t* counts,
                       uint64_t* loads, hipStream_t st, srg_route_result* res) {
    if (res) *res = srg_route_result{0, 0, UINT64_MAX, 0, 0, 0.0};
    route_check_table(g, t);
    const uint32_t V = g->num_vertices;
    const uint64_t N = (uint64_t)V * V;
    if (N >= 0x7FFFFFFFull) fail(SRG_ERR_ARG, "counts table too large (n * n >= 2^31 - 1)");
    if (N == 0) return;
    const unsigned long long* cnt = (const unsigned long long*)counts;
    const RoutePrep prep = route_prepare(c, g, t, false, st);
    const RouteIn& in = prep.in;
    RouteState* sd = prep.state_dev;
    // the nonzero entries, in row-major order (already grouped by source)
    unsigned long long* nsel = (unsigned long long*)c.b_rt_nsel.get(16);
    HIP_CHECK(hipMemsetAsync(nsel, 0, 16, st));
    k_rt_count_nonzero<<<grid_for(N), kThreads, 0, st>>>(cnt, N, nsel);
    HIP_CHECK(hipGetLastError());
    unsigned long long nnz = 0;
    HIP_CHECK(hipMemcpyAsync(&nnz, nsel, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (res) res->num_pairs = nnz;
    if (nnz == 0) return;
    unsigned long long* pairs = (unsigned long long*)c.b_rt_pairs.get(nnz * 8);
    hipcub::CountingInputIterator<unsigned long long> first(0ull);
    size_t sb = 0;
    HIP_CHECK(hipcub::DeviceSelect::If(nullptr, sb, first, pairs, nsel + 1, (int)N, RtNonZero{cnt}, st));
    void* stmp = c.b_rt_tmp.get(sb);
    HIP_CHECK(hipcub::DeviceSelect::If(stmp, sb, first, pairs, nsel + 1, (int)N, RtNonZero{cnt}, st));
    k_rt_walk<0><<<route_walk_grid(nnz), kThreads, 0, st>>>(in, nnz, nullptr, nullptr, nullptr, pairs, nullptr, nullptr,
                                                           nullptr, nullptr, nullptr, nullptr, sd);
    HIP_CHECK(hipGetLastError());
    const RouteState s = route_read_state(sd, st);
    if (s.noedge_q != ~0ull || s.bad_q != ~0ull) {
        const uint64_t q = std::min(s.noedge_q, s.bad_q);
        route_fail_pass0(s, g, (uint32_t)(q / V), s.bad_q / V, s.bad_q % V, "pair", st, res);
    }
    if (res) {
        res->total_hops = s.total;
        res->max_hops = s.max_hops;
    }
    // every pair is explained: commit
    k_rt_walk<2><<<route_walk_grid(nnz), kThreads, 0, st>>>(in, nnz, nullptr, nullptr, nullptr, pairs, nullptr, nullptr,
                                                           nullptr, nullptr, cnt, (unsigned long long*)loads, sd);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));
}
