// sparse_run.hip.h -- the sparse build (run_sparse) and the dense / sparse choice
// (choose_sparse).  A section of routing.hip's translation unit, included there after
// dense.hip.h (it uses srg_ctx, DevGraph, Prelude and Timer from the text above it); not a
// header to include elsewhere.
// ---- sparse path: batched lexicographic Bellman-Ford (sparse.hip.h) ----------------------
// Rank r routes the used sources at positions [r*n/G, (r+1)*n/G) (contiguous output rows).
// Returns false when a used pair came out saturated/unreachable and the graph's latencies
// could exceed the u32 keys: the caller then reruns on the wide (u64-key) labels.
bool run_sparse(srg_ctx& c, const DevGraph& g, const uint32_t* nodes, uint32_t n, uint64_t* out_lat,
                float* out_loss, hipStream_t st, const Prelude& P, srg_stats* stats, bool wide = false) {
    if (wide && c.kout_key) fail(SRG_INTERNAL_NEED_U64, "the build needs u64 latency keys: no u32 key table");
    const uint32_t V = g.V;
    const bool multi = c.comm && c.comm->nranks > 1;
    const int G = multi ? c.comm->nranks : 1, rk = multi ? c.comm->rank : 0;
    Timer tm(st);
    uint32_t* off = (uint32_t*)c.b_indeg.get(((size_t)V + 1) * 4);
    uint32_t* cur = (uint32_t*)c.b_cscfill.get(((size_t)V + 1) * 4);
    const uint32_t* esrc = g.src;
    const uint32_t* edst = g.dst;
    const uint64_t* selflat = P.selflat;
    const float* selfloss = P.selfloss;
    const uint32_t* cols = nodes;
    // CSR of in-arcs
    HIP_CHECK(hipMemsetAsync(cur, 0, ((size_t)V + 1) * 4, st));
    if (g.E) k_csr_count<<<grid_for(g.E), kThreads, 0, st>>>(g.E, esrc, edst, g.directed, cur);
    size_t tb = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cur, off, (int)(V + 1), st));
    void* tmp = c.b_scantmp.get(tb);
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cur, off, (int)(V + 1), st));
    uint32_t arcs = 0;
    HIP_CHECK(hipMemcpyAsync(&arcs, off + V, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    uint32_t* in_src = (uint32_t*)c.b_entkey.get(std::max<size_t>(arcs, 1) * 4);
    uint32_t* in_w = (uint32_t*)c.b_entw.get(std::max<size_t>(arcs, 1) * 4);
    float* in_b = (float*)c.b_entb.get(std::max<size_t>(arcs, 1) * 4);
    uint64_t* in_w64 = wide ? (uint64_t*)c.b_cscent.get(std::max<size_t>(arcs, 1) * 8) : nullptr;
    HIP_CHECK(hipMemsetAsync(cur, 0, ((size_t)V + 1) * 4, st));
    if (g.E)
        k_csr_fill<<<grid_for(g.E), kThreads, 0, st>>>(g.E, esrc, edst, g.lat, P.unit, g.loss, g.directed, off, cur,
                                                       in_src, in_w, in_b, in_w64);
    // out-arcs for the work marks: the in-CSR itself when undirected
    const uint32_t* out_off = off;
    const uint32_t* out_dst = in_src;
    if (g.directed) {
        uint32_t* ooff = (uint32_t*)c.b_outoff.get(((size_t)V + 1) * 4);
        uint32_t* odst = (uint32_t*)c.b_outdst.get(std::max<size_t>(arcs, 1) * 4);
        HIP_CHECK(hipMemsetAsync(cur, 0, ((size_t)V + 1) * 4, st));
        k_csr_count_out<<<grid_for(g.E), kThreads, 0, st>>>(g.E, esrc, edst, cur);
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cur, ooff, (int)(V + 1), st));
        HIP_CHECK(hipMemsetAsync(cur, 0, ((size_t)V + 1) * 4, st));
        k_csr_fill_out<<<grid_for(g.E), kThreads, 0, st>>>(g.E, esrc, edst, ooff, cur, odst);
        out_off = ooff;
        out_dst = odst;
    }
    // this rank's sources, in graph-locality (BFS) order, in batches of 64 lanes: sources of
    // one batch are close to each other, so their Bellman-Ford frontiers move together
    const Range own = rank_rows(n, rk, G);  // this rank's rows: positions [p0, p1) of `nodes`
    const uint32_t p0 = (uint32_t)own.lo, p1 = (uint32_t)own.hi;
    const uint32_t nloc = p1 - p0;
    const uint32_t nbatch = (nloc + 63) / 64;
    const int dbg = srg_env::debug_sparse();  // (read once per build)
    const double ms_csr = dbg ? tm.lap() : 0.0;  // (debug split of ms_build)
    const auto t_host0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> h_off(V + 1), h_src(arcs);
    HIP_CHECK(hipMemcpyAsync(h_off.data(), off, ((size_t)V + 1) * 4, hipMemcpyDeviceToHost, st));
    if (arcs) HIP_CHECK(hipMemcpyAsync(h_src.data(), in_src, (size_t)arcs * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const auto t_host1 = std::chrono::steady_clock::now();
    std::vector<uint32_t> order(V, 0xFFFFFFFFu), queue;
    queue.reserve(V);
    uint32_t next = 0;
    for (uint32_t root_pass = 0; root_pass < 2 && next < V; ++root_pass) {
        for (uint32_t r = 0; r < V; ++r) {
            // first pass: start at the highest-degree vertex; then any unvisited vertex
            uint32_t start = r;
            if (root_pass == 0) {
                uint32_t best = 0;
                for (uint32_t v = 0; v < V; ++v)
                    if (h_off[v + 1] - h_off[v] > h_off[best + 1] - h_off[best]) best = v;
                start = best;
            }
            if (order[start] != 0xFFFFFFFFu) continue;
            order[start] = next++;
            queue.assign(1, start);
            for (size_t qi = 0; qi < queue.size(); ++qi) {
                const uint32_t v = queue[qi];
                for (uint32_t k = h_off[v]; k < h_off[v + 1]; ++k) {
                    const uint32_t u = h_src[k];
                    if (order[u] == 0xFFFFFFFFu) {
                        order[u] = next++;
                        queue.push_back(u);
                    }
                }
            }
            if (root_pass == 0) break;
        }
    }
    const auto t_host2 = std::chrono::steady_clock::now();
    std::vector<uint32_t> loc(nloc);
    for (uint32_t i = 0; i < nloc; ++i) loc[i] = p0 + i;
    if (c.sparse_locality) {  // stable by BFS position: a counting sort over the V positions
        std::vector<uint32_t> cnt((size_t)V + 1, 0);
        for (uint32_t i = 0; i < nloc; ++i) ++cnt[order[P.nodes_h[p0 + i]] + 1];
        for (uint32_t v = 0; v < V; ++v) cnt[v + 1] += cnt[v];
        for (uint32_t i = 0; i < nloc; ++i) loc[cnt[order[P.nodes_h[p0 + i]]]++] = p0 + i;
    }
    std::vector<uint32_t> bsrc((size_t)std::max<uint32_t>(nbatch, 1) * 64), brow(bsrc.size());
    for (uint32_t i = 0; i < (uint32_t)bsrc.size(); ++i) {
        const bool real = i < nloc;
        bsrc[i] = P.nodes_h[real ? loc[i] : (nloc ? loc[0] : 0)];
        brow[i] = real ? loc[i] : 0xFFFFFFFFu;
    }
    const auto t_host3 = std::chrono::steady_clock::now();
    uint32_t* d_bsrc = (uint32_t*)c.b_lnodes.get(bsrc.size() * 4);
    uint32_t* d_brow = (uint32_t*)c.b_lpos.get(brow.size() * 4);
    HIP_CHECK(hipMemcpyAsync(d_bsrc, bsrc.data(), bsrc.size() * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_brow, brow.data(), brow.size() * 4, hipMemcpyHostToDevice, st));
    uint32_t* fl = (uint32_t*)c.b_red.get(128);
    HIP_CHECK(hipMemsetAsync(fl, 0, 128, st));
    HIP_CHECK(hipGetLastError());
    const double ms_build = tm.lap() + ms_csr;
    if (dbg)
        std::fprintf(stderr, "sparse build: CSR %.2f ms, host order + batches %.2f ms (of %.2f): CSR to host %.2f, BFS %.2f, batches %.2f\n", ms_csr,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count(), ms_build,
                     std::chrono::duration<double, std::milli>(t_host1 - t_host0).count(),
                     std::chrono::duration<double, std::milli>(t_host2 - t_host1).count(),
                     std::chrono::duration<double, std::milli>(t_host3 - t_host2).count());

    int dev_cus = 256;
    HIP_CHECK(hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, c.device));
    // wide labels take the 128-VGPR budget: one workgroup per CU
    const int wpc = wide ? 1 : 2;
    uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(nbatch, (uint32_t)dev_cus * (uint32_t)wpc));

    // u32 latency keys take the two-phase kernel (latency-only delta-stepping, then the loss fold
    // over the tight arcs, sparse_ds.hip.h); wide labels keep the lexicographic sweeps.
    // SRG_SPARSE_KERNEL=bf selects the lexicographic sweeps for u32 keys too (A/B)
    const bool two_phase = !wide && !srg_env::sparse_kernel_bf();
    // per resident batch: labels V x 64 x 8 B (16 B wide); two-phase: u32 latency + f32 loss
    // labels, a u64 tight mask per arc and a u64 final-lane mask per vertex
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t slot_bytes = (size_t)V * 64 * (wide ? 16 : two_phase ? 4 : 8);
    const size_t ds_extra = two_phase ? (size_t)V * 64 * 4 + (size_t)std::max<uint32_t>(arcs, 1) * 16 + (size_t)V * 16 : 0;
    // two launches (phase 1, then phases 2 + output) when every batch's latency labels fit beside the
    // rest (C4: 782 x 12.8 MB = 10 GB): each launch gets its own register allocation
    // (SRG_SPARSE_SPLIT=0: one fused launch, A/B)
    const size_t d_all = (size_t)nbatch * V * 64 * 4;
    const bool split = two_phase && nbatch && !srg_env::sparse_split_off() && d_all <= free_b / 3;
    grid = (uint32_t)std::max<size_t>(
        1, std::min<size_t>(grid, (free_b / 2 - (split ? d_all : 0)) / std::max<size_t>((split ? 0 : slot_bytes) + ds_extra, 1)));
    const uint32_t nwv = (V + 63) / 64;
    const size_t bitmap_bytes = two_phase ? ds_state_bytes(V) : (size_t)nwv * 5 * 8;
    const size_t scr_bytes = two_phase ? ds_scratch_bytes() : sp_scratch_bytes();
    // bitmaps in LDS while a CU still fits the requested workgroups, else in global memory
    const bool gbits = c.sparse_global_bitmaps || bitmap_bytes + scr_bytes > (size_t)160 * 1024 / wpc;
    const size_t lds = (gbits ? 0 : bitmap_bytes) + scr_bytes;
    if (nbatch) {
        unsigned long long* slots = (unsigned long long*)c.b_D.get(split ? d_all : (size_t)grid * slot_bytes);
        unsigned long long* gb = gbits ? (unsigned long long*)c.b_W.get((size_t)grid * bitmap_bytes) : nullptr;
        // 16 rows in flight was measured 2.5x slower (the row array no longer unrolls into
        // registers); 4 ties with 8 at 2 workgroups per CU
        // 8 rows in flight at two workgroups per CU: 4 rows tied, 16 rows / one workgroup per CU
        // (128 VGPRs, no spills) ran 2.5x / 1.2x slower
        auto kern = gbits ? k_sparse_bf<SP_G, true> : k_sparse_bf<SP_G, false>;
        if (wide) kern = gbits ? k_sparse_bf<SP_G, true, 4, LabelU64> : k_sparse_bf<SP_G, false, 4, LabelU64>;
        if (two_phase) {
            // 8 rows in flight per wave: 16 and 32 spill at the 64-VGPR budget and measured 375 / 712 ms
            // against 293 on C4 (profiles/r06/sparse_ds/c4_g*.json)
            kern = gbits ? k_sparse_ds<true, 8, 8> : k_sparse_ds<false, 8, 8>;
        }
        set_lds(kern, lds);
        SparseArgs a{off, in_src, in_w, in_b, out_off, out_dst, V, d_bsrc, d_brow, nbatch, slots, fl + 4, cols, n,
                     selflat, selfloss, out_lat, out_loss, fl, P.unit, ~0ull, gb, c.kout_key, c.kout_diag,
                     in_w64, min_edge_key(P.es.min_lat_inv, P.unit), nullptr, nullptr, nullptr, arcs};
        if (two_phase) {
            a.lo_slots = (float*)c.b_WL.get((size_t)grid * V * 64 * 4);
            // tight records (16 B per in-arc slot), final-lane masks + tight-record counts (16 B per vertex)
            a.tmask = (unsigned long long*)c.b_PRED.get((size_t)grid * std::max<uint32_t>(arcs, 1) * 16);
            a.fmask = (unsigned long long*)c.b_L0.get((size_t)grid * V * 16);
        }
        // bucket width: the largest edge latency / sparse_delta_div (0 = one bucket, plain BF)
        if (c.sparse_delta_div > 0)
            a.delta = std::max<unsigned long long>(1ull, P.max_key / (unsigned long long)c.sparse_delta_div);
        const bool dbg_batches = two_phase && dbg == 2;
        if (dbg_batches) {
            a.dbg = (uint32_t*)c.b_L1.get((size_t)nbatch * 6 * 4);
            HIP_CHECK(hipMemsetAsync(a.dbg, 0, (size_t)nbatch * 6 * 4, st));
        }
        if (c.profiling) {
            ensure_prof_events(c, 2);
            HIP_CHECK(hipEventRecord(c.prof_events[0], st));
        }
        if (split) {
            auto k1 = gbits ? k_sparse_ds<true, 8, 8, 1> : k_sparse_ds<false, 8, 8, 1>;
            auto k2 = gbits ? k_sparse_ds<true, 8, 8, 2> : k_sparse_ds<false, 8, 8, 2>;
            // (phase 1 in 8-wave workgroups at 128 VGPRs with 32 rows in flight per wave, no spills, was
            // measured slower: 151 vs 115 ms per workgroup, profiles/r06/sparse_p1w/)
            set_lds(k1, lds);
            set_lds(k2, lds);
            k1<<<grid, SP_THREADS, lds, st>>>(a);
            SparseArgs a2 = a;
            a2.queue = fl + 9;  // (zeroed with the flags)
            k2<<<grid, SP_THREADS, lds, st>>>(a2);
        } else {
            kern<<<grid, SP_THREADS, lds, st>>>(a);
        }
        HIP_CHECK(hipGetLastError());
        if (c.profiling) HIP_CHECK(hipEventRecord(c.prof_events[1], st));
        if (dbg_batches) {  // per-batch durations (100-MHz ticks): what sets the launches' makespan
            std::vector<uint32_t> h((size_t)nbatch * 6);
            HIP_CHECK(hipMemcpyAsync(h.data(), a.dbg, h.size() * 4, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            for (int ph = 0; ph < 2; ++ph) {
                std::vector<double> d(nbatch);
                for (uint32_t b = 0; b < nbatch; ++b) {
                    d[b] = h[b * 6 + 1 + 4 * ph] / 1e5;
                }
                std::vector<double> srt = d;
                std::sort(srt.begin(), srt.end());
                std::fprintf(stderr, "sparse batches phase %d (ms): min %.1f p10 %.1f median %.1f p90 %.1f max %.1f; by batch decile:",
                             ph + 1, srt[0], srt[nbatch / 10], srt[nbatch / 2], srt[nbatch * 9 / 10], srt[nbatch - 1]);
                for (int q = 0; q < 10; ++q) {
                    double m = 0;
                    uint32_t cnt = 0;
                    for (uint32_t b = q * nbatch / 10; b < (q + 1) * nbatch / 10; ++b) m += d[b], ++cnt;
                    std::fprintf(stderr, " %.1f", cnt ? m / cnt : 0.0);
                }
                std::fprintf(stderr, "\n");
            }
            std::fprintf(stderr, "sparse batches phase-1 sweeps:");
            for (uint32_t b = 0; b < nbatch; b += std::max<uint32_t>(1, nbatch / 20)) std::fprintf(stderr, " %u", h[b * 6 + 3]);
            std::fprintf(stderr, "\n");
        }
    }
    // every rank agrees on the outcome before any exchange
    if (multi) {
        c.comm->allreduce_max_u32(fl, 2, st);
        c.comm->allreduce_max_u32(fl + 5, 3, st);  // saturated, impossible, fold incomplete
    }
    uint32_t hfl[26] = {};
    HIP_CHECK(hipMemcpyAsync(hfl, fl, 104, hipMemcpyDeviceToHost, st));
    const double ms_sssp = tm.lap();
    if (hfl[7])
        fail(SRG_ERR_INTERNAL, "the sparse build's loss fold left a used pair without a final loss");
    if (hfl[6])
        fail(SRG_ERR_INTERNAL, "the sparse build produced an impossible table: a used pair's latency is below the "
                               "smallest edge latency (" + std::to_string(~P.es.min_lat_inv) + " ns)");
    if (dbg) {
        const unsigned long long ev = (unsigned long long)hfl[2] | (unsigned long long)hfl[3] << 32;
        const unsigned long long p2 = (unsigned long long)hfl[10] | (unsigned long long)hfl[11] << 32;
        std::fprintf(stderr,
                     "sparse: %s, %u batches, grid %u, max sweeps %u, lane evaluations %llu, fold sweeps %u, "
                     "fold row pulls %llu, arcs %u\n",
                     two_phase ? "two-phase" : "lexicographic", nbatch, grid, hfl[1], ev, hfl[8], p2, arcs);
        if (two_phase) {  // per-phase wall clock summed over workgroups (100 MHz), as ms per workgroup
            double t[4];
            for (int p = 0; p < 4; ++p)
                t[p] = (double)((unsigned long long)hfl[12 + 2 * p] | (unsigned long long)hfl[13 + 2 * p] << 32) / 1e5 / grid;
            std::fprintf(stderr, "sparse phases (ms per workgroup): latency %.1f, tight masks %.1f, fold %.1f, output %.1f\n",
                         t[0], t[1], t[2], t[3]);
            double b[3];  // wave utilisation: ticks inside window visits / (16 waves x the phase's ticks)
            for (int p = 0; p < 3; ++p)
                b[p] = (double)((unsigned long long)hfl[20 + 2 * p] | (unsigned long long)hfl[21 + 2 * p] << 32) / 1e5 / grid /
                       (16.0 * std::max(t[p], 1e-9));
            std::fprintf(stderr, "sparse wave utilisation: latency %.2f, tight masks %.2f, fold %.2f\n", b[0], b[1], b[2]);
        }
    }
    if (hfl[0]) {
        // a used pair came out INF: only a relaxation that saturated the u32 key can have hidden a
        // finite (>= 2^32-1 ns) path; otherwise the pair is unreachable -- the reference's panic
        if (hfl[5] && !wide) return false;  // rerun on the wide labels
        fail(SRG_ERR_UNREACHABLE,
             "assertion `left == right` failed: paths.len() != nodes.len().pow(2) (a used node is unreachable "
             "from another used node)");
    }
    double ms_exchange = 0;
    if (multi && c.gather_output) {
        std::vector<size_t> offs, lens;
        for (int elem : {8, 4}) {
            slice_tables(n, G, (size_t)n * elem, offs, lens);
            c.comm->allgatherv(elem == 8 ? (void*)out_lat : (void*)out_loss, offs.data(), lens.data(), st);
        }
        ms_exchange = tm.lap();
    }
    if (stats && c.profiling && nbatch) {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, c.prof_events[0], c.prof_events[1]));
        stats->prof_launches += 1;
        stats->prof_kernel_ms += ms;
        stats->prof_relaxations += nloc;  // sparse: sources routed by the profiled launch
    }
    if (stats) {
        stats->ms_build += ms_build;
        stats->ms_fw += ms_sssp;
        stats->ms_exchange += ms_exchange;
        stats->path_kind = wide ? SRG_PATH_SPARSE_U64 : SRG_PATH_SPARSE_U32;
        stats->loss_rounds = (int)hfl[1];
        stats->relaxations = (((uint64_t)hfl[3] << 32) | hfl[2]) * 64;
        stats->nranks = G;
        stats->rank = rk;
        stats->local_sources = nloc;
    }
    return true;
}

bool choose_sparse(const srg_ctx& c, const DevGraph& g) {
    if (c.algorithm == SRG_ALGO_DENSE) return false;
    if (c.algorithm == SRG_ALGO_SPARSE) return true;
    const double arcs = (double)g.E * (g.directed ? 1.0 : 2.0);
    return g.V >= 2048 && arcs * 32.0 < (double)g.V * g.V;
}
