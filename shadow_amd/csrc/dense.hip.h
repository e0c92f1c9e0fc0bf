// dense.hip.h -- the dense build (run_dense): W, FW, certification, latency rows, tight scan,
// loss rows.  A section of routing.hip's translation unit, included there after the FW schedules
// (it uses srg_ctx, Prelude, HostSink, SymFw and FwOverlap from the text above it); not a
// header to include elsewhere.
// Dense path for key type K. Returns false (u32 only) when certification fails.
template <class K, int T>
bool run_dense(srg_ctx& c, const DevGraph& g, const Plan& pl, const uint32_t* nodes, uint32_t n, uint64_t* out_lat,
               float* out_loss, hipStream_t st, const Prelude& P, srg_stats* stats, HostSink* sink,
               FwOverlap* ov = nullptr) {
    // the FW already ran beside the H2D (FwOverlap): W, D and the closed D are in place
    const bool pre = ov && ov->on && ov->ok && ov->ended && sizeof(K) == 4 && T == FwOverlap::T;
    if (sizeof(K) == 8 && c.kout_key) {  // a key table needs the u32 keys
        // (the host entry's internal key shipping just falls back to the u64 latency rows)
        if (!(sink && sink->widen)) fail(SRG_INTERNAL_NEED_U64, "the build needs u64 latency keys: no u32 key table");
        sink->widen = false;
        c.kout_key = nullptr;
        c.kout_diag = nullptr;
    }
    const uint32_t V = g.V;
    const size_t Vp = ((size_t)V + T - 1) / T * T;
    const size_t VV = Vp * Vp;
    const bool multi = c.comm && c.comm->nranks > 1;
    Timer tm(st);

    K* W = (K*)c.b_W.get(VV * sizeof(K));
    uint32_t* WL = (uint32_t*)c.b_WL.get(VV * 4);
    K* D = (K*)c.b_D.get(VV * sizeof(K));
    bool wl_late = false;  // late loss: WL is built after FW, once the losses have landed
    if (pre) {
        wl_late = g.late && !g.late->applied;
    } else if constexpr (sizeof(K) == 4) {
        // packed (latency, loss) keys: one atomic pass, then a tiled symmetrize + split pass
        static_assert(T % 64 == 0, "tile");
        unsigned long long* KW = (unsigned long long*)c.b_PRED.get(VV * 8);
        HIP_CHECK(hipMemsetAsync(KW, 0xFF, VV * 8, st));
        wl_late = g.late && !g.late->applied;
        if (g.E) k_w_key<<<grid_for(g.E), kThreads, 0, st>>>(g.E, g.src, g.dst, g.lat, P.unit, wl_late ? nullptr : g.loss, KW, Vp);
        const unsigned nb64 = (unsigned)(Vp / 64);
        k_w_split<false><<<dim3(nb64, nb64), 256, 0, st>>>(KW, Vp, g.directed, (uint32_t*)W, WL, (uint32_t*)D);
    } else {
        loss_arrive(g, P.selfloss, st);
        k_fill<K><<<grid_for(VV), kThreads, 0, st>>>(W, VV, KeyOps<K>::INF);
        HIP_CHECK(hipMemsetAsync(WL, 0xFF, VV * 4, st));
        if (g.E) {
            k_w_lat<K><<<grid_for(g.E), kThreads, 0, st>>>(g.E, g.src, g.dst, g.lat, P.unit, g.directed, W, Vp);
            k_w_loss<K><<<grid_for(g.E), kThreads, 0, st>>>(g.E, g.src, g.dst, g.lat, P.unit, g.loss, g.directed, W, WL,
                                                             Vp);
        }
        k_init_d<K><<<grid_for(VV), kThreads, 0, st>>>(W, D, Vp);
    }
    // local sources and their output rows
    const uint32_t nloc = (uint32_t)pl.lnodes.size();
    uint32_t* lnodes = (uint32_t*)c.b_lnodes.get(std::max<size_t>(nloc, 1) * 4);
    uint32_t* lpos = (uint32_t*)c.b_lpos.get(std::max<size_t>(nloc, 1) * 4);
    if (nloc) {
        HIP_CHECK(hipMemcpyAsync(lnodes, pl.lnodes.data(), (size_t)nloc * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(lpos, pl.lpos.data(), (size_t)nloc * 4, hipMemcpyHostToDevice, st));
    }
    HIP_CHECK(hipGetLastError());
    const double ms_build = tm.lap();

    // ---- blocked Floyd-Warshall; afterwards every rank holds the whole D ----
    uint64_t prof_relax = 0;
    int prof_n = 0;
    double ms_dx = 0;  // multi-rank: D exchange at the end of FW (inside ms_fw, also in ms_exchange)
    if (pre) {
        prof_relax = ov->prof_relax;
        prof_n = ov->prof_n;
    } else if (sym_fw_for<K, T>(c, g)) {
        if constexpr ((sizeof(K) == 4 && T == 128) || (sizeof(K) == 8 && T == 64))
            fw_line_sym<K, T>(c, pl, D, Vp, st, prof_relax, prof_n, ms_dx);
    } else {
        // u32 keys: the pair-packed tile (two relaxations per 64-bit add + v_min3); the add + min3
        // tile (PK = 0) ran the same C3 launch in 0.304 instead of 0.242 ms (profiles/r02c/fw_fold.txt)
        // and is kept for u64 keys only
        if constexpr (sizeof(K) == 4) fw_blocked<K, T, 2>(c, pl, D, Vp, st, prof_relax, prof_n);
        else fw_blocked<K, T, 0>(c, pl, D, Vp, st, prof_relax, prof_n);
        if (multi) gather_rows<K>(c, pl, D, Vp, T, st, ms_dx);
    }
    HIP_CHECK(hipGetLastError());
    if (sym_fw_for<K, T>(c, g)) rb_async(c, MS_TIMEOUT, c.fw_timeout, st);  // read after FW, on its stream
    const double ms_fw = tm.lap();
    if (sym_fw_for<K, T>(c, g) && rb_get<uint32_t>(c, MS_TIMEOUT))
        fail(SRG_ERR_HIP, fw_timeout_message(rb_get<uint32_t>(c, MS_TIMEOUT)));
#ifdef SRG_TEST_HOOKS
    if (c.test_fault == 1)  // TEST HOOK (SRG_OPT_TEST_FAULT): a lost synchronisation's result, for the guard
        HIP_CHECK(hipMemsetAsync(D, 0, VV * sizeof(K), st));
#endif
    if (wl_late) {
        // WL = min loss among the min-latency parallel edges (what k_w_split gives), from the
        // losses that crossed PCIe during FW.  Built here, after FW, rather than beside it: on a
        // narrow grid beside the FW tiles it cost the bulk launches 5 % (0.242 -> 0.255 ms,
        // FW +0.8 ms, profiles/r02g) for about the same total.
        // The packed-key pass again, now with the losses (its buffer is free until the scan
        // writes PRED), splitting out WL only: 0.8 ms where k_w_loss's random W reads took 2.3.
        // It runs on the (idle) FW lookahead stream beside the certification, extract and
        // essential-entry count, which read W and D only; st waits for it before the entry fill.
        hipStream_t ax = c.aux_stream;  // st is synchronised (tm.lap): FW is complete
        const auto tl0 = std::chrono::steady_clock::now();
        loss_arrive(g, P.selfloss, ax);
        if (srg_env::debug_overlap())
            std::fprintf(stderr, "late loss: the host waited %.2f ms for the loss thread after FW\n",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl0).count());
        if constexpr (sizeof(K) == 4) {
            unsigned long long* KW = (unsigned long long*)c.b_PRED.get(VV * 8);
            HIP_CHECK(hipMemsetAsync(KW, 0xFF, VV * 8, ax));
            if (g.E) k_w_key<<<grid_for(g.E), kThreads, 0, ax>>>(g.E, g.src, g.dst, g.lat, P.unit, g.loss, KW, Vp);
            const unsigned nb64 = (unsigned)(Vp / 64);
            k_w_split<true><<<dim3(nb64, nb64), 256, 0, ax>>>(KW, Vp, g.directed, nullptr, WL, nullptr);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipEventRecord(c.ev_wlate, ax));
    }
    if (prof_n && stats) {
        double sum = 0;
        for (int i = 0; i < prof_n; ++i) {
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, c.prof_events[2 * i], c.prof_events[2 * i + 1]));
            sum += ms;
        }
        stats->prof_launches += prof_n;
        stats->prof_kernel_ms += sum;
        stats->prof_relaxations += prof_relax;
    }

    // Every collective after FW runs on the comm stream, in the same order on every rank:
    // allreduce(certify) -> allreduce(unreachable) -> allgather(latency rows, overlapped with
    // the scan) -> allgather(essential bitmask) -> allgather(loss rows).
    hipStream_t cs = c.comm_stream;
    auto cs_after_st = [&]() {
        HIP_CHECK(hipEventRecord(c.ev_a, st));
        HIP_CHECK(hipStreamWaitEvent(cs, c.ev_a, 0));
    };
    auto st_after_cs = [&]() {
        HIP_CHECK(hipEventRecord(c.ev_b, cs));
        HIP_CHECK(hipStreamWaitEvent(st, c.ev_b, 0));
    };
    auto reduce_flag = [&](uint32_t* flag_dev) -> uint32_t {
        uint32_t* red = (uint32_t*)c.b_red.get(16);
        HIP_CHECK(hipMemcpyAsync(red, flag_dev, 4, hipMemcpyDeviceToDevice, st));
        if (multi) {
            cs_after_st();
            c.comm->allreduce_max_u32(red, 1, cs);
            st_after_cs();
        }
        rb_async(c, MS_REDUCE, red, st);
        HIP_CHECK(hipStreamSynchronize(st));
        return rb_get<uint32_t>(c, MS_REDUCE);
    };
    // output rows of every rank: positions [n r / G, n (r+1) / G)
    const bool exchange = multi && c.gather_output;
    auto exchange_rows = [&](void* out, size_t elem) {  // on cs, after st
        const size_t row = (size_t)n * elem;
        std::vector<size_t> offs, lens;
        slice_tables(n, pl.G, row, offs, lens);
        cs_after_st();
        c.comm->allgatherv(out, offs.data(), lens.data(), cs);
    };

    // ---- essential edges (W[u][t] == D[u][t]) counted into the scan's pair-record layout ----
    // One rank: on the comm stream (idle after the H2D), beside the certification / extract and
    // their flag read-backs on st, which read D only; several ranks: on st (cs carries collectives).
    hipStream_t es = multi ? st : c.comm_stream;
    auto drain_es = [&]() {  // (before an early return: a rerun may reallocate these buffers)
        if (es != st) HIP_CHECK(hipStreamSynchronize(es));
    };
    constexpr int TS = 64;
    constexpr int VE = 16 / (int)sizeof(K);
    const size_t nmax = std::max<uint32_t>(nloc, 1);
    uint32_t* PRED = (uint32_t*)c.b_PRED.get(nmax * Vp * 4);
    unsigned long long* multi_cnt = (unsigned long long*)c.b_multi.get(16);
    uint32_t* mirror_cnt = (uint32_t*)(multi_cnt + 1);  // k_pred_mirror's worklist: {pairs wanted, overflow}
    int rounds = 0;
    unsigned long long nmulti = 0;
    uint64_t n_ess = 0;
    int scan_kind = SRG_SCAN_NONE;
    bool loss_written = false;  // out_loss already filled by the per-row kernel
    float* Lfin = nullptr;
    double ms_scan = 0;
    HIP_CHECK(hipMemsetAsync(multi_cnt, 0, 8, st));
    // essential bitmask (V^2/8 bytes): every rank holds the whole D and W, so each builds all of it
    const uint32_t nw64 = (V + 63) / 64;
    unsigned long long* ess = (unsigned long long*)c.b_ess.get((size_t)V * nw64 * 8);
    k_ess_mask<K><<<V, 256, 0, es>>>(W, D, Vp, V, 0u, V, nw64, ess);
    uint32_t* indeg = (uint32_t*)c.b_indeg.get(((size_t)nw64 * 64 + 1) * 4);
    uint32_t* cscoff = (uint32_t*)c.b_cscoff.get(((size_t)nw64 * 64 + 1) * 4);
    HIP_CHECK(hipMemsetAsync(indeg, 0, ((size_t)nw64 * 64 + 1) * 4, es));
    // pair-lane LDS scan (tight_v5); u64 keys run it on the keys' low words (exact together with
    // the loss pass's multi-predecessor check, tight_sparse.hip.h)
    const bool v5lo = sizeof(K) == 8;
    const uint32_t SB = V5_SB;
    const size_t npad = ((size_t)nloc + SB - 1) / SB * SB;
    const size_t dst_bytes = (size_t)nw64 * 64 * std::max<size_t>(npad, 64) * sizeof(K);
    const uint32_t NT = nw64 * 64;
    const uint32_t nK5 = (V + V5_UC - 1) / V5_UC, nbTT5 = (NT + V5_TT - 1) / V5_TT;
    const size_t NG5 = (size_t)nbTT5 * nK5 * V5_WAVES;
    uint32_t* v5_cnt = (uint32_t*)c.b_ecnt.get((size_t)nbTT5 * nK5 * V5_TT * 4);
    uint32_t* v5_goff = (uint32_t*)c.b_eoff.get((NG5 + 1) * 4);
    uint64_t E_ess = 0, E_layout = 0;
    {
        uint32_t* v5_glen = (uint32_t*)c.b_rlen.get((NG5 + 1) * 4);
        HIP_CHECK(hipMemsetAsync(v5_cnt, 0, (size_t)nbTT5 * nK5 * V5_TT * 4, es));
        HIP_CHECK(hipMemsetAsync(v5_glen, 0, (NG5 + 1) * 4, es));
        const size_t nwaves = (size_t)nw64 * nK5;
        k_v5_count<<<(unsigned)((nwaves * 64 + 255) / 256), 256, 0, es>>>(ess, V, nw64, nK5, v5_cnt, v5_glen, indeg);
        HIP_CHECK(hipGetLastError());
        size_t ta = 0, tc = 0;
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, ta, indeg, cscoff, (int)(NT + 1), es));
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tc, v5_glen, v5_goff, (int)(NG5 + 1), es));
        const size_t tbytes = std::max(ta, tc);
        void* tmp = c.b_scantmp.get(tbytes);
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, ta, indeg, cscoff, (int)(NT + 1), es));
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tc, v5_glen, v5_goff, (int)(NG5 + 1), es));
        HIP_CHECK(hipGetLastError());
    }

    // u32 certification: no saturated key in any used row (every rank must agree)
    HIP_CHECK(hipMemsetAsync(&P.flags->inf_in_used_row, 0, 4, st));
    HIP_CHECK(hipMemsetAsync(&P.flags->impossible, 0, 4, st));
    if (nloc)
        k_certify<K><<<nloc, kThreads, 0, st>>>(
            D, Vp, lnodes, nloc, nodes, n,
            // (an edge of >= INF keys counts as absent: the bound is never above INF, which stays legal)
            (K)std::min<uint64_t>(min_edge_key(P.es.min_lat_inv, P.unit), (uint64_t)KeyOps<K>::INF), P.flags);
    // (a simulated rank -- SRG_OPT_SIMULATE_RANK, timing only -- never receives its peers' line
    // segments, so its table is not a result and the guard does not apply)
    const bool simulated = c.comm && std::strcmp(c.comm->kind(), "simulated") == 0;
    // both of k_certify's flags with one read-back when one rank (each read-back is a stream drain)
    uint32_t impossible = 0, inf_any = 0;
    if (multi) {
        impossible = reduce_flag(&P.flags->impossible);
        inf_any = reduce_flag(&P.flags->inf_in_used_row);
    } else {
        rb_async(c, MS_REDUCE, &P.flags->impossible, st);
        rb_async(c, MS_REDUCE2, &P.flags->inf_in_used_row, st);
        HIP_CHECK(hipStreamSynchronize(st));
        impossible = rb_get<uint32_t>(c, MS_REDUCE);
        inf_any = rb_get<uint32_t>(c, MS_REDUCE2);
    }
    if (impossible && !simulated)
        fail(SRG_ERR_INTERNAL, "FW produced an impossible table: a used pair's latency is below the smallest edge "
                               "latency (" + std::to_string(~P.es.min_lat_inv) + " ns)");
    if (sizeof(K) == 4 && inf_any) {
        // a used pair at INF: unreachable -- unless some path could reach 2^31-1 ns, in which case
        // the u64 keys decide (the u32 FW work is redone)
        const unsigned __int128 bound = (unsigned __int128)P.max_key * (V > 1 ? V - 1 : 1);
        if (bound >= KeyOps<uint32_t>::INF) {
            if (wl_late) HIP_CHECK(hipStreamWaitEvent(st, c.ev_wlate, 0));  // the u64 rerun rewrites WL
            drain_es();
            return false;
        }
        fail(SRG_ERR_UNREACHABLE,
             "assertion `left == right` failed: paths.len() != nodes.len().pow(2) (a used node is unreachable "
             "from another used node)");
    }
    if (P.wrap_risk) {
        // max edge latency x V reaches 2^64 ns: check that no relaxation the reference runs wraps
        // its u64 sum (k_wrap_edges), and that outputs D * unit fit u64 (they are below such a sum)
        const unsigned __int128 bound = (unsigned __int128)P.max_key * (V > 1 ? V - 1 : 1);
        const bool inf_known = sizeof(K) == 4 ? bound < KeyOps<uint32_t>::INF : !P.range_risk;
        HIP_CHECK(hipMemsetAsync(&P.flags->wrap, 0, 8, st));
        for (uint32_t r0 = 0; r0 < nloc && g.E; r0 += 32768) {
            const uint32_t nr = std::min<uint32_t>(32768, nloc - r0);
            k_wrap_edges<K><<<dim3(grid_for(g.E, 64), nr), 256, 0, st>>>(g.E, g.src, g.dst, g.lat, g.directed, D, Vp,
                                                                        lnodes + r0, P.unit, inf_known ? 1 : 0, P.flags);
        }
        HIP_CHECK(hipGetLastError());
        const uint32_t wrapped = reduce_flag(&P.flags->wrap);
        if (wrapped)
            fail(SRG_ERR_LATENCY_RANGE, "a shortest-path relaxation sums past 2^64 ns (max edge latency " +
                                            std::to_string(P.es.max_lat) +
                                            " ns): the reference's u64 latency sum would wrap (mod.rs:327)");
        if (reduce_flag(&P.flags->wrap_inf)) {
            if (sizeof(K) == 4) {  // a vertex past the u32 keys: decide on the u64 keys
                if (wl_late) HIP_CHECK(hipStreamWaitEvent(st, c.ev_wlate, 0));
                drain_es();
                return false;
            }
            fail(SRG_ERR_LATENCY_RANGE, "a vertex has no path below 2^62 latency units on a graph whose u64 latency "
                                        "sums can wrap (max edge latency " +
                                            std::to_string(P.es.max_lat) + " ns)");
        }
    }

    // latency outputs (+ diagonal self-loops) of the own rows, right after FW
    HIP_CHECK(hipMemsetAsync(&P.flags->unreachable_used_pair, 0, 4, st));
    // k_extract_ident moves rows by 16-B vectors: the caller's arrays (a device-entry torch view may be
    // offset) must be 16-B aligned too (row offsets are, since n % 4 == 0)
    const bool al16 = (((uintptr_t)out_lat | (uintptr_t)c.kout_key) & 15u) == 0;
    if (nloc && P.ident && n % 4 == 0 && al16)
        k_extract_ident<K><<<nloc, 256, 0, st>>>(D, Vp, lnodes, n, P.selflat, out_lat, P.flags, P.unit, c.kout_key,
                                                 c.kout_diag);
    else if (nloc)
        k_extract<K><<<nloc, kThreads, 0, st>>>(D, nullptr, Vp, lnodes, nloc, nodes, n, lpos,
                                                                      P.selflat, P.selfloss, out_lat, out_loss,
                                                                      P.flags, 1, P.unit, c.kout_key, c.kout_diag);
    HIP_CHECK(hipGetLastError());
    if (reduce_flag(&P.flags->unreachable_used_pair)) {
        if (sizeof(K) == 8 && P.range_risk)
            fail(SRG_ERR_LATENCY_RANGE, "a used pair has no path below 2^62 latency units (max edge latency " +
                                            std::to_string(P.es.max_lat) +
                                            " ns): unreachable, or a latency sum the reference's u64 would wrap");
        fail(SRG_ERR_UNREACHABLE,
             "assertion `left == right` failed: paths.len() != nodes.len().pow(2) (a used node is unreachable "
             "from another used node)");
    }
    if (exchange) exchange_rows(out_lat, 8);  // overlaps the scan and the loss pass below
    // host entry, own rows only (one rank, or several without the exchange): the latency rows are
    // final -- they leave during the scan / loss pass
    const bool sink_rows = sink && !exchange && nloc && sink->ok();
    if (sink && c.kout_key) sink->key_unit = P.unit;
    if (sink_rows) {
        if (c.kout_key && sink->widen) sink->send_keys(st, c.kout_key, pl.p0, nloc, P.unit);  // (widened on the host)
        else if (c.kout_key) sink->send_rows(st, c.kout_key, sink->lat, pl.p0, nloc, 4);  // (sink->lat: the host key table)
        else sink->send_rows(st, out_lat, sink->lat, pl.p0, nloc, 8);
        sink->lat_sent = true;
    }

    // ---- tight-predecessor scan, loss (the essential entries were counted above) ----
    {
        rb_async(c, MS_TAIL0, cscoff + NT, es);
        rb_async(c, MS_TAIL1, v5_goff + NG5, es);
        HIP_CHECK(hipStreamSynchronize(es));
        E_ess = rb_get<uint32_t>(c, MS_TAIL0);
        E_layout = 2ull * rb_get<uint32_t>(c, MS_TAIL1);
    }
    n_ess = E_ess;
    if (wl_late) HIP_CHECK(hipStreamWaitEvent(st, c.ev_wlate, 0));  // WL (late loss) before the entry fill
    const bool sparse = (double)E_ess <= c.sparse_threshold * (double)V * (double)V &&
                        E_layout + 256 < 0xF0000000ull && dst_bytes < 0xFFFFFFFFull;
    if (sparse) {
        scan_kind = SRG_SCAN_SPARSE;
        // the scan's DST (D columns of the used sources, + their low words for u64 keys) on the aux
        // stream, beside the entry fill: it reads D only (st is past FW)
        K* DST = nullptr;
        const uint32_t* DSTs = nullptr;
        uint32_t dsts_bytes = 0;
        if (nloc) {
            hipStream_t ax = c.aux_stream;
            const uint32_t nbS = (uint32_t)(npad / 64);
            DST = (K*)c.b_DST.get(dst_bytes);
            k_build_dst<K><<<dim3(nw64, nbS), 256, 0, ax>>>(D, Vp, lnodes, nloc, DST, npad);
            DSTs = (const uint32_t*)DST;
            dsts_bytes = (uint32_t)std::min<size_t>(dst_bytes, 0xFFFFFFFFull);
            if (v5lo) {
                const size_t cnt = dst_bytes / 8;
                uint32_t* lo = (uint32_t*)c.b_DST2.get(cnt * 4);
                k_low_words<<<grid_for(cnt), kThreads, 0, ax>>>(reinterpret_cast<const uint64_t*>(DST), cnt, lo);
                DSTs = lo;
                dsts_bytes = (uint32_t)(cnt * 4);
            }
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipEventRecord(c.ev_dst, ax));
        }
        const size_t Eb = E_layout + 256;
        uint32_t* cscpos = (uint32_t*)c.b_cscfill.get((size_t)nbTT5 * nK5 * V5_TT * 4);
        K* ent_w = (K*)c.b_entw.get(Eb * sizeof(K));
        uint2* ent_ub = (uint2*)c.b_grpe.get(Eb * 8);  // {u, 1 - loss bits}: one gather in the loss pass
        uint32_t* cscent = (uint32_t*)c.b_cscent.get(std::max<uint64_t>(E_ess, 1) * 4);
        k_v5_cscpos<<<(NT + 255) / 256, 256, 0, st>>>(v5_cnt, cscoff, NT, nK5, cscpos);
        uint2* rec = (uint2*)c.b_entkey.get((Eb + V5_SLACK) * 8);
        {
            const size_t nwaves = (size_t)nw64 * nK5;
            k_v5_fill<K><<<(unsigned)((nwaves * 64 + 255) / 256), 256, 0, st>>>(ess, W, WL, Vp, V, nw64, nK5, v5_cnt,
                                                                                  v5_goff, cscpos, rec, ent_w,
                                                                                  ent_ub, cscent);
        }
        HIP_CHECK(hipGetLastError());
        const size_t lds_rows = loss_rows_lds(V);
        // the per-row LDS fold when a row fits (SRG_LOSS_ROWS_MAX_V, tests: only below that V)
        const bool rows_lds = V <= srg_env::loss_rows_max_v(LOSS_ROWS_MAX_V);
        // Triangular scan (SRG_OPT_SCAN_MIRROR): on an undirected graph whose rows are
        // the vertices in order, one rank, u32 keys, per-row LDS loss, tight_v5 scans only the pairs
        // (source block c, target tile b >= c) and k_pred_mirror derives the packed entries below
        // the diagonal.  Every other build scans every pair.
        bool mirror = c.scan_mirror && !g.directed && pl.G == 1 && !multi && !simulated && nloc == n && P.ident &&
                      !v5lo && rows_lds;
        // host entry, one rank, per-row LDS loss: scan groups interleaved with the loss rows (mirrored:
        // one group more, the later groups scan little and their rows keep the link fed: C3 host entry
        // 3 / 4 / 5 groups 44.3 / 43.0 / 42.7 ms, profiles/r07/scan_mirror)
        const uint32_t scan_groups = c.scan_groups ? (uint32_t)c.scan_groups : mirror ? 4u : 3u;
        const bool interleave = sink_rows && rows_lds && scan_groups > 1;
        if (interleave) set_lds(k_loss_rows<K, true>, lds_rows);
        // the per-row LDS loss pass reads PRED packed with each single predecessor's {u, 1 - loss}
        // (k_pred_pack, after each scan group); the global-memory fold the entry indices
        uint32_t* PREDK = rows_lds ? (uint32_t*)c.b_PRED2.get(nmax * Vp * 8) : nullptr;
        auto pack_pred = [&](uint32_t r0, uint32_t r1) {
            const uint32_t nsb = (r1 - r0 + 127) / 128, nt8 = (nbTT5 + 7) / 8;
            k_pred_pack<<<8u * nt8 * nsb, 256, 0, st>>>(PRED, Vp, r0, r1, NT, nbTT5, nsb, ent_ub, (uint2*)PREDK,
                                                        multi_cnt, mirror ? 1u : 0u);
            HIP_CHECK(hipGetLastError());
        };
        // the pairs below the diagonal of the rows [r0, r1), after pack_pred(r0, r1) (r0 on a block
        // bound; the rows before r0 are packed and mirrored).  The worklist of the pairs that need
        // the exact keys lies in the PRED rows [r0, r1), which are dead once packed (room for half
        // of all the rows' pairs).  A worklist pair costs a wave that gathers the whole CSC list of
        // its column, about what the scan spends on a thousand pairs, so the capacity is 1 / 1024 of
        // the rows' pairs (at least 256): the slow launch stays a small fraction of the scan.  A pair
        // that does not fit raises mirror_cnt[1]; the mirror kernels then return at once and the
        // whole scan stage runs again without mirroring (below).
        auto mirror_rows = [&](uint32_t r0, uint32_t r1) {
            if (r1 <= r0 || r1 <= SB) return;  // rows of the first block only: nothing below the diagonal
            const size_t pairs = (size_t)(r1 - r0) * Vp, room = std::min<size_t>(pairs / 2, (size_t)1 << 30);
            const uint32_t cap = (uint32_t)std::min<size_t>(
                room, c.scan_mirror_cap ? (size_t)c.scan_mirror_cap : std::max<size_t>(pairs / 1024, 256));
            uint2* work = (uint2*)(PRED + (size_t)r0 * Vp);
            HIP_CHECK(hipMemsetAsync(mirror_cnt, 0, 4, st));
            const uint32_t nlow = (r1 - 1) / SB * SB;  // columns below the last row's diagonal block
            k_pred_mirror<<<dim3(nlow / 64, (r1 - r0 + 63) / 64), 256, 0, st>>>((uint2*)PREDK, Vp, r0, r1, V, work, cap,
                                                                               mirror_cnt, multi_cnt);
            k_mirror_slow<K><<<1024, 256, 0, st>>>(work, mirror_cnt, cap, DST, npad, ent_ub, ent_w, cscoff, cscent,
                                                   (uint2*)PREDK, Vp, multi_cnt);
            HIP_CHECK(hipGetLastError());
        };
        std::vector<uint32_t> tri_h;  // the triangular launches' block lists (tri_scan_blocks), one after another
        if (nloc) HIP_CHECK(hipStreamWaitEvent(st, c.ev_dst, 0));  // (the scan's DST, built on the aux stream)
        // (a second pass only after a mirrored pass whose worklist overflowed)
        for (bool again = nloc != 0; again;) {
            again = false;
            if (interleave) HIP_CHECK(hipMemsetAsync(&P.flags->changed, 0, 4, st));  // (loss_rounds: this pass's)
            const uint32_t inf_check = v5lo ? 0u : 1u;
            const uint32_t nbS5 = (uint32_t)(npad / SB);
            // host entry: the scan runs in source-block groups, each group's loss rows folded right
            // after it and shipped while later groups scan (loss rows on a second stream beside the
            // next group's scan were starved of CUs: 24.7 ms vs 20.8)
            const uint32_t ng = interleave ? std::min<uint32_t>(scan_groups, nbS5) : 1u;
            // group bounds on multiples of 8 source blocks, in ascending order: a row's mirrored
            // pairs read the packed rows before it (scan_group_cut / scan_group_cut_tri, plan.h)
            auto cut = [&](uint32_t q) { return mirror ? scan_group_cut_tri(q, ng, nbS5) : scan_group_cut(q, ng, nbS5); };
            const uint32_t* tri_d = nullptr;
            std::vector<size_t> tri_off(ng + 1, 0);
            if (mirror) {
                tri_h.clear();
                for (uint32_t gi = 0; gi < ng; ++gi) {
                    tri_scan_blocks(cut(gi), cut(gi + 1), nbTT5, tri_h);
                    tri_off[gi + 1] = tri_h.size();
                }
                uint32_t* d = (uint32_t*)c.b_tri.get(std::max<size_t>(tri_h.size(), 1) * 4);
                if (!tri_h.empty()) HIP_CHECK(hipMemcpyAsync(d, tri_h.data(), tri_h.size() * 4, hipMemcpyHostToDevice, st));
                HIP_CHECK(hipMemsetAsync(mirror_cnt, 0, 8, st));
                tri_d = d;
            }
            for (uint32_t gi = 0; gi < ng; ++gi) {
                const uint32_t c0 = cut(gi), c1 = cut(gi + 1);
                if (c1 == c0) continue;
                // blocks of 4 target tiles x 8 source blocks; mirrored: those that touch the triangle
                const uint32_t nblk = mirror ? (uint32_t)(tri_off[gi + 1] - tri_off[gi])
                                             : (nbTT5 + 3) / 4 * ((c1 - c0 + 7) / 8);
                if (nblk)
                    tight_v5<<<8u * 32u * ((nblk + 7) / 8), V5_WAVES * 64, 0, st>>>(
                        DSTs, npad, dsts_bytes, lnodes, nloc, V, NT, nbTT5, c1, nK5, c0, v5_goff,
                        (const uint32_t*)c.b_entkey.get(0), PRED, Vp, inf_check, mirror ? tri_d + tri_off[gi] : nullptr);
                HIP_CHECK(hipGetLastError());
                if (interleave) {
                    const uint32_t r0 = c0 * SB, r1 = std::min<uint32_t>(c1 * SB, nloc);
                    if (r1 <= r0) continue;
                    pack_pred(r0, r1);
                    if (mirror) mirror_rows(r0, r1);
                    k_loss_rows<K, true><<<r1 - r0, 1024, lds_rows, st>>>(PREDK, Vp, V, lnodes, nloc, ent_ub, ent_w,
                                                                   DST, npad, cscoff, cscent, P.selfloss, nodes, n,
                                                                   lpos, out_loss, &P.flags->changed, r0,
                                                                   mirror ? mirror_cnt + 1 : nullptr);
                    HIP_CHECK(hipGetLastError());
                    sink->send_rows(st, out_loss, sink->loss, pl.p0 + r0, r1 - r0, 4);
                }
            }
            if (!PREDK) k_count_multi<<<nloc, kThreads, 0, st>>>(PRED, nloc, V, Vp, multi_cnt);  // (else k_pred_pack counted)
            HIP_CHECK(hipGetLastError());
            ms_scan += tm.lap();
            if (interleave) {  // loss rows already folded and shipped, group by group
                sink->loss_sent = true;
                rb_async(c, MS_CHANGED, &P.flags->changed, st);
                if (mirror) rb_async(c, MS_MIRROR, mirror_cnt + 1, st);
                HIP_CHECK(hipStreamSynchronize(st));
                rounds = (int)rb_get<uint32_t>(c, MS_CHANGED);
                loss_written = true;
                c.loss_kind = SRG_LOSS_ROWS_LDS;
            } else if (rows_lds) {
                // per-row Gauss-Seidel in LDS, writes out_loss directly
                set_lds(k_loss_rows<K, true>, lds_rows);
                HIP_CHECK(hipMemsetAsync(&P.flags->changed, 0, 4, st));
                // host entry: row chunks, each chunk's loss rows sent as soon as it is done
                pack_pred(0, nloc);
                if (mirror) mirror_rows(0, nloc);
                const uint32_t nchunk = std::max<uint32_t>(1, std::min<uint32_t>(c.loss_chunks ? c.loss_chunks : sink_rows ? 8 : 1, nloc));
                for (uint32_t q = 0; q < nchunk; ++q) {
                    const uint32_t r0 = (uint32_t)((uint64_t)nloc * q / nchunk);
                    const uint32_t r1 = (uint32_t)((uint64_t)nloc * (q + 1) / nchunk);
                    if (r1 == r0) continue;
                    k_loss_rows<K, true><<<r1 - r0, 1024, lds_rows, st>>>(PREDK, Vp, V, lnodes, nloc, ent_ub, ent_w,
                                                                   DST, npad, cscoff, cscent, P.selfloss, nodes, n,
                                                                   lpos, out_loss, &P.flags->changed, r0,
                                                                   mirror ? mirror_cnt + 1 : nullptr);
                    HIP_CHECK(hipGetLastError());
                    if (sink_rows) sink->send_rows(st, out_loss, sink->loss, pl.p0 + r0, r1 - r0, 4);
                }
                if (sink_rows) sink->loss_sent = true;
                rb_async(c, MS_CHANGED, &P.flags->changed, st);
                if (mirror) rb_async(c, MS_MIRROR, mirror_cnt + 1, st);
                HIP_CHECK(hipStreamSynchronize(st));
                rounds = (int)rb_get<uint32_t>(c, MS_CHANGED);
                loss_written = true;
                c.loss_kind = SRG_LOSS_ROWS_LDS;
            } else {
                c.loss_kind = SRG_LOSS_GLOBAL_ENTRIES;
                float* L0 = (float*)c.b_L0.get(nmax * Vp * 4);
                float* L1 = (float*)c.b_L1.get(nmax * Vp * 4);
                k_fill<float><<<grid_for((size_t)nloc * Vp), kThreads, 0, st>>>(L0, (size_t)nloc * Vp, 1.0f);
                float* Lin = L0;
                float* Lout = L1;
                for (;;) {
                    HIP_CHECK(hipMemsetAsync(&P.flags->changed, 0, 4, st));
                    k_loss_round_sparse<K><<<grid_for((size_t)nloc * V, 256 * 64), kThreads, 0, st>>>(
                        PRED, Vp, DST, npad, lnodes, nloc, V, ent_ub, ent_w, cscoff, cscent, Lin, Lout,
                        &P.flags->changed);
                    HIP_CHECK(hipGetLastError());
                    ++rounds;
                    rb_async(c, MS_CHANGED, &P.flags->changed, st);
                    HIP_CHECK(hipStreamSynchronize(st));
                    const uint32_t ch = rb_get<uint32_t>(c, MS_CHANGED);
                    std::swap(Lin, Lout);
                    if (!ch) break;
                    if (rounds > (int)V + 2) fail(SRG_ERR_INTERNAL, "loss rounds did not converge");
                }
                Lfin = Lin;
            }
            if (mirror) {
                // (both mirrored branches above read the overflow word back with their last sync)
                c.scan_mirrored = 1;
                if (rb_get<uint32_t>(c, MS_MIRROR)) {
                    // the worklist overflowed (a tie-heavy graph): some mirrored pairs are undecided.
                    // The scan stage again with every pair scanned -- as the u64 rerun, one wasted
                    // pass; every loss row is folded and shipped again
                    c.scan_mirrored = 2;
                    mirror = false;
                    again = true;
                    rounds = 0;
                    loss_written = false;
                    HIP_CHECK(hipMemsetAsync(multi_cnt, 0, 8, st));
                }
            }
        }
    } else {
        scan_kind = SRG_SCAN_DENSE;
        if (nloc) {
            c.loss_kind = SRG_LOSS_DENSE_SCAN;
            const size_t lds3 = (size_t)2 * KC * (TS + VE) * sizeof(K);
            set_lds(tight_scan<K, TS, KC>, lds3);
            tight_scan<K, TS, KC><<<dim3((unsigned)(Vp / TS), (nloc + TS - 1) / TS), 256, lds3, st>>>(D, W, Vp, lnodes,
                                                                                                    nloc, PRED);
            k_count_multi<<<nloc, kThreads, 0, st>>>(PRED, nloc, V, Vp, multi_cnt);
            float* L0 = (float*)c.b_L0.get(nmax * Vp * 4);
            float* L1 = (float*)c.b_L1.get(nmax * Vp * 4);
            k_fill<float><<<grid_for((size_t)nloc * Vp), kThreads, 0, st>>>(L0, (size_t)nloc * Vp, 1.0f);
            HIP_CHECK(hipGetLastError());
            ms_scan = tm.lap();
            float* Lin = L0;
            float* Lout = L1;
            for (;;) {
                HIP_CHECK(hipMemsetAsync(&P.flags->changed, 0, 4, st));
                k_loss_round<K><<<grid_for((size_t)nloc * V, 256 * 64), kThreads, 0, st>>>(
                    PRED, D, W, WL, lnodes, nloc, V, Vp, Lin, Lout, P.flags);
                HIP_CHECK(hipGetLastError());
                ++rounds;
                rb_async(c, MS_CHANGED, &P.flags->changed, st);
                HIP_CHECK(hipStreamSynchronize(st));
                const uint32_t ch = rb_get<uint32_t>(c, MS_CHANGED);
                std::swap(Lin, Lout);
                if (!ch) break;
                if (rounds > (int)V + 2) fail(SRG_ERR_INTERNAL, "loss rounds did not converge");
            }
            Lfin = Lin;
        }
    }
    rb_async(c, MS_NMULTI, multi_cnt, st);
    const double ms_loss = tm.lap();
    nmulti = rb_get<unsigned long long>(c, MS_NMULTI);

    if (nloc && !loss_written)
        k_extract<K><<<nloc, kThreads, 0, st>>>(D, Lfin, Vp, lnodes, nloc, nodes, n, lpos,
                                                                      P.selflat, P.selfloss, out_lat, out_loss,
                                                                      P.flags, 2, P.unit);
    HIP_CHECK(hipGetLastError());
    const double ms_extract = tm.lap();

    // ---- output exchange: every rank ends with all n x n rows ----
    double ms_exchange = 0;
    if (exchange) {
        exchange_rows(out_loss, 4);
        st_after_cs();
        ms_exchange = tm.lap();
    }
    if (stats) {
        stats->ms_build += ms_build;
        stats->ms_fw += ms_fw;
        stats->ms_scan += ms_scan;
        stats->ms_loss += ms_loss;
        stats->ms_extract += ms_extract;
        stats->ms_exchange += ms_exchange + ms_dx;
        stats->path_kind = sizeof(K) == 4 ? SRG_PATH_DENSE_U32 : SRG_PATH_DENSE_U64;
        stats->loss_rounds = rounds;
        stats->multi_pred_pairs = nmulti;
        uint64_t own_tiles = 0;  // symmetric FW: this rank's stored tiles ((I + J) mod G == g)
        for (int I = 0; I < pl.nb; ++I)
            for (int J = I; J < pl.nb; ++J) own_tiles += (I + J) % pl.G == pl.g;
        stats->relaxations = sym_fw_for<K, T>(c, g) ? own_tiles * (uint64_t)pl.nb * T * T * T
                                                    : (uint64_t)(pl.rb1 - pl.rb0) * T * Vp * Vp;
        stats->essential_edges = n_ess;
        stats->scan_kind = scan_kind;
        stats->nranks = pl.G;
        stats->rank = pl.g;
        stats->local_sources = nloc;
    }
    return true;
}
