// host_entry.hip.h -- the host entry (host arrays in, host tables out), stage by stage; host_entry()
// at the end is the list of the stages, and the decisions that are pure functions of the call's
// arguments come from entry_plan.h.  A section of routing.hip's translation unit, included there
// after h2d_codec.hip.h and guard() (it uses srg_ctx, HostSink, FwOverlap, compute_device and
// direct_device from the text above it); not a header to include elsewhere.

// ---- argument checks ----
int check_entry_args(const srg_ctx* c, const srg_edge_list* g, const uint32_t* nodes, uint32_t num_nodes,
                     const uint64_t* out_lat, const float* out_loss, bool direct, const uint32_t* out_key,
                     const uint64_t* out_diag, char* errbuf, size_t errlen) {
    const bool keys = out_key != nullptr;
    if (keys && (direct || (c && c->comm && c->comm->nranks > 1) || (num_nodes && !out_diag))) {
        set_err(errbuf, errlen, "key table: one rank, shortest paths only");
        return SRG_ERR_ARG;
    }
    if (!c || !g || (num_nodes && (!nodes || !(out_lat || keys) || !out_loss)) ||
        (g->num_edges && (!g->src || !g->dst || !g->latency_ns || !g->packet_loss))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return SRG_OK;
}

// ---- OutputPinning ----
// Page-locks the caller's output arrays on a helper thread, concurrently with the H2D copy
// and FW (≈10 ms for the 1.2 GB C3 table, measured), so finished rows can be DMA'd out
// asynchronously while later kernels run.  Small tables are copied at the end.
struct OutputPinning {
    int device = 0;
    std::thread th;
    bool ok = false;
    double ms = 0;
    void* p[2] = {nullptr, nullptr};
    void* view[2] = {nullptr, nullptr};  // device pointers of the mapped registrations
    size_t b[2] = {0, 0};
    hipStream_t wait = nullptr;
    bool fault = true;
    srg_table* tab[2] = {nullptr, nullptr};  // pooled tables (RoutingInfo): stay registered after the call
    bool join() {
        if (th.joinable()) th.join();
        return ok;
    }
    void run() {
        const auto t0 = std::chrono::steady_clock::now();
        if (!b[0] || hipSetDevice(device) != hipSuccess) return;
        for (int i = 0; i < 2; ++i) {
            if (tab[i] && tab[i]->registered) {  // a recycled pooled table: nothing to do
                view[i] = tab[i]->view;
                continue;
            }
            advise_huge(p[i], b[i]);
            if (fault) prefault(p[i], b[i], 8);
            if (hipHostRegister(p[i], b[i], hipHostRegisterMapped) != hipSuccess) {
                if (i == 1 && !tab[0]) (void)hipHostUnregister(p[0]);
                return;
            }
            if (hipHostGetDevicePointer(&view[i], p[i], 0) != hipSuccess) view[i] = nullptr;
            if (tab[i]) tab[i]->registered = true, tab[i]->view = view[i];
        }
        ms = ms_since(t0);
        ok = true;
    }
    ~OutputPinning() {
        if (th.joinable()) th.join();
        if (ok) {
            (void)hipStreamSynchronize(wait);  // no copy into the buffers may be in flight
            for (int i = 0; i < 2; ++i)
                if (!tab[i]) (void)hipHostUnregister(p[i]);
        }
    }
};

// Starts it when rows leave early and the caller has not page-locked the tables itself (ext).
// A rank that fills only its own rows of a table the ranks share (ep.rows_part, one process per
// GPU) page-locks only those rows: N processes pinning the whole shared table each cost N times the
// pinning, and a shared-memory table is typically 4-KB pages (~50 ms per 1.2 GB)
void start_pinning(OutputPinning& reg, const srg_ctx& c, const EntryPlan& ep, bool ext, unsigned char* lat_b,
                   size_t lat_elem, float* out_loss, size_t n, srg_table* const* tabs) {
    reg.device = c.device;
    reg.wait = c.d2h_stream;
    reg.fault = srg_env::prefault_on();  // A/B
    if (!ep.early || ext) return;
    // pooled tables (srg_internal_compute_table): the whole mapping is registered once and kept
    const bool pooled = !ep.rows_part && tabs && tabs[0] && tabs[1] && tabs[0]->p == lat_b &&
                        tabs[1]->p == (void*)out_loss && tabs[0]->cap >= n * n * lat_elem && tabs[1]->cap >= n * n * 4;
    reg.p[0] = lat_b + ep.rows.lo * n * lat_elem;
    reg.b[0] = ep.rows.size() * n * lat_elem;
    reg.p[1] = out_loss + ep.rows.lo * n;
    reg.b[1] = ep.rows.size() * n * 4;
    if (pooled)
        for (int i = 0; i < 2; ++i) reg.tab[i] = tabs[i], reg.b[i] = tabs[i]->cap;
    reg.th = std::thread([r = &reg]() { r->run(); });
}

// ---- ship_edges ----
struct Shipped {
    bool coded = false;                        // the codec carried this rank's edges (else they went plain)
    bool all_narrow = false, all_seq = false;  // codec_in's: what of them stays narrowed on the device
    hipStream_t hst = nullptr;                 // the stream the edges crossed on
};
// This rank's edges ep.edges over PCIe into dg's full-length device arrays: the overlap decision,
// the codec or the plain copy, the late-loss start, a simulated rank's other slices.  dg is the
// caller's: the late-loss thread keeps its address.  sparse: choose_sparse of the edge list.
Shipped ship_edges(srg_ctx& c, const srg_edge_list* g, const uint32_t* nodes, size_t n, bool direct, bool sparse,
                   const EntryPlan& ep, bool sim, hipStream_t st, DevGraph& dg, FwOverlap& ov, LateLoss& late,
                   srg_stats* stats) {
    const size_t E = g->num_edges, a0 = ep.edges.lo, a1 = ep.edges.hi;
    Shipped sh;
    // narrowed edge list over PCIe when it fits (falls back to the plain arrays otherwise)
    // late loss: the losses follow the endpoints and latencies on their own stream, beside
    // the W build and FW (dense u32 path: WL is built from them on c.loss_stream)
    // (edge-sharded ranks ship their slices' losses late too; the slices are exchanged when
    // the losses are first read, after FW -- loss_arrive)
    const bool want_late = c.late_loss && !direct;
    // FW beside the H2D (FwOverlap): one rank, undirected, the dense symmetric two-stream FW on
    // 128-tiles, the codec with late losses; the chunks then cross on the comm stream (idle on
    // one rank) while FW runs on the main stream
    const bool ov_want = c.fw_overlap && !direct && ep.nr == 1 && want_late && c.h2d_codec && E >= ((size_t)1 << 20) &&
                         !g->directed && c.fw_symmetric && (c.fw_tile == 0 || c.fw_tile == 128) &&
                         g->num_vertices >= 256 && n > 0 && !sparse;
    if (ov_want) {
        HIP_CHECK(hipStreamSynchronize(c.aux_stream));  // nothing of an aborted call still runs
        ov.init(c, g->num_vertices, std::vector<uint32_t>(nodes, nodes + n));
    }
    const hipStream_t hst = sh.hst = ov.on ? c.comm_stream : st;
    ChunkFn on_chunk = nullptr;
    if (ov.on) on_chunk = [&](size_t e0, size_t ne, const uint32_t* exc, size_t nexc, bool last) {
        ov.chunk(dg, e0, ne, exc, nexc, last);
    };
    // (V > 65536: only a row-ordered list, through the sequential-pair chunks, can be narrowed;
    // codec_in gives up on the first chunk that is neither)
    const bool coded = sh.coded = c.h2d_codec && a1 - a0 >= ((size_t)1 << 20) &&
                                  codec_in(c, g, dg, hst, a0, a1, !want_late, sh.all_narrow, sh.all_seq, on_chunk);
    if (ov.on) ov.finish();  // the FW thread has enqueued every landed chunk's work
    if (ov.on && !coded) ov.ok = false;
    const int ov_early = ov.next;  // pivots enqueued while chunks were still crossing
    if (stats && ov.on && ov.ok) stats->fw_overlap_pivots = ov_early;
    if (ov.on && ov.ok && !ov.ended) ov.advance(ov.nb - 1);
    if (ov.on && srg_env::debug_overlap()) {
        std::fprintf(stderr, "fw-overlap: ok=%d pivots_during_h2d=%d of %d\n", ov.ok ? 1 : 0, ov_early, ov.nb);
        if (ov.ok) ov.report();
    }
    // (started here, after the remaining pivots are enqueued -- an enqueue that holds this thread
    // until FW nears its end -- the losses land ~3 ms after FW, but that wait overlaps GPU work:
    // starting the thread before it measured 46.9-47.4 vs 46.5-46.6 ms, profiles/r06/late_loss/)
    late.ls = c.loss_stream;
    if (coded && want_late) start_late_loss(c, g, dg, hst, late, a0, a1);
    if (!coded) {
        const size_t cnt = std::max<size_t>(E, 1);
        dg.src = (uint32_t*)c.b_src.get(cnt * 4);
        dg.dst = (uint32_t*)c.b_dst.get(cnt * 4);
        dg.lat = (uint64_t*)c.b_lat.get(cnt * 8);
        dg.loss = (float*)c.b_loss.get(cnt * 4);
        copy_plain(dg, g, a0, a1, true, st);
    }
    if (sim && (c.sim_edges != g->src || c.sim_E != E)) {
        // SRG_OPT_SIMULATE_RANK elides the exchange: the other slices are shipped once per
        // edge list (a warm-up call), so later calls time this rank's slice and stay valid
        copy_plain(dg, g, 0, a0, true, st);
        copy_plain(dg, g, a1, E, true, st);
        c.sim_edges = g->src;
        c.sim_E = E;
    }
    return sh;
}

// ---- exchange_slices ----
// Multi-rank: every rank needs the whole edge list (W's rows feed the essential-entry records of
// every source), but each GPU has its own PCIe link and the GPUs a mesh of their own: rank r ships
// the edges rank_rows(E, r, N) (ep.edges, the same on every rank's count) and the slices are
// exchanged here, device to device on st.  Every rank runs the same sequence of collectives and
// host synchronisations.
void exchange_slices(srg_ctx& c, const srg_edge_list* g, const DevGraph& dg, const EntryPlan& ep, const Shipped& sh,
                     bool sim, hipStream_t st) {
    const size_t E = g->num_edges, a0 = ep.edges.lo, a1 = ep.edges.hi;
    const int nr = ep.nr, rk = ep.rk;
    std::vector<size_t> offs(nr), lens(nr);
    auto gather = [&](const void* p, size_t elem) {
        slice_tables(E, nr, elem, offs, lens);
        c.comm->allgatherv(const_cast<void*>(p), offs.data(), lens.data(), st);
    };
    // the narrowest form every rank has: 0 = sequential-pair (each slice's u32 latencies +
    // exceptions: 4 B per edge with the loss 8), 1 = u16 narrowing (8 B, 12 with the loss),
    // 2 = plain (a rank shipped its slice plain: 20 B)
    // forms 0 / 1: every rank is coded, so every rank ships its losses late -- exchanged when
    // first read (loss_arrive); else now
    auto late_or_gather_loss = [&]() {
        if (dg.late) {
            dg.late->comm = c.comm;
            slice_tables(E, nr, 4, dg.late->offs, dg.late->lens);
        } else {
            gather(dg.loss, 4);
        }
    };
    // the other ranks' slices, received narrowed, to the wide arrays
    // (a simulated rank received nothing: its other slices are the wide ones put once)
    auto decode_others = [&](auto&& launch) {
        for (auto [e0, e1] : {std::pair<size_t, size_t>{0, a0}, std::pair<size_t, size_t>{a1, E}})
            if (e1 > e0 && !sim) launch(e0, e1);
        HIP_CHECK(hipGetLastError());
    };
    uint32_t* plain = (uint32_t*)c.b_red.get(16);
    const uint32_t mine = offered_form(sh.coded, sh.all_seq, sh.all_narrow);
    HIP_CHECK(hipMemcpyAsync(plain, &mine, 4, hipMemcpyHostToDevice, st));
    c.comm->allreduce_max_u32(plain, 1, st);
    uint32_t form = 2;
    HIP_CHECK(hipMemcpyAsync(&form, plain, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (form == 0) {
        // every slice's exception count, then every slice's exceptions (global index, src,
        // dst), the u32 latencies and the losses; the other slices are decoded here
        const size_t xbase = ((size_t)nr * 4 + 255) / 256 * 256;
        uint32_t* xc = (uint32_t*)c.b_xexc.get(xbase);
        const uint32_t my_n = (uint32_t)(c.slice_exc.size() / 3);
        HIP_CHECK(hipMemcpyAsync(xc + rk, &my_n, 4, hipMemcpyHostToDevice, st));
        for (int q = 0; q < nr; ++q) {
            offs[q] = (size_t)q * 4;
            lens[q] = 4;
        }
        c.comm->allgatherv(xc, offs.data(), lens.data(), st);
        std::vector<uint32_t> cnt(nr);
        HIP_CHECK(hipMemcpyAsync(cnt.data(), xc, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (sim)
            for (int q = 0; q < nr; ++q) cnt[q] = my_n;  // (a simulated rank hears nothing: its own size)
        size_t tot = 0, mine_at = 0;
        for (int q = 0; q < nr; ++q) {
            if (q == rk) mine_at = tot;
            offs[q] = xbase + tot * 12;
            lens[q] = (size_t)cnt[q] * 12;
            tot += cnt[q];
        }
        unsigned char* xb = (unsigned char*)c.b_xexc.get(xbase + std::max<size_t>(tot, 1) * 12);
        if (my_n)
            HIP_CHECK(hipMemcpyAsync(xb + xbase + mine_at * 12, c.slice_exc.data(), (size_t)my_n * 12,
                                     hipMemcpyHostToDevice, st));
        c.comm->allgatherv(xb, offs.data(), lens.data(), st);
        uint32_t* l32 = (uint32_t*)c.b_n32l.p;
        gather(l32, 4);
        late_or_gather_loss();
        decode_others([&](size_t e0, size_t e1) {
            k_decode_seq_global<<<grid_for(e1 - e0), kThreads, 0, st>>>(e0, e1, l32, (const uint32_t*)(xb + xbase),
                                                                         (uint32_t)tot, (uint32_t*)dg.src,
                                                                         (uint32_t*)dg.dst, (uint64_t*)dg.lat);
        });
    } else if (form == 1) {
        uint16_t* s16 = (uint16_t*)c.b_n16s.p;
        uint16_t* d16 = (uint16_t*)c.b_n16d.p;
        uint32_t* l32 = (uint32_t*)c.b_n32l.p;
        gather(s16, 2);
        gather(d16, 2);
        gather(l32, 4);
        late_or_gather_loss();
        decode_others([&](size_t e0, size_t e1) {
            k_widen_edges<<<grid_for(e1 - e0), kThreads, 0, st>>>(e1 - e0, s16 + e0, d16 + e0, l32 + e0, (uint32_t*)dg.src + e0,
                                                                   (uint32_t*)dg.dst + e0, (uint64_t*)dg.lat + e0);
        });
    } else {
        gather(dg.src, 4);
        gather(dg.dst, 4);
        gather(dg.lat, 8);
        if (dg.late) {  // (some rank shipped plain: no late exchange; this rank's losses first)
            dg.late->join();
            HIP_CHECK(hipStreamWaitEvent(st, dg.late->ev_in, 0));
        }
        gather(dg.loss, 4);
    }
}

// ---- device tables and key mode ----
struct DevTables {
    uint64_t* lat = nullptr;   // n x n latencies, indexed by absolute row
    float* loss = nullptr;     // n x n losses, likewise
    uint32_t* key = nullptr;   // key mode: the u32 key table in the latency buffer's room
    uint64_t* diag = nullptr;  // key mode: the diagonal beside it (raw self-loop latencies per position)
};

// The device holds this rank's rows ep.rows only -- all n, or without the output exchange the
// plan's split [p0, p1) (make_plan / run_sparse); lat / loss then point p0 rows before that
// allocation, so the kernels' absolute row indices land in it (C4 at 8 ranks: 3.75 GB per
// GPU instead of 30 GB)
DevTables output_tables(srg_ctx& c, const EntryPlan& ep, size_t n) {
    const size_t q0 = ep.rows.lo, dev_nn = ep.rows.size() * n;
    DevTables t;
    t.lat = reinterpret_cast<uint64_t*>(reinterpret_cast<uintptr_t>(c.b_olat.get(std::max<size_t>(dev_nn, 1) * 8)) -
                                        q0 * n * 8);
    t.loss = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(c.b_oloss.get(std::max<size_t>(dev_nn, 1) * 4)) -
                                      q0 * n * 4);
    return t;
}

// u64 output of a dense u32 build on one rank: the latency rows cross PCIe as the build's u32
// keys and are widened on the host (HostSink::send_keys; 0.6 GB less D2H at C3); a build that
// turns out to need u64 keys ships the u64 rows instead (run_dense clears sink.widen)
bool wants_key_rows(const srg_ctx& c, const EntryPlan& ep, bool keys, bool direct, size_t n, bool sparse) {
    return !keys && !direct && ep.early && ep.nr == 1 && c.sdma.ok && c.d2h_mode == 1 && c.h_ring && c.pool &&
           n * 4 <= c.h_ring_bytes / 3 && !srg_env::no_key_d2h() && !sparse;
}

// key mode: the device key table in the latency buffer's room, the diagonal beside it; the
// kernels see them through the context for this call
struct KeyScope {
    srg_ctx& c;
    KeyScope(srg_ctx& c_, DevTables& t, bool kmode, size_t n) : c(c_) {
        t.key = kmode ? reinterpret_cast<uint32_t*>(t.lat) : nullptr;
        t.diag = kmode ? (uint64_t*)c.b_odiag.get(std::max<size_t>(n, 1) * 8) : nullptr;
        c.kout_key = t.key;
        c.kout_diag = t.diag;
    }
    ~KeyScope() { c.kout_key = nullptr, c.kout_diag = nullptr; }
};

// the sink the build hands finished rows to; with ep.early they leave while later kernels run,
// once the tables are page-locked (by reg, or by the caller: ext)
void wire_sink(HostSink& sink, srg_ctx& c, const EntryPlan& ep, bool ext, OutputPinning& reg, uint64_t* host_lat,
               float* out_loss, size_t n, bool ikeys) {
    sink.lat = host_lat;
    sink.widen = ikeys;
    sink.pool = c.pool;
    sink.ring = (unsigned char*)c.h_ring;
    sink.ring_slot = c.h_ring_bytes / 3;
    sink.loss = out_loss;
    sink.n = n;
    sink.cs = c.d2h_stream;
    sink.ev = c.ev_e;
    if (!ep.early) return;
    sink.mode = c.d2h_mode;
    sink.sdma = &c.sdma;
    sink.device = c.device;
    if (ext) {
        sink.ready = [cp = &c, pin = &reg, s = &sink]() {
            void* v[2] = {nullptr, nullptr};
            if (!cp->ext_reg(v, &pin->ms)) return false;
            s->lat_view = v[0];
            s->loss_view = v[1];
            return true;
        };
    } else {
        sink.ready = [pin = &reg, s = &sink, reg_r0 = ep.rows.lo, n]() {
            if (!pin->join()) return false;
            // views of rows [reg_r0, ...): based so that row r lands at view + r * n
            s->lat_view = (unsigned char*)pin->view[0] - reg_r0 * n * 8;
            s->loss_view = (unsigned char*)pin->view[1] - reg_r0 * n * 4;
            return true;
        };
    }
}

// ---- ship_tail ----
// What is left on the device after the build: the minimum-latency reduction, whatever rows were
// not sent early, the diagonal.  Multi-rank without the output exchange: only this rank's rows
// ep.rows leave the device (possibly none), and the minimum is over those rows only.
// Returns the smallest latency over those rows (~0: none, or no stats asked for).
unsigned long long ship_tail(srg_ctx& c, const EntryPlan& ep, size_t n, bool keys, bool ikeys, const DevTables& t,
                             HostSink& sink, uint64_t* out_lat, uint32_t* out_key, uint64_t* out_diag, float* out_loss,
                             const srg_stats* stats, hipStream_t st) {
    const bool kmode = keys || ikeys;
    const size_t r0 = ep.rows.lo, r1 = ep.rows.hi;
    const size_t rows_off = r0 * n, rows_nn = r1 > r0 ? (r1 - r0) * n : 0;
    unsigned long long hmin = ~0ull;
    if (rows_nn && stats) {  // smallest latency over the table (feeds the runahead, manager.rs:238-243)
        unsigned long long* dmin = (unsigned long long*)c.b_multi.get(16);
        HIP_CHECK(hipMemsetAsync(dmin, 0xFF, 16, st));
        if (kmode) {  // smallest key (x unit below) and smallest diagonal latency
            k_min_u32<<<grid_for(rows_nn, 1024), kThreads, 0, st>>>(t.key + rows_off, rows_nn, dmin);
            k_min_u64<<<grid_for(n, 1024), kThreads, 0, st>>>(t.diag, n, dmin + 1);
        } else {
            k_min_u64<<<grid_for(rows_nn, 1024), kThreads, 0, st>>>(t.lat + rows_off, rows_nn, dmin);
        }
        HIP_CHECK(hipMemcpyAsync(c.hbox + 64 * MS_MIN, dmin, 16, hipMemcpyDeviceToHost, st));
    }
    if (rows_nn && !sink.lat_sent) {
        if (keys)
            HIP_CHECK(hipMemcpyAsync(out_key + rows_off, t.key + rows_off, rows_nn * 4, hipMemcpyDeviceToHost, st));
        else if (!ikeys)
            HIP_CHECK(hipMemcpyAsync(out_lat + rows_off, t.lat + rows_off, rows_nn * 8, hipMemcpyDeviceToHost, st));
    }
    if (keys && n) HIP_CHECK(hipMemcpyAsync(out_diag, t.diag, n * 8, hipMemcpyDeviceToHost, st));
    std::vector<uint64_t> hdiag(ikeys ? n : 0);  // the diagonal the widened rows are patched with
    if (ikeys && n) HIP_CHECK(hipMemcpyAsync(hdiag.data(), t.diag, n * 8, hipMemcpyDeviceToHost, st));
    if (rows_nn && !sink.loss_sent)
        HIP_CHECK(hipMemcpyAsync(out_loss + rows_off, t.loss + rows_off, rows_nn * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (rows_nn && stats) {
        hmin = rb_get<unsigned long long>(c, MS_MIN);
        if (kmode) {
            const unsigned long long dmin = *reinterpret_cast<const unsigned long long*>(c.hbox + 64 * MS_MIN + 8);
            const uint64_t unit = stats->latency_unit_ns ? stats->latency_unit_ns : 1;
            hmin = std::min<unsigned long long>(hmin == ~0ull ? ~0ull : hmin * unit, dmin);
        }
    }
    if (ikeys && rows_nn && !sink.lat_sent) {
        // the rows were not shipped early (the caller's tables could not be page-locked): keys now
        sink.send_keys(st, t.key, r0, r1 - r0, sink.key_unit);
        sink.lat_sent = true;
    }
    sink.finish();
    if (ikeys)
        for (size_t r = r0; r < r1; ++r) out_lat[r * n + r] = hdiag[r];  // raw self-loop weights (mod.rs:211-217)
    return hmin;
}

// ---- the host entry ----
// out_key / out_diag (srg_internal_compute_table, RoutingInfo's key table): non-null = the latencies
// leave as the build's u32 keys plus the diagonal's raw self-loop latencies; out_lat is unused then
int host_entry(srg_ctx* c, const srg_edge_list* g, const uint32_t* nodes, uint32_t num_nodes, uint64_t* out_lat,
               float* out_loss, srg_stats* stats, char* errbuf, size_t errlen, bool direct,
               uint32_t* out_key = nullptr, uint64_t* out_diag = nullptr, srg_table* const* tabs = nullptr) {
    if (const int rc = check_entry_args(c, g, nodes, num_nodes, out_lat, out_loss, direct, out_key, out_diag, errbuf, errlen))
        return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    const bool keys = out_key != nullptr;
    const size_t n = num_nodes;
    const EntryPlan ep = make_entry_plan(direct, n, g->num_edges, c->comm ? c->comm->nranks : 1,
                                         c->comm ? c->comm->rank : 0, c->gather_output, c->edge_shard);
    const bool ext = (bool)c->ext_reg;  // the caller page-locked the tables (srg_multi)
    OutputPinning reg;
    start_pinning(reg, *c, ep, ext, keys ? (unsigned char*)out_key : (unsigned char*)out_lat, keys ? 4 : 8, out_loss, n,
                  tabs);
    return guard(errbuf, errlen, [&]() {
        auto t0 = std::chrono::steady_clock::now();
        if (stats) std::memset(stats, 0, sizeof(*stats));
        HIP_CHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        DevGraph dg{g->num_vertices, (int)g->directed, g->num_edges, nullptr, nullptr, nullptr, nullptr,
                    nullptr, g->node_ids};
        const bool sparse = choose_sparse(*c, dg);  // (of V, E and directed only)
        const bool sim = ep.shard && std::strcmp(c->comm->kind(), "simulated") == 0;
        FwOverlap ov;
        LateLoss late;
        const Shipped sh = ship_edges(*c, g, nodes, n, direct, sparse, ep, sim, st, dg, ov, late, stats);
        if (ep.shard) exchange_slices(*c, g, dg, ep, sh, sim, st);
        const uint32_t* dn = stage_in(c->b_nodes, nodes, n, sh.hst);
        if (sh.hst != st) {  // the main stream's later work reads the landed edges and nodes
            HIP_CHECK(hipEventRecord(c->ev_c, sh.hst));
            HIP_CHECK(hipStreamWaitEvent(st, c->ev_c, 0));
        }
        DevTables dt = output_tables(*c, ep, n);
        HIP_CHECK(hipStreamSynchronize(sh.hst));  // (beside FW when it started early: st still runs it)
        const double ms_h2d = ms_since(t0);
        bool ikeys = wants_key_rows(*c, ep, keys, direct, n, sparse);
        KeyScope key_scope(*c, dt, keys || ikeys, n);
        HostSink sink;
        // (a host table pointer either way)
        wire_sink(sink, *c, ep, ext, reg, keys ? reinterpret_cast<uint64_t*>(out_key) : out_lat, out_loss, n, ikeys);
        if (direct) {
            direct_device(*c, dg, dn, num_nodes, dt.lat, dt.loss, st);
        } else {
            compute_device(*c, dg, dn, num_nodes, dt.lat, dt.loss, st, stats, ep.early ? &sink : nullptr,
                           ov.on ? &ov : nullptr);
            if (ikeys && !sink.widen) {  // the build took u64 keys (run_dense dropped the key table)
                ikeys = false;
                dt.key = nullptr, dt.diag = nullptr;
            }
        }
        if (dg.late) {  // a path that never read the losses (error-free early return): drain
            dg.late->join();
            HIP_CHECK(hipStreamSynchronize(c->loss_stream));
        }
        auto t1 = std::chrono::steady_clock::now();
        const unsigned long long hmin =
            ship_tail(*c, ep, n, keys, ikeys, dt, sink, out_lat, out_key, out_diag, out_loss, stats, st);
        if (stats) {
            stats->ms_h2d = ms_h2d;
            stats->ms_d2h = ms_since(t1);  // the D2H not hidden behind kernels
            stats->ms_total = ms_since(t0);
            stats->ms_host_register = ext ? (sink.registered ? reg.ms : -1.0) : reg.join() ? reg.ms : -1.0;
            stats->d2h_overlapped_bytes = sink.early_bytes;
            stats->d2h_key_rows = ikeys ? 1 : 0;
            stats->ms_key_widen = sink.ms_widen;
            stats->min_latency_ns = hmin;
            if (direct) stats->path_kind = SRG_PATH_DIRECT;
        }
    });
}
