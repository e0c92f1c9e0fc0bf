// h2d_codec.hip.h -- how the host entry's edge list crosses PCIe: the plain copy (copy_plain),
// the narrowing codec with its device-side decoders, worker pool and page-locked rings
// (codec_in), and the late-loss thread (start_late_loss).  A section of routing.hip's translation
// unit, included there after the context and DevGraph / LateLoss (it uses srg_ctx, DevBuf and
// HostPool from the text above it); not a header to include elsewhere.
__global__ void k_widen_edges(size_t n, const uint16_t* __restrict__ s16, const uint16_t* __restrict__ d16,
                              const uint32_t* __restrict__ l32, uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                              uint64_t* __restrict__ lat) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        src[i] = s16[i];
        dst[i] = d16[i];
        lat[i] = l32[i];
    }
}

// Sequential-pair codec, device side: edge i of a chunk is (src, dst) = (es[j], ed[j] + i - ei[j])
// for the last exception j with ei[j] <= i (ei[0] = 0: a chunk starts with one), latency = l32[i].
// Consecutive lanes search the same few exceptions (wave-broadcast loads).
__global__ void k_decode_seq(size_t ne, const uint32_t* __restrict__ l32, const uint32_t* __restrict__ exc, uint32_t nexc,
                             uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint64_t* __restrict__ lat) {
    const uint32_t* ei = exc;
    const uint32_t* es = exc + nexc;
    const uint32_t* ed = exc + 2 * (size_t)nexc;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < ne; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = nexc - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (ei[mid] <= (uint32_t)i) lo = mid;
            else hi = mid - 1;
        }
        src[i] = es[lo];
        dst[i] = ed[lo] + ((uint32_t)i - ei[lo]);
        lat[i] = l32[i];
    }
}

// The edge-sharded exchange's sequential-pair form: edges [e0, e1) of the whole list from every
// slice's exceptions ex = (global index, src, dst) x nexc in index order (each slice starts with
// one, so index 0 is covered) and the u32 latencies.
__global__ void k_decode_seq_global(size_t e0, size_t e1, const uint32_t* __restrict__ l32,
                                    const uint32_t* __restrict__ ex, uint32_t nexc, uint32_t* __restrict__ src,
                                    uint32_t* __restrict__ dst, uint64_t* __restrict__ lat) {
    for (size_t i = e0 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < e1; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = nexc - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (ex[3 * (size_t)mid] <= (uint32_t)i) lo = mid;
            else hi = mid - 1;
        }
        src[i] = ex[3 * (size_t)lo + 1];
        dst[i] = ex[3 * (size_t)lo + 2] + ((uint32_t)i - ex[3 * (size_t)lo]);
        lat[i] = l32[i];
    }
}

template <class T>
T* stage_in(DevBuf& b, const T* host, size_t count, hipStream_t st) {
    T* d = (T*)b.get(std::max<size_t>(count, 1) * sizeof(T));
    if (count) HIP_CHECK(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st));
    return d;
}

// The plain copy: edges [e0, e1) of the caller's four arrays, as they are, into the full-length
// device arrays of dg on st (the losses only with_loss).
void copy_plain(const DevGraph& dg, const srg_edge_list* g, size_t e0, size_t e1, bool with_loss, hipStream_t st) {
    if (e1 <= e0) return;
    const size_t ne = e1 - e0;
    HIP_CHECK(hipMemcpyAsync((uint32_t*)dg.src + e0, g->src + e0, ne * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync((uint32_t*)dg.dst + e0, g->dst + e0, ne * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync((uint64_t*)dg.lat + e0, g->latency_ns + e0, ne * 8, hipMemcpyHostToDevice, st));
    if (with_loss) HIP_CHECK(hipMemcpyAsync((float*)dg.loss + e0, g->packet_loss + e0, ne * 4, hipMemcpyHostToDevice, st));
}

// the host entry's codec worker pool and its page-locked rings (first use, or srg_create's warm-up)
constexpr size_t kCodecChunk = (size_t)2 << 20;  // edges per chunk: 32 MB narrowed (+ loss); losses per chunk: 8 MB
constexpr int kRingSlots = 3;
void ensure_pool(srg_ctx& c) {
    if (c.pool) return;
    c.pool = new HostPool();
    const unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)std::max(1u, std::min(8u, hw ? hw : 1u));
    if (const int e = srg_env::codec_threads()) nt = e;  // experiments
    c.pool->start(nt);
}
void ensure_rings(srg_ctx& c) {
    const size_t slot = kCodecChunk * 16;
    if (c.h_ring_bytes < slot * kRingSlots) {
        if (c.h_ring) HIP_CHECK(hipHostFree(c.h_ring));
        c.h_ring = nullptr;
        c.h_ring_bytes = 0;
        HIP_CHECK(hipHostMalloc(&c.h_ring, slot * kRingSlots, hipHostMallocDefault));
        c.h_ring_bytes = slot * kRingSlots;
    }
    for (Event& e : c.ev_ring) e.create();
    if (!c.h_lring) HIP_CHECK(hipHostMalloc(&c.h_lring, kCodecChunk * 4 * kRingSlots, hipHostMallocDefault));
    for (Event* e : {&c.ev_lring[0], &c.ev_lring[1], &c.ev_lring[2], &c.ev_lin, &c.ev_ldone}) e->create();
}

// H2D codec of the host entry (SRG_OPT_H2D_CODEC): the edge list crosses PCIe narrowed -- u16
// endpoints (V <= 65536) and u32 latencies -- 12 B instead of 20 B per edge, then is widened on
// the device.  Host threads narrow chunk i+1 into a page-locked ring while chunk i is in flight.
// Returns false (nothing usable staged) when an endpoint >= 65536 or a latency >= 2^32 is seen:
// the caller then ships the plain arrays, whose checks report such edges as the reference does.
// on_chunk(e0, ne, exc, nexc, last): edges [e0, e0 + ne) are decoded on the device (in st order); exc =
// their exceptions (global index, src, dst) when the chunk went sequential-pair, else null
// Ships edges [a0, a1) into the full-length device arrays (the rank's slice when the edge list
// is sharded, else all of it).
// Sequential-pair mode (whole lists only; SRG_CODEC_SEQ=0 turns it off): an edge list in
// row order -- a GML complete graph lists (i, i), (i, i+1), ... (i, V-1), then row i+1 -- needs
// no endpoints over PCIe: an edge (s, d) following (s, d - 1) is implied, and only the others
// (row starts, ~V of them) cross as exceptions, so a chunk is its u32 latencies (4 B per edge
// instead of 8) plus ~12 B per row.  A chunk with more than 1/8 exceptions is re-narrowed to
// u16 endpoints and the rest of the list stays in that mode.
// all_narrow: every edge of the slice also stays narrowed on the device (b_n16s / b_n16d / b_n32l),
// false when the host-slow switch shipped the rest of the slice plain.
// all_seq: every chunk of the slice went sequential-pair: its u32 latencies are in b_n32l and its
// exceptions (GLOBAL edge index, src, dst) in c.slice_exc -- the edge-sharded exchange then ships
// that form (4 B per edge) instead of the u16 narrowing (8 B).
using ChunkFn = std::function<void(size_t, size_t, const uint32_t*, size_t, bool)>;
bool codec_in(srg_ctx& c, const srg_edge_list* g, DevGraph& dg, hipStream_t st, size_t a0, size_t a1, bool with_loss,
              bool& all_narrow, bool& all_seq, const ChunkFn& on_chunk = nullptr) {
    all_narrow = true;
    all_seq = false;
    c.slice_exc.clear();
    const auto t_setup = std::chrono::steady_clock::now();
    const size_t E = g->num_edges, A = a1 - a0;
    constexpr size_t CE = kCodecChunk;  // edges per chunk: 32 MB narrowed (+ loss)
    constexpr int NB = kRingSlots;      // ring slots
    const size_t slot = CE * 16;
    ensure_pool(c);
    ensure_rings(c);
    uint16_t* s16 = (uint16_t*)c.b_n16s.get(E * 2);
    uint16_t* d16 = (uint16_t*)c.b_n16d.get(E * 2);
    uint32_t* l32 = (uint32_t*)c.b_n32l.get(E * 4);
    dg.src = (uint32_t*)c.b_src.get(E * 4);
    dg.dst = (uint32_t*)c.b_dst.get(E * 4);
    dg.lat = (uint64_t*)c.b_lat.get(E * 8);
    dg.loss = (float*)c.b_loss.get(E * 4);
    const double ms_setup = ms_since(t_setup);  // (first call: worker threads, pinned ring, device arrays)
    std::atomic<bool> bad{false};     // a latency >= 2^32: the codec cannot carry the list
    std::atomic<bool> bad_ep{false};  // an endpoint >= 65536: only the sequential-pair chunks can
    const bool dbg = srg_env::debug_codec();
    double t_conv = 0, t_wait = 0;
    const size_t nch = (A + CE - 1) / CE;
    bool seq = !srg_env::codec_seq_off();  // (a slice of a row-ordered list is row-ordered too)
    uint32_t* dexc = seq ? (uint32_t*)c.b_exc.get(CE * 4) : nullptr;
    const int nwk = c.pool->size();
    if ((int)c.codec_ex.size() < nwk) c.codec_ex.resize(nwk);
    size_t seq_chunks = 0;
    for (size_t ch = 0; ch < nch; ++ch) {
        const int b = (int)(ch % NB);
        auto tw = std::chrono::steady_clock::now();
        if (ch >= (size_t)NB) HIP_CHECK(hipEventSynchronize(c.ev_ring[b]));  // the slot's previous DMA is done
        const size_t e0 = a0 + ch * CE, ne = std::min(CE, a1 - e0);
        unsigned char* base = (unsigned char*)c.h_ring + (size_t)b * slot;
        uint16_t* hs = (uint16_t*)base;
        uint16_t* hd = hs + CE;
        uint32_t* hl = (uint32_t*)(hd + CE);
        float* hb = (float*)(hl + CE);
        auto tc = std::chrono::steady_clock::now();
        t_wait += std::chrono::duration<double, std::milli>(tc - tw).count();
        std::atomic<bool> dense{false};
        const bool seq_ch = seq;
        c.pool->run([&](int w, int nw) {
            const size_t a = ne * w / nw, z = ne * (w + 1) / nw;
            const uint32_t* src = g->src + e0;
            const uint32_t* dst = g->dst + e0;
            const uint64_t* lat = g->latency_ns + e0;
            uint32_t orx = 0;
            uint64_t orl = 0;
            if (seq_ch) {
                std::vector<uint32_t>& ex = c.codec_ex[w];
                ex.clear();
                if (!seq_encode_slice(src, dst, lat, hl, a, z, ex, 3 * ((z - a) / 8 + 1), orx, orl))
                    dense.store(true, std::memory_order_relaxed);  // (redone below with u16 endpoints)
            } else {
                for (size_t i = a; i < z; ++i) {
                    const uint32_t x = src[i], y = dst[i];
                    const uint64_t l = lat[i];
                    orx |= x | y;
                    orl |= l;
                    hs[i] = (uint16_t)x;
                    hd[i] = (uint16_t)y;
                    hl[i] = (uint32_t)l;
                }
            }
            if (with_loss) std::memcpy(hb + a, g->packet_loss + e0 + a, (z - a) * 4);  // f32 as is
            if (orl >> 32) bad.store(true, std::memory_order_relaxed);
            if (orx >> 16) bad_ep.store(true, std::memory_order_relaxed);
        });
        // sequential-pair chunks never carry u16 endpoints (exceptions are u32): only the u16
        // narrowing needs every endpoint below 65536
        if (seq_ch && dense.load() && bad_ep.load()) bad.store(true);
        if (seq_ch && dense.load() && !bad.load()) {
            // not a row-ordered list: this chunk's endpoints narrowed after all, u16 from here on
            seq = false;
            c.pool->run([&](int w, int nw) {
                const size_t a = ne * w / nw, z = ne * (w + 1) / nw;
                for (size_t i = a; i < z; ++i) {
                    hs[i] = (uint16_t)g->src[e0 + i];
                    hd[i] = (uint16_t)g->dst[e0 + i];
                }
            });
        }
        const bool chunk_seq = seq_ch && !dense.load();
        if (!chunk_seq && bad_ep.load()) bad.store(true);
        const double dt = ms_since(tc);
        t_conv += dt;
        if (bad.load()) {
            HIP_CHECK(hipStreamSynchronize(st));  // no DMA may still read the ring
            return false;
        }
        // the host is busy (narrowing takes longer than shipping the chunks plain would at ~55 GB/s):
        // the remaining edges go plain, straight from the caller's arrays.  Judged on the average over
        // the chunks so far, past the first, with a 1.5x margin: shipping plain also gives up the FW
        // beside the H2D (~5 ms at C3), and a single chunk slowed by the caller's fresh table being
        // faulted in beside it (0.79 ms against 0.76) switched a C3 first call over (round 6)
        const double plain_ms = (double)ne * 20.0 / 55e9 * 1e3;
        bool slow = ch + 1 < nch && ch >= 1 && t_conv / (double)(ch + 1) > 1.5 * plain_ms;
        if (size_t k = 0; srg_env::codec_slow_after(k)) slow = ch + 1 < nch && ch >= k;  // tests
        if (chunk_seq) {
            // the workers' exception lists, in order, as SoA (index | src | dst) where the u16
            // endpoints would have gone
            size_t nexc = 0;
            for (int w = 0; w < nwk; ++w) nexc += c.codec_ex[w].size() / 3;
            uint32_t* hx = (uint32_t*)hs;
            size_t q = 0;
            const size_t x0 = c.slice_exc.size();
            for (int w = 0; w < nwk; ++w) {
                const std::vector<uint32_t>& ex = c.codec_ex[w];
                for (size_t k = 0; k + 2 < ex.size(); k += 3, ++q) {
                    hx[q] = ex[k];
                    hx[nexc + q] = ex[k + 1];
                    hx[2 * nexc + q] = ex[k + 2];
                    c.slice_exc.push_back((uint32_t)(e0 + ex[k]));  // global index, src, dst
                    c.slice_exc.push_back(ex[k + 1]);
                    c.slice_exc.push_back(ex[k + 2]);
                }
            }
            HIP_CHECK(hipMemcpyAsync(l32 + e0, hl, ne * 4, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(dexc, hx, nexc * 12, hipMemcpyHostToDevice, st));
            if (with_loss) HIP_CHECK(hipMemcpyAsync((float*)dg.loss + e0, hb, ne * 4, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipEventRecord(c.ev_ring[b], st));
            k_decode_seq<<<grid_for(ne), kThreads, 0, st>>>(ne, l32 + e0, dexc, (uint32_t)nexc, (uint32_t*)dg.src + e0,
                                                             (uint32_t*)dg.dst + e0, (uint64_t*)dg.lat + e0);
            ++seq_chunks;
            if (on_chunk) on_chunk(e0, ne, c.slice_exc.data() + x0, nexc, ch + 1 == nch && !slow);
        } else {
            HIP_CHECK(hipMemcpyAsync(s16 + e0, hs, ne * 2, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(d16 + e0, hd, ne * 2, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(l32 + e0, hl, ne * 4, hipMemcpyHostToDevice, st));
            if (with_loss) HIP_CHECK(hipMemcpyAsync((float*)dg.loss + e0, hb, ne * 4, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipEventRecord(c.ev_ring[b], st));
            k_widen_edges<<<grid_for(ne), kThreads, 0, st>>>(ne, s16 + e0, d16 + e0, l32 + e0, (uint32_t*)dg.src + e0,
                                                              (uint32_t*)dg.dst + e0, (uint64_t*)dg.lat + e0);
            if (on_chunk) on_chunk(e0, ne, nullptr, 0, ch + 1 == nch && !slow);
        }
        HIP_CHECK(hipGetLastError());
        if (slow) {
            const size_t r0 = e0 + ne, rn = a1 - r0;
            copy_plain(dg, g, r0, a1, with_loss, st);
            if (dbg) std::fprintf(stderr, "codec: host slow after chunk %zu (%.2f ms), rest plain\n", ch, dt);
            if (on_chunk) on_chunk(r0, rn, nullptr, 0, true);
            all_narrow = false;
            break;
        }
    }
    if (seq_chunks) all_narrow = false;  // (the endpoints are not on the device narrowed)
    all_seq = seq_chunks == nch && nch > 0;
    if (dbg) std::fprintf(stderr, "codec: %zu chunks (%zu sequential-pair), %d threads, setup %.2f ms, convert %.2f ms, slot waits %.2f ms\n",
                          nch, seq_chunks, c.pool->size(), ms_setup, t_conv, t_wait);
    return true;
}

// Late loss H2D: a helper thread copies the losses chunk by chunk into a pinned ring and queues
// each chunk's DMA on c.loss_stream behind the last endpoint/latency chunk (so the two never
// share the PCIe link); loss_arrive() later joins it and orders the readers after the last DMA.
void start_late_loss(srg_ctx& c, const srg_edge_list* g, DevGraph& dg, hipStream_t st, LateLoss& L, size_t a0 = 0,
                     size_t a1 = ~(size_t)0) {
    ensure_rings(c);
    L.ev_in = c.ev_lin;
    L.ev_done = c.ev_ldone;
    HIP_CHECK(hipEventRecord(c.ev_ledges, st));
    HIP_CHECK(hipStreamWaitEvent(c.loss_stream, c.ev_ledges, 0));
    dg.late = &L;
    const int device = c.device;
    L.th = std::thread([&c, g, &dg, &L, device, a0, a1]() {
        try {
            HIP_CHECK(hipSetDevice(device));
            const bool dbg = srg_env::debug_overlap();
            const auto t0 = std::chrono::steady_clock::now();
            double t_copy = 0, t_wait = 0;
            const size_t E = std::min<size_t>(g->num_edges, a1);  // this rank's slice [a0, E)
            float* dloss = const_cast<float*>(dg.loss);
            for (size_t ch = 0, e0 = a0; e0 < E; ++ch, e0 += kCodecChunk) {
                const int b = (int)(ch % kRingSlots);
                auto ta = std::chrono::steady_clock::now();
                if (ch >= (size_t)kRingSlots) HIP_CHECK(hipEventSynchronize(c.ev_lring[b]));
                auto tb = std::chrono::steady_clock::now();
                const size_t ne = std::min(kCodecChunk, E - e0);
                float* slot = (float*)c.h_lring + (size_t)b * kCodecChunk;
                c.pool->run([&](int w, int nw) {
                    const size_t a = ne * w / nw, z = ne * (w + 1) / nw;
                    std::memcpy(slot + a, g->packet_loss + e0 + a, (z - a) * 4);
                });
                t_wait += std::chrono::duration<double, std::milli>(tb - ta).count();
                t_copy += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count();
                HIP_CHECK(hipMemcpyAsync(dloss + e0, slot, ne * 4, hipMemcpyHostToDevice, c.loss_stream));
                HIP_CHECK(hipEventRecord(c.ev_lring[b], c.loss_stream));
            }
            HIP_CHECK(hipEventRecord(L.ev_in, c.loss_stream));
            if (dbg) {
                HIP_CHECK(hipEventSynchronize(L.ev_in));
                std::fprintf(stderr, "late loss thread: %.2f ms to the last DMA, host copies %.2f ms, ring waits %.2f ms\n",
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                             t_copy, t_wait);
            }
        } catch (const Failure& f) {
            L.err = f.msg;
        } catch (const std::exception& e) {
            L.err = e.what();
        }
    });
}
