// events_run.hip.h -- the host side of the packet-event batch (events.hip.h) and of the device-
// resident per-host event queues (event_queue.hip.h): the drivers behind
// srg_order_packet_events_device, srg_send_packets_device and srg_event_queues_*_device, and the
// srg_event_queues_* entry points themselves (the two batch calls' stay in routing.hip).  A section
// of routing.hip's translation unit, included there once inside its anonymous namespace (it uses
// srg_ctx, DevBuf, fail, grid_for, guard and device_call from the text above it and the helpers of
// stage.hip.h); not a header to include elsewhere.  struct srg_event_queues is the C ABI's opaque
// type and the entry points are extern "C", so the section leaves the anonymous namespace twice --
// around the struct with create / destroy, and around push / pop behind the drivers -- and enters
// it again.
//
// One batch driver serves both batch calls: event_batch_device<false> is the order call (starts at
// the latency lookup), event_batch_device<true> the send call (the drop decision in front, the
// packet counters, the dropped events parked).  Every path that queued work synchronises `st` before
// it returns; the entry points add no synchronise of their own.

inline uint32_t bit_width64(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

// status / n_order: a send batch with dropped events (status[i] == 0) -- they are parked behind host
// num_hosts, and only the n_order sent indices in front of them reach out_order
template <bool WIDE>
void events_sort(srg_ctx& c, const EvIn& in, const uint64_t* deliver, const EvKeyFmt& f, uint32_t bits,
                 uint32_t* out_order, uint64_t* host_off, hipStream_t st, uint32_t& passes,
                 const uint8_t* status = nullptr, uint64_t n_order = ~0ull) {
    const uint64_t n = in.n;
    if (!status) n_order = n;
    unsigned long long* k0 = (unsigned long long*)c.b_ek0.get(n * 8);
    unsigned long long* k1 = (unsigned long long*)c.b_ek1.get(n * 8);
    unsigned long long* h0 = WIDE ? (unsigned long long*)c.b_eh0.get(n * 8) : nullptr;
    unsigned long long* h1 = WIDE ? (unsigned long long*)c.b_eh1.get(n * 8) : nullptr;
    uint32_t* i0 = (uint32_t*)c.b_ei0.get(n * 4);
    uint32_t* i1 = (uint32_t*)c.b_ei1.get(n * 4);
    if (status) k_ev_keys<WIDE, true><<<grid_for(n, 256 * 64), kThreads, 0, st>>>(in, deliver, f, k0, h0, i0, status);
    else k_ev_keys<WIDE><<<grid_for(n, 256 * 64), kThreads, 0, st>>>(in, deliver, f, k0, h0, i0);
    const uint32_t ntiles = (uint32_t)((n + RS_TILE - 1) / RS_TILE);
    const int nh = (int)(256 * (size_t)ntiles);
    uint32_t* hist = (uint32_t*)c.b_ehist.get((size_t)nh * 4);
    uint32_t* offs = (uint32_t*)c.b_eoffs.get((size_t)nh * 4);
    size_t tb = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, hist, offs, nh, st));
    void* tmp = c.b_scantmp.get(tb);
    passes = 0;
    for (uint32_t p = 0; p < bits; p += 8) {
        k_rs_hist<WIDE><<<ntiles, RS_THREADS, 0, st>>>(k0, h0, n, p, ntiles, hist);
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, hist, offs, nh, st));
        k_rs_scatter<WIDE><<<ntiles, RS_THREADS, 0, st>>>(k0, h0, i0, k1, h1, i1, n, p, ntiles, hist, offs);
        std::swap(k0, k1);
        std::swap(h0, h1);
        std::swap(i0, i1);
        ++passes;
    }
    HIP_CHECK(hipGetLastError());
    uint32_t* flag = (uint32_t*)c.b_red.get(64);
    HIP_CHECK(hipMemsetAsync(flag, 0, 4, st));
    if (status)
        k_ev_finish<WIDE, true><<<grid_for(n, 256 * 64), kThreads, 0, st>>>(k0, h0, n, f.sh_dst, in.num_hosts, host_off,
                                                                              flag);
    else
        k_ev_finish<WIDE><<<grid_for(n, 256 * 64), kThreads, 0, st>>>(k0, h0, n, f.sh_dst, in.num_hosts, host_off, flag);
    HIP_CHECK(hipMemcpyAsync(out_order, i0, n_order * 4, hipMemcpyDeviceToDevice, st));
    if (read_back<uint32_t>(flag, st))
        fail(SRG_ERR_EVENT_ORDER,
             "called `Option::unwrap()` on a `None` value: two packet events with equal (time, src_host_id, "
             "src_host_event_id) have no relative order");
}

// what the prep pass refused (EvReduce::bad)
void ev_fail_bad(uint32_t bad) {
    if (bad & 2) fail(SRG_ERR_ARG, "event node position out of range (>= table_n)");
    if (bad & 1) fail(SRG_ERR_ARG, "event dst_host out of range (>= num_hosts)");
    if (bad & 4) fail(SRG_ERR_LATENCY_RANGE, "deliver time overflows EmulatedTime (send + latency)");
}

// The composite key's layout and width from the batch's field ranges; dst_max is the largest value
// the host field has to hold.
EvKeyFmt ev_key_format(const EvReduce& r, uint64_t dst_max, uint32_t& bits) {
    EvKeyFmt f{};
    const uint32_t b_id = bit_width64(r.id_max - r.id_min), b_src = bit_width64(r.src_max),
                   b_t = bit_width64(r.t_max - r.t_min), b_dst = bit_width64(dst_max);
    f.t_min = r.t_min;
    f.id_min = r.id_min;
    f.sh_src = b_id;
    f.sh_t = b_id + b_src;
    f.sh_dst = b_id + b_src + b_t;
    bits = f.sh_dst + b_dst;
    if (bits > 128) fail(SRG_ERR_ARG, "event batch key wider than 128 bits");
    return f;
}

// One batch.  SEND = false (srg_order_packet_events_device): latencies from in.table, every event
// is sent; sx, status and counts are not used.  SEND = true (srg_send_packets_device): the whole
// per-packet tail of send_packet -- the drop decision in front, either table form (sx.tab), the
// packet counters, and the dropped events parked.  Returns the number of sent events.
template <bool SEND>
uint64_t event_batch_device(srg_ctx& c, const EvIn& in, const EvSendIn& sx, uint8_t* status, uint64_t* deliver,
                            uint32_t* out_order, uint64_t* host_off, unsigned long long* counts, hipStream_t st,
                            srg_event_result* res) {
    if (res) {
        res->min_next_event_ns = UINT64_MAX;
        res->min_used_latency_ns = UINT64_MAX;
        res->key_bits = 0;
        res->radix_passes = 0;
    }
    HIP_CHECK(hipMemsetAsync(host_off, 0, ((size_t)in.num_hosts + 1) * 8, st));
    if (in.n == 0) {
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    if (in.n >= 0xFFFFFFFFull) fail(SRG_ERR_ARG, "event batch too large (>= 2^32 events)");
    if (SEND && in.num_hosts == UINT32_MAX)
        fail(SRG_ERR_ARG, "num_hosts too large (host 2^32 - 1 parks the dropped events)");
    EvSendReduce* red = (EvSendReduce*)c.b_ered.get(sizeof(EvSendReduce));
    EvSendReduce init{{~0ull, 0ull, ~0ull, 0ull, ~0ull, 0u, 0u, 0u, 0u}, 0ull};
    HIP_CHECK(hipMemcpyAsync(red, &init, sizeof(EvSendReduce), hipMemcpyHostToDevice, st));
    k_ev_prep<SEND><<<grid_for(in.n, 2048), kThreads, 0, st>>>(in, sx, status, deliver, red);
    HIP_CHECK(hipGetLastError());
    const EvSendReduce sr = read_back<EvSendReduce>(red, st);
    const EvReduce& r = sr.r;
    ev_fail_bad(r.bad);
    const uint64_t sent = SEND ? sr.sent : in.n, drops = in.n - sent;
    // the counters move once the range checks passed (every index is inside the table), as
    // increment_packet_count runs at the send, before any queue is popped
    if (SEND && counts && sent) {
        k_ev_counts<<<grid_for(in.n, 2048), kThreads, 0, st>>>(in, status, counts);
        HIP_CHECK(hipGetLastError());
    }
    uint32_t bits = 0, passes = 0;
    if (sent) {
        // dropped events are parked behind host num_hosts: the host field must hold that value
        const EvKeyFmt f = ev_key_format(r, drops ? in.num_hosts : r.dst_max, bits);
        const uint8_t* parked = drops ? status : nullptr;
        // an all-equal key (bits == 0) needs no pass; a 1-event batch is trivially ordered
        if (bits <= 64) events_sort<false>(c, in, deliver, f, bits, out_order, host_off, st, passes, parked, sent);
        else events_sort<true>(c, in, deliver, f, bits, out_order, host_off, st, passes, parked, sent);
    } else {
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (res) {
        res->min_next_event_ns = r.t_min;
        res->min_used_latency_ns = r.lat_min;
        res->key_bits = bits;
        res->radix_passes = passes;
    }
    return sent;
}

}  // namespace

// ---- device-resident per-host event queues (event_queue.hip.h) ---------------------------
// The stage discipline of stage.hip.h: the current set is the queues, a push builds the merged
// result into the spare one.  A set that is too small is simply reallocated before it is built
// into: the contents live in the other one.
struct srg_event_queues {
    srg_ctx* ctx = nullptr;
    uint32_t num_hosts = 0;
    struct Set {
        DevBuf k0, k1, k2, tag, host_off, head;
        uint64_t cap = 0;
        EvqSet ptrs() const { return EvqSet{(uint64_t*)k0.p, (uint64_t*)k1.p, (uint64_t*)k2.p, (uint64_t*)tag.p}; }
        void reserve(uint64_t n) { grow_columns(cap, n, {{&k0, 8}, {&k1, 8}, {&k2, 8}, {&tag, 8}}); }
    };
    TwoSets<Set> sets;
    DevBuf last_popped, bk0, bk1, bk2, btag, dead, dead_excl, part_a, part_live, new_head, cnt, offs, state, scantmp;
    uint64_t stored = 0;  // events in the current set's arrays, popped ones included
    uint64_t live = 0;
    uint64_t min_next = UINT64_MAX;
};

extern "C" {

int srg_event_queues_create(srg_ctx* ctx, uint32_t num_hosts, uint64_t reserve_events, srg_event_queues** out,
                            char* errbuf, size_t errlen) {
    if (!ctx || !out) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    *out = nullptr;
    return stage_create(ctx, num_hosts, out, errbuf, errlen, [&](srg_event_queues& q, hipStream_t st) {
        const size_t hb = host_row_bytes(num_hosts);
        for (auto& s : q.sets.set) {
            HIP_CHECK(hipMemsetAsync(s.host_off.get(hb), 0, hb, st));
            HIP_CHECK(hipMemsetAsync(s.head.get(hb), 0, hb, st));
            s.reserve(reserve_events);
        }
        HIP_CHECK(hipMemsetAsync(q.last_popped.get(hb), 0, hb, st));
        for (DevBuf* b : {&q.dead, &q.dead_excl, &q.new_head, &q.cnt, &q.offs}) b->get(hb);
        q.state.get(sizeof(EvqState));
    });
}

void srg_event_queues_destroy(srg_event_queues* q) { stage_destroy(q); }

uint32_t srg_event_queues_merge_tile(void) { return (uint32_t)EVQ_TILE; }

}  // extern "C"

namespace {

void evq_fill_result(const srg_event_queues& q, uint64_t moved, srg_queue_result* res) {
    if (!res) return;
    res->num_moved = moved;
    res->num_queued = q.live;
    res->min_next_event_ns = q.min_next;
}

void evq_push(srg_event_queues& q, const srg_event_batch* b, const uint64_t* deliver, const uint32_t* order,
              uint64_t nb, const uint64_t* tag, hipStream_t st, srg_queue_result* res) {
    evq_fill_result(q, 0, res);
    if (nb == 0) return;  // nothing to merge: the queues (their popped prefixes too) stay as they are
    if (nb > b->num_events) fail(SRG_ERR_ARG, "num_order exceeds the batch's num_events");
    if (b->num_events >= 0xFFFFFFFFull) fail(SRG_ERR_ARG, "event batch too large (>= 2^32 events)");
    const uint32_t H = q.num_hosts;
    srg_event_queues::Set& A = q.sets.current();
    srg_event_queues::Set& O = q.sets.spare();
    const EvqSet B{(uint64_t*)q.bk0.get(nb * 8), (uint64_t*)q.bk1.get(nb * 8), (uint64_t*)q.bk2.get(nb * 8),
                   (uint64_t*)q.btag.get(nb * 8)};
    EvqState* ds = (EvqState*)q.state.get(sizeof(EvqState));
    const EvqState init{~0ull, 0u, 0u};
    HIP_CHECK(hipMemcpyAsync(ds, &init, sizeof(EvqState), hipMemcpyHostToDevice, st));
    const EvqGatherIn gi{b->num_events, nb, order, b->dst_host, b->src_host, b->src_event_id, deliver, tag, H};
    k_evq_gather<<<grid_for(nb, 2048), kThreads, 0, st>>>(gi, B, (const uint64_t*)q.last_popped.p, ds);
    HIP_CHECK(hipGetLastError());
    EvqState s = read_back<EvqState>(ds, st);
    if (s.flags & EVQ_BAD_ORDER)
        fail(SRG_ERR_ARG,
             "order is not the batch's queue order (an entry >= num_events, a dst_host >= num_hosts, or keys "
             "not strictly increasing by dst_host, time, src_host, event id)");
    if (s.flags & EVQ_TIME_BACKWARD)
        fail(SRG_ERR_TIME_BACKWARD,
             "assertion failed: event.time() >= self.last_popped_event_time: a pushed event is earlier than "
             "its host's last popped event");
    const uint64_t n_out = q.live + nb, n = q.stored + nb;
    O.reserve(n_out);
    const uint64_t* a_off = (const uint64_t*)A.host_off.p;
    const uint64_t* a_head = (const uint64_t*)A.head.p;
    uint64_t* dead = (uint64_t*)q.dead.p;
    uint64_t* dead_excl = (uint64_t*)q.dead_excl.p;
    k_evq_dead<<<grid_for((size_t)H + 1), kThreads, 0, st>>>(a_off, a_head, H, dead);
    // (const input: the iterator type this scan has always been instantiated with, see exclusive_sum)
    exclusive_sum(q.scantmp, (const uint64_t*)dead, dead_excl, (int)H + 1, st);
    const uint64_t ntiles = (n + EVQ_TILE - 1) / EVQ_TILE;
    if (ntiles >= 0x7FFFFFFFull) fail(SRG_ERR_ARG, "event queues too large for one merge launch");
    uint64_t* part_a = (uint64_t*)q.part_a.get((ntiles + 1) * 8);
    uint64_t* part_live = (uint64_t*)q.part_live.get((ntiles + 1) * 8);
    k_evq_partition<<<grid_for(ntiles + 1), kThreads, 0, st>>>(A.ptrs(), q.stored, B, nb, a_off, a_head, dead_excl, H,
                                                                ntiles, part_a, part_live);
    k_evq_merge<<<(unsigned)ntiles, EVQ_THREADS, 0, st>>>(A.ptrs(), B, n, part_a, part_live, a_head, O.ptrs(), n_out, ds);
    k_evq_finish<<<grid_for(n_out, 2048), kThreads, 0, st>>>((const uint64_t*)O.k0.p, n_out, H, (uint64_t*)O.host_off.p,
                                                             (uint64_t*)O.head.p);
    k_evq_min<<<grid_for(H, 2048), kThreads, 0, st>>>(O.ptrs(), (const uint64_t*)O.host_off.p,
                                                      (const uint64_t*)O.head.p, H, ds);
    HIP_CHECK(hipGetLastError());
    s = read_back<EvqState>(ds, st);
    if (s.flags & EVQ_EQUAL_KEYS)
        fail(SRG_ERR_EVENT_ORDER,
             "called `Option::unwrap()` on a `None` value: two packet events with equal (time, src_host_id, "
             "src_host_event_id) have no relative order");
    q.sets.flip();
    q.stored = q.live = n_out;
    q.min_next = s.min_head;
    evq_fill_result(q, nb, res);
}

void evq_pop(srg_event_queues& q, uint64_t until, uint64_t capacity, uint64_t* out_time, uint32_t* out_src,
             uint64_t* out_id, uint64_t* out_tag, uint64_t* out_off, hipStream_t st, srg_queue_result* res) {
    evq_fill_result(q, 0, res);
    const uint32_t H = q.num_hosts;
    srg_event_queues::Set& A = q.sets.current();
    uint64_t* host_off = (uint64_t*)A.host_off.p;
    uint64_t* head = (uint64_t*)A.head.p;
    uint64_t* new_head = (uint64_t*)q.new_head.p;
    uint64_t* cnt = (uint64_t*)q.cnt.p;
    uint64_t* offs = (uint64_t*)q.offs.p;
    k_evq_pop_find<<<grid_for((size_t)H + 1, 2048), kThreads, 0, st>>>(A.ptrs(), host_off, head, H, until, new_head, cnt);
    HIP_CHECK(hipGetLastError());
    exclusive_sum(q.scantmp, (const uint64_t*)cnt, offs, (int)H + 1, st);  // (const: as above)
    const uint64_t total = read_back<uint64_t>(offs + H, st);
    if (total > capacity) {
        if (res) res->num_moved = total;
        fail(SRG_ERR_ARG, "out_capacity too small: " + std::to_string(total) + " events are due (nothing popped)");
    }
    if (out_off) HIP_CHECK(hipMemcpyAsync(out_off, offs, ((size_t)H + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (total == 0) {
        HIP_CHECK(hipStreamSynchronize(st));
        return;
    }
    EvqState* ds = (EvqState*)q.state.get(sizeof(EvqState));
    const EvqState init{~0ull, 0u, 0u};
    HIP_CHECK(hipMemcpyAsync(ds, &init, sizeof(EvqState), hipMemcpyHostToDevice, st));
    k_evq_pop_copy<<<grid_for(total, 2048), kThreads, 0, st>>>(A.ptrs(), head, offs, H, total, out_time, out_src, out_id,
                                                               out_tag);
    k_evq_pop_commit<<<grid_for(H, 2048), kThreads, 0, st>>>(A.ptrs(), host_off, head, (uint64_t*)q.last_popped.p,
                                                             new_head, H, ds);
    HIP_CHECK(hipGetLastError());
    const EvqState s = read_back<EvqState>(ds, st);
    q.live -= total;
    q.min_next = s.min_head;
    evq_fill_result(q, total, res);
}

}  // namespace

extern "C" {

int srg_event_queues_push_device(srg_event_queues* q, const srg_event_batch* b, const uint64_t* deliver,
                                 const uint32_t* order, uint64_t num_order, const uint64_t* tag, void* hip_stream,
                                 srg_queue_result* res, char* errbuf, size_t errlen) {
    if (!q || !b ||
        (num_order && (!deliver || !order || !b->src_host || !b->dst_host || !b->src_event_id))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(q->ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen,
                       [&](hipStream_t st) { evq_push(*q, b, deliver, order, num_order, tag, st, res); });
}

int srg_event_queues_pop_device(srg_event_queues* q, uint64_t until_ns, uint64_t out_capacity, uint64_t* out_time,
                                uint32_t* out_src, uint64_t* out_id, uint64_t* out_tag, uint64_t* out_off,
                                void* hip_stream, srg_queue_result* res, char* errbuf, size_t errlen) {
    if (!q || (out_capacity && (!out_time || !out_tag || !out_off))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(q->ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        evq_pop(*q, until_ns, out_capacity, out_time, out_src, out_id, out_tag, out_off, st, res);
    });
}

}  // extern "C"

namespace {
