// round_run.hip.h -- the host side of a round on the device (round.hip.h): the drivers behind
// srg_round_send_device and srg_round_receive_device, and the srg_round_* entry points themselves.  A
// section of routing.hip's translation unit, included there once inside its anonymous namespace
// behind events_run, inbound_run and outbound_run (it composes their drivers: out_step,
// event_batch_device<true>, evq_push, evq_pop, inb_step, and changes none of them); not a header to
// include elsewhere.  struct srg_round is the C ABI's opaque type and the entry points are
// extern "C", so the section leaves the anonymous namespace around them and enters it again.
//
// An error leaves everything as it was.  Each part keeps its previous state until its own next
// call (the stage discipline of stage.hip.h); the pop moves only head / last_popped (and the two
// host-side counters).  So:
//   send     offers kernel -> out_step -> count, scan, draw -> send batch -> push.  The push is last.
//            When anything behind the outbound step's commit fails, the outbound part's snapshot
//            is restored; the generator words and event-id counters were built into the spare
//            set, which is simply not made current.
//   receive  head and last_popped are copied aside (2 (H + 1) words, device to device) before the
//            pop and copied back when the sizes kernel or the inbound step fails.
// packet_counts_dev is the one exception, as in srg_send_packets_device.  Every path that queued work
// synchronises `st` before it returns.

}  // namespace

struct srg_round {
    srg_ctx* ctx = nullptr;
    uint32_t num_hosts = 0;
    uint64_t bootstrap_end = 0, sim_end = 0;
    srg_event_queues* q = nullptr;
    srg_inbound* inb = nullptr;
    srg_outbound* out = nullptr;
    srg_path_table_dev tab{};  // a copy of the caller's struct; the arrays stay the caller's
    RoundPackets pk{0, nullptr, nullptr, nullptr};
    struct Set {
        DevBuf rng, eid;  // [H * 4], [H]
    };
    TwoSets<Set> sets;
    DevBuf host_node;  // [H]
    // send half: what the outbound step takes and gives, the send batch, what the send call writes
    DevBuf f_size, f_flags, o_status, o_time, o_tag, o_off, cnt, row0, red, scantmp;
    DevBuf b_src_node, b_dst_node, b_src_host, b_dst_host, b_send, b_eid, b_chance, b_payload, b_tag;
    DevBuf s_status, s_deliver, s_order, s_hoff;
    // receive half
    DevBuf p_time, p_tag, p_off, p_size, i_status, i_time, i_tag, i_off, snap_head, snap_last;
    ~srg_round() {
        srg_event_queues_destroy(q);
        srg_inbound_destroy(inb);
        srg_outbound_destroy(out);
    }
};

namespace {

inline uint64_t min3(uint64_t a, uint64_t b, uint64_t c) { return std::min(a, std::min(b, c)); }

void round_fill_send(const srg_round& r, srg_round_send_result* res) {
    if (!res) return;
    *res = srg_round_send_result{};
    res->min_used_latency_ns = UINT64_MAX;
    res->num_queued_outbound = r.out->ctr.backlog + r.out->ctr.cached;
    res->num_queued_events = r.q->live;
    res->min_next_event_ns = r.q->min_next;
    res->min_inbound_wake_ns = r.inb->min_wake;
    res->min_outbound_wake_ns = r.out->ctr.min_wake;
    res->next_start_ns = min3(r.q->min_next, r.inb->min_wake, r.out->ctr.min_wake);
}

void round_fill_receive(const srg_round& r, srg_round_receive_result* res) {
    if (!res) return;
    *res = srg_round_receive_result{};
    res->num_queued_inbound = r.inb->backlog + r.inb->cached;
    res->num_queued_events = r.q->live;
    res->min_next_event_ns = r.q->min_next;
    res->min_inbound_wake_ns = r.inb->min_wake;
    res->min_outbound_wake_ns = r.out->ctr.min_wake;
    res->next_start_ns = min3(r.q->min_next, r.inb->min_wake, r.out->ctr.min_wake);
}

void round_zero_red(srg_round& r, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(r.red.get(sizeof(RoundReduce)), 0, sizeof(RoundReduce), st));
}

void round_send(srg_round& r, uint64_t until, uint64_t n, const uint64_t* time, const uint32_t* socket,
                const uint64_t* prio, const uint8_t* flags, const uint64_t* tag, const uint64_t* host_off,
                uint64_t* counts, hipStream_t st, srg_round_send_result* res) {
    round_fill_send(r, res);
    const uint32_t H = r.num_hosts;
    srg_outbound& o = *r.out;
    if (n >= (1ull << 32)) fail(SRG_ERR_ARG, "too many packets in one step (queued + offers must stay below 2^32)");
    if ((n || o.ctr.backlog + o.ctr.cached) && !r.pk.dst) fail(SRG_ERR_ARG, "no packet table: call srg_round_set_packets first");
    uint32_t* f_size = (uint32_t*)r.f_size.get(n * 4);
    uint8_t* f_flags = (uint8_t*)r.f_flags.get(n);
    RoundReduce* dred = (RoundReduce*)r.red.get(sizeof(RoundReduce));
    if (n) {
        round_zero_red(r, st);
        k_round_offers<<<grid_for(std::max<uint64_t>(n, (uint64_t)H + 1), 2048), kThreads, 0, st>>>(
            n, tag, flags, host_off, H, r.pk, (const uint64_t*)r.inb->inc.p, f_size, f_flags, dred);
        HIP_CHECK(hipGetLastError());
        const RoundReduce v = read_back<RoundReduce>(dred, st);
        if (v.flags & ROUND_BAD_OFFSETS) fail(SRG_ERR_ARG, "host_offsets are not monotone from 0 to num_offers");
        if (v.flags & ROUND_BAD_TAG) fail(SRG_ERR_ARG, "an offer's tag is not below num_packets");
        if (v.flags & ROUND_BAD_DST)
            fail(SRG_ERR_ARG, "a packet's dst_host is neither below num_hosts nor SRG_NO_HOST");
        if (v.flags & ROUND_BAD_FLAGS)
            fail(SRG_ERR_ARG, "an offer carries a flag bit other than SRG_OFFER_BARRIER (the local bit is derived)");
        if (v.flags & ROUND_BAD_SIZE)
            fail(SRG_ERR_ARG,
                 "a non-local packet is larger than its destination's downstream token bucket (refill + 1500): it "
                 "would never conform");
    }
    const uint64_t cap = o.ctr.backlog + o.ctr.cached + n;
    uint8_t* o_status = (uint8_t*)r.o_status.get(cap);
    uint64_t* o_time = (uint64_t*)r.o_time.get(cap * 8);
    uint64_t* o_tag = (uint64_t*)r.o_tag.get(cap * 8);
    uint64_t* o_off = (uint64_t*)r.o_off.p;
    const srg_outbound::Snapshot before = o.snapshot();
    srg_outbound_result ores{};
    out_step(o, until, OutOffers{n, time, socket, prio, f_size, f_flags, tag, host_off}, cap, o_status, o_time, o_tag,
             o_off, st, &ores);
    srg_event_result eres{};
    srg_queue_result qres{};
    RoundReduce v{};
    uint64_t ndraw = 0, sent = 0;
    try {
        const uint64_t total = ores.num_sent + ores.num_local;
        round_zero_red(r, st);
        uint64_t* cnt = (uint64_t*)r.cnt.p;
        uint64_t* row0 = (uint64_t*)r.row0.p;
        const unsigned wgs = (unsigned)(((uint64_t)H + 1 + ROUND_HOSTS_PER_WG - 1) / ROUND_HOSTS_PER_WG);
        k_round_count<<<wgs, 64 * ROUND_HOSTS_PER_WG, 0, st>>>(o_status, o_time, o_tag, o_off, H, r.pk, r.sim_end, cnt,
                                                               dred);
        HIP_CHECK(hipGetLastError());
        exclusive_sum(r.scantmp, cnt, row0, (int)H + 1, st);  // (non-const input, as always here: see exclusive_sum)
        HIP_CHECK(hipMemcpyAsync(&ndraw, row0 + H, 8, hipMemcpyDeviceToHost, st));  // (rides in the record's synchronise)
        v = read_back<RoundReduce>(dred, st);
        if (v.flags || ndraw > total)
            fail(SRG_ERR_ARG, "the packet table changed under packets still inside the round object");
        RoundRows rows{(uint32_t*)r.b_src_node.get(ndraw * 4), (uint32_t*)r.b_dst_node.get(ndraw * 4),
                       (uint32_t*)r.b_src_host.get(ndraw * 4), (uint32_t*)r.b_dst_host.get(ndraw * 4),
                       (uint64_t*)r.b_send.get(ndraw * 8),     (uint64_t*)r.b_eid.get(ndraw * 8),
                       (double*)r.b_chance.get(ndraw * 8),     (uint32_t*)r.b_payload.get(ndraw * 4),
                       (uint64_t*)r.b_tag.get(ndraw * 8)};
        if (H) {
            k_round_draw<<<(H + ROUND_HOSTS_PER_WG - 1) / ROUND_HOSTS_PER_WG, 64 * ROUND_HOSTS_PER_WG, 0, st>>>(
                o_status, o_time, o_tag, o_off, row0, H, r.pk, (const uint32_t*)r.host_node.p, r.tab.packet_loss, r.tab.n,
                r.bootstrap_end, (const uint64_t*)r.sets.current().rng.p, (const uint64_t*)r.sets.current().eid.p,
                (uint64_t*)r.sets.spare().rng.p, (uint64_t*)r.sets.spare().eid.p, rows);
            HIP_CHECK(hipGetLastError());
        }
        const srg_event_batch b{ndraw,       rows.src_node, rows.dst_node, rows.src_host, rows.dst_host,
                                rows.send_ns, rows.event_id, H,             0,             until};
        const EvIn in{ndraw,        rows.src_node, rows.dst_node, rows.src_host, rows.dst_host, rows.send_ns,
                      rows.event_id, nullptr,       r.tab.n,       H,             until};
        const EvSendIn sx{{r.tab.latency_ns, r.tab.latency_key, r.tab.diag_ns, r.tab.unit_ns, r.tab.n},
                          r.tab.packet_loss, rows.chance, rows.payload, r.bootstrap_end};
        sent = event_batch_device<true>(*r.ctx, in, sx, (uint8_t*)r.s_status.get(ndraw),
                                        (uint64_t*)r.s_deliver.get(ndraw * 8), (uint32_t*)r.s_order.get(ndraw * 4),
                                        (uint64_t*)r.s_hoff.p, (unsigned long long*)counts, st, &eres);
        evq_push(*r.q, &b, (const uint64_t*)r.s_deliver.p, (const uint32_t*)r.s_order.p, sent, rows.tag, st, &qres);
    } catch (...) {
        (void)hipStreamSynchronize(st);
        o.restore(before);
        throw;
    }
    r.sets.flip();
    round_fill_send(r, res);
    if (!res) return;
    res->num_leaving = ores.num_sent + ores.num_local;
    res->status_dev = o_status;
    res->time_ns_dev = o_time;
    res->tag_dev = o_tag;
    res->host_offsets_dev = o_off;
    res->num_sent = sent;
    res->num_dropped = ndraw - sent;
    res->num_local = ores.num_local;
    res->num_after_end = v.after_end;
    res->num_no_host = v.no_dst;
    res->min_used_latency_ns = eres.min_used_latency_ns;
}

void round_receive(srg_round& r, uint64_t until, hipStream_t st, srg_round_receive_result* res) {
    round_fill_receive(r, res);
    const uint32_t H = r.num_hosts;
    srg_event_queues& q = *r.q;
    srg_inbound& ib = *r.inb;
    const uint64_t cap = q.live;
    uint64_t* p_time = (uint64_t*)r.p_time.get(cap * 8);
    uint64_t* p_tag = (uint64_t*)r.p_tag.get(cap * 8);
    uint32_t* p_size = (uint32_t*)r.p_size.get(cap * 4);
    uint64_t* p_off = (uint64_t*)r.p_off.p;
    const size_t hb = ((size_t)H + 1) * 8;
    void* head = q.sets.current().head.p;
    HIP_CHECK(hipMemcpyAsync(r.snap_head.p, head, hb, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(r.snap_last.p, q.last_popped.p, hb, hipMemcpyDeviceToDevice, st));
    const uint64_t q_live = q.live, q_min = q.min_next;
    srg_queue_result qres{};
    evq_pop(q, until, cap, p_time, nullptr, nullptr, p_tag, p_off, st, &qres);
    const uint64_t moved = qres.num_moved;
    srg_inbound_result ires{};
    const uint64_t cap2 = ib.backlog + ib.cached + moved;
    try {
        if (moved) {
            if (!r.pk.size) fail(SRG_ERR_ARG, "no packet table: call srg_round_set_packets first");
            round_zero_red(r, st);
            k_round_sizes<<<grid_for(moved, 2048), kThreads, 0, st>>>(moved, p_tag, r.pk, p_size, (RoundReduce*)r.red.p);
            HIP_CHECK(hipGetLastError());
            if (read_back<RoundReduce>(r.red.p, st).flags)
                fail(SRG_ERR_ARG, "the packet table changed under packets still inside the round object");
        }
        inb_step(ib, until, InbArrivals{moved, p_time, p_size, p_tag, p_off}, cap2, (uint8_t*)r.i_status.get(cap2),
                 (uint64_t*)r.i_time.get(cap2 * 8), (uint64_t*)r.i_tag.get(cap2 * 8), (uint64_t*)r.i_off.p, st, &ires);
    } catch (...) {
        (void)hipMemcpyAsync(head, r.snap_head.p, hb, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(q.last_popped.p, r.snap_last.p, hb, hipMemcpyDeviceToDevice, st);
        (void)hipStreamSynchronize(st);
        q.live = q_live;
        q.min_next = q_min;
        throw;
    }
    round_fill_receive(r, res);
    if (!res) return;
    res->num_popped = moved;
    res->popped_time_ns_dev = p_time;
    res->popped_tag_dev = p_tag;
    res->popped_host_offsets_dev = p_off;
    res->num_leaving = ires.num_forwarded + ires.num_dropped;
    res->status_dev = (const uint8_t*)r.i_status.p;
    res->time_ns_dev = (const uint64_t*)r.i_time.p;
    res->tag_dev = (const uint64_t*)r.i_tag.p;
    res->host_offsets_dev = (const uint64_t*)r.i_off.p;
    res->num_forwarded = ires.num_forwarded;
    res->num_dropped = ires.num_dropped;
}

void round_host_rng(srg_round& r, uint32_t host, uint64_t words[4], uint64_t* next_event_id) {
    if (host >= r.num_hosts) fail(SRG_ERR_ARG, "host out of range (>= num_hosts)");
    HIP_CHECK(hipMemcpy(words, (const uint64_t*)r.sets.current().rng.p + (size_t)host * 4, 32, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(next_event_id, (const uint64_t*)r.sets.current().eid.p + host, 8, hipMemcpyDeviceToHost));
}

void round_set_host_rng(srg_round& r, uint32_t host, const uint64_t words[4], uint64_t next_event_id) {
    if (host >= r.num_hosts) fail(SRG_ERR_ARG, "host out of range (>= num_hosts)");
    if (!(words[0] | words[1] | words[2] | words[3]))
        fail(SRG_ERR_ARG, "the all-zero state is not a state of the generator");
    HIP_CHECK(hipMemcpy((uint64_t*)r.sets.current().rng.p + (size_t)host * 4, words, 32, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy((uint64_t*)r.sets.current().eid.p + host, &next_event_id, 8, hipMemcpyHostToDevice));
}

// the object's own arrays; the three parts were built by their constructors before
void round_init(srg_round& r, const uint32_t* host_node, const uint64_t* node_seed) {
    srg_ctx& c = *r.ctx;
    const uint32_t H = r.num_hosts;
    const size_t hb = host_row_bytes(H);
    for (DevBuf* b : {&r.o_off, &r.cnt, &r.row0, &r.s_hoff, &r.p_off, &r.i_off, &r.snap_head, &r.snap_last})
        HIP_CHECK(hipMemsetAsync(b->get(hb), 0, hb, c.stream));
    r.red.get(sizeof(RoundReduce));
    for (auto& s : r.sets.set) {
        s.rng.get((size_t)H * 32);
        s.eid.get((size_t)H * 8);
    }
    r.host_node.get((size_t)H * 4);
    if (H) {
        HIP_CHECK(hipMemcpyAsync(r.host_node.p, host_node, (size_t)H * 4, hipMemcpyHostToDevice, c.stream));
        uint64_t* seed = (uint64_t*)r.sets.set[1].eid.p;  // (staging: the spare counters are written before they are read)
        HIP_CHECK(hipMemcpyAsync(seed, node_seed, (size_t)H * 8, hipMemcpyHostToDevice, c.stream));
        k_round_seed<<<grid_for(H), kThreads, 0, c.stream>>>(seed, H, (uint64_t*)r.sets.set[0].rng.p,
                                                          (uint64_t*)r.sets.set[0].eid.p);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(c.stream));
}

}  // namespace

extern "C" {

int srg_round_create(srg_ctx* ctx, uint32_t num_hosts, const uint32_t* host_node, const srg_path_table_dev* table,
                     const uint64_t* bw_up_bits, const uint64_t* bw_down_bits, const uint32_t* sockets_per_host,
                     int qdisc, const uint64_t* node_seed, uint64_t sim_start_ns, uint64_t bootstrap_end_ns,
                     uint64_t sim_end_ns, uint64_t reserve_packets, srg_round** out, char* errbuf, size_t errlen) {
    if (!ctx || !out || !table ||
        (num_hosts && (!host_node || !bw_up_bits || !bw_down_bits || !sockets_per_host || !node_seed))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    *out = nullptr;
    if (!table->latency_ns == !table->latency_key) {
        set_err(errbuf, errlen, "path table: exactly one of latency_ns and latency_key must be given");
        return SRG_ERR_ARG;
    }
    if (table->latency_key && (!table->diag_ns || table->unit_ns < 1)) {
        set_err(errbuf, errlen, "path table: latency_key needs diag_ns and unit_ns >= 1");
        return SRG_ERR_ARG;
    }
    for (uint32_t h = 0; h < num_hosts; ++h)
        if (host_node[h] >= table->n) {
            set_err(errbuf, errlen, "host_node out of range (>= table->n)");
            return SRG_ERR_ARG;
        }
    std::unique_ptr<srg_round> r(new (std::nothrow) srg_round);
    if (!r) {
        set_err(errbuf, errlen, "out of host memory");
        return SRG_ERR_OOM;
    }
    r->ctx = ctx;
    r->num_hosts = num_hosts;
    r->bootstrap_end = bootstrap_end_ns;
    r->sim_end = sim_end_ns;
    r->tab = *table;
    // the parts take ctx->mu themselves; a part that fails leaves the others to ~srg_round
    int rc = srg_event_queues_create(ctx, num_hosts, reserve_packets, &r->q, errbuf, errlen);
    if (rc == SRG_OK)
        rc = srg_inbound_create(ctx, num_hosts, bw_down_bits, sim_start_ns, bootstrap_end_ns, reserve_packets, &r->inb,
                                errbuf, errlen);
    if (rc == SRG_OK)
        rc = srg_outbound_create(ctx, num_hosts, bw_up_bits, sockets_per_host, qdisc, sim_start_ns, bootstrap_end_ns,
                                 reserve_packets, &r->out, errbuf, errlen);
    if (rc == SRG_OK) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        rc = guard(errbuf, errlen, [&]() {
            HIP_CHECK(hipSetDevice(ctx->device));
            round_init(*r, host_node, node_seed);
        });
    }
    if (rc == SRG_OK) *out = r.release();
    return rc;
}

void srg_round_destroy(srg_round* r) { stage_destroy(r); }

int srg_round_set_packets(srg_round* r, uint64_t num_packets, const uint32_t* dst_host_dev,
                          const uint32_t* total_size_dev, const uint32_t* payload_size_dev) {
    if (!r || (num_packets && (!dst_host_dev || !total_size_dev || !payload_size_dev))) return SRG_ERR_ARG;
    std::lock_guard<std::mutex> lk(r->ctx->mu);
    r->pk = RoundPackets{num_packets, dst_host_dev, total_size_dev, payload_size_dev};
    return SRG_OK;
}

int srg_round_receive_device(srg_round* r, uint64_t until_ns, void* hip_stream, srg_round_receive_result* res,
                             char* errbuf, size_t errlen) {
    if (!r) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(r->ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen,
                       [&](hipStream_t st) { round_receive(*r, until_ns, st, res); });
}

int srg_round_send_device(srg_round* r, uint64_t until_ns, uint64_t num_offers, const uint64_t* time_ns,
                          const uint32_t* socket, const uint64_t* priority, const uint8_t* flags, const uint64_t* tag,
                          const uint64_t* host_offsets, uint64_t* packet_counts, void* hip_stream,
                          srg_round_send_result* res, char* errbuf, size_t errlen) {
    if (!r || !host_offsets || (num_offers && (!time_ns || !socket || !priority || !tag))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(r->ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        round_send(*r, until_ns, num_offers, time_ns, socket, priority, flags, tag, host_offsets, packet_counts, st, res);
    });
}

int srg_round_host_rng(srg_round* r, uint32_t host, uint64_t words[4], uint64_t* next_event_id) {
    if (!r || !words || !next_event_id) return SRG_ERR_ARG;
    return device_call(r->ctx, nullptr, nullptr, nullptr, 0,
                       [&](hipStream_t) { round_host_rng(*r, host, words, next_event_id); });
}

int srg_round_set_host_rng(srg_round* r, uint32_t host, const uint64_t words[4], uint64_t next_event_id) {
    if (!r || !words) return SRG_ERR_ARG;
    return device_call(r->ctx, nullptr, nullptr, nullptr, 0,
                       [&](hipStream_t) { round_set_host_rng(*r, host, words, next_event_id); });
}

srg_event_queues* srg_round_queues(srg_round* r) { return r ? r->q : nullptr; }
srg_inbound* srg_round_inbound(srg_round* r) { return r ? r->inb : nullptr; }
srg_outbound* srg_round_outbound(srg_round* r) { return r ? r->out : nullptr; }

}  // extern "C"

namespace {
