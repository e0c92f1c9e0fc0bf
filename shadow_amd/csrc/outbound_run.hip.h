// outbound_run.hip.h -- the host side of the hosts' outbound path (outbound.hip.h): the driver behind
// srg_outbound_step_device and the small read-backs of srg_outbound_host_state / _host_order, and the
// srg_outbound_* entry points themselves.  A section of routing.hip's translation unit, included
// there once inside its anonymous namespace (it uses srg_ctx, DevBuf, fail, grid_for and device_call
// from the text above it and the helpers of stage.hip.h); not a header to include elsewhere.  struct
// srg_outbound is the C ABI's opaque type and the entry points are extern "C", so the section leaves
// the anonymous namespace around them and enters it again.
//
// The stage discipline of stage.hip.h: the current set is the state, a step builds its result into
// the spare one and flips after the device flags and totals were read.  The round's send undoes a
// step that succeeded: snapshot() / restore().  Every path that queued work synchronises `st` before
// it returns.

}  // namespace

struct srg_outbound {
    srg_ctx* ctx = nullptr;
    uint32_t num_hosts = 0;
    int qdisc = 0;
    uint64_t sim_start = 0, bootstrap_end = 0;
    std::vector<uint64_t> seg_off_host;  // [H + 1] prefix sums of sockets_per_host
    struct Set {
        DevBuf hosts, ord, ch, ct, dh, dt, nprio;          // the records and the per-socket segments
        DevBuf slot, prio, size, flags, tag, next, host_off;  // the backlog
        uint64_t cap = 0;
        OutSeg seg() const {
            return OutSeg{(uint32_t*)ord.p, (uint32_t*)ch.p, (uint32_t*)ct.p,
                          (uint32_t*)dh.p,  (uint32_t*)dt.p, (uint64_t*)nprio.p};
        }
        OutBacklog ptrs() const {
            return OutBacklog{(uint32_t*)slot.p, (uint64_t*)prio.p, (uint32_t*)size.p, (uint8_t*)flags.p,
                              (uint64_t*)tag.p,  (uint32_t*)next.p, (uint64_t*)host_off.p};
        }
        void reserve(uint64_t n) {
            grow_columns(cap, n, {{&slot, 4}, {&prio, 8}, {&size, 4}, {&flags, 1}, {&tag, 8}, {&next, 4}});
        }
    };
    TwoSets<Set> sets;
    DevBuf inc, seg_off, lnk, gone, newidx, o_idx, o_time, o_status, cnt, rem, offs, red, scantmp;
    // What a step changes on the host side.  A snapshot is all of it and which set is current: the
    // spare set still holds the previous state until the next step builds into it.
    struct Counters {
        uint64_t backlog = 0;  // packets in the current set's backlog arrays
        uint64_t cached = 0;   // hosts whose relay holds a cached packet
        uint64_t min_wake = UINT64_MAX;
    } ctr;
    struct Snapshot {
        int cur;
        Counters ctr;
    };
    Snapshot snapshot() const { return Snapshot{sets.cur, ctr}; }
    void restore(const Snapshot& s) {
        sets.cur = s.cur;
        ctr = s.ctr;
    }
};

extern "C" {

int srg_outbound_create(srg_ctx* ctx, uint32_t num_hosts, const uint64_t* bw_up_bits, const uint32_t* sockets_per_host,
                        int qdisc, uint64_t sim_start_ns, uint64_t bootstrap_end_ns, uint64_t reserve_packets,
                        srg_outbound** out, char* errbuf, size_t errlen) {
    if (!ctx || !out || (num_hosts && (!bw_up_bits || !sockets_per_host))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    *out = nullptr;
    if (!sim_start_ok(sim_start_ns, errbuf, errlen)) return SRG_ERR_ARG;
    if (qdisc != SRG_QDISC_FIFO && qdisc != SRG_QDISC_ROUND_ROBIN) {
        set_err(errbuf, errlen, "qdisc is neither SRG_QDISC_FIFO nor SRG_QDISC_ROUND_ROBIN");
        return SRG_ERR_ARG;
    }
    for (uint32_t h = 0; h < num_hosts; ++h)
        if (sockets_per_host[h] >= (1u << 31)) {
            set_err(errbuf, errlen, "sockets_per_host outside the domain (>= 2^31)");
            return SRG_ERR_ARG;
        }
    return stage_create(ctx, num_hosts, out, errbuf, errlen, [&](srg_outbound& q, hipStream_t st) {
        q.qdisc = qdisc;
        q.sim_start = sim_start_ns;
        q.bootstrap_end = bootstrap_end_ns;
        q.seg_off_host.assign((size_t)num_hosts + 1, 0);
        for (uint32_t h = 0; h < num_hosts; ++h) q.seg_off_host[h + 1] = q.seg_off_host[h] + sockets_per_host[h];
        const uint64_t slots = q.seg_off_host[num_hosts];
        const size_t hb = host_row_bytes(num_hosts);
        for (auto& s : q.sets.set) {
            HIP_CHECK(hipMemsetAsync(s.host_off.get(hb), 0, hb, st));
            s.hosts.get((size_t)num_hosts * sizeof(OutHost));
            for (DevBuf* b : {&s.ord, &s.ch, &s.ct, &s.dh, &s.dt}) b->get(slots * 4);
            s.nprio.get(slots * 8);
            s.reserve(reserve_packets);
        }
        for (DevBuf* b : {&q.cnt, &q.rem, &q.offs}) b->get(hb);
        q.red.get(sizeof(OutReduce));
        HIP_CHECK(hipMemcpyAsync(q.seg_off.get(hb), q.seg_off_host.data(), hb, hipMemcpyHostToDevice, st));
        uint64_t* inc = (uint64_t*)q.inc.get((size_t)num_hosts * 8);
        if (num_hosts) {
            uint64_t* bw = (uint64_t*)q.o_time.get((size_t)num_hosts * 8);
            HIP_CHECK(hipMemcpyAsync(bw, bw_up_bits, (size_t)num_hosts * 8, hipMemcpyHostToDevice, st));
            k_out_init<<<grid_for(std::max<uint64_t>(num_hosts, slots)), kThreads, 0, st>>>(
                bw, num_hosts, slots, sim_start_ns, inc, (OutHost*)q.sets.set[0].hosts.p, (OutHost*)q.sets.set[1].hosts.p,
                q.sets.set[0].seg(), q.sets.set[1].seg());
            HIP_CHECK(hipGetLastError());
        }
    });
}

void srg_outbound_destroy(srg_outbound* q) { stage_destroy(q); }

}  // extern "C"

namespace {

void out_fill_result(const srg_outbound& q, uint64_t sent, uint64_t local, srg_outbound_result* res) {
    if (!res) return;
    res->num_sent = sent;
    res->num_local = local;
    res->num_queued = q.ctr.backlog + q.ctr.cached;
    res->min_next_wake_ns = q.ctr.min_wake;
}

void out_step(srg_outbound& q, uint64_t until, const OutOffers& A, uint64_t capacity, uint8_t* out_status,
              uint64_t* out_time, uint64_t* out_tag, uint64_t* out_off, hipStream_t st, srg_outbound_result* res) {
    out_fill_result(q, 0, 0, res);
    if (until > INB_TIME_END) fail(SRG_ERR_ARG, "until_ns outside the time domain (> 2^62)");
    const uint32_t H = q.num_hosts;
    // a host's packets are indexed in 32 bits (OUT_NIL is the end of a FIFO)
    if (A.n >= (1ull << 32) || q.ctr.backlog + A.n + H >= 0xffffffffull)
        fail(SRG_ERR_ARG, "too many packets in one step (queued + offers must stay below 2^32)");
    srg_outbound::Set& C = q.sets.current();
    srg_outbound::Set& O = q.sets.spare();
    OutReduce* dred = (OutReduce*)q.red.p;
    const OutReduce init{~0ull, 0ull, 0ull, 0ull, 0u, 0u};
    HIP_CHECK(hipMemcpyAsync(dred, &init, sizeof(OutReduce), hipMemcpyHostToDevice, st));
    // the step walks the offsets and trusts slots, sizes and the order of the times: validated
    // first, read back first
    const uint64_t* seg_off = (const uint64_t*)q.seg_off.p;
    k_out_validate<<<grid_for(std::max<uint64_t>(A.n, (uint64_t)H + 1), 2048), kThreads, 0, st>>>(
        A, (const OutHost*)C.hosts.p, (const uint64_t*)q.inc.p, seg_off, H, q.sim_start, until, dred);
    HIP_CHECK(hipGetLastError());
    OutReduce r = read_back<OutReduce>(dred, st);
    if (r.flags & OUT_BAD_OFFSETS) fail(SRG_ERR_ARG, "host_offsets are not monotone from 0 to num_offers");
    if (r.flags & OUT_BAD_TIME)
        fail(SRG_ERR_ARG, "an offer's time is outside [sim_start_ns, 2^62) or not below until_ns");
    if (r.flags & OUT_BAD_SLOT) fail(SRG_ERR_ARG, "an offer's socket slot is not below its host's sockets_per_host");
    if (r.flags & OUT_BAD_FLAGS)
        fail(SRG_ERR_ARG, "an offer carries a flag bit other than SRG_OFFER_LOCAL | SRG_OFFER_BARRIER");
    if (r.flags & OUT_BAD_SIZE)
        fail(SRG_ERR_ARG,
             "a non-local packet is larger than its host's token bucket (refill + 1500): it would never conform");
    if (r.flags & OUT_TIME_BACKWARD)
        fail(SRG_ERR_TIME_BACKWARD, "an offer is earlier than its host's previous offer or its last executed forward task");
    const uint64_t nseq = q.ctr.backlog + A.n;
    OutScratch X;
    X.lnk = (uint32_t*)q.lnk.get(nseq * 4);
    X.gone = (uint8_t*)q.gone.get(nseq);
    X.newidx = (uint32_t*)q.newidx.get(nseq * 4);
    X.o_idx = (uint32_t*)q.o_idx.get((nseq + H) * 4);
    X.o_time = (uint64_t*)q.o_time.get((nseq + H) * 8);
    X.o_status = (uint8_t*)q.o_status.get(nseq + H);
    if (nseq) HIP_CHECK(hipMemsetAsync(X.gone, 0, nseq, st));
    uint64_t* cnt = (uint64_t*)q.cnt.p;
    uint64_t* rem = (uint64_t*)q.rem.p;
    uint64_t* offs = (uint64_t*)q.offs.p;
    uint64_t* new_off = (uint64_t*)O.host_off.p;
    const unsigned wgs = (unsigned)(((uint64_t)H + 1 + OUT_HOSTS_PER_WG - 1) / OUT_HOSTS_PER_WG);
    k_out_step<<<wgs, 64 * OUT_HOSTS_PER_WG, 0, st>>>((const OutHost*)C.hosts.p, (OutHost*)O.hosts.p,
                                                      (const uint64_t*)q.inc.p, seg_off, C.seg(), O.seg(), C.ptrs(), A, X, H,
                                                      q.qdisc, until, q.bootstrap_end, cnt, rem, dred);
    HIP_CHECK(hipGetLastError());
    // (const inputs: the iterator type these scans have always been instantiated with, see exclusive_sum)
    exclusive_sum(q.scantmp, (const uint64_t*)cnt, offs, (int)H + 1, st);
    exclusive_sum(q.scantmp, (const uint64_t*)rem, new_off, (int)H + 1, st);
    uint64_t total = 0, kept = 0;  // (the two totals ride in the record's synchronise)
    HIP_CHECK(hipMemcpyAsync(&total, offs + H, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&kept, new_off + H, 8, hipMemcpyDeviceToHost, st));
    r = read_back<OutReduce>(dred, st);
    if (total > capacity) {
        if (res) {
            res->num_sent = r.sent;
            res->num_local = r.local;
        }
        fail(SRG_ERR_ARG, "out_capacity too small: " + std::to_string(total) + " packets leave (nothing changed)");
    }
    O.reserve(kept);
    if (out_off) HIP_CHECK(hipMemcpyAsync(out_off, offs, ((size_t)H + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (H && (total || kept)) {
        k_out_commit<<<(H + OUT_HOSTS_PER_WG - 1) / OUT_HOSTS_PER_WG, 64 * OUT_HOSTS_PER_WG, 0, st>>>(
            (const OutHost*)C.hosts.p, seg_off, O.seg(), C.ptrs(), A, X, H, cnt, offs, out_status, out_time, out_tag,
            O.ptrs());
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(st));
    q.sets.flip();
    q.ctr = srg_outbound::Counters{kept, r.cached, r.min_wake};
    out_fill_result(q, r.sent, r.local, res);
}

OutHost out_read_host(srg_outbound& q, uint32_t host) {
    if (host >= q.num_hosts) fail(SRG_ERR_ARG, "host out of range (>= num_hosts)");
    OutHost s;
    HIP_CHECK(hipMemcpy(&s, (const OutHost*)q.sets.current().hosts.p + host, sizeof(OutHost), hipMemcpyDeviceToHost));
    return s;
}

void out_host_state(srg_outbound& q, uint32_t host, struct srg_outbound_host_state* out) {
    const OutHost s = out_read_host(q, host);
    out->balance = s.balance;
    out->last_refill_ns = s.last_refill;
    out->wake_ns = s.pending ? s.wake : 0;
    out->cached_tag = s.has_cached ? s.cached_tag : 0;
    out->queued = s.queued;
    out->qdisc_len = s.qlen;
    out->pending = s.pending;
    out->has_cached = s.has_cached;
    out->reserved[0] = out->reserved[1] = 0;
}

void out_host_order(srg_outbound& q, uint32_t host, uint32_t* slots, uint32_t capacity, uint32_t* n) {
    const OutHost s = out_read_host(q, host);
    *n = s.qlen;
    const uint64_t s0 = q.seg_off_host[host];
    const uint32_t cap = (uint32_t)(q.seg_off_host[host + 1] - s0);
    if (!s.qlen || !capacity) return;
    std::vector<uint32_t> ord(cap);
    HIP_CHECK(hipMemcpy(ord.data(), (const uint32_t*)q.sets.current().ord.p + s0, (size_t)cap * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < s.qlen && i < capacity; ++i)
        slots[i] = ord[q.qdisc == OUT_QDISC_ROUND_ROBIN ? (s.rr_head + i) % cap : i];
}

}  // namespace

extern "C" {

int srg_outbound_step_device(srg_outbound* q, uint64_t until_ns, uint64_t num_offers, const uint64_t* time_ns,
                             const uint32_t* socket, const uint64_t* priority, const uint32_t* total_size,
                             const uint8_t* flags, const uint64_t* tag, const uint64_t* host_offsets, uint64_t out_capacity,
                             uint8_t* out_status, uint64_t* out_time, uint64_t* out_tag, uint64_t* out_off, void* hip_stream,
                             srg_outbound_result* res, char* errbuf, size_t errlen) {
    if (!q || !host_offsets || (num_offers && (!time_ns || !socket || !priority || !total_size || !tag)) ||
        (out_capacity && (!out_status || !out_time || !out_tag || !out_off))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(q->ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        out_step(*q, until_ns, OutOffers{num_offers, time_ns, socket, priority, total_size, flags, tag, host_offsets},
                 out_capacity, out_status, out_time, out_tag, out_off, st, res);
    });
}

int srg_outbound_host_state(srg_outbound* q, uint32_t host, struct srg_outbound_host_state* out) {
    if (!q || !out) return SRG_ERR_ARG;
    return device_call(q->ctx, nullptr, nullptr, nullptr, 0, [&](hipStream_t) { out_host_state(*q, host, out); });
}

int srg_outbound_host_order(srg_outbound* q, uint32_t host, uint32_t* slots, uint32_t capacity, uint32_t* n) {
    if (!q || !n || (capacity && !slots)) return SRG_ERR_ARG;
    return device_call(q->ctx, nullptr, nullptr, nullptr, 0,
                       [&](hipStream_t) { out_host_order(*q, host, slots, capacity, n); });
}

}  // extern "C"

namespace {
