// inbound_run.hip.h -- the host side of the hosts' inbound path (inbound.hip.h): the driver behind
// srg_inbound_step_device and the small read-back of srg_inbound_host_state, and the srg_inbound_*
// entry points themselves.  A section of routing.hip's translation unit, included there once inside
// its anonymous namespace (it uses srg_ctx, DevBuf, fail, grid_for and device_call from the text
// above it and the helpers of stage.hip.h); not a header to include elsewhere.  struct srg_inbound
// is the C ABI's opaque type and the entry points are extern "C", so the section leaves the
// anonymous namespace around them and enters it again.
//
// The stage discipline of stage.hip.h: the current set is the state, a step builds its result into
// the spare one and flips after the device flags and totals were read.  Every path that queued work
// synchronises `st` before it returns.

}  // namespace

struct srg_inbound {
    srg_ctx* ctx = nullptr;
    uint32_t num_hosts = 0;
    uint64_t sim_start = 0, bootstrap_end = 0;
    struct Set {
        DevBuf hosts, time, size, tag, host_off;
        uint64_t cap = 0;
        InbBacklog ptrs() const { return InbBacklog{(uint64_t*)time.p, (uint32_t*)size.p, (uint64_t*)tag.p, (uint64_t*)host_off.p}; }
        void reserve(uint64_t n) { grow_columns(cap, n, {{&time, 8}, {&size, 4}, {&tag, 8}}); }
    };
    TwoSets<Set> sets;
    DevBuf inc, scr_status, scr_time, hout, cnt, rem, offs, red, scantmp;
    uint64_t backlog = 0;  // packets in the current set's backlog arrays
    uint64_t cached = 0;   // hosts whose relay holds a cached packet
    uint64_t min_wake = UINT64_MAX;
};

extern "C" {

int srg_inbound_create(srg_ctx* ctx, uint32_t num_hosts, const uint64_t* bw_down_bits, uint64_t sim_start_ns,
                       uint64_t bootstrap_end_ns, uint64_t reserve_packets, srg_inbound** out, char* errbuf,
                       size_t errlen) {
    if (!ctx || !out || (num_hosts && !bw_down_bits)) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    *out = nullptr;
    if (!sim_start_ok(sim_start_ns, errbuf, errlen)) return SRG_ERR_ARG;
    return stage_create(ctx, num_hosts, out, errbuf, errlen, [&](srg_inbound& q, hipStream_t st) {
        q.sim_start = sim_start_ns;
        q.bootstrap_end = bootstrap_end_ns;
        const size_t hb = host_row_bytes(num_hosts);
        for (auto& s : q.sets.set) {
            HIP_CHECK(hipMemsetAsync(s.host_off.get(hb), 0, hb, st));
            s.hosts.get((size_t)num_hosts * sizeof(InbHost));
            s.reserve(reserve_packets);
        }
        for (DevBuf* b : {&q.cnt, &q.rem, &q.offs}) b->get(hb);
        q.hout.get((size_t)num_hosts * sizeof(InbHostOut));
        q.red.get(sizeof(InbReduce));
        uint64_t* inc = (uint64_t*)q.inc.get((size_t)num_hosts * 8);
        if (num_hosts) {
            uint64_t* bw = (uint64_t*)q.scr_time.get((size_t)num_hosts * 8);
            HIP_CHECK(hipMemcpyAsync(bw, bw_down_bits, (size_t)num_hosts * 8, hipMemcpyHostToDevice, st));
            k_inb_init<<<grid_for(num_hosts), kThreads, 0, st>>>(bw, num_hosts, sim_start_ns, inc,
                                                                 (InbHost*)q.sets.set[0].hosts.p,
                                                                 (InbHost*)q.sets.set[1].hosts.p);
            HIP_CHECK(hipGetLastError());
        }
    });
}

void srg_inbound_destroy(srg_inbound* q) { stage_destroy(q); }

}  // extern "C"

namespace {

void inb_fill_result(const srg_inbound& q, uint64_t fwd, uint64_t drop, srg_inbound_result* res) {
    if (!res) return;
    res->num_forwarded = fwd;
    res->num_dropped = drop;
    res->num_queued = q.backlog + q.cached;
    res->min_next_wake_ns = q.min_wake;
}

void inb_step(srg_inbound& q, uint64_t until, const InbArrivals& A, uint64_t capacity, uint8_t* out_status,
              uint64_t* out_time, uint64_t* out_tag, uint64_t* out_off, hipStream_t st, srg_inbound_result* res) {
    inb_fill_result(q, 0, 0, res);
    if (until > INB_TIME_END) fail(SRG_ERR_ARG, "until_ns outside the time domain (> 2^62)");
    if (A.n >= (1ull << 40)) fail(SRG_ERR_ARG, "too many arrivals in one step");
    const uint32_t H = q.num_hosts;
    srg_inbound::Set& C = q.sets.current();
    srg_inbound::Set& O = q.sets.spare();
    InbReduce* dred = (InbReduce*)q.red.p;
    const InbReduce init{~0ull, 0ull, 0ull, 0ull, 0u, 0u};
    HIP_CHECK(hipMemcpyAsync(dred, &init, sizeof(InbReduce), hipMemcpyHostToDevice, st));
    // the step walks the offsets and trusts the order of the times: validated first, read back first
    k_inb_validate<<<grid_for(std::max<uint64_t>(A.n, (uint64_t)H + 1), 2048), kThreads, 0, st>>>(
        A, (const InbHost*)C.hosts.p, (const uint64_t*)q.inc.p, H, q.sim_start, until, dred);
    HIP_CHECK(hipGetLastError());
    InbReduce r = read_back<InbReduce>(dred, st);
    if (r.flags & INB_BAD_OFFSETS)
        fail(SRG_ERR_ARG, "host_offsets are not monotone from 0 to num_arrivals");
    if (r.flags & INB_BAD_TIME)
        fail(SRG_ERR_ARG, "an arrival time is outside [sim_start_ns, 2^62) or not below until_ns");
    if (r.flags & INB_BAD_SIZE)
        fail(SRG_ERR_ARG, "a packet is larger than its host's token bucket (refill + 1500): it would never conform");
    if (r.flags & INB_TIME_BACKWARD)
        fail(SRG_ERR_TIME_BACKWARD,
             "an arrival is earlier than its host's previous arrival or its last executed forward task");
    const uint64_t nseq = q.backlog + A.n;
    uint8_t* scr_status = (uint8_t*)q.scr_status.get(nseq);
    uint64_t* scr_time = (uint64_t*)q.scr_time.get(nseq * 8);
    InbHostOut* hout = (InbHostOut*)q.hout.p;
    uint64_t* cnt = (uint64_t*)q.cnt.p;
    uint64_t* rem = (uint64_t*)q.rem.p;
    uint64_t* offs = (uint64_t*)q.offs.p;
    uint64_t* new_off = (uint64_t*)O.host_off.p;
    const unsigned wgs = (unsigned)(((uint64_t)H + 1 + INB_HOSTS_PER_WG - 1) / INB_HOSTS_PER_WG);
    k_inb_step<<<wgs, 64 * INB_HOSTS_PER_WG, 0, st>>>((const InbHost*)C.hosts.p, (InbHost*)O.hosts.p,
                                                      (const uint64_t*)q.inc.p, C.ptrs(), A, H, until, q.bootstrap_end,
                                                      scr_status, scr_time, hout, cnt, rem, dred);
    HIP_CHECK(hipGetLastError());
    // (const inputs: the iterator type these scans have always been instantiated with, see exclusive_sum)
    exclusive_sum(q.scantmp, (const uint64_t*)cnt, offs, (int)H + 1, st);
    exclusive_sum(q.scantmp, (const uint64_t*)rem, new_off, (int)H + 1, st);
    uint64_t total = 0, kept = 0;  // (the two totals ride in the record's synchronise)
    HIP_CHECK(hipMemcpyAsync(&total, offs + H, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&kept, new_off + H, 8, hipMemcpyDeviceToHost, st));
    r = read_back<InbReduce>(dred, st);
    if (total > capacity) {
        if (res) {
            res->num_forwarded = r.forwarded;
            res->num_dropped = r.dropped;
        }
        fail(SRG_ERR_ARG, "out_capacity too small: " + std::to_string(total) + " packets leave (nothing changed)");
    }
    O.reserve(kept);
    if (out_off) HIP_CHECK(hipMemcpyAsync(out_off, offs, ((size_t)H + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (H && (total || kept)) {
        k_inb_commit<<<(H + INB_HOSTS_PER_WG - 1) / INB_HOSTS_PER_WG, 64 * INB_HOSTS_PER_WG, 0, st>>>(
            (const InbHost*)C.hosts.p, C.ptrs(), A, H, scr_status, scr_time, hout, offs, out_status, out_time, out_tag,
            O.ptrs());
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(st));
    q.sets.flip();
    q.backlog = kept;
    q.cached = r.cached;
    q.min_wake = r.min_wake;
    inb_fill_result(q, r.forwarded, r.dropped, res);
}

void inb_host_state(srg_inbound& q, uint32_t host, struct srg_inbound_host_state* out) {
    if (host >= q.num_hosts) fail(SRG_ERR_ARG, "host out of range (>= num_hosts)");
    const srg_inbound::Set& C = q.sets.current();
    InbHost s;
    uint64_t off[2];
    HIP_CHECK(hipMemcpy(&s, (const InbHost*)C.hosts.p + host, sizeof(InbHost), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(off, (const uint64_t*)C.host_off.p + host, 16, hipMemcpyDeviceToHost));
    out->balance = s.balance;
    out->last_refill_ns = s.last_refill;
    out->interval_end_ns = s.interval_end;
    out->drop_next_ns = s.drop_next;
    out->current_drop_count = s.cur_drops;
    out->previous_drop_count = s.prev_drops;
    out->bytes_stored = s.bytes;
    out->queued = off[1] - off[0];
    out->wake_ns = s.pending ? s.wake : 0;
    out->cached_tag = s.has_cached ? s.cached_tag : 0;
    out->mode = s.mode;
    out->has_interval_end = s.has_interval_end;
    out->has_drop_next = s.has_drop_next;
    out->pending = s.pending;
    out->has_cached = s.has_cached;
    out->reserved[0] = out->reserved[1] = out->reserved[2] = 0;
}

}  // namespace

extern "C" {

int srg_inbound_step_device(srg_inbound* q, uint64_t until_ns, uint64_t num_arrivals, const uint64_t* time_ns,
                            const uint32_t* total_size, const uint64_t* tag, const uint64_t* host_offsets,
                            uint64_t out_capacity, uint8_t* out_status, uint64_t* out_time, uint64_t* out_tag,
                            uint64_t* out_off, void* hip_stream, srg_inbound_result* res, char* errbuf, size_t errlen) {
    if (!q || !host_offsets || (num_arrivals && (!time_ns || !total_size || !tag)) ||
        (out_capacity && (!out_status || !out_time || !out_tag || !out_off))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(q->ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        inb_step(*q, until_ns, InbArrivals{num_arrivals, time_ns, total_size, tag, host_offsets}, out_capacity,
                 out_status, out_time, out_tag, out_off, st, res);
    });
}

int srg_inbound_host_state(srg_inbound* q, uint32_t host, struct srg_inbound_host_state* out) {
    if (!q || !out) return SRG_ERR_ARG;
    return device_call(q->ctx, nullptr, nullptr, nullptr, 0, [&](hipStream_t) { inb_host_state(*q, host, out); });
}

#ifdef SRG_TEST_HOOKS
// TEST HOOK (test build only, not in the header): the device's control-law increments for counts[n]
int srg_test_inbound_control_law(srg_ctx* ctx, const uint64_t* counts, uint32_t n, uint64_t* out) {
    if (!ctx || !counts || !out || !n) return SRG_ERR_ARG;
    return device_call(ctx, nullptr, nullptr, nullptr, 0, [&](hipStream_t st) {
        DevBuf in, res;
        in.get((size_t)n * 8);
        res.get((size_t)n * 8);
        HIP_CHECK(hipMemcpyAsync(in.p, counts, (size_t)n * 8, hipMemcpyHostToDevice, st));
        k_inb_test_law<<<grid_for(n), kThreads, 0, st>>>((const uint64_t*)in.p, n, (uint64_t*)res.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out, res.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    });
}
#endif

}  // extern "C"

namespace {
