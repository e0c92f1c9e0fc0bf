// outbound_run.hip.h -- the host side of the hosts' outbound path (outbound.hip.h): the driver behind
// srg_outbound_step_device and the small read-backs of srg_outbound_host_state / _host_order.  A
// section of routing.hip's translation unit, included there once inside its anonymous namespace (it
// uses srg_ctx, DevBuf, fail and grid_for from the text above it); not a header to include elsewhere.
// struct srg_outbound is the C ABI's opaque type, so the section leaves the anonymous namespace
// around it and enters it again.
//
// Two sets of resident arrays, as in the inbound path: `cur` is the state, the other one is where a
// step builds its result; it becomes `cur` only after the device flags and totals were read (an
// error leaves the state as it was).  Every path that queued work synchronises `st` before it
// returns.

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
            if (n <= cap) return;
            const uint64_t want = std::max(n, 2 * cap);
            cap = 0;  // (a failed allocation leaves the set empty, not half grown)
            slot.get(want * 4);
            prio.get(want * 8);
            size.get(want * 4);
            flags.get(want);
            tag.get(want * 8);
            next.get(want * 4);
            cap = want;
        }
    } set[2];
    int cur = 0;
    DevBuf inc, seg_off, lnk, gone, newidx, o_idx, o_time, o_status, cnt, rem, offs, red, scantmp;
    uint64_t backlog = 0;  // packets in the current set's backlog arrays
    uint64_t cached = 0;   // hosts whose relay holds a cached packet
    uint64_t min_wake = UINT64_MAX;
};

namespace {

void out_scan(srg_outbound& q, const uint64_t* in, uint64_t* out, hipStream_t st) {
    const int n = (int)q.num_hosts + 1;
    size_t tb = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, n, st));
    void* tmp = q.scantmp.get(tb);
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, out, n, st));
}

void out_fill_result(const srg_outbound& q, uint64_t sent, uint64_t local, srg_outbound_result* res) {
    if (!res) return;
    res->num_sent = sent;
    res->num_local = local;
    res->num_queued = q.backlog + q.cached;
    res->min_next_wake_ns = q.min_wake;
}

void out_step(srg_outbound& q, uint64_t until, const OutOffers& A, uint64_t capacity, uint8_t* out_status,
              uint64_t* out_time, uint64_t* out_tag, uint64_t* out_off, hipStream_t st, srg_outbound_result* res) {
    out_fill_result(q, 0, 0, res);
    if (until > INB_TIME_END) fail(SRG_ERR_ARG, "until_ns outside the time domain (> 2^62)");
    const uint32_t H = q.num_hosts;
    // a host's packets are indexed in 32 bits (OUT_NIL is the end of a FIFO)
    if (A.n >= (1ull << 32) || q.backlog + A.n + H >= 0xffffffffull)
        fail(SRG_ERR_ARG, "too many packets in one step (queued + offers must stay below 2^32)");
    srg_outbound::Set& C = q.set[q.cur];
    srg_outbound::Set& O = q.set[q.cur ^ 1];
    OutReduce* dred = (OutReduce*)q.red.p;
    const OutReduce init{~0ull, 0ull, 0ull, 0ull, 0u, 0u};
    HIP_CHECK(hipMemcpyAsync(dred, &init, sizeof(OutReduce), hipMemcpyHostToDevice, st));
    // the step walks the offsets and trusts slots, sizes and the order of the times: validated
    // first, read back first
    const uint64_t* seg_off = (const uint64_t*)q.seg_off.p;
    k_out_validate<<<grid_for(std::max<uint64_t>(A.n, (uint64_t)H + 1), 2048), kThreads, 0, st>>>(
        A, (const OutHost*)C.hosts.p, (const uint64_t*)q.inc.p, seg_off, H, q.sim_start, until, dred);
    HIP_CHECK(hipGetLastError());
    OutReduce r;
    HIP_CHECK(hipMemcpyAsync(&r, dred, sizeof(OutReduce), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
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
    const uint64_t nseq = q.backlog + A.n;
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
    out_scan(q, cnt, offs, st);
    out_scan(q, rem, new_off, st);
    uint64_t total = 0, kept = 0;
    HIP_CHECK(hipMemcpyAsync(&total, offs + H, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&kept, new_off + H, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&r, dred, sizeof(OutReduce), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
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
    q.cur ^= 1;
    q.backlog = kept;
    q.cached = r.cached;
    q.min_wake = r.min_wake;
    out_fill_result(q, r.sent, r.local, res);
}

OutHost out_read_host(srg_outbound& q, uint32_t host) {
    if (host >= q.num_hosts) fail(SRG_ERR_ARG, "host out of range (>= num_hosts)");
    OutHost s;
    HIP_CHECK(hipMemcpy(&s, (const OutHost*)q.set[q.cur].hosts.p + host, sizeof(OutHost), hipMemcpyDeviceToHost));
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
    HIP_CHECK(hipMemcpy(ord.data(), (const uint32_t*)q.set[q.cur].ord.p + s0, (size_t)cap * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < s.qlen && i < capacity; ++i)
        slots[i] = ord[q.qdisc == OUT_QDISC_ROUND_ROBIN ? (s.rr_head + i) % cap : i];
}
