// sockets_in_run.hip.h -- the host side of interface receive (sockets_in.hip.h): the driver behind
// srg_sockets_in_step_device, the host-side batch calls (configure, associate, disassociate) and the
// two small read-backs, and the srg_sockets_in_* entry points themselves.  A section of routing.hip's
// translation unit, included there once inside its anonymous namespace (it uses srg_ctx, DevBuf,
// fail, grid_for, k_fill and device_call from the text above it and the helpers of stage.hip.h);
// not a header to include elsewhere.  struct srg_sockets_in is the C ABI's opaque type and the entry
// points are extern "C", so the section leaves the anonymous namespace around them and enters it
// again.
//
// The stage discipline of stage.hip.h: the current set is the state, a step builds its result
// (socket records, counters, message store) into the spare one and flips after the device flags and
// totals were read.  The associations live in a host map; the device table is rebuilt from it by
// the first step after a change, so a batch of association calls costs one upload.  Every path that
// queued work synchronises `st` before it returns.

}  // namespace

struct srg_sockets_in {
    srg_ctx* ctx = nullptr;
    uint32_t num_hosts = 0, num_socks = 0;
    std::vector<uint64_t> sock_off_h;  // [H + 1]
    struct Set {
        DevBuf socks, counters, tag, time, payload, off;
        uint64_t cap = 0;
        SinMsgs ptrs() const { return SinMsgs{(uint64_t*)tag.p, (uint64_t*)time.p, (uint32_t*)payload.p, (uint64_t*)off.p}; }
        void reserve(uint64_t n) { grow_columns(cap, n, {{&tag, 8}, {&time, 8}, {&payload, 4}}); }
    };
    TwoSets<Set> sets;
    SinPackets pk{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool have_packets = false;
    std::map<std::pair<uint64_t, uint64_t>, uint32_t> assoc;  // (sin_key_a, sin_key_b) -> slot
    bool table_dirty = true;
    uint64_t table_mask = 0;
    DevBuf sock_off, table, red, act, pos, key, c_time, c_row, coff, mkey, mval, skey, sval, ops_off, bufl, cnt, sout,
        sorttmp, scantmp, stage, zero_off;
    uint64_t messages = 0;  // messages in the current set's store
};

extern "C" {

int srg_sockets_in_create(srg_ctx* ctx, uint32_t num_hosts, const uint32_t* sockets_per_host, uint64_t reserve_messages,
                          srg_sockets_in** out, char* errbuf, size_t errlen) {
    if (!ctx || !out || (num_hosts && !sockets_per_host)) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    *out = nullptr;
    return stage_create(ctx, num_hosts, out, errbuf, errlen, [&](srg_sockets_in& q, hipStream_t st) {
        q.sock_off_h.assign((size_t)num_hosts + 1, 0);
        for (uint32_t h = 0; h < num_hosts; ++h) q.sock_off_h[h + 1] = q.sock_off_h[h] + sockets_per_host[h];
        if (q.sock_off_h[num_hosts] >= (1ull << 31)) fail(SRG_ERR_ARG, "too many socket slots (>= 2^31)");
        const uint32_t S = q.num_socks = (uint32_t)q.sock_off_h[num_hosts];
        const size_t hb = host_row_bytes(num_hosts), sb = ((size_t)S + 1) * 8;
        HIP_CHECK(hipMemcpyAsync(q.sock_off.get(hb), q.sock_off_h.data(), hb, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(q.zero_off.get(hb), 0, hb, st));
        for (auto& s : q.sets.set) {
            HIP_CHECK(hipMemsetAsync(s.off.get(sb), 0, sb, st));
            HIP_CHECK(hipMemsetAsync(s.counters.get((size_t)num_hosts * 40), 0, (size_t)num_hosts * 40, st));
            s.socks.get((size_t)S * sizeof(SinSocket));
            s.reserve(reserve_messages);
        }
        if (S) {
            k_sin_init<<<grid_for(S), kThreads, 0, st>>>(S, (SinSocket*)q.sets.set[0].socks.p);
            HIP_CHECK(hipGetLastError());
        }
        q.coff.get(((size_t)num_hosts + 1) * 4);
        q.ops_off.get(((size_t)S + 2) * 4);
        q.cnt.get(sb);
        q.sout.get((size_t)S * sizeof(SinSockOut));
        q.red.get(sizeof(SinReduce));
    });
}

void srg_sockets_in_destroy(srg_sockets_in* q) { stage_destroy(q); }

}  // extern "C"

namespace {

void sin_fill_result(const srg_sockets_in& q, const SinReduce* r, srg_sockets_in_result* res) {
    if (!res) return;
    const double ms = res->ms_total;
    *res = srg_sockets_in_result{};
    res->ms_total = ms;
    if (r) {
        res->num_skipped = r->status[SIN_SKIPPED];
        res->num_no_socket = r->status[SIN_NO_SOCKET];
        res->num_external = r->status[SIN_RCV_EXTERNAL];
        res->num_peer_mismatch = r->status[SIN_PEER_MISMATCH];
        res->num_full = r->status[SIN_FULL];
        res->num_buffered = r->status[SIN_BUFFERED];
        res->num_read = r->num_read;
        res->num_would_block = r->num_would_block;
    }
    res->num_buffered_messages = q.messages;
}

// the device table from the host map (load factor <= 1/2)
void sin_upload_table(srg_sockets_in& q, hipStream_t st) {
    const uint64_t cap = sin_table_capacity(q.assoc.size());
    std::vector<SinEntry> t(cap, SinEntry{0, 0, 0, 0, 0});
    for (const auto& kv : q.assoc) sin_table_insert(t.data(), cap - 1, kv.first.first, kv.first.second, kv.second);
    void* d = q.table.get(cap * sizeof(SinEntry));
    HIP_CHECK(hipMemcpyAsync(d, t.data(), cap * sizeof(SinEntry), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));  // (t is pageable and leaves scope)
    q.table_mask = cap - 1;
    q.table_dirty = false;
}

void sin_step(srg_sockets_in& q, const SinRows& R, const SinReads& Q, uint8_t* out_status, uint32_t* out_slot,
              uint8_t* r_status, uint64_t* r_tag, uint64_t* r_time, uint32_t* r_payload, hipStream_t st,
              srg_sockets_in_result* res) {
    sin_fill_result(q, nullptr, res);
    if (!q.have_packets) fail(SRG_ERR_ARG, "no packet table (srg_sockets_in_set_packets)");
    if (R.n + Q.n >= (1ull << 31)) fail(SRG_ERR_ARG, "too many rows and reads in one step");
    const uint32_t H = q.num_hosts, S = q.num_socks;
    const uint32_t n = (uint32_t)R.n, nr = (uint32_t)Q.n, M = n + nr;
    if (q.table_dirty) sin_upload_table(q, st);
    srg_sockets_in::Set& C = q.sets.current();
    srg_sockets_in::Set& O = q.sets.spare();
    SinReduce* dred = (SinReduce*)q.red.p;
    HIP_CHECK(hipMemsetAsync(dred, 0, sizeof(SinReduce), st));
    uint32_t* act = (uint32_t*)q.act.get(((size_t)n + 1) * 4);
    uint32_t* pos = (uint32_t*)q.pos.get(((size_t)n + 1) * 4);
    uint32_t* key = (uint32_t*)q.key.get((size_t)n * 4);
    uint64_t* c_time = (uint64_t*)q.c_time.get((size_t)n * 8);
    uint32_t* c_row = (uint32_t*)q.c_row.get((size_t)n * 4);
    uint32_t* coff = (uint32_t*)q.coff.p;
    uint32_t* mkey = (uint32_t*)q.mkey.get((size_t)M * 4);
    uint32_t* mval = (uint32_t*)q.mval.get((size_t)M * 4);
    uint32_t* skey = (uint32_t*)q.skey.get((size_t)M * 4);
    uint32_t* sval = (uint32_t*)q.sval.get((size_t)M * 4);
    uint32_t* bufl = (uint32_t*)q.bufl.get((size_t)M * 4);
    uint32_t* ops_off = (uint32_t*)q.ops_off.p;
    uint64_t* cnt = (uint64_t*)q.cnt.p;
    SinSockOut* sout = (SinSockOut*)q.sout.p;
    unsigned long long* ncnt = (unsigned long long*)O.counters.p;
    const SinSocket* csocks = (const SinSocket*)C.socks.p;
    const uint64_t* sock_off = (const uint64_t*)q.sock_off.p;
    if (H) HIP_CHECK(hipMemcpyAsync(ncnt, C.counters.p, (size_t)H * 40, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemsetAsync(act + n, 0, 4, st));
    // the later kernels walk the offsets and gather by tag: validated first, read back first
    k_sin_lookup<<<grid_for(std::max<uint64_t>(n, (uint64_t)H + 1), 2048), kThreads, 0, st>>>(
        R, Q, q.pk, (const SinEntry*)q.table.p, q.table_mask, csocks, sock_off, H, S, out_status, out_slot, act, key, ncnt,
        dred);
    HIP_CHECK(hipGetLastError());
    SinReduce r = read_back<SinReduce>(dred, st);
    if (r.flags & SIN_BAD_OFFSETS)
        fail(SRG_ERR_ARG, "host_offsets are not monotone from 0 to the number of rows / reads");
    if (r.flags & SIN_BAD_TAG) fail(SRG_ERR_ARG, "a delivery's tag is >= num_packets");
    exclusive_sum(q.scantmp, act, pos, (int)n + 1, st);  // (non-const inputs, as always here: see exclusive_sum)
    k_sin_compact<<<grid_for(std::max<uint64_t>(n, (uint64_t)H + 1), 2048), kThreads, 0, st>>>(R, act, pos, H, c_time,
                                                                                             c_row, coff);
    HIP_CHECK(hipGetLastError());
    if (M) {
        // (rows that are no buffer operation leave holes in the merged order: key S sorts them last)
        k_fill<uint32_t><<<grid_for(M, 2048), kThreads, 0, st>>>(mkey, (size_t)M, S);
        HIP_CHECK(hipGetLastError());
    }
    if (nr) {
        k_sin_reads<<<grid_for(nr, 2048), kThreads, 0, st>>>(Q, csocks, sock_off, H, S, c_time, coff, mkey, mval, dred);
        HIP_CHECK(hipGetLastError());
    }
    if (n) {
        k_sin_delivs<<<grid_for(n, 2048), kThreads, 0, st>>>(pos, n, Q, H, c_time, c_row, coff, key, mkey, mval, dred);
        HIP_CHECK(hipGetLastError());
    }
    if (M) {
        int end_bit = 1;
        while (end_bit < 32 && (S >> end_bit)) ++end_bit;
        size_t tb = 0;
        HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, mkey, skey, mval, sval, (int)M, 0, end_bit, st));
        void* tmp = q.sorttmp.get(tb);
        HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, tb, mkey, skey, mval, sval, (int)M, 0, end_bit, st));
    }
    k_sin_segments<<<grid_for((size_t)S + 2, 2048), kThreads, 0, st>>>(skey, M, S, ops_off);
    HIP_CHECK(hipGetLastError());
    const unsigned wgs = (unsigned)(((uint64_t)S + 1 + SIN_SOCKS_PER_WG - 1) / SIN_SOCKS_PER_WG);
    k_sin_chain<<<wgs, 64 * SIN_SOCKS_PER_WG, 0, st>>>(csocks, (SinSocket*)O.socks.p, C.ptrs(), R, Q, q.pk, S, sval, ops_off,
                                                       bufl, out_status, r_status, r_tag, r_time, r_payload, cnt, sout, dred);
    HIP_CHECK(hipGetLastError());
    uint64_t* new_off = (uint64_t*)O.off.p;
    exclusive_sum(q.scantmp, cnt, new_off, (int)S + 1, st);
    uint64_t kept = 0;  // (the total rides in the record's synchronise)
    HIP_CHECK(hipMemcpyAsync(&kept, new_off + S, 8, hipMemcpyDeviceToHost, st));
    r = read_back<SinReduce>(dred, st);
    if (r.flags & SIN_BAD_FLAG) fail(SRG_ERR_ARG, "a read carries an unknown flag bit");
    if (r.flags & SIN_BAD_SLOT) fail(SRG_ERR_ARG, "a read on a slot >= sockets_per_host[h] or on an EXTERNAL slot");
    if (r.flags & SIN_CONTRADICT)
        fail(SRG_ERR_ARG, "a read with SRG_READ_FIRST follows a read without it at the same time on one host");
    if (r.flags & SIN_BACKWARD)
        fail(SRG_ERR_TIME_BACKWARD, "a delivery or a read is earlier than its host's previous one");
    O.reserve(kept);
    if (S && kept) {
        k_sin_commit<<<(S + SIN_SOCKS_PER_WG - 1) / SIN_SOCKS_PER_WG, 64 * SIN_SOCKS_PER_WG, 0, st>>>(
            csocks, C.ptrs(), O.ptrs(), R, q.pk, S, ops_off, bufl, sout);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(st));
    q.sets.flip();
    q.messages = kept;
    sin_fill_result(q, &r, res);
}

uint32_t sin_sidx(const srg_sockets_in& q, uint32_t host, uint32_t slot, const char* what) {
    if (host >= q.num_hosts) fail(SRG_ERR_ARG, std::string(what) + ": host out of range (>= num_hosts)");
    if (slot >= q.sock_off_h[host + 1] - q.sock_off_h[host])
        fail(SRG_ERR_ARG, std::string(what) + ": slot out of range (>= sockets_per_host[host])");
    return (uint32_t)(q.sock_off_h[host] + slot);
}

void sin_configure(srg_sockets_in& q, uint64_t n, const uint32_t* host, const uint32_t* slot, const uint8_t* kind,
                   const uint8_t* has_peer, const uint32_t* peer_ip, const uint16_t* peer_port, const uint64_t* limit,
                   hipStream_t st) {
    std::map<uint32_t, SinConfig> last;  // a slot named twice keeps its last entry, as a sequence of calls would
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t sidx = sin_sidx(q, host[i], slot[i], "srg_sockets_in_configure");
        if (kind[i] > SIN_EXTERNAL || has_peer[i] > 1) fail(SRG_ERR_ARG, "srg_sockets_in_configure: unknown kind or has_peer");
        last[sidx] = SinConfig{limit[i], sidx, peer_ip[i], peer_port[i], kind[i], has_peer[i], 0};
    }
    if (last.empty()) return;
    std::vector<SinConfig> v;
    v.reserve(last.size());
    for (const auto& kv : last) v.push_back(kv.second);
    void* d = q.stage.get(v.size() * sizeof(SinConfig));
    HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(SinConfig), hipMemcpyHostToDevice, st));
    k_sin_configure<<<grid_for(v.size()), kThreads, 0, st>>>((const SinConfig*)d, v.size(), (SinSocket*)q.sets.current().socks.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));
}

void sin_associate(srg_sockets_in& q, uint64_t n, const uint32_t* host, const uint8_t* protocol, const uint16_t* local_port,
                   const uint32_t* peer_ip, const uint16_t* peer_port, const uint32_t* slot) {
    std::map<std::pair<uint64_t, uint64_t>, uint32_t> add;
    for (uint64_t i = 0; i < n; ++i) {
        sin_sidx(q, host[i], slot[i], "srg_sockets_in_associate");
        const auto k = std::make_pair(sin_key_a(host[i], peer_ip[i]), sin_key_b(protocol[i], local_port[i], peer_port[i]));
        // network_interface.c:85: utility_debugAssert(!g_hash_table_contains(...))
        if (q.assoc.count(k) || !add.emplace(k, slot[i]).second)
            fail(SRG_ERR_ARG, "srg_sockets_in_associate: the key is already associated (nothing added)");
    }
    if (q.assoc.size() + add.size() >= (1ull << 30)) fail(SRG_ERR_ARG, "srg_sockets_in_associate: too many associations");
    q.assoc.insert(add.begin(), add.end());
    if (!add.empty()) q.table_dirty = true;
}

void sin_disassociate(srg_sockets_in& q, uint64_t n, const uint32_t* host, const uint8_t* protocol,
                      const uint16_t* local_port, const uint32_t* peer_ip, const uint16_t* peer_port) {
    for (uint64_t i = 0; i < n; ++i)  // network_interface.c:113: removing a missing key is no error
        if (q.assoc.erase(std::make_pair(sin_key_a(host[i], peer_ip[i]), sin_key_b(protocol[i], local_port[i], peer_port[i]))))
            q.table_dirty = true;
}

void sin_socket_state(srg_sockets_in& q, uint32_t host, uint32_t slot, struct srg_sockets_in_socket_state* out) {
    const uint32_t sidx = sin_sidx(q, host, slot, "srg_sockets_in_socket_state");
    SinSocket s;
    HIP_CHECK(hipMemcpy(&s, (const SinSocket*)q.sets.current().socks.p + sidx, sizeof(SinSocket), hipMemcpyDeviceToHost));
    out->len_bytes = s.len;
    out->num_messages = s.count;
    out->soft_limit_bytes = s.limit;
    out->peer_ip = s.peer_ip;
    out->peer_port = s.peer_port;
    out->kind = s.kind;
    out->has_peer = s.has_peer;
}

void sin_host_counters(srg_sockets_in& q, uint32_t host, struct srg_sockets_in_host_counters* out, int reset) {
    if (host >= q.num_hosts) fail(SRG_ERR_ARG, "host out of range (>= num_hosts)");
    uint64_t* c = (uint64_t*)q.sets.current().counters.p + (size_t)host * 5;
    uint64_t v[5];
    HIP_CHECK(hipMemcpy(v, c, 40, hipMemcpyDeviceToHost));
    out->packets_control = v[0];
    out->packets_data = v[1];
    out->bytes_control_header = v[2];
    out->bytes_data_header = v[3];
    out->bytes_data_payload = v[4];
    if (reset) HIP_CHECK(hipMemset(c, 0, 40));  // tracker.c:608
}

}  // namespace

extern "C" {

int srg_sockets_in_set_packets(srg_sockets_in* q, uint64_t num_packets, const uint8_t* protocol, const uint32_t* src_ip,
                               const uint16_t* src_port, const uint16_t* dst_port, const uint32_t* total_size,
                               const uint32_t* payload_size) {
    if (!q || (num_packets && (!protocol || !src_ip || !src_port || !dst_port || !total_size || !payload_size)))
        return SRG_ERR_ARG;
    std::lock_guard<std::mutex> lk(q->ctx->mu);
    q->pk = SinPackets{num_packets, protocol, src_ip, src_port, dst_port, total_size, payload_size};
    q->have_packets = true;
    return SRG_OK;
}

int srg_sockets_in_configure(srg_sockets_in* q, uint64_t n, const uint32_t* host, const uint32_t* slot, const uint8_t* kind,
                             const uint8_t* has_peer, const uint32_t* peer_ip, const uint16_t* peer_port,
                             const uint64_t* soft_limit_bytes, char* errbuf, size_t errlen) {
    if (!q || (n && (!host || !slot || !kind || !has_peer || !peer_ip || !peer_port || !soft_limit_bytes))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(q->ctx, nullptr, nullptr, errbuf, errlen, [&](hipStream_t st) {
        sin_configure(*q, n, host, slot, kind, has_peer, peer_ip, peer_port, soft_limit_bytes, st);
    });
}

int srg_sockets_in_associate(srg_sockets_in* q, uint64_t n, const uint32_t* host, const uint8_t* protocol,
                             const uint16_t* local_port, const uint32_t* peer_ip, const uint16_t* peer_port,
                             const uint32_t* slot, char* errbuf, size_t errlen) {
    if (!q || (n && (!host || !protocol || !local_port || !peer_ip || !peer_port || !slot))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(q->ctx->mu);
    return guard(errbuf, errlen, [&]() { sin_associate(*q, n, host, protocol, local_port, peer_ip, peer_port, slot); });
}

int srg_sockets_in_disassociate(srg_sockets_in* q, uint64_t n, const uint32_t* host, const uint8_t* protocol,
                                const uint16_t* local_port, const uint32_t* peer_ip, const uint16_t* peer_port,
                                char* errbuf, size_t errlen) {
    if (!q || (n && (!host || !protocol || !local_port || !peer_ip || !peer_port))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(q->ctx->mu);
    return guard(errbuf, errlen, [&]() { sin_disassociate(*q, n, host, protocol, local_port, peer_ip, peer_port); });
}

int srg_sockets_in_step_device(srg_sockets_in* q, uint64_t num_rows, const uint8_t* status, const uint64_t* time_ns,
                               const uint64_t* tag, const uint64_t* host_offsets, uint8_t deliver_status,
                               uint64_t num_reads, const uint64_t* read_time_ns, const uint32_t* read_slot,
                               const uint8_t* read_flags, const uint64_t* read_host_offsets, uint8_t* out_status,
                               uint32_t* out_slot, uint8_t* out_read_status, uint64_t* out_read_tag,
                               uint64_t* out_read_time_ns, uint32_t* out_read_payload, void* hip_stream,
                               srg_sockets_in_result* res, char* errbuf, size_t errlen) {
    if (!q || (num_rows && (!time_ns || !tag || !host_offsets || !out_status || !out_slot)) ||
        (num_reads && (!read_time_ns || !read_slot || !read_host_offsets || !out_read_status || !out_read_tag ||
                       !out_read_time_ns || !out_read_payload))) {
        set_err(errbuf, errlen, "null argument");
        return SRG_ERR_ARG;
    }
    return device_call(q->ctx, hip_stream, res ? &res->ms_total : nullptr, errbuf, errlen, [&](hipStream_t st) {
        const uint64_t* zero = (const uint64_t*)q->zero_off.p;  // (no rows / no reads: the offsets may be NULL)
        sin_step(*q, SinRows{num_rows, status, time_ns, tag, host_offsets ? host_offsets : zero, deliver_status},
                 SinReads{num_reads, read_time_ns, read_slot, read_flags, read_host_offsets ? read_host_offsets : zero},
                 out_status, out_slot, out_read_status, out_read_tag, out_read_time_ns, out_read_payload, st, res);
    });
}

int srg_sockets_in_socket_state(srg_sockets_in* q, uint32_t host, uint32_t slot, struct srg_sockets_in_socket_state* out) {
    if (!q || !out) return SRG_ERR_ARG;
    return device_call(q->ctx, nullptr, nullptr, nullptr, 0, [&](hipStream_t) { sin_socket_state(*q, host, slot, out); });
}

int srg_sockets_in_host_counters(srg_sockets_in* q, uint32_t host, struct srg_sockets_in_host_counters* out, int reset) {
    if (!q || !out) return SRG_ERR_ARG;
    return device_call(q->ctx, nullptr, nullptr, nullptr, 0,
                       [&](hipStream_t) { sin_host_counters(*q, host, out, reset); });
}

}  // extern "C"

namespace {
