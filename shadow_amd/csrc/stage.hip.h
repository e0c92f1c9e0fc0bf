// stage.hip.h -- what the resident stages of the host path share (events_run, inbound_run,
// outbound_run, round_run, sockets_in_run): the plumbing around their kernels, not their logic.  A
// section of routing.hip's translation unit, included there once inside its anonymous namespace in
// front of the run sections (it uses srg_ctx, DevBuf, fail, guard and HIP_CHECK from the text above
// it); not a header to include elsewhere.
//
// The stage discipline ("Resident stages"): a stage keeps two sets of resident arrays.
// A step seeds a small reduce record, launches, reads the record back and tests its flags; it builds
// into the spare set and flips last, so an error leaves the stage as it was.  A caller that composes
// stages and has to undo a step that succeeded takes the stage's snapshot() before and restore()s it.

// out[i] = in[0] + ... + in[i - 1].  tmp is the caller's own scratch: objects may run on different
// streams.  In is deduced, not const T*: hipcub's kernels are instantiated by iterator type, and a call
// site that changed its pointer's constness would add or drop scan kernels in the code object.  The
// call sites pass what they always passed (const uint64_t* in the queues, inbound and outbound;
// plain pointers in the round and interface receive).
template <class In, class T>
void exclusive_sum(DevBuf& tmp, In in, T* out, int n, hipStream_t st) {
    size_t tb = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, n, st));
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.get(tb), tb, in, out, n, st));
}

// A small record (or one scalar) from the device: the copy, the synchronise, the value.  Copies the
// caller queued on st before this land in the same synchronise.
template <class R>
R read_back(const void* dev, hipStream_t st) {
    R r;
    HIP_CHECK(hipMemcpyAsync(&r, dev, sizeof(R), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return r;
}

// A set's per-element columns grow together: to max(n, 2 * cap).
struct Column {
    DevBuf* buf;
    size_t elem;
};
inline void grow_columns(uint64_t& cap, uint64_t n, std::initializer_list<Column> cols) {
    if (n <= cap) return;
    const uint64_t want = std::max(n, 2 * cap);
    cap = 0;  // (a failed allocation leaves the set empty, not half grown)
    for (const Column& c : cols) c.buf->get(want * c.elem);
    cap = want;
}

// The two sets: current() is the state, spare() is where a step builds; flip() comes last.
template <class Set>
struct TwoSets {
    Set set[2];
    int cur = 0;
    Set& current() { return set[cur]; }
    const Set& current() const { return set[cur]; }
    Set& spare() { return set[cur ^ 1]; }
    void flip() { cur ^= 1; }
};

// srg_*_create behind its argument checks: under ctx->mu, on the context's device, a new S with ctx
// and num_hosts set, init(S&, stream) allocates and queues, one synchronise, then *out.
template <class S, class F>
int stage_create(srg_ctx* ctx, uint32_t num_hosts, S** out, char* errbuf, size_t errlen, F&& init) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    return guard(errbuf, errlen, [&]() {
        HIP_CHECK(hipSetDevice(ctx->device));
        std::unique_ptr<S> s(new S);
        s->ctx = ctx;
        s->num_hosts = num_hosts;
        init(*s, ctx->stream);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *out = s.release();
    });
}

// srg_*_destroy: the DevBufs free themselves on the context's device
template <class S>
void stage_destroy(S* s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(s->ctx->mu);
        (void)hipSetDevice(s->ctx->device);
    }
    delete s;
}

// the creates that take sim_start_ns: false (and the message) when it is outside the time domain
inline bool sim_start_ok(uint64_t sim_start_ns, char* errbuf, size_t errlen) {
    if (sim_start_ns < INB_TIME_END) return true;
    set_err(errbuf, errlen, "sim_start_ns outside the time domain (>= 2^62)");
    return false;
}

// one word per host and one more (offsets, heads, counts)
inline size_t host_row_bytes(uint32_t num_hosts) { return ((size_t)num_hosts + 1) * 8; }
