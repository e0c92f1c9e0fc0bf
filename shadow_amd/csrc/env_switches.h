// env_switches.h -- every SRG_* environment switch read by routing.hip, one function each.
// A switch is read where its function is called, on every call: tests and bench.py set these
// between calls on a live process, so nothing here is cached.  Each is tagged
//   [debug]  prints to stderr, changes no result
//   [A/B]    selects between two implementations for measurement
//   [test]   forces a path that tests need to reach
// Plain C++: no HIP include.  (comm.hip reads its own SRG_SIM_* variables.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace srg_env {

static inline bool is_set(const char* name) { return std::getenv(name) != nullptr; }
static inline bool first_char_is(const char* name, char ch) {
    const char* e = std::getenv(name);
    return e && e[0] == ch;
}
static inline bool equals(const char* name, const char* value) {
    const char* e = std::getenv(name);
    return e && std::strcmp(e, value) == 0;
}

// [A/B] SRG_STREAM_HOPS=events: the FW's cross-stream hops use events, never signal values
static inline bool stream_hops_events() { return equals("SRG_STREAM_HOPS", "events"); }
// [A/B] SRG_FW_BULK_Q=0... / 1...: the symmetric FW's quadrant bulk forced off (0) / on (1); -1 = auto
static inline int fw_bulk_q() {
    const char* e = std::getenv("SRG_FW_BULK_Q");
    return !e ? -1 : e[0] == '0' ? 0 : e[0] == '1' ? 1 : -1;
}
// [debug] SRG_DEBUG_OVERLAP (set): timings of the FW beside the H2D and of the late-loss thread
static inline bool debug_overlap() { return is_set("SRG_DEBUG_OVERLAP"); }
// [debug] SRG_DEBUG_SPARSE: 0 = unset, 1 = set (build / phase timings), 2 = first character '2'
// (also per-batch durations, which adds a device buffer and a synchronisation)
static inline int debug_sparse() {
    const char* e = std::getenv("SRG_DEBUG_SPARSE");
    return !e ? 0 : e[0] == '2' ? 2 : 1;
}
// [debug] SRG_DEBUG_CODEC (set): the H2D codec's chunk counts and host times
static inline bool debug_codec() { return is_set("SRG_DEBUG_CODEC"); }
// [debug] SRG_DEBUG_CREATE (set): where srg_create's time goes
static inline bool debug_create() { return is_set("SRG_DEBUG_CREATE"); }
// [A/B] SRG_SPARSE_KERNEL=bf: the lexicographic sweeps for u32 keys instead of the two-phase kernel
static inline bool sparse_kernel_bf() { return equals("SRG_SPARSE_KERNEL", "bf"); }
// [A/B] SRG_SPARSE_SPLIT=0...: the two-phase sparse kernel as one fused launch instead of two
static inline bool sparse_split_off() { return first_char_is("SRG_SPARSE_SPLIT", '0'); }
// [test] SRG_LATENCY_UNIT=1: nanosecond keys instead of the latencies' gcd unit (also A/B, bench.py)
static inline bool latency_unit_ns() { return equals("SRG_LATENCY_UNIT", "1"); }
// [A/B] SRG_CODEC_THREADS=n: the host pool's size (at least 1); 0 = unset
static inline int codec_threads() {
    const char* e = std::getenv("SRG_CODEC_THREADS");
    return e ? std::max(1, std::atoi(e)) : 0;
}
// [A/B] SRG_CODEC_SEQ=0: the H2D codec without its sequential-pair chunks
static inline bool codec_seq_off() { return equals("SRG_CODEC_SEQ", "0"); }
// [test] SRG_CODEC_SLOW_AFTER=k: the codec's host-slow switch fires after chunk k, whatever the times
static inline bool codec_slow_after(size_t& chunk) {
    const char* e = std::getenv("SRG_CODEC_SLOW_AFTER");
    if (e) chunk = (size_t)std::atoll(e);
    return e != nullptr;
}
// [A/B] SRG_PREFAULT=0: the caller's fresh output arrays are not faulted in before page-locking
static inline bool prefault_on() { return !equals("SRG_PREFAULT", "0"); }
// [A/B] SRG_NO_KEY_D2H (set): latency rows leave as u64 ns, not as u32 keys widened on the host
static inline bool no_key_d2h() { return is_set("SRG_NO_KEY_D2H"); }
// [test] SRG_LOSS_ROWS_MAX_V=n: the dense build's per-row LDS loss fold only for V <= n, so a small
// graph takes the global-memory fold (and, as at large V, neither the mirrored scan, the interleaved
// scan groups nor the packed predecessor rows).  Only ever lowers the limit: `limit` is the largest V
// whose rows fit LDS, and a value above it (or no value) returns it unchanged.
static inline unsigned loss_rows_max_v(unsigned limit) {
    const char* e = std::getenv("SRG_LOSS_ROWS_MAX_V");
    if (!e || !*e) return limit;
    char* end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    if (end == e || *end) return limit;  // not a number: ignored
    return v < limit ? (unsigned)v : limit;
}
// [A/B] SRG_ROUTE_TREE_GROUP=16 / 64: the route trees' predecessor kernel with 16 lanes or a wave per target
// (route_trees.hip.h); 0 = unset: chosen by the average list length
static inline int route_tree_group() {
    return equals("SRG_ROUTE_TREE_GROUP", "64") ? 64 : equals("SRG_ROUTE_TREE_GROUP", "16") ? 16 : 0;
}
// [test] SRG_ROUTE_TREE_LDS_MAX_V=n: the route trees keep a row's doubling jumps and subtree sums in LDS
// only for V <= n, so a small graph takes the global-scratch paths of a large one.  Only ever lowers
// the limit (as SRG_LOSS_ROWS_MAX_V above).
static inline unsigned route_tree_lds_max_v(unsigned limit) {
    const char* e = std::getenv("SRG_ROUTE_TREE_LDS_MAX_V");
    if (!e || !*e) return limit;
    char* end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    if (end == e || *end) return limit;  // not a number: ignored
    return v < limit ? (unsigned)v : limit;
}
// [A/B] SRG_CREATE_WARM=0...: srg_create skips its warm-up
static inline bool create_warm_off() { return first_char_is("SRG_CREATE_WARM", '0'); }

}  // namespace srg_env
