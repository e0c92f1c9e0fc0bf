// send_rule.h — the per-packet decisions of Worker::send_packet that the send batch makes on the
// device, shared by the kernel (k_ev_prep<true>, events.hip.h) and a CPU unit test
// (tests/cpp/send_rule_check.cpp, built with g++).
//
// Reference, src/main/core/worker.rs:
//   :337-338  is_bootstrapping = current_time < bootstrap_end_time
//   :374-377  reliability = 1.0f32 - packet_loss (worker.rs:563-568: the subtraction in f32, then
//             widened to f64); chance = src_host.random_mut().gen::<f64>(), drawn for every packet
//   :381-389  dropped iff !is_bootstrapping && chance >= reliability && payload_size > 0
//   :392      delay = RoutingInfo latency(src, dst)
// The latency comes from either form a RoutingInfo keeps (routing_info.cpp): u64 ns, or the build's
// u32 keys (latency = key * unit off the diagonal, the raw self-loop latency on it).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SRG_SEND_HD __host__ __device__
#else
#define SRG_SEND_HD
#endif

namespace srg {

SRG_SEND_HD inline bool dropped(float loss, double chance, uint32_t payload, uint64_t send_ns,
                                uint64_t bootstrap_end_ns) {
    const float reliability = 1.0f - loss;  // f32 first: a loss below half an ulp of 1 never drops
    return send_ns >= bootstrap_end_ns && chance >= (double)reliability && payload > 0;
}

// a routing table by node position: lat (u64 ns), or key + diag + unit when lat is null
struct PathLatency {
    const uint64_t* lat;
    const uint32_t* key;
    const uint64_t* diag;
    uint64_t unit;
    uint32_t n;
};

SRG_SEND_HD inline uint64_t path_latency(const PathLatency& t, uint32_t a, uint32_t b) {
    const size_t k = (size_t)a * t.n + b;
    if (t.lat) return t.lat[k];
    return a == b ? t.diag[a] : (uint64_t)t.key[k] * t.unit;
}

}  // namespace srg
