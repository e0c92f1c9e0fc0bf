// sockets_in_rule.h — what lies behind the inbound relay on a host: the interface's socket lookup,
// the UDP socket's receive buffer and the tracker's input counters.  The rule the sockets-in step
// runs on the device (sockets_in.hip.h), shared with a CPU unit test
// (tests/cpp/sockets_in_rule_check.cpp, built with g++).  Plain C++, no HIP types.
//
// Reference (src/main/):
//   relay/mod.rs:261-271                 a forwarded packet: dst.push(packet) -> networkinterface_push
//   host/network/network_interface.c:77-117   associate (a key collision is utility_debugAssert) /
//                                        disassociate (removing a missing key is no error)
//   network_interface.c:140-202          networkinterface_push: the specific key (protocol, bind port,
//                                        peer ip, peer port), else the wildcard key (peer 0:0); no
//                                        socket: PDS_RCV_INTERFACE_DROPPED; the tracker counts the
//                                        packet if and only if a socket was found (:192-197)
//   host/descriptor/socket/inet/udp.rs:108-168   UdpSocket::push_in_packet: the peer filter on the
//                                        whole SocketAddrV4 (:116-135), then has_space (:140)
//   udp.rs:1081-1157                     MessageBuffer: has_space is len_bytes < soft_limit_bytes, a
//                                        push adds the payload length, a pop subtracts it; the limit
//                                        is soft (one message may carry len_bytes past it) and may be
//                                        changed under a non-empty buffer (:1154)
//   udp.rs:497-546                       recvmsg: empty -> EWOULDBLOCK; MSG_PEEK leaves the message
//   host/tracker.c:188-252               _tracker_updateCounters: payload 0 is a control packet
//
// The interface's own address is part of the reference's key and constant per host: the host id
// stands for it.  A socket is a slot (host, slot); the table maps a key to a slot.
//
// Order on a host.  Its deliveries come in the order given, its reads in execution order, both with
// non-decreasing times.  A read at t runs after every delivery with time < t; at equal time it runs
// before the deliveries if and only if it carries SIN_READ_FIRST (in the reference both are local
// events of one nanosecond, ordered by event id).  sin_read_before is that predicate; over a valid
// read list it is monotone for any delivery, which is what lets the device find a merged position
// by binary search.  A read without the bit followed at the same time by a read with it contradicts
// itself (the first ran after the deliveries at t, the second before them) and is refused.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SRG_SIN_HD __host__ __device__
#else
#define SRG_SIN_HD
#endif

namespace srg {

constexpr uint8_t SIN_UDP = 0, SIN_EXTERNAL = 1;
constexpr uint8_t SIN_SKIPPED = 0, SIN_NO_SOCKET = 1, SIN_RCV_EXTERNAL = 2, SIN_PEER_MISMATCH = 3, SIN_FULL = 4,
                  SIN_BUFFERED = 5;
constexpr uint8_t SIN_READ_PEEK = 1, SIN_READ_FIRST = 2;
constexpr uint32_t SIN_NO_SLOT = 0xFFFFFFFFu;
constexpr uint64_t SIN_DEFAULT_LIMIT = 174760;  // CONFIG_RECV_BUFFER_SIZE, definitions.h:82

// one socket slot (32 bytes; one record per slot, in HBM on the device)
struct SinSocket {
    uint64_t limit, len, count;  // soft_limit_bytes, len_bytes, messages in the buffer
    uint32_t peer_ip;
    uint16_t peer_port;
    uint8_t kind, has_peer;
};

// tracker.c:188-219, the remote-in counters of a host
struct SinCounters {
    uint64_t packets_control, packets_data, bytes_control_header, bytes_data_header, bytes_data_payload;
};

// ---- the association table: open addressing, linear probing, 32-byte entries ----
// b carries bit 40 on every stored key, so an empty entry is b == 0.
struct SinEntry {
    uint64_t a, b;
    uint32_t slot, pad0;
    uint64_t pad1;
};

SRG_SIN_HD inline uint64_t sin_key_a(uint32_t host, uint32_t peer_ip) { return ((uint64_t)host << 32) | peer_ip; }
SRG_SIN_HD inline uint64_t sin_key_b(uint8_t protocol, uint16_t local_port, uint16_t peer_port) {
    return (1ull << 40) | ((uint64_t)protocol << 32) | ((uint64_t)local_port << 16) | peer_port;
}

// any mixing hash will do: lookups are exact-match (the finaliser of splitmix64 over both words)
SRG_SIN_HD inline uint64_t sin_hash(uint64_t a, uint64_t b) {
    uint64_t x = a * 0x9E3779B97F4A7C15ull + b;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// capacity for n keys: a power of two >= 2 n (load factor <= 1/2), at least 4 (one 128-byte line)
SRG_SIN_HD inline uint64_t sin_table_capacity(uint64_t n) {
    uint64_t c = 4;
    while (c < 2 * n) c <<= 1;
    return c;
}

SRG_SIN_HD inline uint32_t sin_table_find(const SinEntry* t, uint64_t mask, uint64_t a, uint64_t b) {
    for (uint64_t i = sin_hash(a, b) & mask;; i = (i + 1) & mask) {  // ends: the table is never full
        const uint64_t eb = t[i].b;
        if (eb == 0) return SIN_NO_SLOT;
        if (eb == b && t[i].a == a) return t[i].slot;
    }
}

// (building only; the key is not in the table)
inline void sin_table_insert(SinEntry* t, uint64_t mask, uint64_t a, uint64_t b, uint32_t slot) {
    uint64_t i = sin_hash(a, b) & mask;
    while (t[i].b != 0) i = (i + 1) & mask;
    t[i].a = a;
    t[i].b = b;
    t[i].slot = slot;
}

// network_interface.c:157-170
SRG_SIN_HD inline uint32_t sin_lookup(const SinEntry* t, uint64_t mask, uint32_t host, uint8_t protocol, uint16_t dst_port,
                                      uint32_t src_ip, uint16_t src_port) {
    const uint32_t s = sin_table_find(t, mask, sin_key_a(host, src_ip), sin_key_b(protocol, dst_port, src_port));
    if (s != SIN_NO_SLOT) return s;
    return sin_table_find(t, mask, sin_key_a(host, 0), sin_key_b(protocol, dst_port, 0));
}

// tracker.c:188-219 without the retransmit classes
SRG_SIN_HD inline void sin_count(SinCounters& c, uint32_t total, uint32_t payload) {
    if (payload > 0) {
        c.packets_data += 1;
        c.bytes_data_header += total - payload;
        c.bytes_data_payload += payload;
    } else {
        c.packets_control += 1;
        c.bytes_control_header += total;
    }
}

// What a found socket says before its buffer is looked at: SIN_RCV_EXTERNAL, SIN_PEER_MISMATCH
// (udp.rs:116-135), or SIN_BUFFERED for "goes on to the buffer".
SRG_SIN_HD inline uint8_t sin_filter(const SinSocket& s, uint32_t src_ip, uint16_t src_port) {
    if (s.kind == SIN_EXTERNAL) return SIN_RCV_EXTERNAL;
    if (s.has_peer && (s.peer_ip != src_ip || s.peer_port != src_port)) return SIN_PEER_MISMATCH;
    return SIN_BUFFERED;
}

// udp.rs:140, 1139: has_space with `before` payload bytes of this run already accepted
SRG_SIN_HD inline bool sin_has_space(uint64_t len, uint64_t before, uint64_t limit) { return len + before < limit; }

// udp.rs:140-165, 1103-1116: one message offered to the buffer
SRG_SIN_HD inline uint8_t sin_push(SinSocket& s, uint32_t payload) {
    if (!sin_has_space(s.len, 0, s.limit)) return SIN_FULL;
    s.len += payload;
    s.count += 1;
    return SIN_BUFFERED;
}

// udp.rs:497-546, 1120-1130: one recvmsg; true = a message (the front one); `payload` is the front
// message's, subtracted unless peeking
SRG_SIN_HD inline bool sin_read(SinSocket& s, uint8_t flags, uint32_t payload) {
    if (s.count == 0) return false;
    if (!(flags & SIN_READ_PEEK)) {
        s.len -= payload;
        s.count -= 1;
    }
    return true;
}

// the merge: does a read at (t_read, flags) run before a delivery at t_delivery?
SRG_SIN_HD inline bool sin_read_before(uint64_t t_read, uint8_t flags, uint64_t t_delivery) {
    return t_read < t_delivery || (t_read == t_delivery && (flags & SIN_READ_FIRST));
}

// a host's read j after read j - 1: SIN_READ_FIRST behind a read without it at the same time
SRG_SIN_HD inline bool sin_reads_contradict(uint64_t t_prev, uint8_t f_prev, uint64_t t, uint8_t f) {
    return t == t_prev && (f & SIN_READ_FIRST) && !(f_prev & SIN_READ_FIRST);
}

}  // namespace srg
