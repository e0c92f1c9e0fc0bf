// CPU check of shadow_amd/csrc/sockets_in_rule.h (the rule the sockets-in step's kernels run).
//   sockets_in_rule_check FILE    replays a scenario (tests/sockets_in_scenarios.py or a KAT of
//                                 tests/golden/sockets_in_kats.json, flattened by the test) one
//                                 operation at a time through the header's functions -- the table
//                                 rebuilt with sin_table_insert on a change and probed with sin_lookup,
//                                 sin_count, sin_filter, sin_push, sin_read, the merge by sin_read_before
//                                 -- and prints every output row, the result, and after every
//                                 operation every socket's state and every host's counters, in the
//                                 format of test_sockets_in_cpu.py
// Input: "H", H socket counts, "P" (-1: no packet table), P lines "protocol src_ip src_port dst_port
// total payload", then operations:
//   configure n     n lines "host slot kind has_peer peer_ip peer_port limit"
//   associate n     n lines "host protocol local_port peer_ip peer_port slot"
//   disassociate n  n lines "host protocol local_port peer_ip peer_port"
//   step n has_status deliver_status nr    n lines "status time tag", H + 1 offsets, nr lines
//                                          "time slot flags", H + 1 offsets
//   reset host
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../shadow_amd/csrc/sockets_in_rule.h"

using namespace srg;

struct Msg {
    uint64_t tag, time;
    uint32_t payload;
};
struct Packet {
    uint8_t protocol;
    uint32_t src_ip;
    uint16_t src_port, dst_port;
    uint32_t total, payload;
};

struct World {
    uint32_t H = 0;
    std::vector<uint64_t> sock_off;
    std::vector<SinSocket> socks;
    std::vector<std::vector<Msg>> msgs;  // per socket, front first
    std::vector<SinCounters> counters;
    bool have_packets = false;
    std::vector<Packet> packets;
    std::map<std::pair<uint64_t, uint64_t>, uint32_t> assoc;
    std::vector<SinEntry> table;
    void rebuild() {
        table.assign(sin_table_capacity(assoc.size()), SinEntry{0, 0, 0, 0, 0});
        for (const auto& kv : assoc)
            sin_table_insert(table.data(), table.size() - 1, kv.first.first, kv.first.second, kv.second);
    }
    bool slot_ok(uint64_t h, uint64_t slot) const { return h < H && slot < sock_off[h + 1] - sock_off[h]; }
};

static void print_state(const World& w) {
    for (uint32_t h = 0; h < w.H; ++h) {
        for (uint64_t i = w.sock_off[h]; i < w.sock_off[h + 1]; ++i) {
            const SinSocket& s = w.socks[i];
            if (s.count != w.msgs[i].size()) {
                std::fprintf(stderr, "count out of step with the buffer\n");
                std::exit(3);
            }
            std::printf("S %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u %u\n", h, i - w.sock_off[h], s.len,
                        s.count, s.limit, s.peer_ip, (unsigned)s.peer_port, (unsigned)s.kind, (unsigned)s.has_peer);
        }
        const SinCounters& c = w.counters[h];
        std::printf("H %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", h, c.packets_control,
                    c.packets_data, c.bytes_control_header, c.bytes_data_header, c.bytes_data_payload);
    }
}

struct Row {
    unsigned status;
    uint64_t time, tag;
};
struct Read {
    uint64_t time, slot;
    unsigned flags;
};

static bool offsets_ok(const std::vector<uint64_t>& off, uint64_t n) {
    if (off.front() != 0 || off.back() != n) return false;
    for (size_t i = 0; i + 1 < off.size(); ++i)
        if (off[i] > off[i + 1]) return false;
    return true;
}

// -> 0 or the error code (1 SRG_ERR_ARG, 12 SRG_ERR_TIME_BACKWARD); validation first, so an error changes nothing
static int step(World& w, const std::vector<Row>& rows, bool has_status, unsigned deliver_status,
                const std::vector<uint64_t>& off, const std::vector<Read>& reads, const std::vector<uint64_t>& roff) {
    if (!w.have_packets) return 1;
    if (!offsets_ok(off, rows.size()) || !offsets_ok(roff, reads.size())) return 1;
    std::vector<char> deliver(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) {
        deliver[i] = !has_status || rows[i].status == deliver_status;
        if (deliver[i] && rows[i].tag >= w.packets.size()) return 1;
    }
    for (const Read& r : reads)
        if (r.flags & ~(unsigned)(SIN_READ_PEEK | SIN_READ_FIRST)) return 1;
    for (uint32_t h = 0; h < w.H; ++h)
        for (uint64_t j = roff[h]; j < roff[h + 1]; ++j)
            if (!w.slot_ok(h, reads[j].slot) || w.socks[w.sock_off[h] + reads[j].slot].kind == SIN_EXTERNAL) return 1;
    for (uint32_t h = 0; h < w.H; ++h)
        for (uint64_t j = roff[h] + 1; j < roff[h + 1]; ++j)
            if (sin_reads_contradict(reads[j - 1].time, (uint8_t)reads[j - 1].flags, reads[j].time, (uint8_t)reads[j].flags))
                return 1;
    std::vector<std::vector<size_t>> mine(w.H);
    for (uint32_t h = 0; h < w.H; ++h) {
        for (uint64_t i = off[h]; i < off[h + 1]; ++i)
            if (deliver[i]) mine[h].push_back(i);
        for (size_t k = 1; k < mine[h].size(); ++k)
            if (rows[mine[h][k]].time < rows[mine[h][k - 1]].time) return 12;
        for (uint64_t j = roff[h] + 1; j < roff[h + 1]; ++j)
            if (reads[j].time < reads[j - 1].time) return 12;
    }
    uint64_t by_status[6] = {0, 0, 0, 0, 0, 0}, num_read = 0;
    std::vector<unsigned> out_status(rows.size(), SIN_SKIPPED);
    std::vector<uint32_t> out_slot(rows.size(), SIN_NO_SLOT);
    struct Got {
        unsigned status;
        uint64_t tag, time;
        uint32_t payload;
    };
    std::vector<Got> got(reads.size(), Got{0, 0, 0, 0});
    for (uint32_t h = 0; h < w.H; ++h) {
        size_t di = 0;
        uint64_t j = roff[h];
        while (di < mine[h].size() || j < roff[h + 1]) {
            if (j < roff[h + 1] &&
                (di == mine[h].size() || sin_read_before(reads[j].time, (uint8_t)reads[j].flags, rows[mine[h][di]].time))) {
                const uint64_t sidx = w.sock_off[h] + reads[j].slot;
                SinSocket& s = w.socks[sidx];
                const Msg front = s.count ? w.msgs[sidx].front() : Msg{0, 0, 0};
                if (sin_read(s, (uint8_t)reads[j].flags, front.payload)) {
                    got[j] = Got{1, front.tag, front.time, front.payload};
                    if (!(reads[j].flags & SIN_READ_PEEK)) w.msgs[sidx].erase(w.msgs[sidx].begin());
                    ++num_read;
                }
                ++j;
            } else {
                const size_t i = mine[h][di++];
                const Packet& p = w.packets[rows[i].tag];
                const uint32_t slot = sin_lookup(w.table.data(), w.table.size() - 1, h, p.protocol, p.dst_port, p.src_ip, p.src_port);
                out_status[i] = SIN_NO_SOCKET;
                if (slot == SIN_NO_SLOT) continue;
                out_slot[i] = slot;
                sin_count(w.counters[h], p.total, p.payload);
                const uint64_t sidx = w.sock_off[h] + slot;
                uint8_t st = sin_filter(w.socks[sidx], p.src_ip, p.src_port);
                if (st == SIN_BUFFERED) {
                    st = sin_push(w.socks[sidx], p.payload);
                    if (st == SIN_BUFFERED) w.msgs[sidx].push_back(Msg{rows[i].tag, rows[i].time, p.payload});
                }
                out_status[i] = st;
            }
        }
    }
    for (size_t i = 0; i < rows.size(); ++i) {
        ++by_status[out_status[i]];
        std::printf("D %zu %u %u\n", i, out_status[i], out_slot[i]);
    }
    for (size_t j = 0; j < reads.size(); ++j)
        std::printf("R %zu %u %" PRIu64 " %" PRIu64 " %u\n", j, got[j].status, got[j].tag, got[j].time, got[j].payload);
    uint64_t total = 0;
    for (const auto& m : w.msgs) total += m.size();
    std::printf("T %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n",
                by_status[0], by_status[1], by_status[2], by_status[3], by_status[4], by_status[5], num_read,
                (uint64_t)reads.size() - num_read, total);
    return 0;
}

#define NEED(n, ...)                                  \
    if (std::fscanf(f, __VA_ARGS__) != (n)) {         \
        std::fprintf(stderr, "bad input near %s\n", op); \
        return 2;                                     \
    }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    World w;
    char op[32] = "header";
    NEED(1, "%u", &w.H);
    w.sock_off.assign((size_t)w.H + 1, 0);
    for (uint32_t h = 0; h < w.H; ++h) {
        uint64_t n;
        NEED(1, "%" SCNu64, &n);
        w.sock_off[h + 1] = w.sock_off[h] + n;
    }
    SinSocket fresh{};
    fresh.limit = SIN_DEFAULT_LIMIT;
    w.socks.assign(w.sock_off[w.H], fresh);
    w.msgs.resize(w.sock_off[w.H]);
    w.counters.assign(w.H, SinCounters{0, 0, 0, 0, 0});
    w.rebuild();
    long long P;
    NEED(1, "%lld", &P);
    w.have_packets = P >= 0;
    for (long long i = 0; i < P; ++i) {
        unsigned a, c, d;
        uint32_t b, e, g;
        NEED(6, "%u %u %u %u %u %u", &a, &b, &c, &d, &e, &g);
        w.packets.push_back(Packet{(uint8_t)a, b, (uint16_t)c, (uint16_t)d, e, g});
    }
    while (std::fscanf(f, "%31s", op) == 1) {
        int err = 0;
        if (!std::strcmp(op, "configure")) {
            uint64_t n;
            NEED(1, "%" SCNu64, &n);
            std::vector<std::pair<uint64_t, SinSocket>> todo;
            for (uint64_t i = 0; i < n; ++i) {
                uint64_t h, slot, limit;
                unsigned kind, hp, pport;
                uint32_t pip;
                NEED(7, "%" SCNu64 " %" SCNu64 " %u %u %u %u %" SCNu64, &h, &slot, &kind, &hp, &pip, &pport, &limit);
                if (!w.slot_ok(h, slot) || kind > SIN_EXTERNAL || hp > 1) {
                    err = 1;
                    continue;
                }
                SinSocket s{};
                s.limit = limit, s.peer_ip = pip, s.peer_port = (uint16_t)pport, s.kind = (uint8_t)kind, s.has_peer = (uint8_t)hp;
                todo.emplace_back(w.sock_off[h] + slot, s);
            }
            if (!err)
                for (const auto& t : todo) {
                    SinSocket& s = w.socks[t.first];
                    s.limit = t.second.limit, s.peer_ip = t.second.peer_ip, s.peer_port = t.second.peer_port;
                    s.kind = t.second.kind, s.has_peer = t.second.has_peer;
                }
        } else if (!std::strcmp(op, "associate") || !std::strcmp(op, "disassociate")) {
            const bool add = op[0] == 'a';
            uint64_t n;
            NEED(1, "%" SCNu64, &n);
            std::map<std::pair<uint64_t, uint64_t>, uint32_t> batch;
            for (uint64_t i = 0; i < n; ++i) {
                uint64_t h, slot = 0;
                unsigned proto, lport, pport;
                uint32_t pip;
                NEED(5, "%" SCNu64 " %u %u %u %u", &h, &proto, &lport, &pip, &pport);
                if (add) NEED(1, "%" SCNu64, &slot);
                const auto k = std::make_pair(sin_key_a((uint32_t)h, pip), sin_key_b((uint8_t)proto, (uint16_t)lport, (uint16_t)pport));
                if (!add) {
                    w.assoc.erase(k);
                } else if (!w.slot_ok(h, slot) || w.assoc.count(k) || !batch.emplace(k, (uint32_t)slot).second) {
                    err = 1;
                }
            }
            if (add && !err) w.assoc.insert(batch.begin(), batch.end());
            w.rebuild();
        } else if (!std::strcmp(op, "step")) {
            uint64_t n, nr;
            unsigned has_status, ds;
            NEED(4, "%" SCNu64 " %u %u %" SCNu64, &n, &has_status, &ds, &nr);
            std::vector<Row> rows(n);
            std::vector<Read> reads(nr);
            std::vector<uint64_t> off((size_t)w.H + 1), roff((size_t)w.H + 1);
            for (auto& r : rows) NEED(3, "%u %" SCNu64 " %" SCNu64, &r.status, &r.time, &r.tag);
            for (auto& o : off) NEED(1, "%" SCNu64, &o);
            for (auto& r : reads) NEED(3, "%" SCNu64 " %" SCNu64 " %u", &r.time, &r.slot, &r.flags);
            for (auto& o : roff) NEED(1, "%" SCNu64, &o);
            err = step(w, rows, has_status != 0, ds, off, reads, roff);
        } else if (!std::strcmp(op, "reset")) {
            uint32_t h;
            NEED(1, "%u", &h);
            const SinCounters& c = w.counters[h];
            std::printf("C %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", h, c.packets_control,
                        c.packets_data, c.bytes_control_header, c.bytes_data_header, c.bytes_data_payload);
            w.counters[h] = SinCounters{0, 0, 0, 0, 0};
        } else {
            std::fprintf(stderr, "unknown operation %s\n", op);
            return 2;
        }
        if (err) std::printf("E %d\n", err);
        print_state(w);
    }
    std::fclose(f);
    return 0;
}
