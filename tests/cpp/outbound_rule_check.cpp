// CPU check of shadow_amd/csrc/outbound_rule.h (the rule the outbound step's kernels run).
//   outbound_rule_check FILE   "H qdisc sim_start bootstrap_end", H lines "bw_up_bits sockets", then per
//                              step "step until n" and n lines "host time slot priority size flags tag"
//                              (grouped by host); prints every leaving packet (L), the step's result
//                              (R) or its error (E), and every host's state (S) and qdisc array (O), in
//                              the format of test_outbound_cpu.py
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <deque>
#include <vector>

#include "../../shadow_amd/csrc/outbound_rule.h"

using namespace srg;

struct Offer {
    uint64_t t;
    uint32_t slot;
    uint64_t prio;
    uint32_t size;
    uint8_t flags;
    uint64_t tag;
};
struct Left {
    uint32_t status;
    uint64_t time, tag;
};
struct Sock {
    std::deque<Offer> control, data;
    bool has() const { return !control.empty() || !data.empty(); }
};

// outbound_rule.h's queue over one host's sockets and offers
struct CpuQ {
    std::vector<uint32_t>& ord;
    std::vector<Sock>& socks;
    const std::vector<Offer>& offers;
    size_t next = 0;
    Offer last{}, cached{};
    bool cached_here = false;
    uint64_t old_tag = 0;
    std::vector<Left> out;
    CpuQ(std::vector<uint32_t>& o, std::vector<Sock>& s, const std::vector<Offer>& a) : ord(o), socks(s), offers(a) {}
    uint32_t ord_get(uint32_t i) const { return ord.at(i); }
    void ord_set(uint32_t i, uint32_t slot) { ord.at(i) = slot; }
    uint64_t nprio(uint32_t slot) const {
        const Sock& s = socks.at(slot);
        return !s.control.empty() ? s.control.front().prio : s.data.at(0).prio;
    }
    bool has_offer() const { return next < offers.size(); }
    uint64_t offer_time() const { return offers[next].t; }
    uint8_t offer_flags() const { return offers[next].flags; }
    bool push_offer(uint32_t& slot) {
        const Offer& o = offers[next++];
        slot = o.slot;
        Sock& s = socks.at(slot);
        const bool was_empty = !s.has();
        (o.prio == 0 ? s.control : s.data).push_back(o);
        return was_empty;
    }
    bool pull(uint32_t slot, uint32_t& size, uint8_t& flags) {
        Sock& s = socks.at(slot);
        std::deque<Offer>& f = !s.control.empty() ? s.control : s.data;
        last = f.at(0);
        f.pop_front();
        size = last.size;
        flags = last.flags;
        return s.has();
    }
    void leave(uint8_t status, uint64_t now) { out.push_back(Left{status, now, last.tag}); }
    void cache_last() {
        cached = last;
        cached_here = true;
    }
    void leave_cached(uint64_t now) {
        out.push_back(Left{1, now, cached_here ? cached.tag : old_tag});
        cached_here = false;
    }
};

struct HostRec {
    OutHost s;
    uint64_t inc;
    std::vector<uint32_t> ord;
    std::vector<Sock> socks;
};

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: outbound_rule_check FILE\n");
        return 64;
    }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    size_t H;
    int qdisc;
    uint64_t sim_start, bootstrap_end;
    if (std::fscanf(f, "%zu %d %" SCNu64 " %" SCNu64, &H, &qdisc, &sim_start, &bootstrap_end) != 4) return 3;
    std::vector<HostRec> hosts(H);
    for (auto& r : hosts) {
        uint64_t bw;
        uint32_t ns;
        if (std::fscanf(f, "%" SCNu64 " %" SCNu32, &bw, &ns) != 2) return 3;
        r.inc = inb_refill_increment(bw);
        out_host_init(r.s, r.inc, sim_start);
        r.ord.assign(ns, 0);
        r.socks.resize(ns);
    }
    char word[16];
    uint64_t until;
    size_t n;
    while (std::fscanf(f, "%15s %" SCNu64 " %zu", word, &until, &n) == 3 && !std::strcmp(word, "step")) {
        std::vector<std::vector<Offer>> arr(H);
        int err = until > INB_TIME_END ? 1 : 0;
        for (size_t i = 0; i < n; ++i) {
            size_t h;
            Offer o;
            unsigned fl;
            if (std::fscanf(f, "%zu %" SCNu64 " %" SCNu32 " %" SCNu64 " %" SCNu32 " %u %" SCNu64, &h, &o.t, &o.slot, &o.prio,
                            &o.size, &fl, &o.tag) != 7 ||
                h >= H)
                return 3;
            if (fl & ~3u) err = 1;
            o.flags = (uint8_t)fl;
            arr[h].push_back(o);
        }
        for (size_t h = 0; h < H && err != 1; ++h) {
            uint64_t prev = hosts[h].s.last_time;
            for (const Offer& o : arr[h]) {
                if (o.t < sim_start || o.t >= INB_TIME_END || o.t >= until) err = 1;
                else if (o.slot >= hosts[h].socks.size()) err = 1;
                else if (hosts[h].inc && !(o.flags & OUT_OFFER_LOCAL) && o.size > hosts[h].inc + INB_MTU) err = 1;
                else if (o.t < prev && !err) err = 12;
                prev = o.t;
            }
        }
        if (err) {
            std::printf("E %d\n", err);
        } else {
            uint64_t sent = 0, local = 0, queued = 0, min_wake = UINT64_MAX;
            for (size_t h = 0; h < H; ++h) {
                HostRec& r = hosts[h];
                CpuQ q(r.ord, r.socks, arr[h]);
                q.old_tag = r.s.cached_tag;
                out_host_step(r.s, r.inc, q, qdisc, (uint32_t)r.socks.size(), until, bootstrap_end);
                if (r.s.has_cached && q.cached_here) r.s.cached_tag = q.cached.tag;
                for (const Left& l : q.out) {
                    std::printf("L %zu %u %" PRIu64 " %" PRIu64 "\n", h, l.status, l.time, l.tag);
                    if (l.status == 1) ++sent;
                    else ++local;
                }
                queued += r.s.queued + r.s.has_cached;
                if (r.s.pending && r.s.wake < min_wake) min_wake = r.s.wake;
            }
            std::printf("R %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", sent, local, queued, min_wake);
        }
        for (size_t h = 0; h < H; ++h) {
            const HostRec& r = hosts[h];
            const OutHost& s = r.s;
            size_t in_socks = 0;
            for (const Sock& k : r.socks) in_socks += k.control.size() + k.data.size();
            if (in_socks != s.queued) return 4;
            std::printf("S %zu %" PRIu64 " %" PRIu64 " %u %" PRIu64 " %u %" PRIu64 " %u %u\n", h, s.balance, s.last_refill,
                        (unsigned)s.pending, s.pending ? s.wake : 0, (unsigned)s.has_cached, s.has_cached ? s.cached_tag : 0,
                        s.queued, s.qlen);
            std::printf("O %zu", h);
            for (uint32_t i = 0; i < s.qlen; ++i) {
                uint32_t p = i;
                if (qdisc == OUT_QDISC_ROUND_ROBIN) {
                    p = s.rr_head + i;
                    if (p >= r.socks.size()) p -= (uint32_t)r.socks.size();
                }
                std::printf(" %u", r.ord.at(p));
            }
            std::printf("\n");
        }
    }
    std::fclose(f);
    return 0;
}
