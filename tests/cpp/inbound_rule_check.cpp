// CPU check of shadow_amd/csrc/inbound_rule.h (the rule the inbound step's kernels run).
//   inbound_rule_check kat FILE        replays operation lists (tests/golden/inbound_kats.json, flattened
//                                      by the test: "op a b c d" per line, op = index in
//                                      inbound_ref.KAT_OPS) and prints one record per operation
//   inbound_rule_check scenario FILE   "H sim_start bootstrap_end", H bandwidths, then per step
//                                      "step until n" and n lines "host time size tag" (grouped by
//                                      host); prints every leaving packet, the step's result and
//                                      every host's state, in the format of test_inbound_cpu.py
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../shadow_amd/csrc/inbound_rule.h"

using namespace srg;

struct Elem {
    uint64_t t;
    uint32_t size;
    uint64_t tag;
};
struct Left {
    uint32_t status;
    uint64_t time, tag;
};

// inbound_rule.h's queue over a host's sequence (backlog, then arrivals)
struct CpuQ {
    std::vector<Elem> seq;
    size_t head = 0, enq = 0;
    bool old_cached = false;
    uint64_t old_tag = 0;
    std::vector<Left> out;
    bool pop_front(uint64_t& ts, uint32_t& size) {
        if (head == enq) return false;
        ts = seq[head].t;
        size = seq[head].size;
        ++head;
        return true;
    }
    void leave(uint8_t status, uint64_t now) { out.push_back(Left{status, now, seq[head - 1].tag}); }
    void leave_cached(uint8_t status, uint64_t now) {
        if (!old_cached) return leave(status, now);
        old_cached = false;
        out.push_back(Left{status, now, old_tag});
    }
    bool has_arrival() const { return enq < seq.size(); }
    uint64_t next_arrival_time() const { return seq[enq].t; }
    void enqueue_upto(uint64_t limit, InbHost& s) {
        while (enq < seq.size() && seq[enq].t <= limit) {
            s.bytes += seq[enq].size;
            if (seq[enq].t > s.last_time) s.last_time = seq[enq].t;
            ++enq;
        }
    }
};

static int run_kat(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) return 2;
    InbHost s{};
    CpuQ q;
    uint64_t cap = 0, inc = 0, interval = 0, balance = 0, last_refill = 0;
    bool is_cq = false;
    unsigned op;
    uint64_t a, b, c, d;
    while (std::fscanf(f, "%u %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &op, &a, &b, &c, &d) == 5) {
        uint64_t ret = 0, value = 0, now = 0;
        switch (op) {
            case 0:  // tb_new capacity increment interval last_refill
                cap = balance = a, inc = b, interval = c, last_refill = d, is_cq = false;
                break;
            case 1: {  // tb_remove decrement now
                uint64_t dur = 0;
                if (inb_conforming_remove(cap, inc, interval, balance, last_refill, a, b, &dur)) ret = 1, value = balance;
                else value = dur;
                break;
            }
            case 2:  // cq_new
                s = InbHost{};
                q = CpuQ{};
                is_cq = true;
                break;
            case 3:  // cq_push count now (size c)
                now = b;
                for (uint64_t i = 0; i < a; ++i) {
                    q.seq.push_back(Elem{b, (uint32_t)c, 0});
                    q.enqueue_upto(UINT64_MAX, s);
                }
                break;
            case 4: {  // cq_pop now
                uint32_t size;
                now = a;
                ret = inb_codel_pop(s, q, now, size) ? 1 : 0;
                break;
            }
            case 5:  // cq_psd now delay
                now = a;
                ret = inb_process_standing_delay(s, now, b) ? 1 : 0;
                break;
            case 6:  // cq_set_mode
                s.mode = (uint8_t)a;
                break;
            case 7:  // law time count
                value = inb_control_law(a, b) - a;
                break;
            case 8:  // cq_probe now
                now = a;
                break;
            default:
                return 3;
        }
        if (is_cq)
            std::printf("%" PRIu64 " %" PRIu64 " %zu %u %" PRIu64 " %" PRIu64 " %u %" PRIu64 " %u %" PRIu64 " %d %d\n", ret,
                        value, q.enq - q.head, (unsigned)s.mode, s.cur_drops, s.prev_drops, (unsigned)s.has_interval_end,
                        s.interval_end, (unsigned)s.has_drop_next, s.bytes, (int)inb_was_dropping_recently(s, now),
                        (int)inb_should_drop(s, now));
        else
            std::printf("%" PRIu64 " %" PRIu64 " 0 0 0 0 0 0 0 %" PRIu64 " 0 0\n", ret, value, balance);
    }
    std::fclose(f);
    return 0;
}

struct HostRec {
    InbHost s;
    uint64_t inc;
    std::vector<Elem> backlog;
};

static void print_state(size_t h, const HostRec& r) {
    const InbHost& s = r.s;
    std::printf("S %zu %" PRIu64 " %" PRIu64 " %u %u %" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
                " %zu %u %" PRIu64 " %u %" PRIu64 "\n",
                h, s.balance, s.last_refill, (unsigned)s.mode, (unsigned)s.has_interval_end, s.interval_end,
                (unsigned)s.has_drop_next, s.drop_next, s.cur_drops, s.prev_drops, s.bytes, r.backlog.size(),
                (unsigned)s.pending, s.pending ? s.wake : 0, (unsigned)s.has_cached, s.has_cached ? s.cached_tag : 0);
}

static int run_scenario(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) return 2;
    size_t H;
    uint64_t sim_start, bootstrap_end;
    if (std::fscanf(f, "%zu %" SCNu64 " %" SCNu64, &H, &sim_start, &bootstrap_end) != 3) return 3;
    std::vector<HostRec> hosts(H);
    for (auto& r : hosts) {
        uint64_t bw;
        if (std::fscanf(f, "%" SCNu64, &bw) != 1) return 3;
        r.inc = inb_refill_increment(bw);
        inb_host_init(r.s, r.inc, sim_start);
    }
    char word[16];
    uint64_t until;
    size_t n;
    while (std::fscanf(f, "%15s %" SCNu64 " %zu", word, &until, &n) == 3 && !std::strcmp(word, "step")) {
        std::vector<std::vector<Elem>> arr(H);
        int err = until > INB_TIME_END ? 1 : 0;
        for (size_t i = 0; i < n; ++i) {
            size_t h;
            Elem e;
            if (std::fscanf(f, "%zu %" SCNu64 " %" SCNu32 " %" SCNu64, &h, &e.t, &e.size, &e.tag) != 4 || h >= H) return 3;
            arr[h].push_back(e);
        }
        for (size_t h = 0; h < H && err != 1; ++h) {
            uint64_t prev = hosts[h].s.last_time;
            for (const Elem& e : arr[h]) {
                if (e.t < sim_start || e.t >= INB_TIME_END || e.t >= until) err = 1;
                else if (hosts[h].inc && e.size > hosts[h].inc + INB_MTU) err = 1;
                else if (e.t < prev && !err) err = 12;
                prev = e.t;
            }
        }
        if (err) {
            std::printf("E %d\n", err);
        } else {
            uint64_t fwd = 0, drop = 0, queued = 0, min_wake = UINT64_MAX;
            for (size_t h = 0; h < H; ++h) {
                HostRec& r = hosts[h];
                CpuQ q;
                q.seq = r.backlog;
                q.enq = q.seq.size();
                q.seq.insert(q.seq.end(), arr[h].begin(), arr[h].end());
                q.old_cached = r.s.has_cached != 0;
                q.old_tag = r.s.cached_tag;
                inb_host_step(r.s, r.inc, q, until, bootstrap_end);
                if (r.s.has_cached && !q.old_cached) r.s.cached_tag = q.seq[q.head - 1].tag;
                r.backlog.assign(q.seq.begin() + q.head, q.seq.end());
                for (const Left& l : q.out) {
                    std::printf("L %zu %u %" PRIu64 " %" PRIu64 "\n", h, l.status, l.time, l.tag);
                    if (l.status) ++fwd;
                    else ++drop;
                }
                queued += r.backlog.size() + r.s.has_cached;
                if (r.s.pending && r.s.wake < min_wake) min_wake = r.s.wake;
            }
            std::printf("R %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", fwd, drop, queued, min_wake);
        }
        for (size_t h = 0; h < H; ++h) print_state(h, hosts[h]);
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "kat")) return run_kat(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "scenario")) return run_scenario(argv[2]);
    std::fprintf(stderr, "usage: inbound_rule_check kat|scenario FILE\n");
    return 64;
}
