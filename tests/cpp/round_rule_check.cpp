// round_rule_check.cpp -- shadow_amd/csrc/round_rule.h on the CPU (g++, -Werror, -ffp-contract=off,
// ASan + UBSan): replays a script and prints one line per result; tests/test_round_cpu.py compares
// the lines with tests/round_ref.py's.  Script lines:
//   state s0 s1 s2 s3 n     -> n lines "U <next_u64>"
//   seed x                  -> "W s0 s1 s2 s3" of seed_from_u64(x)
//   chance x n              -> n lines "C <bits of gen::<f64>()>" from seed_from_u64(x)
//   host x next_event_id have_loss bootstrap_end sim_end n, then n lines
//        "out_status leave_ns dst_host loss_bits payload"
//                           -> n lines "P status chance_bits event_id" (chance_bits 0 and event_id -1
//                              where none), then "G s0 s1 s2 s3 next_event_id"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../shadow_amd/csrc/round_rule.h"

using namespace srg;

static uint64_t bits_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::string op;
        if (!(is >> op)) continue;
        if (op == "state") {
            RoundRng g;
            uint64_t n;
            is >> g.s[0] >> g.s[1] >> g.s[2] >> g.s[3] >> n;
            for (uint64_t i = 0; i < n; ++i) std::printf("U %" PRIu64 "\n", round_next_u64(g));
        } else if (op == "seed") {
            uint64_t x;
            is >> x;
            RoundRng g;
            round_seed_from_u64(g, x);
            std::printf("W %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", g.s[0], g.s[1], g.s[2], g.s[3]);
        } else if (op == "chance") {
            uint64_t x, n;
            is >> x >> n;
            RoundRng g;
            round_seed_from_u64(g, x);
            for (uint64_t i = 0; i < n; ++i) std::printf("C %" PRIu64 "\n", bits_of(round_chance(round_next_u64(g))));
        } else if (op == "host") {
            uint64_t x, eid, boot, sim_end, n;
            int have_loss;
            is >> x >> eid >> have_loss >> boot >> sim_end >> n;
            RoundRng g;
            round_seed_from_u64(g, x);
            for (uint64_t i = 0; i < n; ++i) {
                if (!std::getline(f, line)) return 3;
                std::istringstream ps(line);
                unsigned st;
                uint64_t t;
                uint32_t dst, loss_bits, payload;
                ps >> st >> t >> dst >> loss_bits >> payload;
                float loss;
                std::memcpy(&loss, &loss_bits, 4);
                uint8_t c = round_classify((uint8_t)st, t, dst, sim_end);
                if (c != ROUND_SENT) {
                    std::printf("P %u 0 -1\n", (unsigned)c);
                    continue;
                }
                double chance;
                uint64_t id;
                c = round_draw_one(g, eid, have_loss != 0, loss, payload, t, boot, &chance, &id);
                if (c == ROUND_SENT) std::printf("P 1 %" PRIu64 " %" PRIu64 "\n", bits_of(chance), id);
                else std::printf("P 0 %" PRIu64 " -1\n", bits_of(chance));
            }
            std::printf("G %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", g.s[0], g.s[1], g.s[2], g.s[3],
                        eid);
        } else {
            return 4;
        }
    }
    return 0;
}
