// CPU check of shadow_amd/csrc/send_rule.h (the same header k_ev_prep<true> includes): the drop
// predicate of Worker::send_packet (worker.rs:374-390, 563-568) and the latency fetch from either
// table form, on hand-written cases.  Prints "ok" and exits 0, or names the first failing case.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../shadow_amd/csrc/send_rule.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
            ++failures;                                                 \
        }                                                               \
    } while (0)

int main() {
    using srg::dropped;
    const uint64_t boot = 1000, later = 5000;
    const double below_one = std::nextafter(1.0, 0.0);

    // drop boundary at loss 0.25: reliability 0.75 exactly; chance >= reliability drops
    CHECK(dropped(0.25f, 0.75, 100, later, boot));
    CHECK(!dropped(0.25f, std::nextafter(0.75, 0.0), 100, later, boot));
    CHECK(dropped(0.25f, std::nextafter(0.75, 1.0), 100, later, boot));

    // loss 0: reliability 1.0, chance is in [0, 1) -> never dropped
    CHECK(!dropped(0.0f, 0.0, 1, later, boot));
    CHECK(!dropped(0.0f, 0.5, 1, later, boot));
    CHECK(!dropped(0.0f, below_one, 1, later, boot));

    // loss 1: reliability 0.0, every chance >= 0 -> always dropped when there is a payload
    CHECK(dropped(1.0f, 0.0, 1, later, boot));
    CHECK(dropped(1.0f, 0.5, 1460, later, boot));
    CHECK(dropped(1.0f, below_one, 1, later, boot));

    // payload 0 (a bare ACK): never dropped
    CHECK(!dropped(1.0f, 0.0, 0, later, boot));
    CHECK(!dropped(0.25f, 0.99, 0, later, boot));

    // bootstrapping: send < bootstrap_end never drops, send == bootstrap_end is eligible
    CHECK(!dropped(1.0f, 0.5, 1, boot - 1, boot));
    CHECK(dropped(1.0f, 0.5, 1, boot, boot));
    CHECK(!dropped(1.0f, 0.5, 1, 0, boot));
    CHECK(dropped(1.0f, 0.5, 1, 0, 0));
    CHECK(!dropped(1.0f, 0.5, 1, UINT64_MAX - 1, UINT64_MAX));

    // f32 first, then widened: 1.0f - 1e-8f rounds to 1.0f (half an ulp of 1 is 2^-25 ~ 2.98e-8), so
    // the packet is never dropped; computed in f64 the reliability would be 0.99999999 and the
    // chance below_one would drop it
    CHECK(1.0 - (double)1e-8f < below_one);
    CHECK(!dropped(1e-8f, below_one, 1, later, boot));
    // and a loss whose f32 reliability is not the f64 one: 0.1f
    const double rel_f32 = (double)(1.0f - 0.1f);
    CHECK(rel_f32 != 1.0 - (double)0.1f);
    CHECK(dropped(0.1f, rel_f32, 1, later, boot));
    CHECK(!dropped(0.1f, std::nextafter(rel_f32, 0.0), 1, later, boot));

    // latency fetch: u64 table
    const uint64_t lat[9] = {11, 12, 13, 21, 22, 23, 31, 32, 33};
    const srg::PathLatency wide{lat, nullptr, nullptr, 1, 3};
    CHECK(srg::path_latency(wide, 0, 0) == 11);
    CHECK(srg::path_latency(wide, 1, 2) == 23);
    CHECK(srg::path_latency(wide, 2, 1) == 32);
    // key table: off-diagonal = key * unit, diagonal = diag (the key there is not used)
    const uint32_t key[9] = {7, 2, 3, 4, 7, 0xFFFFFFFFu, 5, 6, 7};
    const uint64_t diag[3] = {1, 999999, 123456789012345ull};
    const srg::PathLatency keys{nullptr, key, diag, 1000, 3};
    CHECK(srg::path_latency(keys, 0, 1) == 2000);
    CHECK(srg::path_latency(keys, 2, 0) == 5000);
    CHECK(srg::path_latency(keys, 1, 2) == 0xFFFFFFFFull * 1000);  // widened before the multiply
    CHECK(srg::path_latency(keys, 0, 0) == 1);
    CHECK(srg::path_latency(keys, 1, 1) == 999999);
    CHECK(srg::path_latency(keys, 2, 2) == 123456789012345ull);

    if (failures) return 1;
    std::puts("ok");
    return 0;
}
