// CPU check of the host worker pool (shadow_amd/csrc/host_pool.h): every run() calls the job once
// per worker with the pool's size, callers on several threads never mix their runs, and a pool
// joins whether or not it ever ran.  Built plain and with -fsanitize=thread
// (tests/test_host_pool_cpu.py).
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../shadow_amd/csrc/host_pool.h"

static std::atomic<int> g_fail{0};

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (g_fail++ < 10) {              \
                std::fprintf(stderr, __VA_ARGS__); \
                std::fprintf(stderr, "\n");   \
            }                                 \
        }                                     \
    } while (0)

// `runs` back-to-back run() calls on a pool of n; each job marks (w, nw) in this caller's array
static void back_to_back(HostPool& p, int n, int runs, const char* who) {
    std::vector<int> calls(n), nws(n);
    std::atomic<int> out_of_range{0};
    for (int r = 0; r < runs; ++r) {
        for (int w = 0; w < n; ++w) calls[w] = 0, nws[w] = -1;
        p.run([&](int w, int nw) {
            if (w < 0 || w >= n) {
                ++out_of_range;
                return;
            }
            ++calls[w];  // (worker w alone writes slot w; run() returning orders the reads below)
            nws[w] = nw;
        });
        for (int w = 0; w < n; ++w) {
            CHECK(calls[w] == 1, "%s: n=%d run %d: worker %d called %d times", who, n, r, w, calls[w]);
            CHECK(nws[w] == n, "%s: n=%d run %d: worker %d saw nw=%d", who, n, r, w, nws[w]);
        }
    }
    CHECK(out_of_range == 0, "%s: n=%d: %d calls with w outside [0, n)", who, n, out_of_range.load());
}

int main() {
    for (int n : {1, 2, 8}) {
        HostPool p;
        p.start(n);
        CHECK(p.size() == n, "size() = %d after start(%d)", p.size(), n);
        back_to_back(p, n, 2000, "single caller");
    }
    {  // two callers on one pool (the codec beside the late-loss or key-widen thread): run_mu
        HostPool p;
        p.start(8);
        std::thread a([&] { back_to_back(p, 8, 500, "caller a"); });
        std::thread b([&] { back_to_back(p, 8, 500, "caller b"); });
        a.join();
        b.join();
    }
    {  // never ran
        HostPool p;
        p.start(8);
    }
    {  // destroyed right after a run
        HostPool p;
        p.start(8);
        std::atomic<int> c{0};
        p.run([&](int, int) { ++c; });
        CHECK(c == 8, "last run: %d calls of 8", c.load());
    }
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail.load());
        return 1;
    }
    std::printf("ok host_pool\n");
    return 0;
}
