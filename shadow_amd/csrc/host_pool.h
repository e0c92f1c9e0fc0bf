// host_pool.h -- the host entry's worker pool (H2D codec, late-loss copies, key widening).
// Plain C++: no HIP include, so tests/cpp/host_pool_check.cpp compiles it alone.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// Host-side worker pool for the host entry's H2D codec: run(f) calls f(w, nw) on nw threads
// (the caller is worker 0) and returns when all are done.
struct HostPool {
    std::vector<std::thread> th;
    std::mutex run_mu;  // one job at a time: job / pending / gen are shared (callers on several threads queue)
    std::mutex mu;
    std::condition_variable cv, done_cv;
    std::function<void(int, int)> job;
    uint64_t gen = 0;
    int pending = 0;
    bool stop = false;
    int size() const { return (int)th.size() + 1; }
    void start(int n) {
        for (int w = 1; w < n; ++w)
            th.emplace_back([this, w] {
                uint64_t seen = 0;
                for (;;) {
                    std::function<void(int, int)> f;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv.wait(lk, [&] { return stop || gen != seen; });
                        if (stop) return;
                        seen = gen;
                        f = job;
                    }
                    f(w, size());
                    std::lock_guard<std::mutex> lk(mu);
                    if (--pending == 0) done_cv.notify_one();
                }
            });
    }
    void run(const std::function<void(int, int)>& f) {
        std::lock_guard<std::mutex> serial(run_mu);
        {
            std::lock_guard<std::mutex> lk(mu);
            job = f;
            pending = (int)th.size();
            ++gen;
        }
        cv.notify_all();
        f(0, size());
        std::unique_lock<std::mutex> lk(mu);
        done_cv.wait(lk, [&] { return pending == 0; });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv.notify_all();
        for (auto& t : th) t.join();
    }
};
