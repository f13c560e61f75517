// phi_host_par.h -- host threads over fixed chunks of work, and the first error any of them raises.  No HIP include:
// phi_ctx.h includes it for the library, dp_steps.h for the stand-alone check of the DP step stream.
#pragma once
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// ---- host threads for the O(walk entries) preparation of phi_set_graph
static inline int phi_host_threads()
{
    const char *e = getenv("PHI_HOST_THREADS");
    int n = e ? atoi(e) : (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    return n > 16 ? 16 : n;
}

// fn(lo, hi, worker) over [0, n) in chunks handed out dynamically; worker < phi_host_threads()
template <class F> static void phi_parallel_chunks(int64_t n, int64_t chunk, F fn)
{
    const int64_t n_chunks = (n + chunk - 1) / chunk;
    int nt = phi_host_threads();
    if (nt > n_chunks) nt = (int)n_chunks;
    if (nt <= 1) {
        for (int64_t i = 0; i < n_chunks; i++) fn(i * chunk, std::min(n, (i + 1) * chunk), 0);
        return;
    }
    std::atomic<int64_t> next{0};
    auto work = [&](int worker) {
        for (;;) {
            const int64_t i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= n_chunks) break;
            fn(i * chunk, std::min(n, (i + 1) * chunk), worker);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
}

// first error raised by any worker
struct PhiHostError {
    std::atomic<int> flag{0};
    std::mutex m;
    int code = 0;
    std::string msg;
    bool failed() const { return flag.load(std::memory_order_relaxed) != 0; }
    void set(int code_, const char *fmt, ...)
    {
        std::lock_guard<std::mutex> g(m);
        if (flag.load()) return;
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        code = code_; msg = buf;
        flag.store(1);
    }
};
