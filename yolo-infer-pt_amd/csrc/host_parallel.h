// The thread pool of the host twins: start, run, join all. Plain C++.
#ifndef YH_HOST_PARALLEL_H
#define YH_HOST_PARALLEL_H

#include <algorithm>
#include <thread>
#include <vector>

namespace yh {

// body(t, nt) for t = 0 .. nt - 1 on nt threads, nt = min(threads, items) with threads <= 0 meaning
// every hardware thread; nt <= 1 runs body(0, 1) on the caller's thread.
template <class Body>
void run_joined(int items, int threads, Body body) {
    int nt = threads > 0 ? threads : (int)std::max(1u, std::thread::hardware_concurrency());
    nt = std::min(nt, items);
    if (nt <= 1) {
        body(0, 1);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t) pool.emplace_back(body, t, nt);
    for (auto& th : pool) th.join();
}

// run(i) for every i in [0, n); thread t takes i = t, t + nt, ...
template <class Run>
void parallel_strided(int n, int threads, Run run) {
    run_joined(n, threads, [&](int t, int nt) {
        for (int i = t; i < n; i += nt) run(i);
    });
}

// run(lo, hi) once per thread: [0, n) cut into nt contiguous blocks
template <class Run>
void parallel_blocks(int n, int threads, Run run) {
    run_joined(n, threads, [&](int t, int nt) {
        run((int)((long long)n * t / nt), (int)((long long)n * (t + 1) / nt));
    });
}

}  // namespace yh

#endif
