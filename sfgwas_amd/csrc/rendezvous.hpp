// rendezvous.hpp — the host-side meeting point of the rank threads of one process (mgpu.hip: the agreement point of every exchanging call and the direct transport).
// Plain standard C++, no HIP: tests/host/rendezvous_test.cpp compiles this header with g++ alone and drives it from plain threads.
#pragma once
#include <atomic>
#include <condition_variable>
#include <mutex>

struct Rendezvous {
    std::mutex m; std::condition_variable cv; int n = 1, count = 0; unsigned long gen = 0; std::atomic<bool> failed{false};
    const void *ptr[64] = {};
    bool barrier() {       // false: a peer has failed (nobody will arrive)
        std::unique_lock<std::mutex> lk(m);
        if (failed.load()) return false;
        const unsigned long g = gen;
        if (++count == n) { count = 0; gen++; cv.notify_all(); return true; }
        cv.wait(lk, [&] { return gen != g || failed.load(); });
        return gen != g;
    }
    void fail() { std::unique_lock<std::mutex> lk(m); failed.store(true); cv.notify_all(); }
    // Before a call's rank threads start (none is inside barrier()): a round that fail() cut short leaves the arrivals of its released waiters in `count`, and the
    // next call's first barrier would release its ranks before all of them have arrived.  A fresh generation, no arrivals, no failure.
    void reset() { std::lock_guard<std::mutex> lk(m); count = 0; gen++; failed.store(false); }
};
