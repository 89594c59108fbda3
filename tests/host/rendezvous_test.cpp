// CPU test of the rank threads' meeting point (sfgwas_amd/csrc/rendezvous.hpp; tests/test_rendezvous.py builds it with g++ -pthread and runs it).
// For n = 2, 3 and 8 threads:
//   (a) plain rounds: no thread leaves barrier() before all n have arrived (an arrival counter, read right after barrier() returns, holds all n);
//   (b) k threads wait inside barrier() when another calls fail(): every waiter, the failing thread and the late arrivals return false, none hangs;
//   (c) after (b) and reset() (what the engine does between calls), a full round again releases nobody before all n have arrived;
//   (d) (b) - (c) many times back to back, the failing thread and the number of waiters chosen at random.
// Every round runs under a deadline of its own: a regression prints FAIL and exits instead of hanging.
#include "rendezvous.hpp"
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <future>
#include <random>
#include <thread>
#include <vector>

static const auto DEADLINE = std::chrono::seconds(10);
static int g_fail = 0;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); std::fflush(stdout); g_fail++; } } while (0)

// runs fn(i) on n threads and waits for all of them under the deadline (a thread still blocked after it: the program ends, it cannot be joined)
static void run_threads(int n, const char *what, const std::function<void(int)> &fn) {
    std::vector<std::future<void>> f;
    for (int i = 0; i < n; i++) f.push_back(std::async(std::launch::async, fn, i));
    const auto until = std::chrono::steady_clock::now() + DEADLINE;
    for (int i = 0; i < n; i++)
        if (f[(size_t)i].wait_until(until) != std::future_status::ready) {
            std::printf("FAIL: %s: n = %d, thread %d still inside barrier() after the deadline (hang)\n", what, n, i);
            std::fflush(stdout);
            std::_Exit(1);
        }
}

static int waiting(Rendezvous &rv) { std::lock_guard<std::mutex> lk(rv.m); return rv.count; }

// (a) / (c): `rounds` full rounds of n threads; after each, every thread must see all n arrivals of that round
static void full_rounds(Rendezvous &rv, int n, int rounds, const char *what) {
    std::atomic<int> arrived{0};
    run_threads(n, what, [&](int i) {
        for (int r = 0; r < rounds; r++) {
            arrived.fetch_add(1);
            const bool ok = rv.barrier();
            const int seen = arrived.load();
            CHECK(ok, "%s: n = %d, round %d, thread %d: barrier() returned false without a failure", what, n, r, i);
            CHECK(seen >= n * (r + 1), "%s: n = %d, round %d, thread %d released after %d of %d arrivals", what, n, r, i, seen - n * r, n);
            if (!ok) return;
        }
    });
}

// (b): k of the other threads wait inside barrier(), then `victim` fails; the rest arrive after the failure
static void failed_round(Rendezvous &rv, int n, int victim, int k, const char *what) {
    std::atomic<int> order{0};
    std::vector<int> first(n, 0);
    for (int i = 0, c = 0; i < n && c < k; i++) if (i != victim) { first[(size_t)i] = 1; c++; }
    run_threads(n, what, [&](int i) {
        if (i == victim) {
            while (waiting(rv) < k) std::this_thread::yield();             // the k waiters are inside barrier()
            rv.fail();
            CHECK(!rv.barrier(), "%s: n = %d: the failing thread %d passed barrier()", what, n, i);
            order.store(1);
            return;
        }
        if (!first[(size_t)i]) while (!order.load()) std::this_thread::yield();     // a late arrival: after the failure
        CHECK(!rv.barrier(), "%s: n = %d, victim %d, %d waiting: thread %d passed barrier() although a peer failed", what, n, victim, k, i);
    });
}

int main() {
    std::mt19937 rnd(20261016);
    for (int n : {2, 3, 8}) {
        {
            Rendezvous rv; rv.n = n;
            full_rounds(rv, n, 50, "(a) plain rounds");
        }
        {
            Rendezvous rv; rv.n = n;
            failed_round(rv, n, n - 1, n - 1, "(b) all others waiting");
            rv.reset();
            full_rounds(rv, n, 2, "(c) after a failure with every peer waiting");
            failed_round(rv, n, 0, 1, "(b) one waiting");
            rv.reset();
            full_rounds(rv, n, 2, "(c) after a failure with one peer waiting");
        }
        {
            Rendezvous rv; rv.n = n;
            for (int rep = 0; rep < 200 && !g_fail; rep++) {
                const int victim = (int)(rnd() % (unsigned)n), k = (int)(rnd() % (unsigned)n);      // 0 .. n - 1 peers already waiting
                failed_round(rv, n, victim, k, "(d) random failure");
                rv.reset();
                full_rounds(rv, n, 1 + (int)(rnd() % 2u), "(d) after a random failure");
            }
        }
        if (g_fail) break;
        std::printf("n = %d ok\n", n);
    }
    if (g_fail) { std::printf("FAILED (%d checks)\n", g_fail); return 1; }
    std::printf("OK\n");
    return 0;
}
