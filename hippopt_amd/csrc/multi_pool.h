// One launching thread per shard of a multi-device handle (hipnlp_multi_set_threads): the pool, and nothing of HIP.
// ONE text: hipnlp.hip runs it with bind = hipSetDevice(the shard's device) and jobs that stage / launch / wait for a shard;
// tests/multi_pool_check/multi_pool_check.cpp runs it on the CPU with a recorder in place of both.
//
// Enqueueing a kernel costs the host 4 - 6 us and waiting for a stream a few more: done by the caller's thread one shard after the
// other, the last of eight shards would start 40 us after the first — longer than the whole callback of one device.  With threads on,
// shard i > 0 has a worker bound to its device: the caller publishes a job (a ticket number), runs shard 0's part itself and waits
// for the others; every worker stages / launches / waits for ITS shard.  A worker polls for the next ticket for `spin_us` after its
// last job (IPOPT's callbacks come in bursts, microseconds apart) and sleeps on a condition variable after that (between bursts
// IPOPT factorises for milliseconds: no core is burnt meanwhile; the first callback of a burst pays one wake-up).
//
// The contract (tests/multi_pool_check):
//   - a worker starts with `seen` = the ticket its spawner read before creating the thread: a ticket issued before a stop() is never
//     taken for a new one by the workers of the next start();
//   - no job outlives run(): the pool holds the callable from the ticket's issue until every shard has returned, and drops it before
//     run() returns, whatever the shards returned — a job may capture its caller's frame by reference;
//   - start() leaves the done count at 0, the return codes at 0 and no job;
//   - the sleep / wake handshake: a worker announces itself (sleepers + 1, seq_cst) and THEN looks at the ticket (seq_cst), holding the
//     mutex from before the announcement until the wait has released it; the caller issues the ticket (seq_cst) and THEN looks at the
//     sleepers (seq_cst), and notifies under the mutex.  In the one order of the four seq_cst operations either the worker's look comes
//     after the issue — it does not sleep — or the caller's look comes after the announcement — it notifies, and the mutex makes the
//     notification wait until the worker does.  (With an acquire load of the ticket both could miss each other.)  While it waits for
//     the shards the caller looks at the sleepers again every few thousand polls and notifies again: a wake-up lost all the same
//     would be a delay, not a caller that never returns.  There is no wall-clock limit on the wait: a job waits for a kernel of
//     unknown length.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

struct MultiPool {
    std::vector<std::thread> workers;     // shard i > 0: workers[i - 1]
    std::function<int(size_t)> job;       // what every shard does for the ticket in flight; rc per shard in job_rc
    std::vector<int> job_rc;
    std::atomic<unsigned long long> ticket{0};
    std::atomic<int> done{0};
    std::atomic<int> sleepers{0};
    std::atomic<bool> quit{false};
    std::mutex mx;
    std::condition_variable cv;
    std::atomic<double> spin_us{200.0};   // (may be set while the workers run: they read it at every poll)
    bool threads = false;

    MultiPool() = default;
    MultiPool(const MultiPool&) = delete;
    MultiPool& operator=(const MultiPool&) = delete;
    ~MultiPool() { stop(); }

    void worker(size_t i, unsigned long long seen, const std::function<void(size_t)>& bind) {
        bind(i);   // (what belongs to the thread — the current device — is set once)
        auto last = std::chrono::steady_clock::now();
        for (;;) {
            unsigned long long t = ticket.load(std::memory_order_acquire);
            if (t == seen) {
                if (quit.load(std::memory_order_relaxed)) return;
                if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - last).count() < spin_us.load(std::memory_order_relaxed)) { __builtin_ia32_pause(); continue; }
                std::unique_lock<std::mutex> lock(mx);
                sleepers.fetch_add(1, std::memory_order_seq_cst);
                cv.wait(lock, [&] { return ticket.load(std::memory_order_seq_cst) != seen || quit.load(std::memory_order_relaxed); });
                sleepers.fetch_sub(1, std::memory_order_seq_cst);
                continue;
            }
            seen = t;
            job_rc[i] = job(i);
            done.fetch_add(1, std::memory_order_release);
            last = std::chrono::steady_clock::now();
        }
    }

    // one worker for each of the shards 1 .. n_shards - 1, each running bind(its shard) first; a pool that runs already stays as it is.
    // false: the threads could not be created (none is left running)
    bool start(size_t n_shards, std::function<void(size_t)> bind) {
        if (threads) return true;
        job_rc.assign(n_shards, 0);
        job = nullptr;
        done.store(0, std::memory_order_relaxed);
        const unsigned long long issued = ticket.load(std::memory_order_relaxed);   // (the caller's own last ticket: nothing is in flight)
        try {
            for (size_t i = 1; i < n_shards; ++i) workers.emplace_back([this, i, issued, bind] { worker(i, issued, bind); });
        } catch (...) {
            stop();
            return false;
        }
        threads = true;
        return true;
    }

    void stop() {
        if (workers.empty()) return;
        {
            std::lock_guard<std::mutex> lock(mx);
            quit.store(true, std::memory_order_seq_cst);
        }
        cv.notify_all();
        for (std::thread& t : workers) t.join();
        workers.clear();
        quit.store(false, std::memory_order_seq_cst);
        threads = false;
    }

    // every shard runs job(i) once: shard 0 on the caller's thread, shard i > 0 on its worker (the pool has been started).  Returns 0, or
    // the code of the lowest shard whose job did not return 0, that shard in *failed
    int run(std::function<int(size_t)> j, size_t* failed) {
        const size_t S = job_rc.size();
        job = std::move(j);
        done.store(0, std::memory_order_relaxed);
        ticket.fetch_add(1, std::memory_order_seq_cst);
        if (sleepers.load(std::memory_order_seq_cst) > 0) { std::lock_guard<std::mutex> lock(mx); cv.notify_all(); }
        job_rc[0] = job(0);
        for (unsigned polls = 1; done.load(std::memory_order_acquire) < int(S) - 1; ++polls) {
            __builtin_ia32_pause();
            if (polls % 4096 == 0 && sleepers.load(std::memory_order_seq_cst) > 0) { std::lock_guard<std::mutex> lock(mx); cv.notify_all(); }
        }
        job = nullptr;   // (every shard has returned: nothing calls it any more, and its captures may die with the caller's frame)
        for (size_t i = 0; i < S; ++i) if (job_rc[i] != 0) { *failed = i; return job_rc[i]; }
        return 0;
    }
};
