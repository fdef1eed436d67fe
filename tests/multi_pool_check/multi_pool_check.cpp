// The launching-thread pool of a multi-device handle (hippopt_amd/csrc/multi_pool.h) on the CPU: the text the library runs, with a
// recorder where the library binds a device and launches kernels.  tests/test_multi_pool.py builds this file twice (plain and with
// ThreadSanitizer) and runs it as a child process.
//
// One line per scenario and configuration; the first violated condition ends the program with status 1 (`--all`: every scenario is
// run and the failing ones are listed, status 1 at the end).  A scenario that has not finished within LIMIT_S is named by the
// watchdog thread, which ends the program with status 3: a lost wake-up is a failed test, not a stuck one.
//
// What a job touches is a record held by a shared_ptr the job captures, and every field of it is atomic: a pool that calls a job late,
// twice or from the wrong thread is seen by defined behaviour.
#include "../../hippopt_amd/csrc/multi_pool.h"

#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>

// The slowest scenario of ten runs against the fixed pool on 8 CPUs: 0.367 s in the five plain runs (the 2000 wake-ups of eight shards
// at spin_us = 0), 0.752 s in the five under ThreadSanitizer (the 200 restarts of eight shards).  The limit is 20 times the slower one
// (profiles/r16_multi_pool.txt).
constexpr double LIMIT_S = 15.0;
constexpr size_t MAX_SHARDS = 8;

using Clock = std::chrono::steady_clock;

static unsigned thread_token() {
    static std::atomic<unsigned> next{0};
    thread_local unsigned mine = next.fetch_add(1) + 1;
    return mine;
}
static void busy_wait_us(double us) {
    const auto t0 = Clock::now();
    while (std::chrono::duration<double, std::micro>(Clock::now() - t0).count() < us) __builtin_ia32_pause();
}
static void sleep_ms(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

// ---- the watchdog ----------------------------------------------------------------------------------------------------------------------
static std::atomic<const char*> g_scenario{nullptr};
static std::atomic<long long> g_started_ns{0};
static std::atomic<int> g_shards{0};
static std::atomic<double> g_spin{0.0};
static long long now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now().time_since_epoch()).count(); }
static void watchdog() {
    for (;;) {
        sleep_ms(20);
        const char* name = g_scenario.load();
        if (name && double(now_ns() - g_started_ns.load()) * 1e-9 > LIMIT_S) {
            std::printf("HUNG %s shards=%d spin_us=%g: not finished after %.0f s\n", name, g_shards.load(), g_spin.load(), LIMIT_S);
            std::fflush(stdout);
            _exit(3);
        }
    }
}

// ---- what the jobs and the binds record -----------------------------------------------------------------------------------------------
struct Binds {   // of one start(): how often bind(i) ran and on which thread
    std::atomic<int> count[MAX_SHARDS];
    std::atomic<unsigned> thread[MAX_SHARDS];
    Binds() { for (size_t i = 0; i < MAX_SHARDS; ++i) { count[i] = 0; thread[i] = 0; } }
};
struct Record {  // of one generation of jobs
    int generation;
    std::atomic<int> calls[MAX_SHARDS];
    std::atomic<unsigned> thread[MAX_SHARDS];   // of the last call
    std::atomic<int> unbound{0};                // calls of a shard i > 0 from a thread whose bind(i) had not run exactly once
    std::atomic<int> late{0};                   // calls after `closed` was set
    std::atomic<bool> closed{false};
    explicit Record(int g) : generation(g) { for (size_t i = 0; i < MAX_SHARDS; ++i) { calls[i] = 0; thread[i] = 0; } }
};
using RecordP = std::shared_ptr<Record>;
using BindsP = std::shared_ptr<Binds>;

static std::function<void(size_t)> make_bind(BindsP b) {
    return [b](size_t i) { b->thread[i].store(thread_token()); b->count[i].fetch_add(1); };
}
// rc(i): what shard i returns; slow_us: how long the LAST shard takes (the caller's shard 0 is done long before it)
static std::function<int(size_t)> make_job(RecordP r, BindsP b, size_t S, std::function<int(size_t)> rc = nullptr, double slow_us = 0.0) {
    return [r, b, S, rc, slow_us](size_t i) -> int {
        const unsigned me = thread_token();
        if (i > 0 && (b->count[i].load() != 1 || b->thread[i].load() != me)) r->unbound.fetch_add(1);
        if (r->closed.load()) r->late.fetch_add(1);
        if (slow_us > 0.0 && i + 1 == S) busy_wait_us(slow_us);
        r->thread[i].store(me);
        r->calls[i].fetch_add(1);
        return rc ? rc(i) : 0;
    };
}

struct Violation { std::string what; };
#define REQUIRE(cond, ...)                                                        \
    do {                                                                          \
        if (!(cond)) {                                                            \
            char buf_[512];                                                       \
            std::snprintf(buf_, sizeof buf_, __VA_ARGS__);                        \
            throw Violation{std::string(#cond) + ": " + buf_};                    \
        }                                                                         \
    } while (0)

// generation r has been called `times` times per shard, shard 0 by this thread, shard i > 0 by the worker bind(i) ran on
static void check_calls(const RecordP& r, const BindsP& b, size_t S, int times) {
    for (size_t i = 0; i < S; ++i) REQUIRE(r->calls[i].load() == times, "generation %d, shard %zu: %d calls, %d expected", r->generation, i, r->calls[i].load(), times);
    for (size_t i = S; i < MAX_SHARDS; ++i) REQUIRE(r->calls[i].load() == 0, "generation %d: shard %zu does not exist and was called", r->generation, i);
    if (times > 0) {
        REQUIRE(r->thread[0].load() == thread_token(), "generation %d: shard 0 ran on thread %u, the caller is %u", r->generation, r->thread[0].load(), thread_token());
        for (size_t i = 1; i < S; ++i) REQUIRE(r->thread[i].load() == b->thread[i].load(), "generation %d: shard %zu ran on thread %u, bound was %u", r->generation, i, r->thread[i].load(), b->thread[i].load());
    }
    for (size_t i = 1; i < S; ++i) REQUIRE(b->count[i].load() == 1, "bind(%zu) ran %d times", i, b->count[i].load());
    REQUIRE(b->count[0].load() == 0, "bind(0) ran: shard 0 belongs to the caller");
    REQUIRE(r->unbound.load() == 0, "generation %d: %d calls from a thread that is not the shard's bound worker", r->generation, r->unbound.load());
    REQUIRE(r->late.load() == 0, "generation %d: %d calls after its run had returned", r->generation, r->late.load());
}
static void check_released(MultiPool& pool, const RecordP& r) {
    REQUIRE(r.use_count() == 1, "generation %d is still held after run returned (use_count %ld)", r->generation, long(r.use_count()));
    REQUIRE(!pool.job, "the pool holds a job after run returned");
}
// one run of a fresh generation, checked
static RecordP run_checked(MultiPool& pool, const BindsP& b, size_t S, int generation) {
    RecordP r = std::make_shared<Record>(generation);
    size_t failed = 99;
    const int rc = pool.run(make_job(r, b, S), &failed);
    r->closed.store(true);
    REQUIRE(rc == 0, "run returned %d", rc);
    check_calls(r, b, S, 1);
    check_released(pool, r);
    return r;
}
static BindsP start_checked(MultiPool& pool, size_t S, double spin) {
    BindsP b = std::make_shared<Binds>();
    pool.spin_us = spin;
    REQUIRE(pool.start(S, make_bind(b)), "start failed");
    REQUIRE(pool.workers.size() == S - 1, "%zu workers for %zu shards", pool.workers.size(), S);
    return b;
}
static void wait_for_sleepers(MultiPool& pool, int n) {   // (the watchdog bounds it)
    while (pool.sleepers.load() != n) sleep_ms(1);
}

// ---- the scenarios ---------------------------------------------------------------------------------------------------------------------
// run, stop, start, wait, check, run a new generation: nothing of generation 1 happens after its run
static void off_on(size_t S, double spin) {
    MultiPool pool;
    BindsP b1 = start_checked(pool, S, spin);
    RecordP g1 = std::make_shared<Record>(1);
    size_t failed = 99;
    const int rc = pool.run(make_job(g1, b1, S), &failed);
    g1->closed.store(true);
    REQUIRE(rc == 0, "run returned %d", rc);
    check_calls(g1, b1, S, 1);
    pool.stop();
    REQUIRE(pool.workers.empty(), "workers left after stop");
    BindsP b2 = start_checked(pool, S, spin);
    sleep_ms(50);
    for (size_t i = 0; i < S; ++i) REQUIRE(g1->calls[i].load() == 1, "generation 1, shard %zu: %d calls after stop and start with no new run", i, g1->calls[i].load());
    REQUIRE(g1->late.load() == 0, "generation 1: %d calls after its run had returned", g1->late.load());
    REQUIRE(pool.done.load() == 0, "done count %d after start", pool.done.load());
    for (size_t i = 0; i < pool.job_rc.size(); ++i) REQUIRE(pool.job_rc[i] == 0, "return code of shard %zu is %d after start", i, pool.job_rc[i]);
    check_released(pool, g1);
    run_checked(pool, b2, S, 2);
    check_calls(g1, b1, S, 1);   // only generation 2 has been called
}
static void one_call_per_shard(size_t S, double spin) {
    MultiPool pool;
    BindsP b = start_checked(pool, S, spin);
    for (int g = 1; g <= 20; ++g) run_checked(pool, b, S, g);
}
static void job_released(size_t S, double spin) {
    MultiPool pool;
    BindsP b = start_checked(pool, S, spin);
    RecordP r = run_checked(pool, b, S, 1);
    pool.stop();
    check_released(pool, r);
}
// two runs with no pause between them (the enqueue-then-wait pair of an evaluation): the first has finished on every shard when it
// returns — its last shard is slow —, and nothing of it happens during the second
static void back_to_back(size_t S, double spin) {
    MultiPool pool;
    BindsP b = start_checked(pool, S, spin);
    for (int pair = 0; pair < 20; ++pair) {
        RecordP r1 = std::make_shared<Record>(2 * pair + 1), r2 = std::make_shared<Record>(2 * pair + 2);
        size_t failed = 99;
        const int rc1 = pool.run(make_job(r1, b, S, nullptr, 200.0), &failed);
        r1->closed.store(true);
        // (a call of the second generation that preceded this line would be one the pool made before it was given the job)
        const int rc2 = pool.run(make_job(r2, b, S), &failed);
        r2->closed.store(true);
        REQUIRE(rc1 == 0 && rc2 == 0, "runs returned %d, %d", rc1, rc2);
        check_calls(r1, b, S, 1);
        check_calls(r2, b, S, 1);
        check_released(pool, r1);
        check_released(pool, r2);
    }
}
static void restarts(size_t S, double spin) {
    MultiPool pool;
    std::vector<RecordP> gens;
    std::vector<BindsP> binds;
    for (int g = 1; g <= 200; ++g) {
        binds.push_back(start_checked(pool, S, spin));
        REQUIRE(pool.done.load() == 0, "done count %d after start %d", pool.done.load(), g);
        gens.push_back(run_checked(pool, binds.back(), S, g));
        pool.stop();
    }
    sleep_ms(5);
    for (size_t g = 0; g < gens.size(); ++g) check_calls(gens[g], binds[g], S, 1);
}
// 2000 runs a seeded 0 .. 300 us apart: the workers cross the boundary between polling and sleeping in both directions
static void wake_ups(size_t S, double spin) {
    MultiPool pool;
    BindsP b = start_checked(pool, S, spin);
    RecordP r = std::make_shared<Record>(1);
    const std::function<int(size_t)> job = make_job(r, b, S);
    std::mt19937 rng(20240611u + unsigned(S));
    std::uniform_real_distribution<double> pause(0.0, 300.0);
    for (int k = 1; k <= 2000; ++k) {
        size_t failed = 99;
        const int rc = pool.run(job, &failed);
        REQUIRE(rc == 0, "run %d returned %d", k, rc);
        for (size_t i = 0; i < S; ++i) REQUIRE(r->calls[i].load() == k, "after run %d shard %zu has %d calls", k, i, r->calls[i].load());
        REQUIRE(r.use_count() == 2, "run %d: use_count %ld (this scenario's copy and the record's owner)", k, long(r.use_count()));
        busy_wait_us(pause(rng));
    }
    check_calls(r, b, S, 2000);
}
static void return_codes(size_t S, double spin) {
    MultiPool pool;
    BindsP b = start_checked(pool, S, spin);
    const unsigned masks[] = {0x01, 0x02, 0x80, 0x08, 0x0A, 0x88, 0xFE, 0xFF, 0x81, 0xC0};
    int g = 0;
    for (unsigned m : masks) {
        const unsigned mask = m & ((1u << S) - 1u);
        if (!mask) continue;
        size_t lowest = 0;
        while (!(mask >> lowest & 1u)) ++lowest;
        RecordP r = std::make_shared<Record>(++g);
        size_t failed = 99;
        const int rc = pool.run(make_job(r, b, S, [mask](size_t i) { return (mask >> i & 1u) ? 100 + int(i) : 0; }), &failed);
        r->closed.store(true);
        REQUIRE(rc == 100 + int(lowest) && failed == lowest, "mask %#x: run returned %d for shard %zu, expected %d for shard %zu", mask, rc, failed, 100 + int(lowest), lowest);
        check_calls(r, b, S, 1);   // (a failing shard does not keep the others from running: their kernels are in flight anyway)
        check_released(pool, r);
        run_checked(pool, b, S, ++g);   // the next run is clean
    }
}
static std::vector<std::thread::id> worker_ids(const MultiPool& pool) {
    std::vector<std::thread::id> ids;
    for (const std::thread& t : pool.workers) ids.push_back(t.get_id());
    return ids;
}
static void lifecycle_edges(size_t S, double) {
    {   // start twice: the second is a no-op (its bind is never run), the same threads
        MultiPool pool;
        BindsP b = start_checked(pool, S, 50.0), b2 = std::make_shared<Binds>();
        const auto ids = worker_ids(pool);
        run_checked(pool, b, S, 1);
        REQUIRE(pool.start(S, make_bind(b2)), "second start failed");
        REQUIRE(worker_ids(pool) == ids, "the second start changed the worker threads");
        run_checked(pool, b, S, 2);
        for (size_t i = 0; i < S; ++i) REQUIRE(b2->count[i].load() == 0, "the second start ran bind(%zu)", i);
        pool.stop();
        pool.stop();   // stop twice
        REQUIRE(pool.workers.empty(), "workers after stop");
        BindsP b3 = start_checked(pool, S, 50.0);
        run_checked(pool, b3, S, 3);
    }
    {   // stop with the workers asleep
        MultiPool pool;
        BindsP b = start_checked(pool, S, 0.0);
        run_checked(pool, b, S, 1);
        wait_for_sleepers(pool, int(S) - 1);
        pool.stop();
        REQUIRE(pool.sleepers.load() == 0, "%d sleepers after stop", pool.sleepers.load());
    }
    {   // stop while they poll
        MultiPool pool;
        BindsP b = start_checked(pool, S, 1e6);
        run_checked(pool, b, S, 1);
        REQUIRE(pool.sleepers.load() == 0, "%d sleepers with spin_us = 1e6", pool.sleepers.load());
        pool.stop();
    }
    { MultiPool pool; }   // a pool that was never started ...
    { MultiPool pool; start_checked(pool, S, 0.0); }   // ... or never ran: destroyed with workers asleep, polling or still starting
    { MultiPool pool; start_checked(pool, S, 1e6); }
    { MultiPool pool; pool.stop(); pool.stop(); }
    {   // spin_us changed between two starts: the second start's workers follow the new value
        MultiPool pool;
        BindsP b = start_checked(pool, S, 1e6);
        run_checked(pool, b, S, 1);
        sleep_ms(2);
        REQUIRE(pool.sleepers.load() == 0, "%d sleepers with spin_us = 1e6", pool.sleepers.load());
        pool.stop();
        BindsP b2 = start_checked(pool, S, 0.0);
        wait_for_sleepers(pool, int(S) - 1);   // (asleep before their first job)
        run_checked(pool, b2, S, 2);
        wait_for_sleepers(pool, int(S) - 1);
        run_checked(pool, b2, S, 3);
    }
    if (S == 1) {   // one shard: no workers, the caller runs it
        MultiPool pool;
        BindsP b = start_checked(pool, 1, 0.0);
        REQUIRE(pool.workers.empty(), "a worker for one shard");
        run_checked(pool, b, 1, 1);
        REQUIRE(b->count[0].load() == 0, "bind ran for one shard");
    }
}

struct Scenario { const char* name; void (*fn)(size_t, double); unsigned spins; };   // spins: bit j set = run at SPINS[j]
static const double SPINS[] = {0.0, 50.0, 1e6};   // sleep at once; poll, then sleep; never sleep
static const Scenario SCENARIOS[] = {
    {"off -> on", off_on, 7},
    {"one call per shard", one_call_per_shard, 7},
    {"job released", job_released, 7},
    {"back-to-back runs", back_to_back, 7},
    {"repeated restarts", restarts, 7},
    {"wake-ups", wake_ups, 3},                 // (a worker that never sleeps is never woken)
    {"return codes", return_codes, 7},
    {"lifecycle edges", lifecycle_edges, 1},   // (sets spin_us itself)
};

int main(int argc, char** argv) {
    const bool all = argc > 1 && !std::strcmp(argv[1], "--all");
    std::thread(watchdog).detach();
    const size_t shards[] = {1, 2, 4, 8};
    int failures = 0;
    double slowest = 0.0;
    for (const Scenario& sc : SCENARIOS)
        for (size_t S : shards)
            for (size_t j = 0; j < 3; ++j) {
                if (!(sc.spins >> j & 1u)) continue;
                const double spin = SPINS[j];
                g_shards.store(int(S)); g_spin.store(spin); g_started_ns.store(now_ns()); g_scenario.store(sc.name);
                const auto t0 = Clock::now();
                std::string verdict = "ok";
                try { sc.fn(S, spin); } catch (const Violation& v) { verdict = "FAIL"; ++failures; std::printf("FAIL %s shards=%zu spin_us=%g: %s\n", sc.name, S, spin, v.what.c_str()); }
                g_scenario.store(nullptr);
                const double s = std::chrono::duration<double>(Clock::now() - t0).count();
                if (s > slowest) slowest = s;
                if (verdict == "ok") std::printf("ok %s shards=%zu spin_us=%g %.1f ms\n", sc.name, S, spin, s * 1e3);
                std::fflush(stdout);
                if (failures && !all) return 1;
            }
    std::printf("%s: %d failing, slowest scenario %.3f s (limit %.0f s)\n", failures ? "FAILED" : "passed", failures, slowest, LIMIT_S);
    return failures ? 1 : 0;
}
