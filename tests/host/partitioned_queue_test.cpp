// partitioned_queue_test.cpp -- PartitionedRedisQueueingTokenBucketRateLimiter: queueing limit
// classes behind ClassOf and one replenish timer per period.  Run by
// tests/test_host_partitioned_queue.py.
//
//   partitioned_queue_test cpu   option validation (no device needed)
//   partitioned_queue_test gpu   two classes with periods 1 s and 30 s, different QueueLimits and
//                                orders, injected clock, AutoReplenishment off (no waiting on wall
//                                time): the timers' classes; queued waits that complete at the tick
//                                of their own class only; OnRefresh's masks; TryReplenish; eviction
//                                and failure under each class's QueueLimit; a canceled wait;
//                                GetAvailablePermits of an unseen name; an out-of-range ClassOf;
//                                GetStatistics; ReclaimExpired and a reused key's class
//
// Class 0 (the options): TokenLimit 5, 2 tokens per 1 s, QueueLimit 4, OldestFirst; its rows lapse
// after 3 s (TB:234).  Class 1 ("slow:" names): TokenLimit 3, 3 tokens per 30 s (0.1 per second),
// QueueLimit 2, NewestFirst; its rows lapse after 30 s.  The clock moves in steps of 20 s or more,
// so every grant below holds whatever the last bit of a refill is.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <future>
#include <mutex>
#include <string>
#include <vector>

#include "rate_limiting.hpp"
#include "tbe.h"

using namespace tbe::rate_limiting;

static int g_fail = 0, g_pass = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (g_fail < 20) std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                                 \
        } else {                                                                      \
            ++g_pass;                                                                 \
        }                                                                             \
    } while (0)

static const int64_t T0 = 1760000000000000LL;
static const int64_t SEC = 1000000;
static std::atomic<int64_t> g_now{T0};
static std::mutex g_trace_mu;
static std::vector<RefreshTrace> g_trace;
static std::atomic<int> g_class_of_calls{0};
using Limiter = PartitionedRedisQueueingTokenBucketRateLimiter;

static RedisQueueingTokenBucketRateLimiterOptions options() {
    RedisQueueingTokenBucketRateLimiterOptions o;
    o.TokenLimit = 5;
    o.TokensPerPeriod = 2;
    o.ReplenishmentPeriod = TimeSpan::FromSeconds(1.0);
    o.QueueLimit = 4;
    o.InstanceName = "qclasses:";
    o.Device = 0;
    o.PartitionLimit = 3;
    o.AutoReplenishment = false;
    o.TrackStatistics = true;
    o.TimeSource = [] { return g_now.load(); };
    QueueingTokenBucketClass slow;
    slow.TokenLimit = 3;
    slow.TokensPerPeriod = 3;
    slow.ReplenishmentPeriod = TimeSpan::FromSeconds(30.0);
    slow.QueueLimit = 2;
    slow.QueueProcessingOrder = QueueProcessingOrder::NewestFirst;
    o.QueueingClasses.push_back(slow);
    o.ClassOf = [](const std::string &id) {
        ++g_class_of_calls;
        if (id.rfind("slow:", 0) == 0) return 1;
        if (id.rfind("bad:", 0) == 0) return 7;
        return 0;
    };
    o.OnRefresh = [](const RefreshTrace &t) {
        std::lock_guard<std::mutex> g(g_trace_mu);
        g_trace.push_back(t);
    };
    return o;
}

template <class Ex, class F>
static bool throws(F &&f) {
    try {
        f();
    } catch (const Ex &) {
        return true;
    } catch (...) {
        return false;
    }
    return false;
}

static bool throws_erange(Limiter &lim, const std::string &name) {
    try {
        lim.AttemptAcquire(name, 1);
    } catch (const RateLimiterEngineException &e) {
        return e.Status == TBE_ERANGE;
    } catch (...) {
    }
    return false;
}

static bool last_mask_is(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, size_t n_traces) {
    std::lock_guard<std::mutex> g(g_trace_mu);
    if (g_trace.size() != n_traces) return false;
    const RefreshTrace &t = g_trace.back();
    return t.ts_us == g_now.load() && t.ClassMask[0] == w0 && t.ClassMask[1] == w1 && t.ClassMask[2] == w2 &&
           t.ClassMask[3] == w3;
}

static bool pending(std::future<RateLimitLease> &f) {
    return f.wait_for(std::chrono::seconds(0)) == std::future_status::timeout;
}
// ready now (every tick and batch below has returned before this is asked) and acquired or not
static bool done(std::future<RateLimitLease> &f, bool acquired) {
    return f.wait_for(std::chrono::seconds(0)) == std::future_status::ready && f.get().IsAcquired() == acquired;
}
static int64_t queued(Limiter &lim, const std::string &name) {
    return lim.GetStatistics(name)->CurrentQueuedCount;   // (runs behind every batch submitted before it)
}

// ---- cpu: the constructor's checks come before the engine is created
static void test_option_validation() {
    auto bad = [](auto edit) {
        RedisQueueingTokenBucketRateLimiterOptions o = options();
        edit(o);
        return throws<ArgumentException>([&] { Limiter lim(o); });
    };
    CHECK(bad([](auto &o) { o.QueueingClasses[0].TokenLimit = 0; }));
    CHECK(bad([](auto &o) { o.QueueingClasses[0].TokensPerPeriod = -1; }));
    CHECK(bad([](auto &o) { o.QueueingClasses[0].QueueLimit = -1; }));
    CHECK(bad([](auto &o) { o.QueueingClasses[0].ReplenishmentPeriod = TimeSpan::FromTicks(-1); }));
    CHECK(bad([](auto &o) { o.QueueingClasses.resize(256, o.QueueingClasses[0]); }));
    // the token bucket's three-field Classes stay refused by every queueing limiter
    CHECK(bad([](auto &o) { o.Classes.push_back(TokenBucketClass{3, 1, TimeSpan::FromSeconds(1.0)}); }));
    CHECK(throws<ArgumentException>([] {
        RedisQueueingTokenBucketRateLimiterOptions o = options();
        o.QueueingClasses.clear();
        o.Classes.push_back(TokenBucketClass{3, 1, TimeSpan::FromSeconds(1.0)});
        RedisQueueingTokenBucketRateLimiter lim(o);
    }));
    // the non-partitioned queueing limiter and both approximate limiters throw on QueueingClasses
    CHECK(throws<ArgumentException>([] { RedisQueueingTokenBucketRateLimiter lim(options()); }));
    RedisApproximateTokenBucketRateLimiterOptions a;
    static_cast<RedisQueueingTokenBucketRateLimiterOptions &>(a) = options();
    CHECK(throws<ArgumentException>([&] { RedisApproximateTokenBucketRateLimiter lim(a); }));
    CHECK(throws<ArgumentException>([&] { PartitionedRedisApproximateTokenBucketRateLimiter lim(a); }));
}

// ---- gpu
static void test_classes_and_timers() {
    g_now = T0;
    g_trace.clear();
    Limiter lim(options());
    // one timer per distinct ReplenishmentPeriod, each with the classes of its period
    auto timers = lim.ReplenishmentTimers();
    CHECK(timers.size() == 2);
    CHECK(timers[0].first.ticks == 1 * TimeSpan::TicksPerSecond && timers[0].second == std::vector<int>{0});
    CHECK(timers[1].first.ticks == 30 * TimeSpan::TicksPerSecond && timers[1].second == std::vector<int>{1});
    // an unseen name reports the TokenLimit of its class and takes no key; an out-of-range ClassOf throws
    CHECK(lim.GetAvailablePermits("slow:x") == 3 && lim.GetAvailablePermits("x") == 5);
    CHECK(lim.GetStatistics("slow:x")->CurrentAvailablePermits == 3 && queued(lim, "slow:x") == 0);
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.GetAvailablePermits("bad:x"); }));
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire("bad:x", 1); }));
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AcquireAsync("bad:x", 1); }));
    // the first request of a new name is decided under its class
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire("slow:a", 4); }));   // TokenLimit 3
    CHECK(lim.AttemptAcquire("slow:a", 3).IsAcquired());
    CHECK(lim.AttemptAcquire("a", 5).IsAcquired());
    CHECK(lim.GetAvailablePermits("slow:a") == 0 && lim.GetAvailablePermits("a") == 0);
    CHECK(!lim.AttemptAcquire("a", 1).IsAcquired());

    // ---- a queued wait completes at the tick of its own class: class 1's timer first
    std::future<RateLimitLease> wa = lim.AcquireAsync("a", 2), ws = lim.AcquireAsync("slow:a", 1);
    CHECK(queued(lim, "a") == 2 && queued(lim, "slow:a") == 1);
    CHECK(pending(wa) && pending(ws));
    g_now = T0 + 20 * SEC;   // a: full again; slow:a: 2 tokens
    lim.TickTimer(1);
    CHECK(last_mask_is(2, 0, 0, 0, 1));
    CHECK(done(ws, true) && pending(wa));
    lim.TickTimer(0);
    CHECK(last_mask_is(1, 0, 0, 0, 2));
    CHECK(done(wa, true));
    // ---- and the reverse: class 0's timer first (a: 3 tokens left, slow:a: 1)
    CHECK(lim.AttemptAcquire("a", 3).IsAcquired());
    std::future<RateLimitLease> wa2 = lim.AcquireAsync("a", 1), ws2 = lim.AcquireAsync("slow:a", 2);
    CHECK(queued(lim, "a") == 1 && queued(lim, "slow:a") == 2);
    g_now = T0 + 40 * SEC;   // slow:a: 3 tokens
    lim.TickTimer(0);
    CHECK(last_mask_is(1, 0, 0, 0, 3));
    CHECK(done(wa2, true) && pending(ws2));
    lim.TickTimer(1);
    CHECK(last_mask_is(2, 0, 0, 0, 4));
    CHECK(done(ws2, true));
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.TickTimer(2); }));
    // ---- TryReplenish ticks every class (a: 4 tokens left, slow:a: 1)
    CHECK(lim.AttemptAcquire("a", 4).IsAcquired());
    std::future<RateLimitLease> wa3 = lim.AcquireAsync("a", 2), ws3 = lim.AcquireAsync("slow:a", 2);
    CHECK(queued(lim, "a") == 2 && queued(lim, "slow:a") == 2);
    g_now = T0 + 60 * SEC;
    CHECK(lim.TryReplenish());
    CHECK(last_mask_is(~0ull, ~0ull, ~0ull, ~0ull, 5));
    CHECK(done(wa3, true) && done(ws3, true));

    // ---- each class's QueueLimit and order (a: 3 tokens left, slow:a: 1)
    // class 1, NewestFirst, QueueLimit 2: the second wait of 2 evicts the first
    std::future<RateLimitLease> e1 = lim.AcquireAsync("slow:a", 2);
    CHECK(queued(lim, "slow:a") == 2 && pending(e1));
    std::future<RateLimitLease> e2 = lim.AcquireAsync("slow:a", 2);
    CHECK(queued(lim, "slow:a") == 2);
    CHECK(done(e1, false) && pending(e2));
    // class 0, OldestFirst, QueueLimit 4: 3 queued, a wait of 2 fails at once
    CHECK(lim.AttemptAcquire("a", 3).IsAcquired());
    std::future<RateLimitLease> f1 = lim.AcquireAsync("a", 3), f2 = lim.AcquireAsync("a", 2);
    CHECK(queued(lim, "a") == 3);
    CHECK(done(f2, false) && pending(f1));
    // ---- a canceled queued wait throws OperationCanceledException and frees its permits
    CancellationTokenSource cts;
    std::future<RateLimitLease> c1 = lim.AcquireAsync("a", 1, cts.Token());
    CHECK(queued(lim, "a") == 4 && pending(c1));
    cts.Cancel();
    CHECK(c1.wait_for(std::chrono::seconds(30)) == std::future_status::ready);   // (the submitter applies it at once)
    CHECK(throws<OperationCanceledException>([&] { c1.get(); }));
    CHECK(queued(lim, "a") == 3);
    std::future<RateLimitLease> c2 = lim.AcquireAsync("a", 1);   // fits again
    CHECK(queued(lim, "a") == 4 && pending(c2));
    // ---- statistics: grants at once and at ticks are successful; a failed wait and an evicted one failed
    auto sa = lim.GetStatistics("a"), ss = lim.GetStatistics("slow:a");
    CHECK(sa && sa->TotalSuccessfulLeases == 7 && sa->TotalFailedLeases == 2 && sa->CurrentQueuedCount == 4);
    CHECK(ss && ss->TotalSuccessfulLeases == 4 && ss->TotalFailedLeases == 1 && ss->CurrentQueuedCount == 2);

    // ---- ReclaimExpired: a name with a queued wait keeps its key, a lapsed one frees it
    CHECK(lim.AttemptAcquire("b", 1).IsAcquired());
    CHECK(throws_erange(lim, "c"));     // all three keys held, none lapsed
    g_now = T0 + 100 * SEC;             // every row has lapsed (3 s, 30 s); a and slow:a have queued waits
    CHECK(lim.ReclaimExpired() == 1);
    CHECK(lim.GetAvailablePermits("b") == 5);   // unseen again
    CHECK(queued(lim, "a") == 4 && queued(lim, "slow:a") == 2);
    // the reused key takes its new name's class
    const int calls = g_class_of_calls.load();
    CHECK(lim.AttemptAcquire("slow:n", 3).IsAcquired());
    CHECK(g_class_of_calls.load() > calls);
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire("slow:n", 4); }));
    CHECK(lim.GetAvailablePermits("slow:n") == 0);
    CHECK(!lim.AttemptAcquire("slow:n", 1).IsAcquired());   // (class 0 would have 2 tokens left)
    auto sn = lim.GetStatistics("slow:n");
    CHECK(sn && sn->TotalSuccessfulLeases == 1 && sn->TotalFailedLeases == 1);   // b's counters are gone
    CHECK(throws_erange(lim, "z"));     // the reclaim that runs by itself finds nothing: two queued, one fresh
    // the kept waits complete at the next tick of everything
    CHECK(lim.TryReplenish());
    CHECK(done(e2, true) && done(f1, true) && done(c2, true));
    lim.Dispose();
    CHECK(throws<ObjectDisposedException>([&] { lim.TickTimer(0); }));
}

static void test_auto_replenishment_timers() {
    RedisQueueingTokenBucketRateLimiterOptions o = options();
    o.AutoReplenishment = true;
    o.ReplenishmentPeriod = TimeSpan::FromSeconds(3600.0);
    o.TokensPerPeriod = 7200;
    o.QueueingClasses[0].ReplenishmentPeriod = TimeSpan::FromSeconds(7200.0);
    QueueingTokenBucketClass third = o.QueueingClasses[0];
    third.ReplenishmentPeriod = TimeSpan::FromSeconds(3600.0);   // shares class 0's timer
    o.QueueingClasses.push_back(third);
    Limiter lim(o);
    auto timers = lim.ReplenishmentTimers();
    CHECK(timers.size() == 2);
    CHECK(timers[0].first.ticks == 3600 * TimeSpan::TicksPerSecond && (timers[0].second == std::vector<int>{0, 2}));
    CHECK(timers[1].first.ticks == 7200 * TimeSpan::TicksPerSecond && timers[1].second == std::vector<int>{1});
    CHECK(!lim.TryReplenish());
    CHECK(lim.AttemptAcquire("slow:x", 3).IsAcquired());
    CHECK(!lim.AttemptAcquire("slow:x", 1).IsAcquired());
    lim.Dispose();   // (joins both timer threads, hours before their first tick)
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    test_option_validation();
    if (gpu) {
        test_classes_and_timers();
        test_auto_replenishment_timers();
    }
    std::printf("partitioned_queue_test %s: %d checks passed, %d failed\n", gpu ? "gpu" : "cpu", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
