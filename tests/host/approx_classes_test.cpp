// approx_classes_test.cpp -- approximate limit classes behind ClassOf on
// PartitionedRedisApproximateTokenBucketRateLimiter.  Run by tests/test_host_approx_classes.py.
//
//   approx_classes_test cpu   option validation (no device needed)
//   approx_classes_test gpu   two classes with different periods and QueueLimits; the first
//                             request of a name decided under its class; an out-of-range ClassOf;
//                             GetAvailablePermits of an unseen name; the per-period timers' ticks
//                             (through TickTimer and OnRefresh, no waiting on wall time);
//                             TryReplenish over both classes; a reused key takes its new name's class
//
// Class 0 (the options): TokenLimit 5, 2 tokens per 1 s, QueueLimit 4.  Class 1 ("slow:" names):
// TokenLimit 3, 1 token per 2 s (0.5 per second), QueueLimit 0.  Injected clock.
//   a class's first sync   local count -> global score; the measured interval is 0, so the
//                          instance estimate is infinite and AvailableTokens 0
//   10 s later             every row has decayed to 0; interval 0.2 * 10 = 2 s, estimates
//                          max(1, round(1 / 2)) = 1 and round(2 / 2) = 1: caps 5 and 3
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
static std::atomic<int64_t> g_now{T0};
static std::mutex g_trace_mu;
static std::vector<RefreshTrace> g_trace;
static std::atomic<int> g_class_of_calls{0};

static RedisApproximateTokenBucketRateLimiterOptions options() {
    RedisApproximateTokenBucketRateLimiterOptions o;
    o.TokenLimit = 5;
    o.TokensPerPeriod = 2;
    o.ReplenishmentPeriod = TimeSpan::FromSeconds(1.0);
    o.QueueLimit = 4;
    o.InstanceName = "aclasses:";
    o.Device = 0;
    o.PartitionLimit = 3;
    o.AutoReplenishment = false;
    o.TimeSource = [] { return g_now.load(); };
    ApproximateTokenBucketClass slow;
    slow.TokenLimit = 3;
    slow.TokensPerPeriod = 1;
    slow.ReplenishmentPeriod = TimeSpan::FromSeconds(2.0);
    slow.QueueLimit = 0;
    o.ApproximateClasses.push_back(slow);
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

static bool throws_erange(PartitionedRedisApproximateTokenBucketRateLimiter &lim, const std::string &name) {
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

// ---- cpu: the constructor's checks come before the engine is created
static void test_option_validation() {
    using L = PartitionedRedisApproximateTokenBucketRateLimiter;
    auto bad = [](auto edit) {
        RedisApproximateTokenBucketRateLimiterOptions o = options();
        edit(o);
        return throws<ArgumentException>([&] { L lim(o); });
    };
    CHECK(bad([](auto &o) { o.ApproximateClasses[0].TokenLimit = 0; }));
    CHECK(bad([](auto &o) { o.ApproximateClasses[0].TokensPerPeriod = -1; }));
    CHECK(bad([](auto &o) { o.ApproximateClasses[0].QueueLimit = -1; }));
    CHECK(bad([](auto &o) { o.ApproximateClasses[0].ReplenishmentPeriod = TimeSpan::FromTicks(-1); }));
    CHECK(bad([](auto &o) { o.ApproximateClasses.resize(256, o.ApproximateClasses[0]); }));
    // the token bucket's three-field Classes stay refused here
    CHECK(bad([](auto &o) { o.Classes.push_back(TokenBucketClass{3, 1, TimeSpan::FromSeconds(1.0)}); }));
    // the non-partitioned approximate limiter keeps throwing on classes
    CHECK(throws<ArgumentException>([] { RedisApproximateTokenBucketRateLimiter lim(options()); }));
}

// ---- gpu
static void test_classes_behind_class_of() {
    g_now = T0;
    g_trace.clear();
    PartitionedRedisApproximateTokenBucketRateLimiter lim(options());
    // one timer per distinct ReplenishmentPeriod, each with the classes of its period
    auto timers = lim.ReplenishmentTimers();
    CHECK(timers.size() == 2);
    CHECK(timers[0].first.ticks == 1 * TimeSpan::TicksPerSecond && timers[0].second == std::vector<int>{0});
    CHECK(timers[1].first.ticks == 2 * TimeSpan::TicksPerSecond && timers[1].second == std::vector<int>{1});
    // an unseen name reports the TokenLimit of its class and takes no key
    CHECK(lim.GetAvailablePermits("slow:x") == 3);
    CHECK(lim.GetAvailablePermits("x") == 5);
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.GetAvailablePermits("bad:x"); }));
    // the first request of a new name is decided under its class
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire("slow:a", 4); }));   // TokenLimit 3
    CHECK(lim.AttemptAcquire("slow:a", 3).IsAcquired());
    CHECK(lim.GetAvailablePermits("slow:a") == 0);
    RateLimitLease denied = lim.AttemptAcquire("slow:a", 1);
    TimeSpan ra;
    // A:390-395 with the class's TokenLimit and rate: deficit 0 + 3 + 1 + 0 - 3 = 1, times 0.5 per second
    CHECK(!denied.IsAcquired() && denied.TryGetRetryAfter(ra) && ra.ticks == TimeSpan::TicksPerSecond / 2);
    // QueueLimit 0: a wait fails at once where class 0 queues
    std::future<RateLimitLease> w_slow = lim.AcquireAsync("slow:a", 1);
    CHECK(w_slow.wait_for(std::chrono::seconds(30)) == std::future_status::ready && !w_slow.get().IsAcquired());
    CHECK(lim.AttemptAcquire("a", 4).IsAcquired());                                          // TokenLimit 5
    CHECK(lim.GetAvailablePermits("a") == 1);
    std::future<RateLimitLease> wait_a = lim.AcquireAsync("a", 3);                           // QueueLimit 4
    CHECK(lim.GetAvailablePermits("a") == 1);   // (also orders this thread behind the wait's batch)
    CHECK(wait_a.wait_for(std::chrono::seconds(0)) == std::future_status::timeout);
    // an out-of-range ClassOf throws to its caller and assigns no key: the third key is still there
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire("bad:z", 1); }));
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AcquireAsync("bad:z", 1); }));
    CHECK(lim.AttemptAcquire("b", 1).IsAcquired());
    CHECK(throws_erange(lim, "c"));                                                          // all three keys held
    // the 2 s timer's tick refreshes class 1 alone: slow:a syncs (estimate infinite), a and b do not
    lim.TickTimer(1);
    CHECK(last_mask_is(2, 0, 0, 0, 1));
    CHECK(lim.GetAvailablePermits("slow:a") == 0 && lim.GetAvailablePermits("a") == 1 &&
          lim.GetAvailablePermits("b") == 4);
    denied = lim.AttemptAcquire("slow:a", 1);   // deficit: global 3 + local 0 + 1 + 0 - 3 = 1
    CHECK(!denied.IsAcquired() && denied.TryGetRetryAfter(ra) && ra.ticks == TimeSpan::TicksPerSecond / 2);
    // the 1 s timer's tick refreshes class 0 alone
    lim.TickTimer(0);
    CHECK(last_mask_is(1, 0, 0, 0, 2));
    CHECK(lim.GetAvailablePermits("a") == 0 && lim.GetAvailablePermits("b") == 0);
    CHECK(wait_a.wait_for(std::chrono::seconds(0)) == std::future_status::timeout);
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.TickTimer(2); }));
    // TryReplenish refreshes every class: 10 s later both rows have decayed and both caps are back
    g_now = T0 + 10000000;
    CHECK(lim.TryReplenish());
    CHECK(last_mask_is(~0ull, ~0ull, ~0ull, ~0ull, 3));
    CHECK(wait_a.wait_for(std::chrono::seconds(30)) == std::future_status::ready && wait_a.get().IsAcquired());
    CHECK(lim.GetAvailablePermits("a") == 2);        // cap 5, the granted wait's 3
    CHECK(lim.GetAvailablePermits("slow:a") == 3);   // cap 3 with class 1's period: round(2 s / 2 s) = 1 client
    CHECK(lim.GetAvailablePermits("b") == 5);
    // slow:a and b are idle, a holds 3: two keys come back, and each goes to a name of the other class
    CHECK(lim.ReclaimIdle() == 2);
    CHECK(lim.GetAvailablePermits("slow:a") == 3 && lim.GetAvailablePermits("b") == 5);   // unseen again
    const int calls = g_class_of_calls.load();
    CHECK(lim.AttemptAcquire("slow:n", 1).IsAcquired());
    CHECK(g_class_of_calls.load() > calls);          // asked when the name took its (reused) key
    CHECK(lim.GetAvailablePermits("slow:n") == 2);
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire("slow:n", 4); }));
    CHECK(lim.AttemptAcquire("m", 5).IsAcquired());  // class 0 on the other reused key: TokenLimit 5
    CHECK(lim.GetAvailablePermits("m") == 0);
    CHECK(lim.AttemptAcquire("slow:n", 2).IsAcquired() && !lim.AttemptAcquire("slow:n", 1).IsAcquired());
    CHECK(throws_erange(lim, "slow:o"));
    lim.Dispose();
    CHECK(throws<ObjectDisposedException>([&] { lim.TickTimer(0); }));
}

static void test_auto_replenishment_timers() {
    RedisApproximateTokenBucketRateLimiterOptions o = options();
    o.AutoReplenishment = true;
    o.ReplenishmentPeriod = TimeSpan::FromSeconds(3600.0);
    o.ApproximateClasses[0].ReplenishmentPeriod = TimeSpan::FromSeconds(7200.0);
    ApproximateTokenBucketClass third = o.ApproximateClasses[0];
    third.ReplenishmentPeriod = TimeSpan::FromSeconds(3600.0);   // shares class 0's timer
    o.ApproximateClasses.push_back(third);
    PartitionedRedisApproximateTokenBucketRateLimiter lim(o);
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
        test_classes_behind_class_of();
        test_auto_replenishment_timers();
    }
    std::printf("approx_classes_test %s: %d checks passed, %d failed\n", gpu ? "gpu" : "cpu", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
