// partitioned_approx_test.cpp -- PartitionedRedisApproximateTokenBucketRateLimiter through
// the C++ host classes.  Run by tests/test_host_partitioned_approx.py.
//
//   partitioned_approx_test cpu   option validation (no device needed)
//   partitioned_approx_test gpu   PartitionLimit 4: names go idle and give their keys back,
//                                 a queued wait keeps its name, a reused key starts as a
//                                 new limiter, TBE_ERANGE while nothing is idle
//
// The numbers (TokenLimit 5, 2 tokens per 1 s period, injected clock):
//   first refresh   every name's local 2 becomes global 2; the period estimate is 0, so the
//                   instance estimate is infinite and AvailableTokens 0 (SURVEY A.6 warm-up)
//   2 s later       the row decays to max(0, 2 - 2 * 2) = 0: global 0; period 0.2 * 2 = 0.4,
//                   estimate round(1 / 0.4) = 2, cap ceil(5 / 2) = 3
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <future>
#include <string>

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

static RedisApproximateTokenBucketRateLimiterOptions options() {
    RedisApproximateTokenBucketRateLimiterOptions o;
    o.TokenLimit = 5;
    o.TokensPerPeriod = 2;
    o.ReplenishmentPeriod = TimeSpan::FromSeconds(1.0);
    o.QueueLimit = 4;
    o.InstanceName = "papprox:";
    o.Device = 0;
    o.PartitionLimit = 4;
    o.AutoReplenishment = false;
    o.TimeSource = [] { return g_now.load(); };
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

// ---- cpu: the constructor's checks come before the engine is created
static void test_option_validation() {
    using L = PartitionedRedisApproximateTokenBucketRateLimiter;
    auto bad = [](auto edit) {
        RedisApproximateTokenBucketRateLimiterOptions o = options();
        edit(o);
        return throws<ArgumentException>([&] { L lim(o); });
    };
    CHECK(bad([](auto &o) { o.TokenLimit = 0; }));
    CHECK(bad([](auto &o) { o.TokensPerPeriod = 0; }));
    CHECK(bad([](auto &o) { o.QueueLimit = -1; }));
    CHECK(bad([](auto &o) { o.ReplenishmentPeriod = TimeSpan::FromTicks(-1); }));
    CHECK(bad([](auto &o) { o.PartitionLimit = 0; }));
    CHECK(bad([](auto &o) { o.MaxBatch = 0; }));
}

// ---- gpu
static void test_reclaim_idle_names() {
    g_now = T0;
    PartitionedRedisApproximateTokenBucketRateLimiter lim(options());
    // an unknown name reports TokenLimit and takes no key: four more names still fit
    CHECK(lim.GetAvailablePermits("nobody") == 5);
    CHECK(lim.GetAvailablePermits("nobody") == 5);
    for (const char *n : {"a", "b", "c", "d"}) {
        CHECK(lim.AttemptAcquire(n, 2).IsAcquired());
        CHECK(lim.GetAvailablePermits(n) == 3);
    }
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire("a", 6); }));
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire("a", -1); }));
    // all four hold tokens: nothing is idle, a fifth name finds no key
    CHECK(lim.ReclaimIdle() == 0);
    CHECK(throws_erange(lim, "e"));
    CHECK(lim.TryReplenish());                   // local 2 -> global 2, estimate infinite
    CHECK(lim.GetAvailablePermits("a") == 0);
    CHECK(lim.ReclaimIdle() == 0);               // ConsumedTokens 2
    CHECK(throws_erange(lim, "e"));
    RateLimitLease denied = lim.AttemptAcquire("b", 1);
    TimeSpan ra;
    // A:390-395: deficit max(0, 2 + 0 + 1 + 0 - 5) = 0
    CHECK(!denied.IsAcquired() && denied.TryGetRetryAfter(ra) && ra.ticks == 0);
    // a wait for 4 on "a": queued now and still queued after the next refresh (cap 3)
    CancellationTokenSource cts;
    std::future<RateLimitLease> wait_a = lim.AcquireAsync("a", 4, cts.Token());
    g_now = T0 + 2000000;
    CHECK(lim.TryReplenish());                   // rows decay to 0: global 0, estimate 2, cap 3
    CHECK(lim.GetAvailablePermits("a") == 3);
    CHECK(lim.GetAvailablePermits("b") == 3);
    CHECK(wait_a.wait_for(std::chrono::seconds(0)) == std::future_status::timeout);
    // b, c, d are idle; the queued wait keeps a
    CHECK(lim.ReclaimIdle() == 3);
    CHECK(lim.GetAvailablePermits("b") == 5);    // no longer known
    CHECK(lim.GetAvailablePermits("a") == 3);
    // a new name on a reused key is a new limiter: cap TokenLimit, not the old estimate's 3
    CHECK(lim.AttemptAcquire("e", 1).IsAcquired());
    CHECK(lim.GetAvailablePermits("e") == 4);
    CHECK(lim.AttemptAcquire("e", 4).IsAcquired());
    CHECK(lim.GetAvailablePermits("e") == 0);
    CHECK(lim.AttemptAcquire("f", 1).IsAcquired());
    CHECK(lim.AttemptAcquire("g", 5).IsAcquired());
    denied = lim.AttemptAcquire("g", 1);         // deficit 0 + 5 + 1 + 0 - 5 = 1, times the fill rate 2
    CHECK(!denied.IsAcquired() && denied.TryGetRetryAfter(ra) && ra.ticks == 2 * TimeSpan::TicksPerSecond);
    CHECK(throws_erange(lim, "h"));              // a queues, e f g hold tokens
    CHECK(wait_a.wait_for(std::chrono::seconds(0)) == std::future_status::timeout);
    // cancel the wait: "a" is idle now and the reclaim that "h" triggers by itself frees it
    cts.Cancel();
    CHECK(throws<OperationCanceledException>([&] { wait_a.get(); }));
    CHECK(lim.AttemptAcquire("h", 1).IsAcquired());
    CHECK(lim.GetAvailablePermits("h") == 4);
    CHECK(lim.GetAvailablePermits("a") == 5);    // gave its key to h
    CHECK(lim.GetAvailablePermits("e") == 0 && lim.GetAvailablePermits("g") == 0);
    // the reused names sync like new ones: first refresh -> warm-up estimate, then cap again
    CHECK(lim.TryReplenish());
    CHECK(lim.GetAvailablePermits("g") == 0);
    lim.Dispose();
    CHECK(throws<ObjectDisposedException>([&] { lim.AttemptAcquire("a", 1); }));
    CHECK(throws<ObjectDisposedException>([&] { lim.GetAvailablePermits("a"); }));
    CHECK(throws<ObjectDisposedException>([&] { lim.ReclaimIdle(); }));
}

static void test_auto_replenishment_refuses_try_replenish() {
    RedisApproximateTokenBucketRateLimiterOptions o = options();
    o.AutoReplenishment = true;
    o.ReplenishmentPeriod = TimeSpan::FromSeconds(3600.0);
    PartitionedRedisApproximateTokenBucketRateLimiter lim(o);
    CHECK(!lim.TryReplenish());
    CHECK(lim.AttemptAcquire("x", 5).IsAcquired());
    CHECK(!lim.AttemptAcquire("x", 1).IsAcquired());
    lim.Dispose();
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    test_option_validation();
    if (gpu) {
        test_reclaim_idle_names();
        test_auto_replenishment_refuses_try_replenish();
    }
    std::printf("partitioned_approx_test %s: %d checks passed, %d failed\n", gpu ? "gpu" : "cpu", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
