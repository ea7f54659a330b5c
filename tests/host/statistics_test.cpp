// statistics_test.cpp -- GetStatistics() of the C++ host classes (RateLimiterStatistics,
// Options.TrackStatistics).  Run by tests/test_host_statistics.py.
//
//   statistics_test cpu   the struct, the option and the base classes' defaults (no device)
//   statistics_test gpu   hand-checked sequences on all five limiters, on an injected clock
//
// Every limiter here has one token per second; AutoReplenishment is off, so a queued wait
// completes only at a TryReplenish() the test makes.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
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

template <class O>
static O options(int limit, bool track) {
    O o;
    o.TokenLimit = limit;
    o.TokensPerPeriod = 1;
    o.ReplenishmentPeriod = TimeSpan::FromSeconds(1.0);
    o.InstanceName = "stats:";
    o.Device = 0;
    o.PartitionLimit = 1;
    o.TimeSource = [] { return g_now.load(); };
    o.TrackStatistics = track;
    return o;
}
template <class O>
static O queue_options(int limit, int queue_limit, QueueProcessingOrder order) {
    O o = options<O>(limit, true);
    o.QueueLimit = queue_limit;
    o.QueueProcessingOrder = order;
    o.AutoReplenishment = false;
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

static bool is(const std::optional<RateLimiterStatistics> &s, int64_t available, int64_t queued, int64_t failed,
               int64_t ok) {
    if (!s) return false;
    const bool same = s->CurrentAvailablePermits == available && s->CurrentQueuedCount == queued &&
                      s->TotalFailedLeases == failed && s->TotalSuccessfulLeases == ok;
    if (!same)
        std::fprintf(stderr, "  got {%lld, %lld, %lld, %lld}\n", (long long)s->CurrentAvailablePermits,
                     (long long)s->CurrentQueuedCount, (long long)s->TotalFailedLeases,
                     (long long)s->TotalSuccessfulLeases);
    return same;
}
static bool pending(std::future<RateLimitLease> &f) {
    return f.wait_for(std::chrono::seconds(0)) != std::future_status::ready;
}

// ---- cpu
struct PlainLimiter final : RateLimiter {   // overrides nothing of the statistics surface
    std::optional<TimeSpan> IdleDuration() const override { return std::nullopt; }
    int GetAvailablePermits() override { return 7; }
    RateLimitLease AttemptAcquireCore(int) override { return RateLimitLease(true); }
    std::future<RateLimitLease> AcquireAsyncCore(int, const CancellationToken &) override {
        std::promise<RateLimitLease> p;
        p.set_value(RateLimitLease(true));
        return p.get_future();
    }
    void DisposeCore() override {}
};
struct PlainPartitioned final : PartitionedRateLimiter<std::string> {
    int GetAvailablePermits(const std::string &) override { return 7; }
    RateLimitLease AttemptAcquireCore(const std::string &, int) override { return RateLimitLease(true); }
    std::future<RateLimitLease> AcquireAsyncCore(const std::string &, int, const CancellationToken &) override {
        std::promise<RateLimitLease> p;
        p.set_value(RateLimitLease(true));
        return p.get_future();
    }
    void DisposeCore() override {}
};

static void test_defaults() {
    const RateLimiterStatistics s;
    CHECK(s.CurrentAvailablePermits == 0 && s.CurrentQueuedCount == 0);
    CHECK(s.TotalFailedLeases == 0 && s.TotalSuccessfulLeases == 0);
    CHECK(!RedisTokenBucketRateLimiterOptions().TrackStatistics);
    CHECK(!RedisApproximateTokenBucketRateLimiterOptions().TrackStatistics);
    PlainLimiter a;
    PlainPartitioned b;
    CHECK(!a.GetStatistics().has_value());           // nothing that exists has to change
    CHECK(!b.GetStatistics("x").has_value());
}

// ---- gpu
static void test_token_bucket() {
    g_now = T0;
    RedisTokenBucketRateLimiter off(options<RedisTokenBucketRateLimiterOptions>(2, false));
    CHECK(off.AttemptAcquire(1).IsAcquired());
    CHECK(!off.GetStatistics().has_value());         // without TrackStatistics
    RedisTokenBucketRateLimiter lim(options<RedisTokenBucketRateLimiterOptions>(2, true));
    CHECK(lim.AttemptAcquire(1).IsAcquired());
    CHECK(is(lim.GetStatistics(), 1, 0, 0, 1));
    CHECK(lim.AttemptAcquire(1).IsAcquired());
    CHECK(!lim.AttemptAcquire(1).IsAcquired());
    CHECK(!lim.AttemptAcquire(2).IsAcquired());
    CHECK(is(lim.GetStatistics(), 0, 0, 2, 2));
    CHECK(lim.GetStatistics()->CurrentAvailablePermits == lim.GetAvailablePermits());
    g_now = T0 + 1000000;                            // one token back
    CHECK(lim.AttemptAcquire(1).IsAcquired());
    CHECK(is(lim.GetStatistics(), 0, 0, 2, 3));
    lim.Dispose();
    CHECK(throws<ObjectDisposedException>([&] { lim.GetStatistics(); }));
}

static void test_partitioned_token_bucket() {
    g_now = T0;
    PartitionedRedisTokenBucketRateLimiter off(options<RedisTokenBucketRateLimiterOptions>(2, false));
    CHECK(!off.GetStatistics("a").has_value());
    PartitionedRedisTokenBucketRateLimiter lim(options<RedisTokenBucketRateLimiterOptions>(2, true));
    CHECK(is(lim.GetStatistics("unseen"), 2, 0, 0, 0));
    CHECK(lim.AttemptAcquire("a", 1).IsAcquired());   // takes the only key (PartitionLimit 1)
    CHECK(lim.AttemptAcquire("a", 1).IsAcquired());
    CHECK(!lim.AttemptAcquire("a", 1).IsAcquired());
    CHECK(is(lim.GetStatistics("a"), 0, 0, 1, 2));
    // an unseen name reads zeros and takes no key: taking one would have to reclaim, and with
    // a's bucket live that throws
    CHECK(is(lim.GetStatistics("unseen"), 2, 0, 0, 0));
    CHECK(throws<RateLimiterEngineException>([&] { lim.AttemptAcquire("b", 1); }));
    CHECK(is(lim.GetStatistics("a"), 0, 0, 1, 2));
    // T0 + 4 s: a's bucket (EXPIRE 2 s) is gone; c takes its key and reads its own leases only
    g_now = T0 + 4000000;
    CHECK(lim.ReclaimExpired() == 1);
    CHECK(is(lim.GetStatistics("a"), 2, 0, 0, 0));    // holds no key any more
    CHECK(lim.AttemptAcquire("c", 1).IsAcquired());
    CHECK(is(lim.GetStatistics("c"), 1, 0, 0, 1));
    lim.Dispose();
}

static void test_queueing() {
    g_now = T0;
    // OldestFirst, QueueLimit 2: a drained wait is a successful lease, a canceled one is none
    RedisQueueingTokenBucketRateLimiter lim(queue_options<RedisQueueingTokenBucketRateLimiterOptions>(
        2, 2, QueueProcessingOrder::OldestFirst));
    CHECK(lim.AttemptAcquire(2).IsAcquired());
    CHECK(!lim.AttemptAcquire(1).IsAcquired());
    CHECK(is(lim.GetStatistics(), 0, 0, 1, 1));
    std::future<RateLimitLease> w1 = lim.AcquireAsync(1);
    CancellationTokenSource cts;
    std::future<RateLimitLease> w2 = lim.AcquireAsync(1, cts.Token());
    CHECK(lim.GetStatistics()->CurrentQueuedCount == 2);
    CHECK(pending(w1) && pending(w2));
    cts.Cancel();
    CHECK(throws<OperationCanceledException>([&] { w2.get(); }));
    CHECK(is(lim.GetStatistics(), 0, 1, 1, 1));       // the canceled wait counts nowhere
    g_now = T0 + 1000000;
    CHECK(lim.TryReplenish());
    CHECK(w1.get().IsAcquired());
    CHECK(is(lim.GetStatistics(), 0, 0, 1, 2));       // the drained one is a successful lease
    lim.Dispose();
    // NewestFirst, QueueLimit 1: the newer wait evicts the older, which fails
    g_now = T0;
    RedisQueueingTokenBucketRateLimiter nf(queue_options<RedisQueueingTokenBucketRateLimiterOptions>(
        2, 1, QueueProcessingOrder::NewestFirst));
    CHECK(nf.AttemptAcquire(2).IsAcquired());
    std::future<RateLimitLease> e1 = nf.AcquireAsync(1);
    CHECK(nf.GetStatistics()->CurrentQueuedCount == 1);
    std::future<RateLimitLease> e2 = nf.AcquireAsync(1);
    CHECK(!e1.get().IsAcquired());                    // evicted
    CHECK(pending(e2));
    CHECK(is(nf.GetStatistics(), 0, 1, 1, 1));
    nf.Dispose();
}

static void test_approximate() {
    g_now = T0;
    RedisApproximateTokenBucketRateLimiter lim(queue_options<RedisApproximateTokenBucketRateLimiterOptions>(
        3, 2, QueueProcessingOrder::OldestFirst));
    CHECK(is(lim.GetStatistics(), 3, 0, 0, 0));
    CHECK(lim.AttemptAcquire(2).IsAcquired());
    CHECK(!lim.AttemptAcquire(2).IsAcquired());       // one token left
    CHECK(is(lim.GetStatistics(), 1, 0, 1, 1));
    CHECK(lim.GetStatistics()->CurrentAvailablePermits == lim.GetAvailablePermits());
    std::future<RateLimitLease> w = lim.AcquireAsync(2);
    CHECK(is(lim.GetStatistics(), 1, 2, 1, 1));       // queued permits, no lease yet
    CHECK(pending(w));
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire(4); }));
    CHECK(is(lim.GetStatistics(), 1, 2, 1, 1));       // an exception is no lease
    lim.Dispose();
}

static void test_partitioned_approximate() {
    g_now = T0;
    PartitionedRedisApproximateTokenBucketRateLimiter lim(
        queue_options<RedisApproximateTokenBucketRateLimiterOptions>(3, 2, QueueProcessingOrder::OldestFirst));
    CHECK(is(lim.GetStatistics("unseen"), 3, 0, 0, 0));
    CHECK(lim.AttemptAcquire("a", 2).IsAcquired());
    CHECK(!lim.AttemptAcquire("a", 2).IsAcquired());
    CHECK(is(lim.GetStatistics("a"), 1, 0, 1, 1));
    CHECK(is(lim.GetStatistics("unseen"), 3, 0, 0, 0));   // and no key: "a" holds the only one
    CHECK(throws<RateLimiterEngineException>([&] { lim.AttemptAcquire("b", 1); }));
    CHECK(is(lim.GetStatistics("a"), 1, 0, 1, 1));
    lim.Dispose();
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    test_defaults();
    if (gpu) {
        test_token_bucket();
        test_partitioned_token_bucket();
        test_queueing();
        test_approximate();
        test_partitioned_approximate();
    }
    std::printf("statistics_test %s: %d checks passed, %d failed\n", gpu ? "gpu" : "cpu", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
