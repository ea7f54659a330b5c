// classes_test.cpp -- limit classes of PartitionedRedisTokenBucketRateLimiter through the C++
// host classes (Options.Classes / Options.ClassOf).  Run by tests/test_host_classes.py.
//
//   classes_test cpu   option validation (no device needed)
//   classes_test gpu   two plans in one limiter, on an injected clock
//
// The numbers:
//   class 0 ("free")  TokenLimit 2, 1 token per 1 s:  rate 1/s,  EXPIRE ceil(max(2 / 1, 1)) = 2 s
//   class 1 ("pro")   TokenLimit 5, 10 tokens per 1 s: rate 10/s, EXPIRE ceil(max(5 / 10, 1)) = 1 s
#include <atomic>
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

static RedisTokenBucketRateLimiterOptions options() {
    RedisTokenBucketRateLimiterOptions o;
    o.TokenLimit = 2;
    o.TokensPerPeriod = 1;
    o.ReplenishmentPeriod = TimeSpan::FromSeconds(1.0);
    o.InstanceName = "plans:";
    o.Device = 0;
    o.PartitionLimit = 3;
    o.TimeSource = [] { return g_now.load(); };
    o.Classes.push_back(TokenBucketClass{5, 10, TimeSpan::FromSeconds(1.0)});
    o.ClassOf = [](const std::string &id) {
        if (id.rfind("pro-", 0) == 0) return 1;
        if (id.rfind("bad-", 0) == 0) return 2;    // one past the last class
        if (id.rfind("neg-", 0) == 0) return -1;
        return 0;
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

// ---- cpu: the constructor's checks come before the engine is created
static void test_option_validation() {
    // only the partitioned token-bucket limiter takes classes
    CHECK(throws<ArgumentException>([] { RedisTokenBucketRateLimiter lim(options()); }));
    auto wide = [] {
        RedisApproximateTokenBucketRateLimiterOptions q;
        static_cast<RedisTokenBucketRateLimiterOptions &>(q) = options();
        q.QueueLimit = 4;
        q.AutoReplenishment = false;
        return q;
    };
    CHECK(throws<ArgumentException>([&] { RedisQueueingTokenBucketRateLimiter lim(wide()); }));
    CHECK(throws<ArgumentException>([&] { RedisApproximateTokenBucketRateLimiter lim(wide()); }));
    CHECK(throws<ArgumentException>([&] { PartitionedRedisApproximateTokenBucketRateLimiter lim(wide()); }));
    // every class gets the constructor's checks
    auto bad = [](auto edit) {
        RedisTokenBucketRateLimiterOptions o = options();
        edit(o);
        return throws<ArgumentException>([&] { PartitionedRedisTokenBucketRateLimiter lim(o); });
    };
    CHECK(bad([](auto &o) { o.Classes[0].TokenLimit = 0; }));
    CHECK(bad([](auto &o) { o.Classes[0].TokensPerPeriod = 0; }));
    CHECK(bad([](auto &o) { o.Classes[0].ReplenishmentPeriod = TimeSpan::FromTicks(-1); }));
    CHECK(bad([](auto &o) { o.Classes[0].ReplenishmentPeriod = TimeSpan::FromTicks(0); }));
    CHECK(bad([](auto &o) { o.Classes.resize(256, o.Classes[0]); }));
}

// ---- gpu
static void test_two_plans() {
    g_now = T0;
    PartitionedRedisTokenBucketRateLimiter lim(options());
    // a name that holds no key reports its class's TokenLimit and takes no key
    CHECK(lim.GetAvailablePermits("unseen") == 2);
    CHECK(lim.GetAvailablePermits("pro-unseen") == 5);
    // free-a, TokenLimit 2: grant, grant, deny
    CHECK(lim.AttemptAcquire("free-a", 1).IsAcquired());
    CHECK(lim.GetAvailablePermits("free-a") == 1);
    CHECK(lim.AttemptAcquire("free-a", 1).IsAcquired());
    CHECK(!lim.AttemptAcquire("free-a", 1).IsAcquired());
    CHECK(lim.GetAvailablePermits("free-a") == 0);
    // pro-b, TokenLimit 5: 3 granted (2 left), 3 denied, 2 granted, 1 denied
    CHECK(lim.AttemptAcquire("pro-b", 3).IsAcquired());
    CHECK(lim.GetAvailablePermits("pro-b") == 2);
    CHECK(!lim.AttemptAcquire("pro-b", 3).IsAcquired());
    CHECK(lim.AttemptAcquire("pro-b", 2).IsAcquired());
    CHECK(!lim.AttemptAcquire("pro-b", 1).IsAcquired());
    // a quarter of a second later: pro-b has 0 + 0.25 * 10 = 2.5 tokens, free-a 0 + 0.25 * 1
    g_now = T0 + 250000;
    CHECK(lim.AttemptAcquire("pro-b", 2).IsAcquired());
    CHECK(lim.GetAvailablePermits("pro-b") == 0);          // trunc(0.5)
    CHECK(!lim.AttemptAcquire("free-a", 1).IsAcquired());
    // a ClassOf result out of range throws to the caller and assigns no key: with two of the
    // three keys held and nothing lapsed, a third name still finds one
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire("bad-x", 1); }));
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.AttemptAcquire("neg-x", 1); }));
    CHECK(throws<ArgumentOutOfRangeException>([&] { lim.GetAvailablePermits("bad-y"); }));
    CHECK(lim.AttemptAcquire("free-c", 2).IsAcquired());
    CHECK(lim.GetAvailablePermits("free-c") == 0);
    // T0 + 1.5 s: pro-b's bucket (last grant T0 + 0.25 s, EXPIRE 1 s) is gone; free-a's (T0,
    // 2 s) and free-c's are not
    g_now = T0 + 1500000;
    CHECK(lim.ReclaimExpired() == 1);
    CHECK(lim.GetAvailablePermits("pro-b") == 5);           // holds no key any more
    CHECK(lim.GetAvailablePermits("free-a") == 0);
    // free-d takes pro-b's key and starts from class 0's full bucket of 2, not from 5
    CHECK(lim.AttemptAcquire("free-d", 1).IsAcquired());
    CHECK(lim.GetAvailablePermits("free-d") == 1);
    CHECK(!lim.AttemptAcquire("free-d", 2).IsAcquired());
    // T0 + 4 s: all three free buckets (EXPIRE 2 s) are gone; a pro name on a reused key
    // starts from 5
    g_now = T0 + 4000000;
    CHECK(lim.ReclaimExpired() == 3);
    CHECK(lim.AttemptAcquire("pro-e", 5).IsAcquired());
    CHECK(lim.GetAvailablePermits("pro-e") == 0);
    CHECK(!lim.AttemptAcquire("pro-e", 1).IsAcquired());
    lim.Dispose();
    CHECK(throws<ObjectDisposedException>([&] { lim.AttemptAcquire("free-a", 1); }));
}

// without ClassOf every name is in class 0, whatever Classes holds
static void test_no_partitioner() {
    g_now = T0;
    RedisTokenBucketRateLimiterOptions o = options();
    o.ClassOf = nullptr;
    PartitionedRedisTokenBucketRateLimiter lim(o);
    CHECK(lim.GetAvailablePermits("pro-x") == 2);
    CHECK(lim.AttemptAcquire("pro-x", 2).IsAcquired());
    CHECK(!lim.AttemptAcquire("pro-x", 1).IsAcquired());
    lim.Dispose();
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    test_option_validation();
    if (gpu) {
        test_two_plans();
        test_no_partitioner();
    }
    std::printf("classes_test %s: %d checks passed, %d failed\n", gpu ? "gpu" : "cpu", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
