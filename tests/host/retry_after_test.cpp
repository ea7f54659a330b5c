// retry_after_test.cpp -- RetryAfter of the approximate limiter's failed leases (A:390-395)
// through the C++ host classes.  Run by tests/test_host_retry_after.py on the GPU.
//
//   1. Decision-time values: several threads submit to one limiter so that a micro-batch
//      holds a failing request followed by a granted one.  The OnBatch trace gives every
//      batch in arrival order; a model of the key's local score walks it, and each failed
//      lease's RetryAfter must be the formula at its own position in the trace (the value
//      read from the key's state after the batch would be larger).
//   2. No per-key query: a micro-batch of 20,000 denied requests completes with every
//      lease's RetryAfter equal to the formula and without one tbe_approx_query call.  This
//      program defines tbe_approx_query itself (the dynamic linker resolves libtbe_host.so's
//      calls to the executable first) and counts the calls before passing them on.
//      RedisApproximateTokenBucketRateLimiter has one bucket (A:9-599: BucketId is the
//      instance name), so the 20,000 requests are on that one throttled key; distinct keys
//      are covered at the C ABI by tests/test_gpu_approx_retry.py.
#include <dlfcn.h>

#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <future>
#include <mutex>
#include <thread>
#include <vector>

#include "rate_limiting.hpp"
#include "tbe.h"

using namespace tbe::rate_limiting;

static std::atomic<uint64_t> g_query_calls{0};

extern "C" tbe_status tbe_approx_query(tbe_engine *engine, uint64_t key, int32_t *local, int32_t *global_score,
                                       double *est, int32_t *available, uint32_t *queued) {
    using Fn = tbe_status (*)(tbe_engine *, uint64_t, int32_t *, int32_t *, double *, int32_t *, uint32_t *);
    static Fn real = reinterpret_cast<Fn>(dlsym(RTLD_NEXT, "tbe_approx_query"));
    g_query_calls.fetch_add(1);
    return real ? real(engine, key, local, global_score, est, available, queued) : TBE_EINVAL;
}

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

// A:390-395 with global 0 (no refresh has run) and nothing queued
static int64_t formula_ticks(int64_t local, int32_t p, int32_t limit, double rate) {
    int64_t deficit = (int32_t)((uint32_t)local + (uint32_t)p - (uint32_t)limit);
    if (deficit < 0) deficit = 0;
    const double s = (double)deficit * rate;
    return (int64_t)(s * 1e7);
}

static RedisApproximateTokenBucketRateLimiterOptions options(int limit, int per_period) {
    RedisApproximateTokenBucketRateLimiterOptions o;
    o.TokenLimit = limit;
    o.TokensPerPeriod = per_period;
    o.ReplenishmentPeriod = TimeSpan::FromSeconds(1.0);
    o.InstanceName = "approx:";
    o.Device = 0;
    o.AutoReplenishment = false;
    o.TimeSource = [] { return T0; };
    return o;
}

// ---- 1. decision-time values
static void test_decision_time_values() {
    constexpr int kThreads = 8, kLimit = 20, kRounds = 100;
    // thread t asks for permits[t] every time: distinct, so a request in the trace names its
    // thread (a thread has one request in flight); 40 in all against TokenLimit 20
    const int32_t permits[kThreads] = {9, 1, 8, 2, 7, 3, 6, 4};
    int batches_with_grant_after_failure = 0, failed_leases = 0, moved = 0;
    for (int round = 0; round < kRounds && batches_with_grant_after_failure == 0; ++round) {
        RedisApproximateTokenBucketRateLimiterOptions o = options(kLimit, 10);
        const double rate = o.FillRatePerSecond();
        int64_t local = 0;                       // the model: submitter thread only (OnBatch)
        int64_t expected[kThreads];              // per thread: ticks of its request (-1: not failed)
        int64_t after_batch[kThreads];           // what the key's state after the batch would give
        int seen = 0;
        o.OnBatch = [&](const BatchTrace &b) {
            if (b.mode != kApproxAttempt) return;
            bool failure = false, grant_after_failure = false;
            std::vector<int> failed_here;
            for (uint64_t i = 0; i < b.n; ++i) {
                int t = 0;
                while (t < kThreads && permits[t] != b.permits[i]) ++t;
                if (t == kThreads) continue;
                if (b.status[i] == TBE_WAIT_GRANTED) {
                    expected[t] = -1;
                    local += b.permits[i];
                    grant_after_failure |= failure;
                } else if (b.status[i] == TBE_WAIT_FAILED) {
                    expected[t] = formula_ticks(local, b.permits[i], kLimit, rate);
                    failed_here.push_back(t);
                    failure = true;
                }
            }
            for (int t : failed_here) after_batch[t] = formula_ticks(local, permits[t], kLimit, rate);
            seen += grant_after_failure;
        };
        RedisApproximateTokenBucketRateLimiter lim(o);
        std::mutex mu;
        std::condition_variable cv;
        int ready = 0;
        bool go = false;
        std::vector<std::thread> th;
        std::atomic<int> bad{0}, nfailed{0}, nmoved{0};
        for (int t = 0; t < kThreads; ++t)
            th.emplace_back([&, t] {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    ++ready;
                    cv.notify_all();
                    cv.wait(lk, [&] { return go; });
                }
                for (int rep = 0; rep < 2; ++rep) {
                    RateLimitLease lease = lim.AttemptAcquire(permits[t]);
                    TimeSpan ra;
                    if (lease.IsAcquired()) {
                        if (lease.TryGetRetryAfter(ra)) ++bad;
                    } else {
                        ++nfailed;
                        // (expected[t] was written by the submitter before it completed the lease)
                        if (!lease.TryGetRetryAfter(ra) || ra.ticks != expected[t]) ++bad;
                        if (expected[t] != after_batch[t]) ++nmoved;
                    }
                }
            });
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return ready == kThreads; });
            go = true;
            cv.notify_all();
        }
        for (auto &x : th) x.join();
        lim.Dispose();
        CHECK(bad.load() == 0);
        CHECK(local <= kLimit);
        failed_leases += nfailed.load();
        moved += nmoved.load();
        batches_with_grant_after_failure += seen;
    }
    std::printf("decision-time: %d failed leases checked, %d batches with a grant after a failure, "
                "%d leases whose value differs from the key's state after the batch\n",
                failed_leases, batches_with_grant_after_failure, moved);
    CHECK(failed_leases > 0);
    CHECK(batches_with_grant_after_failure >= 1);   // else the pattern never produced the case
    CHECK(moved >= 1);
}

// ---- 2. a denial-heavy micro-batch makes no tbe_approx_query call
static void test_no_per_key_query() {
    constexpr int kLimit = 20, kN = 20000;
    RedisApproximateTokenBucketRateLimiterOptions o = options(kLimit, 10);
    const double rate = o.FillRatePerSecond();
    o.QueueLimit = 0;                            // a wait that cannot lease fails (A:159-163)
    std::mutex mu;
    std::condition_variable cv;
    bool blocked = false, release = false;
    uint64_t largest = 0;
    o.OnBatch = [&](const BatchTrace &b) {       // the first batch holds the submitter until all are enqueued
        std::unique_lock<std::mutex> lk(mu);
        largest = std::max(largest, b.n);
        if (blocked) return;
        blocked = true;
        cv.notify_all();
        cv.wait(lk, [&] { return release; });
    };
    RedisApproximateTokenBucketRateLimiter lim(o);
    auto first = lim.AcquireAsync(kLimit);       // takes every token: the key is throttled
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return blocked; });
    }
    std::vector<std::future<RateLimitLease>> fs;
    fs.reserve(kN);
    for (int i = 0; i < kN; ++i) fs.push_back(lim.AcquireAsync(1 + i % kLimit));
    const uint64_t before = g_query_calls.load();
    {
        std::lock_guard<std::mutex> lk(mu);
        release = true;
    }
    cv.notify_all();
    CHECK(first.get().IsAcquired());
    int wrong = 0;
    for (int i = 0; i < kN; ++i) {
        RateLimitLease l = fs[i].get();
        TimeSpan ra;
        // local 20: deficit = 20 + p - 20 = p
        if (l.IsAcquired() || !l.TryGetRetryAfter(ra) || ra.ticks != formula_ticks(kLimit, 1 + i % kLimit, kLimit, rate))
            ++wrong;
    }
    const uint64_t during = g_query_calls.load() - before;
    std::printf("no per-key query: largest micro-batch %llu, %d wrong leases, %llu tbe_approx_query calls\n",
                (unsigned long long)largest, wrong, (unsigned long long)during);
    CHECK(wrong == 0);
    CHECK(largest == (uint64_t)kN);              // they were one micro-batch
    CHECK(during == 0);
    // the counter does see the host's queries: GetAvailablePermits makes one (A:81)
    const uint64_t q0 = g_query_calls.load();
    CHECK(lim.GetAvailablePermits() == 0);
    CHECK(g_query_calls.load() == q0 + 1);
}

int main() {
    test_decision_time_values();
    test_no_per_key_query();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
