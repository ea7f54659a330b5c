// The RetryAfter arithmetic of csrc/tbe_retry.hpp (what k_fold_a and the final un-partition
// compile) against a plain statement of A:390-395 and TimeSpan.FromSeconds:
//
//   deficit = Math.Max(0, global + local + permits + queued - TokenLimit)   // unchecked int32
//   ticks   = trunc((deficit * rate) * 1e7), OverflowException from 2^63 on
//
// The plain statement sums in int64 and wraps once at the end (two's complement addition is
// associative mod 2^32, so that is C#'s term-by-term wrap) and rounds each product to f64
// through a volatile.  Stand-alone: no engine, no GPU.  Built with
// -fsanitize=address,undefined by tests/test_retry_ticks_host.py.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../distributedratelimiting.redis_amd/csrc/tbe_retry.hpp"

static int64_t wrap32(int64_t x) {
    const int64_t m = ((x % 4294967296LL) + 4294967296LL) % 4294967296LL;
    return m >= 2147483648LL ? m - 4294967296LL : m;
}

static int64_t plain_deficit(int32_t g, int32_t l, int32_t p, uint32_t q, int32_t limit) {
    const int64_t d = wrap32((int64_t)g + l + p + (int64_t)q - limit);
    return d > 0 ? d : 0;
}

// volatile: each product is rounded to f64 before the next one, whatever the optimiser does
static int64_t plain_ticks(int64_t deficit, double rate, bool &overflow) {
    volatile double s = (double)deficit * rate;
    volatile double t = s * 1e7;
    overflow = t >= std::ldexp(1.0, 63);
    return overflow ? 0 : (int64_t)std::trunc(t);
}

static int failed = 0, checked = 0;
static void expect(bool ok, const char *what, long long a, long long b) {
    ++checked;
    if (ok) return;
    ++failed;
    if (failed <= 20) std::printf("FAIL %s: got %lld want %lld\n", what, a, b);
}

int main() {
    const int32_t I32MAX = INT32_MAX, I32MIN = INT32_MIN;
    // deficits: every combination of edge terms, the wrap-around ones included
    const std::vector<int32_t> terms = {0, 1, 2, 3, 5, 19, 20, 21, 16382, 16383, 65535, 1 << 30,
                                        I32MAX - 1, I32MAX, I32MIN, I32MIN + 1, -1, -20};
    const std::vector<uint32_t> queued = {0, 1, 16, 65535};
    const std::vector<int32_t> limits = {1, 20, 16382, 16383, I32MAX};
    for (int32_t g : terms)
        for (int32_t l : terms)
            for (int32_t p : {0, 1, 5, 20, 16383, I32MAX})
                for (uint32_t q : queued)
                    for (int32_t lim : limits) {
                        const uint32_t got = tbe::retry_deficit(g, l, p, q, lim);
                        expect((int64_t)got == plain_deficit(g, l, p, q, lim), "deficit", got,
                               plain_deficit(g, l, p, q, lim));
                    }
    // named cases: no deficit, exactly at the limit, one past the wrap, the largest
    expect(tbe::retry_deficit(0, 3, 5, 0, 20) == 0, "below the limit", tbe::retry_deficit(0, 3, 5, 0, 20), 0);
    expect(tbe::retry_deficit(7, 8, 5, 0, 20) == 0, "at the limit", tbe::retry_deficit(7, 8, 5, 0, 20), 0);
    expect(tbe::retry_deficit(7, 8, 5, 1, 20) == 1, "one over", tbe::retry_deficit(7, 8, 5, 1, 20), 1);
    expect(tbe::retry_deficit(I32MAX, 2, 0, 0, 1) == 0, "sum wraps negative", tbe::retry_deficit(I32MAX, 2, 0, 0, 1), 0);
    expect(tbe::retry_deficit(I32MAX, 21, 0, 0, 20) == 0, "wraps to INT32_MIN", tbe::retry_deficit(I32MAX, 21, 0, 0, 20), 0);
    expect(tbe::retry_deficit(I32MIN, -1, 0, 0, 20) == (uint32_t)I32MAX - 20, "wraps positive",
           tbe::retry_deficit(I32MIN, -1, 0, 0, 20), (long long)I32MAX - 20);
    expect(tbe::retry_deficit(I32MAX, 0, 1, 0, 1) == (uint32_t)I32MAX, "largest", tbe::retry_deficit(I32MAX, 0, 1, 0, 1), I32MAX);

    // ticks: the edge deficits times rates from the slowest to the fastest the options allow
    // (tokens_per_period / period seconds: 1 per ~29,000 years ... (2^31 - 1) per tick), and
    // rates that put deficit * rate * 1e7 right at 2^63
    const std::vector<uint32_t> deficits = {0, 1, 2, 3, 7, 19, 20, 999, 16382, 16383, 65535, 1u << 30,
                                            (uint32_t)I32MAX - 1, (uint32_t)I32MAX};
    std::vector<double> rates = {1.0 / 922337203685.4775807, 1e-9, 1.0 / 3.0, 0.1, 0.3, 1.0, 10.0, 10.0 / 3.0,
                                 12345.678, 1e7, 2147483647.0 * 1e7, 9.223372036854775e11, 9.2233720368547758e11,
                                 9.2233720368547768e11, 4294967296.0 / 10.0, 429.49672979999998, 429.4967298,
                                 429.49672980000003};
    for (uint32_t d : deficits)
        if (d) {   // the rates at which d * rate * 1e7 crosses 2^63, one ulp either side
            const double r = std::ldexp(1.0, 63) / 1e7 / (double)d;
            rates.push_back(r);
            rates.push_back(std::nextafter(r, 0.0));
            rates.push_back(std::nextafter(r, DBL_MAX));
        }
    int overflows = 0, exact_edge = 0;
    for (uint32_t d : deficits)
        for (double r : rates) {
            bool ovf;
            const int64_t want = plain_ticks(d, r, ovf);
            const int64_t got = tbe::retry_ticks(d, r);
            overflows += ovf;
            if (ovf) {
                expect(got == INT64_MAX, "overflow", got, INT64_MAX);
            } else {
                expect(got == want, "ticks", got, want);
                expect(got >= 0 && got != INT64_MAX, "in range", got, want);
            }
            volatile double s2 = (double)d * r;
            volatile double t2 = s2 * 1e7;
            exact_edge += t2 == std::ldexp(1.0, 63);
        }
    expect(tbe::retry_ticks(0, 10.0) == 0, "deficit 0 is 0 ticks", tbe::retry_ticks(0, 10.0), 0);
    expect(tbe::retry_ticks(1, 10.0) == 100000000, "1 * 10/s", tbe::retry_ticks(1, 10.0), 100000000);
    expect(tbe::retry_ticks(3, 0.1) == 3000000, "3 * 0.1 (0.30000000000000004 s)", tbe::retry_ticks(3, 0.1), 3000000);
    expect(tbe::retry_ticks(7, 1.0 / 3.0) == 23333333, "7 / 3 s truncates", tbe::retry_ticks(7, 1.0 / 3.0), 23333333);
    expect(tbe::retry_ticks(1, 2147483647.0 * 1e7) == INT64_MAX, "period 1 tick, 2^31-1 tokens", 0, 0);
    expect(overflows > 50 && exact_edge > 0, "edge coverage", overflows, exact_edge);
    std::printf("%d checks, %d overflow cases, %d exactly at 2^63, %d failed\n", checked, overflows, exact_edge, failed);
    return failed ? 1 : 0;
}
