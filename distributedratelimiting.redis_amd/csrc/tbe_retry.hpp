// RetryAfter of the approximate kind's failed leases (A:390-395):
//
//   deficit    = Math.Max(0, ConsumedTokens + permitCount + _queueCount - TokenLimit)
//   RetryAfter = TimeSpan.FromSeconds(deficit * FillRatePerSecond)
//
// with ConsumedTokens = _globalThrottleScore + _localThrottleScore, all in C# unchecked
// int32.  Host and device: k_fold_a computes the deficit where it decides FAILED, the final
// un-partition turns it into .NET ticks, and the stand-alone program
// tests/host/retry_ticks_test.cpp compares both with a plain statement of the formula.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TBE_RETRY_FN __host__ __device__ __forceinline__
#else
#define TBE_RETRY_FN inline
#endif

namespace tbe {

// The sum wraps as C# int32 arithmetic does (computed unsigned: no signed overflow here).
TBE_RETRY_FN uint32_t retry_deficit(int32_t global, int32_t local, int32_t permits, uint32_t qsum,
                                    int32_t token_limit) {
    const uint32_t sum = (uint32_t)global + (uint32_t)local + (uint32_t)permits + qsum - (uint32_t)token_limit;
    return (int32_t)sum > 0 ? sum : 0u;
}

// TimeSpan.FromSeconds (.NET 7 TimeSpan.Interval): ticks = seconds * 1e7 truncated toward
// zero; OverflowException from 2^63 on (INT64_MAX here: TBE_RETRY_OVERFLOW).  Two f64
// multiplies -- the translation units that include this compile with contraction off, and
// a product of products has nothing to contract anyway.  deficit <= INT32_MAX and the rate
// is finite and positive (tbe_create), so there is no NaN and no negative case.
TBE_RETRY_FN int64_t retry_ticks(uint32_t deficit, double rate) {
    const double s = (double)(int32_t)deficit * rate;
    const double t = s * 10000000.0;
    return t >= 9223372036854775808.0 ? INT64_MAX : (int64_t)t;
}

}  // namespace tbe
