// rate_limiting.hpp -- C++ host mirror of the reference's limiter API over the tbe C ABI.
//
// The reference (C#, net7.0) exposes System.Threading.RateLimiting limiters whose every
// decision is one StackExchange.Redis ScriptEvaluateAsync call (TB:63, PTB:42, A:439).
// There is no .NET toolchain in this image, so the host side above include/tbe.h is this
// C++ library: the same classes, option names, argument meaning and error behaviour,
// with the per-request script call replaced by a micro-batching submitter thread that
// turns concurrent callers into one batched engine call (arrival order = batch order,
// the order Redis would serialise the scripts in).  INTEGRATION.md shows the equivalent
// C# P/Invoke binding.
//
// Mapping (reference file:line -> here)
//   RedisTokenBucketRateLimiter            TokenBucket/RedisTokenBucketRateLimiter.cs:7-212
//   PartitionedRedisTokenBucketRateLimiter TokenBucket/PartitionedRedisTokenBucketRateLimiter.cs:7-212
//   RedisQueueingTokenBucketRateLimiter    TokenBucketWithQueue/RedisTokenBucketRateLimiter.cs:9-400
//   RedisApproximateTokenBucketRateLimiter ApproximateTokenBucket/RedisApproximateTokenBucketRateLimiter.cs:9-599
//   PartitionedRedisApproximateTokenBucketRateLimiter   the reference README's second TODO (no file upstream)
//   PartitionedRedisQueueingTokenBucketRateLimiter      Q:9-400 behind the partitioner of PTB:42 (no file upstream)
//   *Options                               */Redis*Options.cs (TBO:9-85, QO, AO)
//   ServiceCollection::AddRedis*           ServiceCollectionExtensions.cs:10-26
// Method names follow the GA System.Threading.RateLimiting API (AttemptAcquire /
// AcquireAsync); the preview-5 names the reference overrides (AcquireCore /
// WaitAsyncCore) are the protected *Core virtuals.
#pragma once

#include <atomic>
#include <cstdint>
#include <functional>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "tbe.h"

namespace tbe::rate_limiting {

// ------------------------------------------------------------------ .NET value types
struct TimeSpan {  // System.TimeSpan: 100 ns ticks
    static constexpr int64_t TicksPerSecond = 10'000'000;
    int64_t ticks = 0;
    static TimeSpan FromTicks(int64_t t) { return TimeSpan{t}; }
    static TimeSpan FromSeconds(double s);
    static TimeSpan FromMilliseconds(double ms) { return FromSeconds(ms / 1000.0); }
    double TotalSeconds() const { return (double)ticks / (double)TicksPerSecond; }
    bool operator<(const TimeSpan &o) const { return ticks < o.ticks; }
    bool operator==(const TimeSpan &o) const { return ticks == o.ticks; }
};

// Exceptions with the .NET names the reference throws (TB:24-42, A:87-90, TB:158-164).
struct ArgumentException : std::invalid_argument {
    std::string ParamName;
    ArgumentException(const std::string &msg, std::string param)
        : std::invalid_argument(msg), ParamName(std::move(param)) {}
};
struct ArgumentNullException : ArgumentException {
    using ArgumentException::ArgumentException;
};
struct ArgumentOutOfRangeException : ArgumentException {
    using ArgumentException::ArgumentException;
};
struct ObjectDisposedException : std::logic_error {
    using std::logic_error::logic_error;
};
// An engine (device) error surfacing through a decision: the counterpart of a
// RedisException propagating out of ScriptEvaluateAsync (TB:63).
struct RateLimiterEngineException : std::runtime_error {
    tbe_status Status;
    RateLimiterEngineException(tbe_status st, const std::string &msg)
        : std::runtime_error(msg), Status(st) {}
};

// TaskCanceledException of a canceled queued wait (CancelQueueState.TrySetCanceled,
// Q:480-506, A:531-557).
struct OperationCanceledException : std::runtime_error {
    OperationCanceledException() : std::runtime_error("The operation was canceled.") {}
};

// System.Threading.CancellationToken / CancellationTokenSource, reduced to what the
// limiters use: CanBeCanceled, IsCancellationRequested and Register (callbacks run once,
// on the thread that calls Cancel, or at once when registered after it).
class CancellationToken {
public:
    CancellationToken() = default;  // CancellationToken.None
    bool CanBeCanceled() const { return (bool)s_; }
    bool IsCancellationRequested() const;
    // Returns a registration handle (0: nothing registered -- CancellationToken.None, or
    // already canceled, in which case fn has run).  Unregister(handle) removes a callback
    // that has not run (CancellationTokenRegistration.Dispose, Q:263, Q:303).
    uint64_t Register(std::function<void()> fn) const;
    void Unregister(uint64_t handle) const;
    size_t RegisteredCount() const;  // diagnostics (tests)
private:
    friend class CancellationTokenSource;
    struct State {
        std::mutex mu;
        bool canceled = false;
        uint64_t next = 1;
        std::map<uint64_t, std::function<void()>> callbacks;
    };
    explicit CancellationToken(std::shared_ptr<State> s) : s_(std::move(s)) {}
    std::shared_ptr<State> s_;
};

class CancellationTokenSource {
public:
    CancellationTokenSource() : s_(std::make_shared<CancellationToken::State>()) {}
    CancellationToken Token() const { return CancellationToken(s_); }
    bool IsCancellationRequested() const { return Token().IsCancellationRequested(); }
    void Cancel();
private:
    std::shared_ptr<CancellationToken::State> s_;
};

enum class QueueProcessingOrder { OldestFirst = 0, NewestFirst = 1 };

// RateLimitLease (the reference's private Lease classes, e.g. A:559-598).  Token-bucket
// leases hold nothing to give back, so a lease is a value.
class RateLimitLease {
public:
    explicit RateLimitLease(bool acquired, std::optional<TimeSpan> retry_after = std::nullopt)
        : acquired_(acquired), retry_after_(retry_after) {}
    bool IsAcquired() const { return acquired_; }
    std::vector<std::string> MetadataNames() const;                  // {"RETRY_AFTER"} (A:561)
    bool TryGetRetryAfter(TimeSpan &out) const;                      // MetadataName.RetryAfter
    std::string ToString() const;                                    // A:587-597
private:
    bool acquired_;
    std::optional<TimeSpan> retry_after_;
};

// System.Threading.RateLimiting.RateLimiterStatistics (the GA surface: GetStatistics()
// replaced GetAvailablePermits).  The two totals are counted on the device per key
// (TBE_FLAG_STATS): a granted lease, at once or at a replenish tick, is
// successful; a failed one and a queued one evicted by a newer request are failed; a canceled
// wait and an ArgumentOutOfRangeException count nothing.
struct RateLimiterStatistics {
    int64_t CurrentAvailablePermits = 0;
    int64_t CurrentQueuedCount = 0;      // _queueCount: the queued permits
    int64_t TotalFailedLeases = 0;
    int64_t TotalSuccessfulLeases = 0;
};

// The role of Redis TIME (TB:202): microseconds since the Unix epoch.  Injectable so
// tests can drive the limiters deterministically.
using Clock = std::function<int64_t()>;
int64_t SystemClockMicros();

// Diagnostic hook: every engine call the submitter makes, with its inputs and replies
// (status: 0/1 granted for the token bucket, TBE_WAIT_* otherwise).
struct BatchTrace {
    int mode;  // BatchMode
    uint64_t n;
    const uint64_t *keys;
    const int32_t *permits;
    const int64_t *ts_us;
    const uint8_t *status;
    const int32_t *remaining;
};
enum BatchMode { kTbAcquire = 0, kQueueWait = 1, kQueueAttempt = 2, kApproxWait = 3, kApproxAttempt = 4 };

// ------------------------------------------------------------------ options
// RedisTokenBucketRateLimiterOptions (TBO:9-85).  The Redis connection settings
// (Configuration, ConfigurationOptions, ConnectionMultiplexerFactory, ProfilingSession)
// become the engine settings below: the "connection" is a GPU.
// One limit class of a partitioned token-bucket limiter: the three options that the
// reference interpolates into a limiter's script (TB:184-185), so that differently configured
// limiters share one store (per-endpoint policies, plans).
struct TokenBucketClass {
    int TokenLimit = 0;
    int TokensPerPeriod = 0;
    TimeSpan ReplenishmentPeriod = TimeSpan::FromSeconds(1);
};

struct RedisTokenBucketRateLimiterOptions {
    TimeSpan ReplenishmentPeriod = TimeSpan::FromSeconds(1);      // TBO:14-22
    int TokensPerPeriod = 0;                                      // TBO:24-32
    int TokenLimit = 0;                                           // TBO:43
    std::string InstanceName;                                     // TBO:65 (key prefix)
    int Device = -1;               // HIP device ordinal (-1: current)
    uint64_t PartitionLimit = 1u << 20;  // partitioned limiters: distinct resource ids
    uint64_t MaxBatch = 1u << 16;  // largest micro-batch one engine call takes
    Clock TimeSource;              // default SystemClockMicros
    std::function<void(const BatchTrace &)> OnBatch;  // diagnostics (tests)
    // Lease statistics: the engine counts every key's successful and failed leases on the
    // device (16 B per key) and GetStatistics() reports them; false: GetStatistics() returns
    // nullopt and nothing is counted or allocated.
    bool TrackStatistics = false;
    // PartitionedRedisTokenBucketRateLimiter only (every other limiter throws
    // ArgumentException when Classes is non-empty): the extra limit classes 1, 2, ...; class 0
    // is the three options above.  ClassOf is the partitioner of PartitionedRateLimiter.Create:
    // called when a resourceID takes a key (a key reused after ReclaimExpired included), its
    // result in [0, Classes.size()] is that bucket's class; anything else throws
    // ArgumentOutOfRangeException to that caller and assigns no key.  Without ClassOf every
    // resourceID is in class 0.
    std::vector<TokenBucketClass> Classes;
    std::function<int(const std::string &resourceID)> ClassOf;
    double FillRatePerSecond() const;                             // TBO:82-85
};

// One limit class of a partitioned queueing limiter: the five options the reference
// interpolates into a limiter's script and keeps in its object (Q:405-461, TB:184-185), so that
// differently configured limiters share one store.
struct QueueingTokenBucketClass {
    int TokenLimit = 0;
    int TokensPerPeriod = 0;
    TimeSpan ReplenishmentPeriod = TimeSpan::FromSeconds(1);
    int QueueLimit = 0;
    ::tbe::rate_limiting::QueueProcessingOrder QueueProcessingOrder =
        ::tbe::rate_limiting::QueueProcessingOrder::OldestFirst;
};

// One refresh as the engine was asked for it (diagnostics, tests): its time and the classes it
// covered (bit c of ClassMask[c >> 6]: class c; all ones: every class, the unmasked call).
struct RefreshTrace {
    int64_t ts_us;
    uint64_t ClassMask[4];
};

// RedisQueueingTokenBucketRateLimiterOptions (TokenBucketWithQueue/...Options.cs).
struct RedisQueueingTokenBucketRateLimiterOptions : RedisTokenBucketRateLimiterOptions {
    int QueueLimit = 0;
    ::tbe::rate_limiting::QueueProcessingOrder QueueProcessingOrder =
        ::tbe::rate_limiting::QueueProcessingOrder::OldestFirst;
    // PartitionedRedisQueueingTokenBucketRateLimiter only (every other limiter throws
    // ArgumentException when it is non-empty): the extra limit classes 1, 2, ...; class 0 is the
    // five options of this struct.  ClassOf (inherited) is the partitioner, with the rules it has
    // on the partitioned token-bucket limiter.  (The inherited three-field Classes stays the
    // token bucket's and is refused by every queueing limiter.)
    std::vector<QueueingTokenBucketClass> QueueingClasses;
    std::function<void(const RefreshTrace &)> OnRefresh;  // diagnostics (tests): every replenish tick / refresh
    // Timer-driven replenishment every ReplenishmentPeriod (the reference's timer);
    // false: call TryReplenish() yourself (as System.Threading.RateLimiting allows).
    bool AutoReplenishment = true;
    // Approximate limiter only: queue entries per key kept for zero-permit waits, which
    // the reference queues without bound while throttled (A:127-181; include/tbe.h).
    int ZeroWaitSlots = 4;
};

// One limit class of a partitioned approximate limiter: the five options the reference
// interpolates into a limiter's sync script and keeps in its object (A:224, A:241-270, A:37,
// A:141-158), so that differently configured limiters share one store.
// ZeroWaitSlots stays one option of the limiter.
struct ApproximateTokenBucketClass {
    int TokenLimit = 0;
    int TokensPerPeriod = 0;
    TimeSpan ReplenishmentPeriod = TimeSpan::FromSeconds(1);
    int QueueLimit = 0;
    ::tbe::rate_limiting::QueueProcessingOrder QueueProcessingOrder =
        ::tbe::rate_limiting::QueueProcessingOrder::OldestFirst;
};

// RedisApproximateTokenBucketRateLimiterOptions (ApproximateTokenBucket/...Options.cs).
struct RedisApproximateTokenBucketRateLimiterOptions : RedisQueueingTokenBucketRateLimiterOptions {
    // PartitionedRedisApproximateTokenBucketRateLimiter only (the non-partitioned limiter throws
    // ArgumentException when it is non-empty): the extra limit classes 1, 2, ...; class 0 is the
    // five options above.  ClassOf (inherited) is the partitioner, with the rules it has on the
    // partitioned token-bucket limiter.  (The inherited three-field Classes stays the token
    // bucket's and is refused here.)
    std::vector<ApproximateTokenBucketClass> ApproximateClasses;
};

// ------------------------------------------------------------------ base classes
class RateLimiter {  // System.Threading.RateLimiting.RateLimiter
public:
    virtual ~RateLimiter() = default;
    virtual std::optional<TimeSpan> IdleDuration() const = 0;
    virtual int GetAvailablePermits() = 0;
    // nullopt unless the limiter was built with TrackStatistics.  CurrentAvailablePermits is
    // GetAvailablePermits(); the other three come from the device through the submitter's
    // queue, so they include every request submitted before the call.
    virtual std::optional<RateLimiterStatistics> GetStatistics() { return std::nullopt; }
    // Base-class argument validation: permitCount < 0 -> ArgumentOutOfRangeException.
    RateLimitLease AttemptAcquire(int permitCount = 1);
    // A queued request whose token is canceled completes with OperationCanceledException
    // (A:166-175); a request decided at once ignores the token, as in the reference.
    std::future<RateLimitLease> AcquireAsync(int permitCount = 1, CancellationToken ct = {});
    void Dispose() { DisposeCore(); }
protected:
    virtual RateLimitLease AttemptAcquireCore(int permitCount) = 0;
    virtual std::future<RateLimitLease> AcquireAsyncCore(int permitCount, const CancellationToken &ct) = 0;
    virtual void DisposeCore() = 0;
};

template <class TResource>
class PartitionedRateLimiter {  // System.Threading.RateLimiting.PartitionedRateLimiter<T>
public:
    virtual ~PartitionedRateLimiter() = default;
    virtual int GetAvailablePermits(const TResource &resource) = 0;
    // As RateLimiter::GetStatistics, for one resource.  A resource that holds no key reads
    // {GetAvailablePermits(resource), 0, 0, 0} and takes no key.
    virtual std::optional<RateLimiterStatistics> GetStatistics(const TResource &) { return std::nullopt; }
    RateLimitLease AttemptAcquire(const TResource &resource, int permitCount = 1) {
        if (permitCount < 0) throw ArgumentOutOfRangeException("permitCount must be >= 0", "permitCount");
        return AttemptAcquireCore(resource, permitCount);
    }
    std::future<RateLimitLease> AcquireAsync(const TResource &resource, int permitCount = 1,
                                             CancellationToken ct = {}) {
        if (permitCount < 0) throw ArgumentOutOfRangeException("permitCount must be >= 0", "permitCount");
        return AcquireAsyncCore(resource, permitCount, ct);
    }
    void Dispose() { DisposeCore(); }
protected:
    virtual RateLimitLease AttemptAcquireCore(const TResource &resource, int permitCount) = 0;
    virtual std::future<RateLimitLease> AcquireAsyncCore(const TResource &resource, int permitCount,
                                                         const CancellationToken &ct) = 0;
    virtual void DisposeCore() = 0;
};

namespace detail {
class LimiterCore;  // engine + key directory + submitter thread (rate_limiting.cpp)
}

// ------------------------------------------------------------------ token bucket
// TB:7-212.  One bucket (BucketId = InstanceName).  AttemptAcquire runs the real decision
// (the reference's AcquireCore is a stub returning FailedLease, TB:53-56).
class RedisTokenBucketRateLimiter final : public RateLimiter {
public:
    explicit RedisTokenBucketRateLimiter(const RedisTokenBucketRateLimiterOptions &options);
    ~RedisTokenBucketRateLimiter() override;
    std::optional<TimeSpan> IdleDuration() const override { return std::nullopt; }  // TB:20
    int GetAvailablePermits() override;                                               // TB:48-51
    std::optional<RateLimiterStatistics> GetStatistics() override;
protected:
    RateLimitLease AttemptAcquireCore(int permitCount) override;
    std::future<RateLimitLease> AcquireAsyncCore(int permitCount, const CancellationToken &ct) override;          // TB:58-82
    void DisposeCore() override;                                                      // TB:85-109
private:
    std::unique_ptr<detail::LimiterCore> core_;
};

// PTB:7-212.  BucketId = InstanceName + resourceID (PTB:42), mapped to a dense key.
// GetAvailablePermits(resourceID) reports the last script reply for that bucket (the
// reference returns 0, PTB:25-28); for a resourceID that holds no key, the TokenLimit of its
// class (ClassOf), without assigning a key.
class PartitionedRedisTokenBucketRateLimiter final : public PartitionedRateLimiter<std::string> {
public:
    explicit PartitionedRedisTokenBucketRateLimiter(const RedisTokenBucketRateLimiterOptions &options);
    ~PartitionedRedisTokenBucketRateLimiter() override;
    int GetAvailablePermits(const std::string &resourceID) override;
    std::optional<RateLimiterStatistics> GetStatistics(const std::string &resourceID) override;
    // Frees the keys of buckets Redis would have expired (TB:232-235) for new resource
    // ids; runs by itself when all PartitionLimit keys are taken.  Returns the number freed.
    uint64_t ReclaimExpired();
protected:
    RateLimitLease AttemptAcquireCore(const std::string &resourceID, int permitCount) override;
    std::future<RateLimitLease> AcquireAsyncCore(const std::string &resourceID, int permitCount,
                                                 const CancellationToken &ct) override;
    void DisposeCore() override;
private:
    std::unique_ptr<detail::LimiterCore> core_;
};

// ------------------------------------------------------------------ token bucket with queue
// Q:9-400 (commented out upstream; semantics fixed in DESIGN.md §2b).  WaitAsync leases,
// else queues (QueueLimit, QueueProcessingOrder), and queued requests complete at the
// replenish ticks.
class RedisQueueingTokenBucketRateLimiter final : public RateLimiter {
public:
    explicit RedisQueueingTokenBucketRateLimiter(const RedisQueueingTokenBucketRateLimiterOptions &options);
    ~RedisQueueingTokenBucketRateLimiter() override;
    std::optional<TimeSpan> IdleDuration() const override { return std::nullopt; }  // Q:29
    int GetAvailablePermits() override;                                               // Q:57-60
    std::optional<RateLimiterStatistics> GetStatistics() override;
    bool TryReplenish();  // one replenish tick now; false when AutoReplenishment is on
protected:
    RateLimitLease AttemptAcquireCore(int permitCount) override;
    std::future<RateLimitLease> AcquireAsyncCore(int permitCount, const CancellationToken &ct) override;          // Q:67-134
    void DisposeCore() override;
private:
    std::unique_ptr<detail::LimiterCore> core_;
};

// One queueing limiter per resourceID (BucketId = InstanceName + resourceID, as PTB:42), all
// of them in one engine with queueing limit classes (tbe_create_queue_classes): each name has
// its own bucket row and queue, and is decided with the five options of its class
// (Options.QueueingClasses, Options.ClassOf).  AttemptAcquire is Q:136-165, AcquireAsync
// Q:67-134; a queued lease completes at the replenish tick of its class.
class PartitionedRedisQueueingTokenBucketRateLimiter final : public PartitionedRateLimiter<std::string> {
public:
    explicit PartitionedRedisQueueingTokenBucketRateLimiter(const RedisQueueingTokenBucketRateLimiterOptions &options);
    ~PartitionedRedisQueueingTokenBucketRateLimiter() override;
    // The last script reply for a name that holds a key; for one that does not, the TokenLimit of
    // ClassOf(name), without assigning a key.
    int GetAvailablePermits(const std::string &resourceID) override;
    std::optional<RateLimiterStatistics> GetStatistics(const std::string &resourceID) override;
    // one replenish tick (Q:237-271) of every name of every class now; false when
    // AutoReplenishment is on
    bool TryReplenish();
    // AutoReplenishment runs one timer per distinct ReplenishmentPeriod among the classes, as the
    // reference runs one timer per limiter object: each drains only the names of the classes of
    // its period (tbe_refresh_classes).  ReplenishmentTimers lists them (period, classes), in the
    // order of each period's first class.
    std::vector<std::pair<TimeSpan, std::vector<int>>> ReplenishmentTimers() const;
    // What timer `index` does at its tick, now (for a host that drives time itself, and tests).
    void TickTimer(size_t index);
    // Frees the keys of buckets Redis would have expired (TB:232-235, by each name's class) for
    // new resource ids; a name with a queued wait keeps its key.  Runs by itself when all
    // PartitionLimit keys are taken.  Returns the number freed.
    uint64_t ReclaimExpired();
protected:
    RateLimitLease AttemptAcquireCore(const std::string &resourceID, int permitCount) override;   // Q:136-165
    std::future<RateLimitLease> AcquireAsyncCore(const std::string &resourceID, int permitCount,
                                                 const CancellationToken &ct) override;           // Q:67-134
    void DisposeCore() override;
private:
    std::unique_ptr<detail::LimiterCore> core_;
};

// ------------------------------------------------------------------ approximate
// A:9-599.  Local tier per instance, periodically synced with the global tier.  This
// limiter is the only client of its engine's global-tier replica; multi-client (multi-GPU)
// sync goes through the cluster layer (cluster.py approx_epoch over RCCL).
class RedisApproximateTokenBucketRateLimiter final : public RateLimiter {
public:
    explicit RedisApproximateTokenBucketRateLimiter(const RedisApproximateTokenBucketRateLimiterOptions &options);
    ~RedisApproximateTokenBucketRateLimiter() override;
    std::optional<TimeSpan> IdleDuration() const override;                            // A:34
    int GetAvailablePermits() override;                                               // A:81
    std::optional<RateLimiterStatistics> GetStatistics() override;
    bool TryReplenish();  // one RefreshAsync (A:412-508) now; false when AutoReplenishment is on
    std::string ToString();                                                           // A:510-513
protected:
    RateLimitLease AttemptAcquireCore(int permitCount) override;                     // A:84-113
    std::future<RateLimitLease> AcquireAsyncCore(int permitCount, const CancellationToken &ct) override;          // A:116-183
    void DisposeCore() override;                                                      // A:274-300
private:
    std::unique_ptr<detail::LimiterCore> core_;
};

// The partitioned approximate limiter the reference's README lists as still to do: one
// approximate limiter per resourceID (BucketId = InstanceName + resourceID, as PTB:42), all
// of them in one engine.  Each name has its own local tier, queue and global-tier row; one
// TryReplenish (or timer tick) is one RefreshAsync (A:412-508) of every name.  Failed leases
// carry RetryAfter (A:390-395).  When all PartitionLimit keys are taken the idle names --
// nothing queued, ConsumedTokens == 0 (A:36, A:503-506) and a global row worth no tokens
// now -- give their keys back (ReclaimIdle, which also runs by itself), and a name that
// takes a reused key starts as a newly constructed limiter does (tbe_approx_reset, tbe.h).
class PartitionedRedisApproximateTokenBucketRateLimiter final : public PartitionedRateLimiter<std::string> {
public:
    explicit PartitionedRedisApproximateTokenBucketRateLimiter(
        const RedisApproximateTokenBucketRateLimiterOptions &options);
    ~PartitionedRedisApproximateTokenBucketRateLimiter() override;
    // A:81 for a name that holds a key; for one that does not, the TokenLimit of ClassOf(name)
    // (what its limiter would report once constructed), without assigning a key.
    int GetAvailablePermits(const std::string &resourceID) override;
    std::optional<RateLimiterStatistics> GetStatistics(const std::string &resourceID) override;
    // one RefreshAsync of every name of every class now; false when AutoReplenishment is on
    bool TryReplenish();
    // AutoReplenishment runs one timer per distinct ReplenishmentPeriod among the classes; each
    // refreshes only the names of the classes of its period (tbe_approx_refresh_classes), so
    // that the instance estimate of A:443 divides a class's period by its own sync interval.
    // ReplenishmentTimers lists them (period, classes), in the order of each period's first class.
    std::vector<std::pair<TimeSpan, std::vector<int>>> ReplenishmentTimers() const;
    // What timer `index` does at its tick, now (for a host that drives time itself, and tests).
    void TickTimer(size_t index);
    uint64_t ReclaimIdle();  // frees the keys of idle names; returns the number freed
protected:
    RateLimitLease AttemptAcquireCore(const std::string &resourceID, int permitCount) override;   // A:84-113
    std::future<RateLimitLease> AcquireAsyncCore(const std::string &resourceID, int permitCount,
                                                 const CancellationToken &ct) override;           // A:116-183
    void DisposeCore() override;
private:
    std::unique_ptr<detail::LimiterCore> core_;
};

// ------------------------------------------------------------------ registration
// ServiceCollectionExtensions (SCE:10-26): registers a singleton RateLimiter built from
// configured options.  Resolution constructs it on first use (as the DI container does).
class ServiceCollection {
public:
    ServiceCollection &AddRedisTokenBucketRateLimiter(
        std::function<void(RedisTokenBucketRateLimiterOptions &)> configureOptions);
    ServiceCollection &AddRedisApproximateTokenBucketRateLimiter(
        std::function<void(RedisApproximateTokenBucketRateLimiterOptions &)> configureOptions);
    // GetRequiredService<RateLimiter>(): the last registration wins (MS.DI semantics).
    std::shared_ptr<RateLimiter> GetRequiredRateLimiter();
private:
    std::mutex mu_;
    std::function<std::shared_ptr<RateLimiter>()> factory_;
    std::shared_ptr<RateLimiter> instance_;
};

}  // namespace tbe::rate_limiting
