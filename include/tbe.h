/*
 * tbe.h -- C ABI of the MI355X batched token-bucket engine ("tbe").
 *
 * This is the drop-in boundary.  In the reference every decision is one
 * StackExchange.Redis script round-trip; the entry points below replace those
 * call sites with batched calls into an HBM-resident bucket table on one GPU.
 * References are to /root/reference/DistributedRateLimiting.Redis/ (aliases as in
 * TB = TokenBucket/RedisTokenBucketRateLimiter.cs, PTB =
 * TokenBucket/PartitionedRedisTokenBucketRateLimiter.cs, TBO = TokenBucket/
 * RedisTokenBucketRateLimiterOptions.cs).
 *
 * Conventions
 *  - Plain pointers and sizes only; no C++ or HIP types cross this boundary.
 *  - Every function returns a tbe_status; no exception ever crosses the ABI.
 *  - An engine is NOT re-entrant: one submitting thread per engine.  Batch order
 *    is arrival order: request i of a batch is decided after request i-1 of the
 *    same batch and after every request of earlier batches (the order Redis
 *    serialises script calls in, TB:63).
 *  - Keys are dense ids in [0, n_keys).  Mapping InstanceName + resourceID
 *    strings (PTB:42) to ids is the caller's job.
 *  - Timestamps are injected microseconds since the Unix epoch (>= 0); they play
 *    the role of Redis `TIME` inside the script (TB:202-203).
 */
#ifndef TBE_H_
#define TBE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TBE_ABI_VERSION 1

typedef enum tbe_status {
    TBE_OK = 0,
    TBE_EINVAL = 1,     /* bad argument / invalid request in a batch (nothing applied):
                           ArgumentException / ArgumentOutOfRangeException (TB:24-42) */
    TBE_ENOMEM = 2,     /* device or host allocation failed */
    TBE_EDEVICE = 3,    /* HIP runtime error; the engine should be destroyed */
    TBE_EDISPOSED = 4,  /* engine already disposed: ObjectDisposedException (TB:158-164) */
    TBE_ERANGE = 5      /* permits > TokenLimit where the limiter forbids it (A:87-90) */
} tbe_status;

typedef enum tbe_kind {
    TBE_KIND_TOKEN_BUCKET = 0,   /* TokenBucket/ (TB, PTB)                                */
    TBE_KIND_QUEUEING = 1,       /* TokenBucketWithQueue/           */
    TBE_KIND_APPROXIMATE = 2     /* ApproximateTokenBucket/        */
} tbe_kind;

/* Limiter options (TBO:9-85) plus engine sizing.  The Redis connection options
 * (Configuration, ConfigurationOptions, ConnectionMultiplexerFactory, TBO:48-60) and
 * the ProfilingSession (TBO:70) have no counterpart: the "connection" is the device. */
typedef struct tbe_config {
    uint32_t struct_size;                 /* sizeof(tbe_config); sizes down to
                                             offsetof(tbe_config, zero_wait_slots) (the first
                                             published layout) are accepted, and the fields
                                             past struct_size read as 0 */
    int32_t kind;                         /* tbe_kind */
    uint64_t n_keys;                      /* table capacity, 1 <= n_keys <= 2^32 */
    int32_t token_limit;                  /* TokenLimit (TBO:43), > 0 */
    int32_t tokens_per_period;            /* TokensPerPeriod (TBO:30), > 0 */
    int64_t replenishment_period_ticks;   /* ReplenishmentPeriod in .NET ticks (100 ns), > 0 */
    int32_t queue_limit;                  /* QueueLimit (queueing kind: 0..65535; ignored otherwise) */
    int32_t queue_order;                  /* 0 = OldestFirst, 1 = NewestFirst */
    int32_t device;                       /* HIP device ordinal; -1 = current device */
    uint32_t flags;                       /* TBE_FLAG_* */
    uint64_t max_batch;                   /* expected largest batch (workspace pre-sizing); 0 = grow on demand */
    int32_t zero_wait_slots;              /* approximate kind: queue entries per key for zero-permit
                                             waits (A:127-181; see tbe_approx_acquire_batch); 0 for
                                             the other kinds.  max(1, queue_limit) + zero_wait_slots
                                             <= 65535 */
    int32_t reserved;                     /* 0 */
} tbe_config;

#define TBE_FLAG_STAGE_TIMING 0x1u        /* record per-stage HIP events (tbe_stage_times) */
#define TBE_FLAG_NO_PACK 0x2u             /* token bucket: keep the wide pass records even where
                                             the packed 8-byte form applies (A/B checks) */
#define TBE_FLAG_NO_HOT 0x4u              /* token bucket: no hot-key runs (A/B checks); keys
                                             that take >= 2048 requests of a batch otherwise get
                                             a run of their own two batches later */
#define TBE_FLAG_NO_PIPELINE 0x8u         /* token bucket: run every stage of a batch on one
                                             stream (A/B checks); by default batch b+1's
                                             partition overlaps batch b's fold */
#define TBE_FLAG_NO_NARROW 0x10u          /* keep 4-byte replies through the fold and the
                                             un-partition passes (A/B checks) instead of the
                                             narrower forms: token bucket 1-byte replies
                                             (packed records, TokenLimit <= 127); queueing kind
                                             1-byte (TokenLimit <= 62) and 2-byte (<= 16382)
                                             replies; approximate kind 2-byte replies
                                             (TokenLimit <= 16382) */
#define TBE_FLAG_UNSCATTER_ALL 0x20u      /* token bucket (A/B checks): the last partition pass
                                             writes plain records and its permutation, and its
                                             own un-partition pass runs.  By default (>= 2
                                             passes, packed records) it writes fold records that
                                             carry each request's position in its input, and the
                                             fold puts every reply straight there */
#define TBE_FLAG_RERANK 0x80u             /* packed records (A/B checks): the final
                                             un-partition re-ranks pass 0's tiles from one-byte
                                             digits the first histogram wrote (k_unrank) instead
                                             of gathering through pass 0's stored permutation:
                                             0.4 GB less traffic per config-B batch, 0.06 ms
                                             slower */
#define TBE_FLAG_FOLD_TIMING 0x100u        /* record HIP events around the fold stage only
                                             (tbe_stage_times reports the fold alone): the
                                             dominant kernel's time at two events per batch
                                             instead of a pair per stage, each event record
                                             leaving the stream idle for microseconds */
#define TBE_FLAG_HIST_RECORDS 0x40u       /* packed records, 2 passes (A/B checks): the second
                                             pass's histogram reads the first pass's 8-byte
                                             records.  By default the first pass also writes each
                                             request's second digit as one byte beside its record,
                                             and that histogram reads those */
#define TBE_FLAG_STATS 0x200u             /* every kind: lease statistics, two
                                             uint64 counters per key (16 B per key, allocated at
                                             create: TBE_ENOMEM when that fails) and two engine
                                             totals, counted on the device behind every batch.
                                             No decision, reply, row or layout changes; without
                                             the flag nothing is allocated or launched for them */

typedef struct tbe_engine tbe_engine;

/* Fill rate the engine computes from the options exactly like FillRatePerSecond
 * (TBO:82-85): (double)tokens_per_period / (ticks / 1e7).  Raw f64, as the script
 * literal `fill_rate` (TB:185) round-trips it. */
double tbe_fill_rate(int32_t tokens_per_period, int64_t replenishment_period_ticks);

/* Replaces the constructor + lazy connect (TB:22-46, TB:111-151).  Allocates the
 * table (16 B per key) on the device, every key absent. */
tbe_status tbe_create(const tbe_config *config, tbe_engine **out_engine);

/* ---- Limit classes: one token-bucket engine, up to 256 differently
 * configured limiters.  In the reference TokenLimit and FillRatePerSecond are interpolated
 * into the script text (TB:184-185), so any number of limiters share one Redis; here every
 * key belongs to one class and is decided by the unchanged script arithmetic with its
 * class's {capacity, fill_rate, EXPIRE seconds}. */
typedef struct tbe_class {
    int32_t token_limit;                  /* TokenLimit (TBO:43), > 0 */
    int32_t tokens_per_period;            /* TokensPerPeriod (TBO:30), > 0 */
    int64_t replenishment_period_ticks;   /* ReplenishmentPeriod in .NET ticks, > 0 */
} tbe_class;

/* tbe_create with extra[0..n_extra) as classes 1..n_extra; class 0 is the config's own
 * three options and every key of a new engine is in class 0.  Each class gets the
 * constructor checks and the parameters tbe_create derives (tbe_fill_rate, then the TB:234
 * clamp).  n_extra == 0 is tbe_create.  TBE_EINVAL, before the device is touched: n_extra >
 * 255, extra == NULL with n_extra > 0, a class that fails the checks, kind !=
 * TBE_KIND_TOKEN_BUCKET.  A classed engine is laid out as with TBE_FLAG_NO_PACK |
 * TBE_FLAG_NO_HOT | TBE_FLAG_NO_NARROW (tbe_layout reports it): wide records, 4-byte
 * replies, no hot-key runs.
 * On a classed engine tbe_query, tbe_expired_device, tbe_export_live(_device) and the
 * fold judge a key's lapse with its class's TTL, and an absent or lapsed row starts from its
 * class's TokenLimit; field v of an absent row (tbe_export_state) is unspecified. */
tbe_status tbe_create_classes(const tbe_config *config, const tbe_class *extra, uint32_t n_extra,
                              tbe_engine **out_engine);

/* The engine's classes, class 0 first: out[0..min(capacity, *n_classes)); out may be NULL.
 * On a queueing engine: the first three options of each of its classes. */
tbe_status tbe_classes(const tbe_engine *engine, tbe_class *out, uint32_t capacity, uint32_t *n_classes);

/* ---- Queueing limit classes: one queueing engine, up to 256 differently
 * configured TokenBucketWithQueue limiters.  A class is the five options of
 * RedisQueueingTokenBucketRateLimiterOptions; the reference interpolates them into each
 * limiter's script text and queue code (Q:405-461, TB:184-185), so any number of limiters
 * share one Redis.  Every request, and every drained entry of a tick, is decided exactly as
 * on a plain engine with the options of its key's class: the REJECTED test (Q:70-73), the
 * script call, the Q:153 test, admission and NewestFirst eviction (Q:92-109), and the head
 * or tail the drain peeks (Q:237-271).  tbe_refresh(_device) and the tick of
 * tbe_wait_batch_tick_device drain every key of every class; the *_classes forms below tick
 * the classes of a mask alone, as each limiter's own timer does in the reference. */
typedef struct tbe_queue_class {
    int32_t token_limit;                  /* TokenLimit (TBO:43), > 0 and < 2^30 - 1 */
    int32_t tokens_per_period;            /* TokensPerPeriod (TBO:30), > 0 */
    int64_t replenishment_period_ticks;   /* ReplenishmentPeriod in .NET ticks, > 0 */
    int32_t queue_limit;                  /* QueueLimit, 0..65535 */
    int32_t queue_order;                  /* 0 = OldestFirst, 1 = NewestFirst */
} tbe_queue_class;                        /* 24 bytes */

/* tbe_create for the queueing kind with extra[0..n_extra) as classes 1..n_extra; class 0 is
 * the config's own five options and every key of a new engine is in class 0.  Each class gets
 * the checks tbe_create makes on the config's options and the parameters it derives
 * (tbe_fill_rate, then the TB:234 clamp).  n_extra == 0 is tbe_create.  TBE_EINVAL, before
 * the device is touched: kind != TBE_KIND_QUEUEING, n_extra > 255, extra == NULL with
 * n_extra > 0, a class that fails a check.
 * Layout: as with TBE_FLAG_NO_PACK | TBE_FLAG_NO_NARROW (wide records, 4-byte replies;
 * tbe_layout bits 0, 3 and 4 clear).  The ring of key k is ring[k*C .. k*C+C), C the largest
 * max(1, QueueLimit) of any class; a key uses the first max(1, QueueLimit) slots of its own
 * class and wraps there.  Queue headers take 32 bits when the largest QueueLimit of any class
 * is <= 1024 (tbe_layout bit 9), else 64.  tbe_refresh_bound is min(entries possibly queued,
 * n_keys * max over classes of min(max(1, QueueLimit), TokenLimit)).
 * tbe_query, tbe_expired_device, tbe_export_live(_device) and `available` of
 * tbe_stats_batch(_device) judge a key by its class's TTL, TokenLimit and fill rate; a key
 * with queued requests is never dead.  tbe_queue_attempt_batch, tbe_queue_cancel,
 * tbe_queue_of, tbe_evicted, TBE_FLAG_STATS counting and the row imports work as on a plain
 * engine. */
tbe_status tbe_create_queue_classes(const tbe_config *config, const tbe_queue_class *extra,
                                    uint32_t n_extra, tbe_engine **out_engine);

/* The classes of a queueing engine with all five options, class 0 first (as tbe_classes);
 * another kind of engine: TBE_EINVAL. */
tbe_status tbe_queue_classes(const tbe_engine *engine, tbe_queue_class *out, uint32_t capacity,
                             uint32_t *n_classes);

/* ---- Approximate limit classes: one approximate engine, up to 256
 * differently configured ApproximateTokenBucket limiters over one global tier.  A class is
 * the five options of tbe_queue_class; zero_wait_slots stays the config's, for every class.
 * The reference interpolates a limiter's options into its sync script and its queue code
 * (A:224, A:241-270, A:37, A:141-158), so any number of limiters share one Redis.  Per class
 * the engine derives what tbe_create derives for the approximate kind: decay_rate =
 * tbe_fill_rate (A:224, A:258), the period in seconds of the instance estimate (A:443) and
 * the ring length max(1, QueueLimit) + zero_wait_slots (<= 65535).  Every request is decided
 * as on a plain engine with the options of its key's class: REJECTED when permits >
 * TokenLimit (A:87-90, A:119-122), the lease test with the class's order (A:191-209),
 * admission and NewestFirst eviction with its QueueLimit (A:141-158); RetryAfter (A:390-395)
 * takes the class's TokenLimit and fill rate; a sync decays, caps, estimates and drains each
 * key with its class's values (A:258, A:37, A:443, A:467-501).  The 86400 s EXPIRE (A:268)
 * does not depend on the class.
 * TBE_EINVAL, before the device is touched: kind != TBE_KIND_APPROXIMATE, n_extra > 255,
 * extra == NULL with n_extra > 0, a class that fails a check tbe_create makes on the
 * config's options (the ring-length bound included).  n_extra == 0 is tbe_create.
 * Layout: as with TBE_FLAG_NO_PACK (wide records; tbe_layout bit 0 clear); two-byte replies
 * (bit 4) only when the largest TokenLimit of any class is <= 16382.  The ring of key k is
 * ring[k*C .. k*C+C), C the largest ring length of any class; a key uses the first slots of
 * its own class's length and wraps there.  A classed engine writes the client view
 * {est, global} of every synced key at every sync (16 more bytes per key than the derived
 * view of a plain engine's one-client sync).
 * tbe_approx_idle(_device) decays with the key's class rate, tbe_approx_reset(_device) gives
 * cap = TokenLimit of the key's class and leaves the class byte; tbe_approx_query,
 * tbe_queue_cancel, tbe_queue_of, tbe_evicted, TBE_FLAG_STATS counting and the tier's
 * exports and imports work as on a plain engine. */
tbe_status tbe_create_approx_classes(const tbe_config *config, const tbe_queue_class *extra,
                                     uint32_t n_extra, tbe_engine **out_engine);

/* The classes of an approximate engine with all five options, class 0 first (as tbe_classes,
 * which reports the first three); another kind of engine: TBE_EINVAL. */
tbe_status tbe_approx_classes(const tbe_engine *engine, tbe_queue_class *out, uint32_t capacity,
                              uint32_t *n_classes);

/* cls[d_ids[i]] = d_cls[i].  The row {v, t_us} stays: the key's next evaluation clamps with
 * the new TokenLimit and refills at the new rate, as when another limiter's script runs on
 * the same Redis hash; the lapse test uses the new class from here on (the reference keeps
 * the last granting script's EXPIRE until the next grant).  Contract of
 * tbe_import_rows_device: ordered after every batch enqueued before the call and before
 * every batch after it, `stream` as in tbe_expired_device; unique ids; every pair is
 * validated before any is written, and an id >= n_keys or a class >= the number of classes
 * voids the whole call, reported by tbe_synchronize.  Without extra classes only class 0 is
 * valid.
 * Queueing engine with extra classes: an id whose queue is not empty voids the whole call in
 * the same way (a shorter ring or another order under live entries has no counterpart in the
 * reference); the queue of a written id stays empty.
 * Approximate engine with extra classes: an id with anything queued (zero-permit
 * registrations included) voids the whole call likewise.  A written id gets the client side
 * of a limiter freshly constructed with the new class's options over the existing Redis key
 * (A:26-28): cap = TokenLimit, local count 0, empty queue, est 1, global 0.  The tier row
 * {v, p, t} stays; a local count not yet synced is dropped, as the reference drops it with
 * the limiter object. */
tbe_status tbe_set_class_device(tbe_engine *engine, const uint64_t *d_ids, const uint8_t *d_cls, uint64_t n,
                                void *stream);
/* The same from host buffers; synchronous, an invalid pair (or, as above, a non-empty
 * queue): TBE_EINVAL, nothing written. */
tbe_status tbe_set_class(tbe_engine *engine, const uint64_t *ids, const uint8_t *cls, uint64_t n);
/* d_cls[i] = class of d_ids[i] (ordering and `stream` as above); an id >= n_keys reads 0
 * and is reported by tbe_synchronize (host form: TBE_EINVAL). */
tbe_status tbe_get_class_device(tbe_engine *engine, const uint64_t *d_ids, uint64_t n, uint8_t *d_cls,
                                void *stream);
tbe_status tbe_get_class(tbe_engine *engine, const uint64_t *ids, uint64_t n, uint8_t *cls);

/* Replaces Dispose / DisposeAsyncCore (TB:85-109).  NULL is ignored. */
void tbe_destroy(tbe_engine *engine);

/* Human-readable description of the last non-OK status on this engine (never NULL);
 * with engine == NULL, of the calling thread's last failed tbe_create. */
const char *tbe_last_error(const tbe_engine *engine);

/* Replaces n sequential IDatabase.ScriptEvaluateAsync(_acquireScript,
 * {BucketId, PermitCount}) calls (TB:63; PTB:42) and their reply parsing (TB:64-81).
 * Host buffers; synchronous.  granted[i] = 1 iff reply[0] == 1 (TB:76); remaining[i]
 * = reply[1] = trunc(new_v) after the decision (TB:73, TB:238).
 * Invalid batch (key >= n_keys, permits < 0, ts_us < 0): TBE_EINVAL, no state change,
 * outputs unspecified. */
tbe_status tbe_acquire_batch(tbe_engine *engine, const uint64_t *keys, const int32_t *permits,
                             const int64_t *ts_us, uint64_t n, uint8_t *granted,
                             int32_t *remaining);

/* Same decision on device-resident buffers.  Returns once enqueued; a batch found
 * invalid on the device is skipped (no state change) and reported by tbe_synchronize.
 * `stream` (a hipStream_t): the engine waits on it for the inputs and makes it wait for
 * the replies, so work enqueued on it afterwards may read the replies and overwrite the
 * inputs.  NULL: the inputs must be complete when the call is made and stay untouched
 * until the replies are; the replies are complete at tbe_synchronize (or for any later
 * call on this engine).  Batches are applied in call order either way; consecutive
 * batches of a token-bucket engine overlap on the device (TBE_FLAG_NO_PIPELINE). */
tbe_status tbe_acquire_batch_device(tbe_engine *engine, const uint64_t *d_keys,
                                    const int32_t *d_permits, const int64_t *d_ts_us,
                                    uint64_t n, uint8_t *d_granted, int32_t *d_remaining,
                                    void *stream);

/* Page-locked host memory for the host-buffer calls' arrays (the caller
 * owns its buffers, pinning recommended).  Copies from it run as direct DMA, without the
 * staging copy a pageable buffer needs; the C# host pins its batch arrays this way
 * instead of GCHandle-pinning managed arrays.  bytes == 0 gives NULL.  Free with
 * tbe_free_host (NULL is ignored). */
tbe_status tbe_alloc_host(uint64_t bytes, void **out);
void tbe_free_host(void *p);

/* Waits for every enqueued batch; TBE_EINVAL if any of them was invalid since the
 * last call (the sticky flag is then cleared). */
tbe_status tbe_synchronize(tbe_engine *engine);

/* Bucket state exactly as the Redis hash would hold it (HGETALL of the key, TB:210):
 * *present = 0 if absent or expired at ts_us (pass ts_us < 0 to skip the expiry test);
 * otherwise *v = field v and *t = field t (= new_t of the last grant, TB:203/230). */
tbe_status tbe_query(tbe_engine *engine, uint64_t key, int64_t ts_us, double *v, double *t,
                     int32_t *present);

/* Bulk state export for parity checks: v[k] and the last grant's injected timestamp
 * t_us[k] (INT64_MIN when never granted) for keys [first, first + count). */
tbe_status tbe_export_state(tbe_engine *engine, uint64_t first, uint64_t count, double *v,
                            int64_t *t_us);

/* Restore of an exported range (snapshot/restore of the bucket hashes, the state Redis
 * persists; the in-process queues of the queueing kind are not part of it, as they are
 * not in the reference): keys [first, first + count) take {v[k], t_us[k]}; t_us =
 * INT64_MIN makes the key absent.  Token-bucket and queueing kinds.  t_us must be
 * INT64_MIN or >= 0; ordered after every batch enqueued before the call. */
tbe_status tbe_import_state(tbe_engine *engine, uint64_t first, uint64_t count, const double *v,
                            const int64_t *t_us);

/* Which keys of [first, first + count) no longer exist in the store: the device-side
 * counterpart of Redis dropping a bucket key at its EXPIRE (TB:232-235).  d_dead (device
 * memory, count bytes) gets d_dead[k - first] = 1 when key k's hash would not exist at
 * ts_us, else 0: its row is absent, or has lapsed by the rule tbe_query and the script
 * replay use, t_us < 1000 * (ts_us / 1000 - ttl_ms).  Queueing kind: a key with queued
 * requests is never dead.  Approximate kind: TBE_EINVAL (its local tier is in-process
 * state without an expiry).  clear != 0 also rewrites every lapsed row of the range
 * absent, which decides identically at ts_us and later but keeps a reused key id on a
 * full bucket even if a later timestamp steps back before the lapse.  The keys' classes
 * (tbe_set_class) are left alone: a caller that hands a reclaimed id to a new key sets its
 * class before that key's first batch.  On an engine with TBE_FLAG_STATS, clear != 0 also
 * zeroes both lease counters of every key flagged dead (the counters are per id; the engine
 * totals stay); clear == 0 zeroes none.
 * Ordered after every batch already enqueued on the engine (pipelined ones included),
 * as tbe_export_state is; `stream` as in tbe_acquire_batch_device: the scan waits for
 * work enqueued on it and it waits for the flags.  ts_us < 0 or a range past n_keys:
 * TBE_EINVAL, nothing written. */
tbe_status tbe_expired_device(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                              uint8_t *d_dead, int32_t clear, void *stream);

/* Portable snapshots: the live bucket rows as (id, v, t_us) lists, so that
 * saved state can be put back behind a directory that hands out other ids, or split over
 * another number of owners.  Token-bucket and queueing kinds (their bucket rows, the state
 * tbe_import_state covers; queues are not part of it); approximate kind: TBE_EINVAL.
 *
 * Export: a row of [first, first + count) is live at ts_us when t_us != INT64_MIN and not
 * t_us < 1000 * (ts_us / 1000 - ttl_ms), the complement of tbe_expired_device's row rule
 * (queue headers play no part); ts_us < 0 skips the lapse test, as in tbe_query.  The live
 * rows are written compacted, in ascending id order: d_ids[j], d_v[j], d_t_us[j] for the
 * j-th live row, j < capacity.  *d_n_live (device u64) always gets the total number of
 * live rows; rows at positions >= capacity are not written and nothing past capacity is
 * touched.  capacity == 0 (the buffers may be NULL) only counts.  Ordered after every
 * batch already enqueued on the engine, `stream` as in tbe_expired_device. */
tbe_status tbe_export_live_device(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                                  uint64_t *d_ids, double *d_v, int64_t *d_t_us, uint64_t capacity,
                                  uint64_t *d_n_live, void *stream);
/* The same into host buffers; synchronous. */
tbe_status tbe_export_live(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                           uint64_t *ids, double *v, int64_t *t_us, uint64_t capacity, uint64_t *n_live);

/* Import by id: table[d_ids[i]] = {d_v[i], d_t_us[i]}; t_us = INT64_MIN makes the row absent
 * ({TokenLimit, absent}).  Ids must be unique: the result for an id given twice is
 * unspecified.  An id >= n_keys, or a t_us < 0 other than INT64_MIN, makes the whole call
 * a no-op (every row is validated before any is written), reported like an invalid device
 * batch: by tbe_synchronize.  Ordered after every batch enqueued before the call and
 * before every batch enqueued after it; `stream` as in tbe_expired_device. */
tbe_status tbe_import_rows_device(tbe_engine *engine, const uint64_t *d_ids, const double *d_v,
                                  const int64_t *d_t_us, uint64_t n, void *stream);
/* The same from host buffers; synchronous, invalid rows: TBE_EINVAL, nothing written. */
tbe_status tbe_import_rows(tbe_engine *engine, const uint64_t *ids, const double *v, const int64_t *t_us,
                           uint64_t n);

/* Live owner-map change, the source side (DESIGN.md §7 "Migrating buckets"; the collective
 * around it is cluster.migrate).  Token-bucket kind, plain or with limit classes; the
 * queueing and approximate kinds: TBE_EINVAL.
 *
 * d_key_of_id[i] is the key that holds id first + i (tbe_dir_keys_of_device writes it),
 * UINT64_MAX where no key does.  dest = d_owner_map ? d_owner_map[tbe_key_vnode(key)] :
 * tbe_key_owner(key, n_owners), as in tbe_route_plan_map_device.  An id whose key has
 * dest != self is leaving: d_leaving[i] = 1 (every other id 0; d_leaving may be NULL).  A
 * leaving id whose row is live at ts_us (tbe_export_live_device's rule, by the key's own class
 * on a classed engine; ts_us < 0 skips the lapse test) contributes one row of four int64
 * {key, bits of v, t_us, class} (class 0 without classes); a leaving id with an absent or
 * lapsed row contributes none: its new owner starts it from a full bucket, which decides the
 * same at ts_us and later.  Rows are written to d_rows grouped by destination in ascending
 * owner order and in ascending id order inside a destination, row j < capacity at
 * d_rows + 4 j (16-byte aligned); nothing at or past capacity is touched, and capacity == 0
 * (d_rows may be NULL) only counts and flags.  d_counts (device u64, n_owners + 2 entries)
 * is always complete: [o] rows for owner o ([self] = 0), [n_owners] leaving ids,
 * [n_owners + 1] orphans -- live rows of the range whose id no key holds, which are never
 * sent and never touched.
 *
 * commit == 0 reads only.  commit != 0 then rewrites every leaving id's row absent
 * ({TokenLimit of its class, absent}) and, with TBE_FLAG_STATS, zeroes both of its lease
 * counters (class bytes and engine totals stay), as tbe_expired_device(clear) does for a
 * dead key.  A commit whose rows do not all fit in capacity or that finds an orphan, and
 * any call that meets a map entry >= n_owners, changes neither table nor counters (every row
 * is judged before any is written; a bad map entry also leaves d_rows unwritten) and is
 * reported like an invalid device batch: by tbe_synchronize.
 *
 * n_owners outside 1..256, self >= n_owners, a range past n_keys, a NULL d_key_of_id or
 * d_counts: TBE_EINVAL, nothing enqueued.  Ordered after every batch enqueued before the
 * call (pipelined ones included) and before every batch enqueued after it; `stream` as in
 * tbe_expired_device.  The engine keeps 8 (n_owners + 2) bytes of
 * workspace per 2048 ids of the range. */
tbe_status tbe_migrate_out_device(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                                  const uint64_t *d_key_of_id, const uint8_t *d_owner_map, uint32_t n_owners,
                                  uint32_t self, int64_t *d_rows, uint64_t capacity, uint64_t *d_counts,
                                  uint8_t *d_leaving, int32_t commit, void *stream);
/* The same with host buffers; synchronous.  A refused commit or a map entry >= n_owners:
 * TBE_EINVAL, nothing changed (counts is still complete for a refused commit). */
tbe_status tbe_migrate_out(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                           const uint64_t *key_of_id, const uint8_t *owner_map, uint32_t n_owners, uint32_t self,
                           int64_t *rows, uint64_t capacity, uint64_t *counts, uint8_t *leaving, int32_t commit);
/* tbe_migrate_out_device / tbe_migrate_out plus one output: d_row_ids[j] (device u64) = the id
 * (first + i) whose row is written at d_rows + 4 j, for every j < capacity that holds a row;
 * nothing at or past capacity is touched in either array.  A migration of text-keyed buckets
 * fetches the rows' key text by these ids (tbe_sdir_text_device) before the reclaim forgets
 * them (DESIGN.md §7 "Migrating text-keyed buckets"); there d_key_of_id holds the routing
 * keys tbe_sdir_route_keys_device writes.  d_row_ids == NULL is exactly the call above: the
 * two entry points above pass NULL.  The host form copies min(rows written, capacity) ids. */
tbe_status tbe_migrate_out_ids_device(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                                      const uint64_t *d_key_of_id, const uint8_t *d_owner_map, uint32_t n_owners,
                                      uint32_t self, int64_t *d_rows, uint64_t capacity, uint64_t *d_counts,
                                      uint8_t *d_leaving, int32_t commit, uint64_t *d_row_ids, void *stream);
tbe_status tbe_migrate_out_ids(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                               const uint64_t *key_of_id, const uint8_t *owner_map, uint32_t n_owners, uint32_t self,
                               int64_t *rows, uint64_t capacity, uint64_t *counts, uint8_t *leaving, int32_t commit,
                               uint64_t *row_ids);

/* ---------------------------------------------------------------- TokenBucketWithQueue
 * Engines created with kind = TBE_KIND_QUEUEING. The reference limiter
 * (TokenBucketWithQueue/RedisTokenBucketRateLimiter.cs, "Q") is commented out and does
 * not compile; its semantics are fixed in DESIGN.md §2b (a lease is one TB script call;
 * queue order follows System.Collections.Generic/Deque.cs).  Per-key queues hold at most
 * QueueLimit entries (permits >= 1 each). */
#define TBE_WAIT_FAILED 0    /* CreateFailedTokenLease (Q:113, Q:383-388) */
#define TBE_WAIT_GRANTED 1   /* SuccessfulLease (Q:85-88) */
#define TBE_WAIT_QUEUED 2    /* registration enqueued (Q:117-132); completes via tbe_refresh */
#define TBE_WAIT_REJECTED 3  /* permits > TokenLimit: ArgumentOutOfRangeException (Q:70-73) */

/* Replaces n WaitAsyncCore calls (Q:67-134).  Request i gets id id_base + i (0 <= id <
 * 2^47).  status[i] is a TBE_WAIT_* code; remaining[i] = trunc(new_v) of the script call
 * made for the request, or -1 when no call was made (OldestFirst with a non-empty queue,
 * or REJECTED).  Queued requests that a NewestFirst admission evicted (Q:94-109) are
 * retrievable with tbe_evicted until the next batch; *n_evicted gets their number. */
tbe_status tbe_wait_batch(tbe_engine *engine, const uint64_t *keys, const int32_t *permits,
                          const int64_t *ts_us, uint64_t n, int64_t id_base, uint8_t *status,
                          int32_t *remaining, uint64_t *n_evicted);

/* AttemptAcquire on a queueing limiter (TryLeaseUnsynchronized only, Q:136-165): like
 * tbe_wait_batch but a request that cannot lease is FAILED instead of queued (nothing is
 * ever enqueued or evicted).  OldestFirst with a non-empty queue fails without a script
 * call (remaining -1).  The reference's own AcquireCore is a stub (Q:62-65). */
tbe_status tbe_queue_attempt_batch(tbe_engine *engine, const uint64_t *keys, const int32_t *permits,
                                   const int64_t *ts_us, uint64_t n, uint8_t *status,
                                   int32_t *remaining);

/* Evictions of the last tbe_wait_batch, sorted by (causing request index, request id):
 * cause_index[j] is the batch index of the request whose admission evicted request_id[j]. */
tbe_status tbe_evicted(tbe_engine *engine, uint64_t *cause_index, int64_t *request_id,
                       uint64_t capacity, uint64_t *n_written);

/* One replenish tick at ts_us (the timer-driven drain, Q:237-271): for every key with a
 * non-empty queue, grant the head (OldestFirst) or tail (NewestFirst) while the script
 * grants.  *n_granted gets the number of queued requests completed; fetch them with
 * tbe_refresh_log. */
tbe_status tbe_refresh(tbe_engine *engine, int64_t ts_us, uint64_t *n_granted);

/* Grants of the last tbe_refresh in (key, drain order): key, request id and
 * trunc(new_v) after the grant. */
tbe_status tbe_refresh_log(tbe_engine *engine, uint64_t *keys, int64_t *request_id,
                           int32_t *remaining, uint64_t capacity, uint64_t *n_written);

/* Device-pointer tbe_wait_batch (wait = 1, Q:67-134) / tbe_queue_attempt_batch (wait = 0,
 * Q:136-165): every buffer is device memory on the engine's GPU, the call only enqueues
 * (stream semantics as tbe_acquire_batch_device) and the replies equal the host-buffer
 * call's.  NewestFirst evictions are fetched with tbe_evicted (which then synchronises).
 * Invalid requests skip the batch and surface at tbe_synchronize. */
tbe_status tbe_wait_batch_device(tbe_engine *engine, const uint64_t *d_keys, const int32_t *d_permits,
                                 const int64_t *d_ts_us, uint64_t n, int64_t id_base, int32_t wait,
                                 uint8_t *d_status, int32_t *d_remaining, void *stream);

/* Upper bound on the grants one tbe_refresh_device can log: min(entries possibly queued,
 * n_keys * min(max(1, QueueLimit), TokenLimit)) -- a queued entry holds >= 1 permit and
 * a tick grants at most TokenLimit tokens per key.  With queueing classes the per-key factor
 * is the largest min(max(1, QueueLimit), TokenLimit) of any class.
 * Approximate kind (the grants one sync can log): per key min(ring length, TokenLimit +
 * zero_wait_slots), the largest of any class -- zero-permit registrations complete beside
 * the TokenLimit permits a sync can grant (A:474). */
tbe_status tbe_refresh_bound(tbe_engine *engine, uint64_t *bound);

/* Device-pointer tbe_refresh (Q:237-271): enqueues one replenish tick at ts_us.  Grants
 * land in the caller's device buffers as (key << 16 | drain position, request id,
 * trunc(new_v)), grouped arbitrarily across keys, and *d_count (device u32) receives
 * their number.  capacity must be >= tbe_refresh_bound (TBE_EINVAL otherwise), so no
 * grant is ever dropped. */
tbe_status tbe_refresh_device(tbe_engine *engine, int64_t ts_us, uint64_t *d_keyseq,
                              int64_t *d_request_id, int32_t *d_remaining, uint64_t capacity,
                              uint32_t *d_count, void *stream);

/* tbe_wait_batch_device followed by tbe_refresh_device(tick_ts_us), fused: the batch's
 * fold drains every key of its bucket at tick_ts_us right after the batch's requests,
 * on the rows and queue headers it already holds in LDS, so the tick costs no separate
 * pass over the table (Q:67-134 then Q:237-271; results, logs and engine state equal
 * the two calls').  capacity must cover tbe_refresh_bound as it stands AFTER the batch
 * (the batch's own enqueues count).  An invalid batch skips the tick too (the call is
 * one unit); it surfaces at tbe_synchronize like any device batch. */
tbe_status tbe_wait_batch_tick_device(tbe_engine *engine, const uint64_t *d_keys, const int32_t *d_permits,
                                      const int64_t *d_ts_us, uint64_t n, int64_t id_base, int32_t wait,
                                      uint8_t *d_status, int32_t *d_remaining, int64_t tick_ts_us,
                                      uint64_t *d_keyseq, int64_t *d_request_id, int32_t *d_log_remaining,
                                      uint64_t capacity, uint32_t *d_count, void *stream);

/* ---- Per-class replenish ticks.  In the reference the replenish timer belongs
 * to one limiter (its own ReplenishmentPeriod) and drains that limiter's queue alone
 * (Q:237-271); these three calls are tbe_refresh, tbe_refresh_device and
 * tbe_wait_batch_tick_device with a class mask, so the classes of one engine tick at their own
 * periods.  mask: host memory, 256 bits, bit c of word c >> 6 = class c (the form
 * tbe_approx_refresh_classes takes); it is read before the call returns.
 *   A key whose class bit is set: the unmasked call for that key -- same grants, same log
 *     entries, same row and header bits.
 *   A key whose class bit is clear: left alone completely.  Its row {v, t}, its queue header
 *     and its ring keep their bits, nothing of it is logged, and a row that would have lapsed
 *     by its class's TTL at ts_us is not rewritten: that passive expiry belongs to the tick of
 *     the key's own limiter.
 *   An engine without extra classes: bit 0 set is the unmasked call; bit 0 clear drains
 *     nothing and writes *d_count = 0 (the fused call is then tbe_wait_batch_device).
 *   An all-clear mask is valid and drains nothing.
 * In tbe_wait_batch_tick_classes_device the batch's requests are decided for every class; only
 * the fused tick is masked.
 * TBE_EINVAL before the device is touched: mask == NULL, a bit at or above the number of
 * classes, an engine that is not of the queueing kind (and what the unmasked call refuses).
 * tbe_refresh_bound is unchanged and remains an upper bound for a masked tick; the capacity
 * checks use it.  The engine's count of queued entries and TBE_FLAG_STATS counting are handled
 * as in the unmasked calls.  tbe_refresh_classes's log is read with tbe_refresh_log. */
tbe_status tbe_refresh_classes(tbe_engine *engine, int64_t ts_us, const uint64_t *mask, uint64_t *n_granted);

tbe_status tbe_refresh_classes_device(tbe_engine *engine, int64_t ts_us, const uint64_t *mask,
                                      uint64_t *d_keyseq, int64_t *d_request_id, int32_t *d_remaining,
                                      uint64_t capacity, uint32_t *d_count, void *stream);

tbe_status tbe_wait_batch_tick_classes_device(tbe_engine *engine, const uint64_t *d_keys,
                                              const int32_t *d_permits, const int64_t *d_ts_us, uint64_t n,
                                              int64_t id_base, int32_t wait, uint8_t *d_status,
                                              int32_t *d_remaining, int64_t tick_ts_us, const uint64_t *mask,
                                              uint64_t *d_keyseq, int64_t *d_request_id,
                                              int32_t *d_log_remaining, uint64_t capacity, uint32_t *d_count,
                                              void *stream);

/* Queue of one key, oldest first (Deque enumeration order, DQ:116-125).  A diagnostic call:
 * synchronous, and on an engine with queueing classes it also reads the key's class byte
 * (one more blocking one-byte copy) to know where the key's ring wraps. */
tbe_status tbe_queue_of(tbe_engine *engine, uint64_t key, int64_t *request_id, int32_t *permits,
                        uint32_t capacity, uint32_t *count);

/* Cancellation of queued requests (the CancellationToken registration of a queued
 * WaitAsync: CancelQueueState.TrySetCanceled, Q:480-506 / A:531-557), queueing and
 * approximate kinds.  Cancels are applied in call order; cancelled[i] = 1 when
 * request_ids[i] was queued on keys[i] and is now removed: _queueCount (qsum) drops by its
 * permits and the entries behind it keep their order.  0 when it is not queued there
 * (already granted, evicted, failed or canceled: TrySetCanceled returns false).  Decision
 * (DESIGN.md §2b): the entry leaves the queue at once, so the drain neither grants it nor
 * waits on it; the reference leaves it in its deque until the drain dequeues it, which
 * consumes its tokens and, in A:489, adds them back twice.
 * Ordered after every batch enqueued before the call; synchronous.  *n_cancelled gets
 * the number of 1s.  key >= n_keys: TBE_EINVAL, nothing canceled. */
tbe_status tbe_queue_cancel(tbe_engine *engine, const uint64_t *keys, const int64_t *request_ids,
                            uint64_t n, uint8_t *cancelled, uint64_t *n_cancelled);

/* ---- Bulk queue export and import by id list (DESIGN.md §7 "Migrating queued waits").
 * Queueing kind only, plain or with queueing classes; token-bucket and approximate engines:
 * TBE_EINVAL (the approximate kind's queue lives beside its local tier, with zero-permit
 * registrations, and does not travel).  Both device forms only enqueue: ordered after every
 * batch enqueued before the call (pipelined ones included) and before every batch enqueued
 * after it; `stream` as in tbe_expired_device.
 *
 * Export: d_qcount[i] (device u32, n entries) = entries queued on d_ids[i], 0 included;
 * d_entry_start (device u64, n + 1 entries, may be NULL) = the exclusive prefix of the counts,
 * [n] the total; *d_n_entries (device u64) = the total.  The entries of id i land at
 * d_entries[d_entry_start[i] + j], j < d_qcount[i], oldest first (Deque enumeration order,
 * DQ:116-125, as tbe_queue_of reports them) in the ring's own format request_id << 16 | permits:
 * the walk starts at the header's head and wraps at the key's own ring length, max(1,
 * QueueLimit) of its class on a classed engine.  Nothing at or past `capacity` (entries) is
 * touched; capacity == 0 (d_entries may be NULL) only counts.  clear != 0: afterwards every
 * listed id's header holds the empty queue with head 0, as tbe_set_class_device leaves it (ring
 * words are not scrubbed); ids must then be unique (the result for an id given twice is
 * unspecified).  A clearing call whose entries do not all fit in capacity changes no header
 * (counts, starts, the total and the entries below capacity are still written); any call that
 * meets an id >= n_keys writes nothing at all, *d_n_entries included.  Both are reported like an
 * invalid device batch: by tbe_synchronize.  The engine keeps 8 bytes of workspace per 2048
 * listed ids.
 *
 * Import: id i takes the next d_qcount[i] entries of d_entries (the call scans the counts
 * itself).  Every id and every entry is judged before anything is written; the call is a no-op,
 * reported by tbe_synchronize, when an id is >= n_keys, a target queue is not empty, a count
 * exceeds the key's ring length (its current class), an entry holds permits < 1 or more than
 * the TokenLimit of the key's class, a key's entries sum to more permits than its class's
 * QueueLimit (Q:92, Q:153), a request id is >= 2^47, or the counts do not sum to n_entries.
 * On success the ring of id i holds its entries at slots 0 .. count - 1 and its header is
 * {head 0, count, sum of permits}.  Ids must be unique.  Bucket rows, class bytes and lease
 * counters are not touched: a caller that moves a key sets its class first (tbe_set_class_device
 * requires an empty queue and resets the header), then its row, then its queue.  The engine's
 * count of queued entries grows by n_entries and stays an upper bound; tbe_refresh_bound and
 * the host tbe_refresh cover the imported entries.
 *
 * Request ids travel verbatim.  A queue that was filled on one engine and imported into
 * another then mixes ids minted by both, so callers that move queues between owners mint ids
 * that are unique across owners, e.g. id_base = (owner << 40) + counter, which stays below
 * 2^47 for 128 owners. */
tbe_status tbe_queue_export_ids_device(tbe_engine *engine, const uint64_t *d_ids, uint64_t n, uint32_t *d_qcount,
                                       uint64_t *d_entry_start, uint64_t *d_entries, uint64_t capacity,
                                       uint64_t *d_n_entries, int32_t clear, void *stream);
/* The same with host buffers; synchronous.  An id >= n_keys, or a clearing call whose entries
 * do not fit: TBE_EINVAL, no header changed (*n_entries is set in the second case). */
tbe_status tbe_queue_export_ids(tbe_engine *engine, const uint64_t *ids, uint64_t n, uint32_t *qcount,
                                uint64_t *entry_start, uint64_t *entries, uint64_t capacity, uint64_t *n_entries,
                                int32_t clear);
tbe_status tbe_queue_import_ids_device(tbe_engine *engine, const uint64_t *d_ids, const uint32_t *d_qcount,
                                       uint64_t n, const uint64_t *d_entries, uint64_t n_entries, void *stream);
/* The same from host buffers; synchronous; a void call: TBE_EINVAL, nothing changed. */
tbe_status tbe_queue_import_ids(tbe_engine *engine, const uint64_t *ids, const uint32_t *qcount, uint64_t n,
                                const uint64_t *entries, uint64_t n_entries);

/* Live owner-map change of a queueing engine, the source side: tbe_migrate_out_ids_device /
 * tbe_migrate_out_ids (above) with these differences.  Queueing kind only, plain or with
 * queueing classes; other kinds: TBE_EINVAL.  A leaving id contributes a row when its bucket
 * row is live at ts_us OR its queue is not empty (tbe_expired_device's rule: a key with queued
 * requests is never dead); a queued key's row travels verbatim, a lapsed t_us or INT64_MIN
 * included.  Row word 3 is class | (queue entries << 8).  An orphan is an id no key holds whose
 * row is live or whose queue is not empty.  commit != 0 rewrites the leaving ids' bucket rows
 * absent and zeroes their lease counters as above; it does NOT touch queue headers.  The
 * leaving ids' queues are taken by tbe_queue_export_ids_device(d_row_ids, clear = 1), which the
 * caller issues next with nothing in between: every id with queued entries has a row, so the
 * rows' ids cover every queue that leaves.  NewestFirst evictions of the last wait batch
 * (tbe_evicted) are fetched before a migration.  The collective around it is
 * cluster.migrate_queueing. */
tbe_status tbe_queue_migrate_out_ids_device(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                                            const uint64_t *d_key_of_id, const uint8_t *d_owner_map,
                                            uint32_t n_owners, uint32_t self, int64_t *d_rows, uint64_t capacity,
                                            uint64_t *d_counts, uint8_t *d_leaving, int32_t commit,
                                            uint64_t *d_row_ids, void *stream);
tbe_status tbe_queue_migrate_out_ids(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                                     const uint64_t *key_of_id, const uint8_t *owner_map, uint32_t n_owners,
                                     uint32_t self, int64_t *rows, uint64_t capacity, uint64_t *counts,
                                     uint8_t *leaving, int32_t commit, uint64_t *row_ids);

/* ---------------------------------------------------------------- ApproximateTokenBucket
 * Engines created with kind = TBE_KIND_APPROXIMATE hold ONE client's local tier for every
 * key (ApproximateTokenBucket/RedisApproximateTokenBucketRateLimiter.cs, "A") plus a
 * replica of the shared global tier (the sync script's Redis hash, A:241-270).  Status
 * codes are the TBE_WAIT_* values; available[i] is AvailableTokens (A:37) after the
 * decision (-1 for REJECTED). */

/* wait = 0: AcquireCore (A:84-113, never queues); wait = 1: WaitAsyncCore (A:116-183).
 * A zero-permit wait while AvailableTokens is 0 queues with Count 0 (A:127-181: TryLease
 * fails on `availableTokens != 0` and `QueueLimit - _queueCount < 0` never holds), holds
 * no queue permits, completes at the first drain that reaches it (A:474: AvailableTokens
 * >= 0) and is evicted from the head like any registration (A:145-156).  The reference
 * queues any number of them; a key holds at most tbe_config.zero_wait_slots, beyond which
 * the wait is FAILED. */
tbe_status tbe_approx_acquire_batch(tbe_engine *engine, const uint64_t *keys, const int32_t *permits,
                                    uint64_t n, int32_t wait, int64_t id_base, uint8_t *status,
                                    int32_t *available, uint64_t *n_evicted);

/* Device-pointer tbe_approx_acquire_batch (A:84-183): device buffers, enqueue only
 * (stream semantics as tbe_acquire_batch_device); evictions via tbe_evicted. */
tbe_status tbe_approx_acquire_batch_device(tbe_engine *engine, const uint64_t *d_keys,
                                           const int32_t *d_permits, uint64_t n, int32_t wait,
                                           int64_t id_base, uint8_t *d_status, int32_t *d_available,
                                           void *stream);

/* RetryAfter of the failed leases (A:390-395), decided on the device per request.
 * retry_after_ticks[i], for request i in arrival order:
 *   status[i] == TBE_WAIT_FAILED: the .NET ticks (100 ns) of
 *       TimeSpan.FromSeconds(deficit * FillRatePerSecond),
 *       deficit = max(0, (int32)(_globalThrottleScore + _localThrottleScore + permits[i]
 *                                + _queueCount - TokenLimit))       (C# unchecked int32)
 *     on the key's state at that request's turn in arrival order -- not after the batch: a
 *     later grant, wait or eviction of the same batch does not change it.  The seconds are
 *     one f64 multiply, the ticks a second one (* 1e7, no contraction), truncated toward
 *     zero; a deficit of 0 gives 0 ticks.  Where seconds * 1e7 >= 2^63 the reference's
 *     FromSeconds throws OverflowException: TBE_RETRY_OVERFLOW.  There is no NaN case:
 *     tbe_create refuses a non-positive period, so the fill rate is finite and positive.
 *     Every FAILED path carries it: AcquireCore with permits > 0, AcquireCore with 0 permits
 *     while throttled, a wait that does not fit the queue, and a zero-permit wait beyond
 *     zero_wait_slots (this engine's own departure; the same formula with permits 0).
 *   GRANTED, QUEUED, REJECTED: TBE_RETRY_NONE (REJECTED is an exception in the reference,
 *     not a lease).
 * _globalThrottleScore is this client's view as of its last sync.  Everything else --
 * validation, TBE_EINVAL with nothing applied, ordering, evictions, the chunked path for
 * page-locked buffers -- is tbe_approx_acquire_batch's; a null retry_after_ticks with
 * n > 0 is TBE_EINVAL. */
#define TBE_RETRY_NONE (-1)
#define TBE_RETRY_OVERFLOW INT64_MAX
tbe_status tbe_approx_acquire_batch_retry(tbe_engine *engine, const uint64_t *keys, const int32_t *permits,
                                          uint64_t n, int32_t wait, int64_t id_base, uint8_t *status,
                                          int32_t *available, int64_t *retry_after_ticks,
                                          uint64_t *n_evicted);

/* Device-pointer tbe_approx_acquire_batch_retry: as tbe_approx_acquire_batch_device, plus
 * d_retry_after_ticks (device memory, n int64).  Enqueue only: after a one-client sync the
 * client view is first written on the engine's stream and the batch's stream waits for it
 * by an event; the host is never synchronised. */
tbe_status tbe_approx_acquire_batch_retry_device(tbe_engine *engine, const uint64_t *d_keys,
                                                 const int32_t *d_permits, uint64_t n, int32_t wait,
                                                 int64_t id_base, uint8_t *d_status, int32_t *d_available,
                                                 int64_t *d_retry_after_ticks, void *stream);

/* Refresh step 1 (A:430-435): d_counts[k] = _localThrottleScore of key k, then 0.
 * d_counts is device memory for n_keys int32 (the caller exchanges it between clients,
 * e.g. an RCCL all-gather over xGMI). */
tbe_status tbe_approx_collect(tbe_engine *engine, int32_t *d_counts, void *stream);

/* Refresh step 2 (A:439-508): replay the sync script for every key, once per client in
 * client order, client r at ts_us + r*stagger_us with LocalCount d_all_counts[r*n_keys+k]
 * (device memory, n_clients * n_keys int32), keep client `my_client`'s reply (global
 * score, period via "%.14g" -> est), then drain the queues; fetch the completed queued
 * requests with tbe_refresh_log.  n_clients = 1 with summed counts makes the node one
 * client (an all-reduce instead of an all-gather).
 * Completion contract: the kernel runs on the engine's stream, ordered after the engine's
 * own earlier batches but after NO other stream, so d_all_counts must be complete when
 * this is called (e.g. the producer stream synchronised).  A caller whose counts come from
 * work still in flight on another stream (an RCCL all-gather, torch.cat on a side stream)
 * uses tbe_approx_sync_stream.  Returns when the replay and the drain log are done. */
tbe_status tbe_approx_sync(tbe_engine *engine, const int32_t *d_all_counts, uint32_t n_clients,
                           uint32_t my_client, int64_t ts_us, int64_t stagger_us, uint64_t *n_granted);

/* tbe_approx_sync ordered after `stream` (a hipStream_t; NULL = tbe_approx_sync): the
 * engine records an event on it and its stream waits for that event before the replay
 * reads d_all_counts, so the counts may still be being produced on `stream` at the call
 * (A:439).  No host synchronisation of `stream` is needed. */
tbe_status tbe_approx_sync_stream(tbe_engine *engine, const int32_t *d_all_counts, uint32_t n_clients,
                                  uint32_t my_client, int64_t ts_us, int64_t stagger_us, void *stream,
                                  uint64_t *n_granted);

/* RefreshAsync of a limiter that is the only client of its global tier (A:412-508): the
 * same as tbe_approx_collect followed by tbe_approx_sync with n_clients = 1, as one kernel
 * pass over the local tier (each key's local count is swapped to 0 and used as the sync
 * call's LocalCount; no host round trip between the two).  Completed queued requests via
 * tbe_refresh_log. */
tbe_status tbe_approx_refresh(tbe_engine *engine, int64_t ts_us, uint64_t *n_granted);

/* The three calls above for a set of classes: mask is host memory, 256 bits, bit c (of word
 * c >> 6) = class c.  For a key whose class bit is clear nothing is read-modify-written: its
 * local count, cap, queue, client view and tier row {v, p, t} keep their bits, nothing of it
 * is drained or logged, and tbe_approx_collect_classes writes d_counts[k] = 0 and leaves its
 * local count.  For a key whose bit is set the call is the unmasked one.  The estimate of
 * A:443 is ReplenishmentPeriod over the measured interval between syncs (field p, A:262), so
 * classes of different periods are only estimated correctly when each is synced at its own
 * period: that is what the mask is for.  The unmasked calls mean every class.  On an engine
 * without extra classes bit 0 set is the unmasked call; bit 0 clear does and logs nothing.
 * A bit at or above the number of classes, or mask == NULL: TBE_EINVAL before the device is
 * touched. */
tbe_status tbe_approx_collect_classes(tbe_engine *engine, int32_t *d_counts, const uint64_t *mask, void *stream);
tbe_status tbe_approx_sync_classes(tbe_engine *engine, const int32_t *d_all_counts, uint32_t n_clients,
                                   uint32_t my_client, int64_t ts_us, int64_t stagger_us, const uint64_t *mask,
                                   uint64_t *n_granted);
tbe_status tbe_approx_sync_classes_stream(tbe_engine *engine, const int32_t *d_all_counts, uint32_t n_clients,
                                          uint32_t my_client, int64_t ts_us, int64_t stagger_us,
                                          const uint64_t *mask, void *stream, uint64_t *n_granted);
tbe_status tbe_approx_refresh_classes(tbe_engine *engine, int64_t ts_us, const uint64_t *mask,
                                      uint64_t *n_granted);

/* Local-tier state of one key: _localThrottleScore, _globalThrottleScore,
 * _instanceCountEstimate, AvailableTokens (GetAvailablePermits, A:81), queued requests. */
tbe_status tbe_approx_query(tbe_engine *engine, uint64_t key, int32_t *local, int32_t *global_score,
                            double *est, int32_t *available, uint32_t *queued);

/* Snapshot/restore of the approximate kind's replica of the global tier: per key the
 * Redis hash {v, p, t} that the sync script writes with a one-day TTL (A:265-268);
 * t_us[k] is the injected TIME of the key's last sync, INT64_MIN when absent (then v = p
 * = 0, the script's default, A:250-252).  The local tier is in-process state in the
 * reference (A:36-40) and is not part of it.  Import: t_us must be INT64_MIN or >= 0;
 * both calls are ordered after every batch and sync enqueued before them.  Every rank of
 * a node imports the same snapshot so that the replicas stay identical. */
tbe_status tbe_approx_export_state(tbe_engine *engine, uint64_t first, uint64_t count, double *v,
                                   double *p, int64_t *t_us);
tbe_status tbe_approx_import_state(tbe_engine *engine, uint64_t first, uint64_t count, const double *v,
                                   const double *p, const int64_t *t_us);

/* Which keys of [first, first + count) an approximate engine could hand to another name
 * (DESIGN.md §2c).  The tier rows never lapse while the engine runs -- every sync rewrites
 * every key's row -- so the rule is not tbe_expired_device's.  d_idle (device memory, count
 * bytes) gets d_idle[k - first] = 1 when all of these hold, else 0:
 *   1. nothing is queued on the key, zero-permit registrations included;
 *   2. ConsumedTokens == 0, the reference's own idle test (A:36, A:503-506):
 *      (int32)((uint32)_globalThrottleScore + (uint32)_localThrottleScore) == 0, the global
 *      score being the client view tbe_approx_query reports;
 *   3. the tier row hands a client that syncs at ts_us nothing: it is absent, or lapsed by
 *      the sync's own test (t_us < 1000 * (ts_us / 1000 - 86 400 000)), or
 *      max(0, v - max(0, new_t(ts_us) - new_t(t_us)) * decay_rate) == 0 with the sync
 *      script's operations in its order (A:255-258), no contraction.
 * Ordered after every batch and sync already enqueued on the engine; `stream` as in
 * tbe_expired_device.  ts_us < 0, a range past n_keys or another kind of engine: TBE_EINVAL,
 * nothing written.  On a replicated tier every client scans and the flags are combined (a
 * key is idle only where every client says so) before anything is reset, which is why scan
 * and reset are two calls. */
tbe_status tbe_approx_idle_device(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                                  uint8_t *d_idle, void *stream);
/* Every key k of the range with d_flags[k - first] != 0 gets the state of a new engine:
 * local tier {cap TokenLimit, local 0, empty queue}, client view {est 1, global 0}, tier
 * row absent (v = p = 0).  A reused id is then what the reference has for a new resourceID:
 * a freshly constructed limiter over an absent Redis key, the estimator's warm-up included.
 * Unflagged rows are not written.  On an engine with TBE_FLAG_STATS both lease counters of
 * every flagged key are zeroed too (the engine totals stay).
 * After a one-client sync the client views of all keys are
 * first written (as tbe_approx_import_state does).  Ordering, `stream` and argument checks
 * as above.
 * Known departure: a name that is reclaimed and returns within a day finds, in the
 * reference, its old row -- worth 0 tokens by rule 3 -- with its old period estimate p;
 * here it finds the script's absent default (A:247-252), as the reference does after its
 * own EXPIRE or a Redis flush.  Only the estimator's warm-up differs. */
tbe_status tbe_approx_reset_device(tbe_engine *engine, uint64_t first, uint64_t count,
                                   const uint8_t *d_flags, void *stream);
/* The same with host buffers; synchronous. */
tbe_status tbe_approx_idle(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count, uint8_t *idle);
tbe_status tbe_approx_reset(tbe_engine *engine, uint64_t first, uint64_t count, const uint8_t *flags);

/* Portable snapshots of the approximate kind's {v, p, t} tier, in the form
 * of tbe_export_live_device / tbe_import_rows_device.  Export: a row of [first, first +
 * count) is written when it is present, not lapsed at ts_us (one-day TTL, A:268; ts_us < 0
 * skips the lapse test) and d_skip is NULL or d_skip[k - first] == 0 (device memory, count
 * bytes: every synced id holds a row, so the caller masks with the idle flags or with "not
 * held by the directory").  Rows are compacted in ascending id order; *d_n_live (device
 * u64) gets their total; nothing at or past `capacity` is touched and capacity == 0 only
 * counts.  Local tiers and client views are in-process state (A:36-40) and not part of it. */
tbe_status tbe_approx_export_live_device(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                                         const uint8_t *d_skip, uint64_t *d_ids, double *d_v, double *d_p,
                                         int64_t *d_t_us, uint64_t capacity, uint64_t *d_n_live, void *stream);
/* The same with host buffers (skip included); synchronous. */
tbe_status tbe_approx_export_live(tbe_engine *engine, int64_t ts_us, uint64_t first, uint64_t count,
                                  const uint8_t *skip, uint64_t *ids, double *v, double *p, int64_t *t_us,
                                  uint64_t capacity, uint64_t *n_live);
/* Import by id: tier[d_ids[i]] = {d_v[i], d_p[i], d_t_us[i]}; t_us = INT64_MIN writes {0, 0,
 * absent}.  Unique ids.  An id >= n_keys, or a t_us < 0 other than INT64_MIN, voids the
 * whole call (every row is validated before any is written) and is reported by
 * tbe_synchronize.  After a one-client sync the client views are first written, as in
 * tbe_approx_import_state.  Every rank of a replicated tier imports every row. */
tbe_status tbe_approx_import_rows_device(tbe_engine *engine, const uint64_t *d_ids, const double *d_v,
                                         const double *d_p, const int64_t *d_t_us, uint64_t n, void *stream);
/* The same from host buffers; synchronous, invalid rows: TBE_EINVAL, nothing written. */
tbe_status tbe_approx_import_rows(tbe_engine *engine, const uint64_t *ids, const double *v, const double *p,
                                  const int64_t *t_us, uint64_t n);

/* ---------------------------------------------------------------- Lease statistics
 * The GA System.Threading.RateLimiting surface: GetStatistics() returns RateLimiterStatistics
 * {CurrentAvailablePermits, CurrentQueuedCount, TotalFailedLeases, TotalSuccessfulLeases}
 * (DESIGN.md §2d).  An engine created with TBE_FLAG_STATS keeps ok[k] and failed[k] per key
 * and the two engine totals, which are the sums of the per-key events:
 *   tbe_acquire_batch(_device): granted[i] == 1 -> ok[key_i] += 1; == 0 -> failed[key_i] += 1.
 *   tbe_wait_batch*, tbe_queue_attempt_batch, tbe_approx_acquire_batch* (_retry included):
 *     TBE_WAIT_GRANTED -> ok; TBE_WAIT_FAILED -> failed; TBE_WAIT_QUEUED nothing yet (it counts
 *     when it completes); TBE_WAIT_REJECTED nothing (an exception in the reference, not a
 *     lease); each NewestFirst eviction (Q:94-109, A:143-158) -> failed on the evicted
 *     entry's key.
 *   tbe_refresh(_device), the tick of tbe_wait_batch_tick_device, their *_classes forms,
 *     tbe_approx_sync(_stream), tbe_approx_refresh: each drained grant -> ok on its key.
 *   tbe_queue_cancel and a batch skipped as invalid count nothing.
 * The counters are per id: tbe_expired_device(clear != 0) and tbe_approx_reset(_device) zero
 * them for the keys they flag; tbe_set_class*, imports and exports of rows leave them alone.
 *
 * Batched query.  Any output pointer may be NULL; keys may repeat.
 *   ok[i], failed[i]  the counters of keys[i] (TBE_EINVAL on an engine without the flag).
 *   available[i]      token-bucket and queueing kinds: trunc(x), x the script's refilled,
 *                     clamped value (TB:218-221) of the key at ts_us -- the `remaining` a
 *                     denied request at ts_us would be told; an absent or lapsed row gives
 *                     the TokenLimit of the key's class; the row is not touched.
 *                     Approximate kind: AvailableTokens (A:37); ts_us is ignored.
 *   queued[i]         _queueCount, the queued permits; 0 on the token-bucket kind.
 * available and queued work on every engine: they are the batched GetAvailablePermits.
 * ts_us < 0 on the two clocked kinds: TBE_EINVAL.  A key >= n_keys voids the device call
 * (nothing is written) and is reported by tbe_synchronize; the host form returns TBE_EINVAL.
 * Ordered after every batch enqueued before the call; `stream` as in tbe_expired_device. */
tbe_status tbe_stats_batch_device(tbe_engine *engine, const uint64_t *d_keys, uint64_t n, int64_t ts_us,
                                  uint64_t *d_ok, uint64_t *d_failed, int32_t *d_available,
                                  uint32_t *d_queued, void *stream);
/* The same with host buffers; synchronous. */
tbe_status tbe_stats_batch(tbe_engine *engine, const uint64_t *keys, uint64_t n, int64_t ts_us, uint64_t *ok,
                           uint64_t *failed, int32_t *available, uint32_t *queued);
/* The engine totals, kept apart from the per-key counters so that reading them scans
 * nothing; synchronous.  TBE_EINVAL on an engine without TBE_FLAG_STATS (as the two below). */
tbe_status tbe_stats_totals(tbe_engine *engine, uint64_t *ok, uint64_t *failed);
/* Range forms, for restore and for tests; synchronous.  An import moves the engine totals by
 * the difference between the imported and the replaced counters. */
tbe_status tbe_stats_export(tbe_engine *engine, uint64_t first, uint64_t count, uint64_t *ok, uint64_t *failed);
tbe_status tbe_stats_import(tbe_engine *engine, uint64_t first, uint64_t count, const uint64_t *ok,
                            const uint64_t *failed);

/* How the engine lays a batch out (for reports and tests): *passes = 8-bit partition
 * passes over the bucket id, *r_bits = log2 of the keys per bucket (one workgroup
 * each), *packed: bit 0 set when the passes move packed 8-byte request records (token
 * bucket kind) rather than the wide {key, permits, ts} records, bit 1 set
 * when hot keys get runs of their own (TBE_FLAG_NO_HOT clears it), bit 2 set when
 * consecutive device batches overlap (TBE_FLAG_NO_PIPELINE clears it), bit 3 set when
 * replies travel as one byte (TBE_FLAG_NO_NARROW clears it), bit 4 set when the queueing
 * or approximate kind's replies travel as two bytes, bit 5 set when the last partition
 * pass writes fold records (TBE_FLAG_UNSCATTER_ALL clears it; used by batches whose
 * reply position and time offset fit), bit 6 set when the second
 * pass's histogram reads the one-byte digit stream (TBE_FLAG_HIST_RECORDS clears it),
 * bit 7 set when the final un-partition re-ranks pass 0's tiles (TBE_FLAG_RERANK sets
 * it), bit 8 set when pass 0 writes narrow 4-byte records (token bucket and queueing kinds
 * with fold records and the digit stream, and the approximate kind's AcquireCore batches; a
 * batch uses them when it uses fold records), bit 9 set when the queueing kind stores its
 * per-key queue headers in 32 bits (QueueLimit <= 1024, of every class). */
tbe_status tbe_layout(const tbe_engine *engine, uint32_t *passes, uint32_t *r_bits, uint32_t *packed);

/* The record layout a batch of n requests takes (diagnostics and tests):
 * out[0] partition passes, out[1] 1 if the last pass writes fold records, out[2] their
 * reply-position bits (ceil_log2 n), out[3] their time-offset bits, out[4] the pass-0
 * record's key bits, out[5] permit-code bits, out[6] pass-0 time-offset bits, out[7]
 * r_bits, and when n_out > 8, out[8] 1 if the batch is a sparse token-bucket batch
 * (fewer than R >> TBE_SPARSE_GATE_SHIFT = R/8 requests per bucket on average, R = 2^r_bits
 * keys per bucket: one wave per sparse bucket, the dense buckets listed for the wide
 * fold; hot-key runs only from 2^TBE_HOT_SPARSE_MIN_LOG2 = 2^20 requests, a smaller
 * sparse batch leaves the hot sets as they are).  n_out must be >= 8.  A request
 * whose time offset does not fit takes the escape form (its time is read from the
 * previous record / the caller's array). */
tbe_status tbe_batch_format(const tbe_engine *engine, uint64_t n, uint32_t *out, uint32_t n_out);

/* Per-stage device time (ms) accumulated since the last call, when
 * TBE_FLAG_STAGE_TIMING is set: out[0..n_out) = {hist, colscan, scatter, bounds,
 * fold, unscatter}.  Returns the number of stages written via *n_written. */
tbe_status tbe_stage_times(tbe_engine *engine, double *out, uint32_t n_out, uint32_t *n_written);

#ifdef __cplusplus
}
#endif

#endif /* TBE_H_ */
