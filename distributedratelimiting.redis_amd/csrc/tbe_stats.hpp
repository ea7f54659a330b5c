// tbe_stats.hpp -- lease statistics (TBE_FLAG_STATS): per-key and engine
// totals of granted and failed leases, counted on the device.  Included by tbe_engine.hip
// inside its anonymous namespace, after the record and header types it reads (Slot,
// TbParams, ClsView, ALocal, qh_widen).
//
// Nothing here runs inside a fold.  A batch is counted after its last reply-writing kernel,
// from what every layout has in common: the caller's arrival-order keys[] and the final reply
// bytes (granted[] of the token-bucket kind, status[] of the other two; in both 1 is a
// granted lease, 0 a failed one, and the wait kinds' QUEUED 2 and REJECTED 3 count nothing).
// Evictions and drained grants are counted from their logs.
#pragma once

#pragma clang fp contract(off)

constexpr int kStatsBlock = 256;
constexpr int kStatsTile = 4096;             // requests per workgroup trip (T)
constexpr uint32_t kStatsSlotBits = 11;
constexpr uint32_t kStatsSlots = 1u << kStatsSlotBits;   // LDS table slots per workgroup (S)
constexpr int kStatsProbe = 8;               // linear probes before a request adds straight to memory
constexpr uint32_t kStatsEmpty = 0xFFFFFFFFu;
constexpr int kStatsMaxBlocks = 2048;
static_assert(kStatsTile % (kStatsBlock * 4) == 0, "four consecutive requests per thread per round");

// The engine's counters: ok[k], failed[k] per key and tot = {ok, failed} of the engine.
struct StatsView {
    unsigned long long *ok;
    unsigned long long *failed;
    unsigned long long *tot;
};

// relaxed, agent scope, result unused: one no-return 64-bit global atomic add
__device__ __forceinline__ void stats_add(unsigned long long *p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t stats_hash(uint32_t k) { return (k * 0x9E3779B1u) >> (32 - kStatsSlotBits); }

// One request: claim the key's slot (LDS compare-and-swap on the key word) and bump its
// delta; a full neighbourhood (or the one key id that equals the empty mark) adds to memory.
__device__ __forceinline__ void stats_count(uint32_t *tkey, uint32_t *tcnt, uint64_t key, uint32_t st,
                                            const StatsView &V, uint32_t &n_ok, uint32_t &n_failed) {
    if (st > 1u) return;                      // QUEUED / REJECTED
    const uint32_t which = st ^ 1u;           // 0: ok, 1: failed
    n_ok += st;
    n_failed += which;
    const uint32_t k32 = (uint32_t)key;
    if (k32 != kStatsEmpty) {
        uint32_t h = stats_hash(k32);
#pragma unroll 1
        for (int p = 0; p < kStatsProbe; ++p) {
            const uint32_t prev = atomicCAS(&tkey[h], kStatsEmpty, k32);
            if (prev == kStatsEmpty || prev == k32) {
                atomicAdd(&tcnt[which * kStatsSlots + h], 1u);
                return;
            }
            h = (h + 1u) & (kStatsSlots - 1u);
        }
    }
    stats_add((which ? V.failed : V.ok) + key, 1ull);
}

// Sum of one value per thread over the workgroup, in thread 0 (others: unspecified).
// `part` is kStatsBlock / 64 words of LDS; one barrier.
__device__ __forceinline__ uint32_t stats_block_sum(uint32_t x, uint32_t *part) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    uint32_t t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kStatsBlock / 64; ++w) t += part[w];
    return t;
}

// Counts one batch.  A workgroup takes tiles of kStatsTile arrival-order requests; per tile
// its LDS table gathers {ok, failed} 32-bit deltas per key (a tile holds 4096 requests, so a
// delta cannot wrap) and every occupied slot then adds each non-zero delta once: a key that
// takes most of a batch costs one global add per tile.  The engine totals are summed in
// registers over the workgroup's tiles and added once.  err: the batch's invalid-request
// flag -- a skipped batch counts nothing, and only a valid one has every key < n_keys.
__global__ __launch_bounds__(kStatsBlock) void k_stats_batch(const uint64_t *__restrict__ keys,
                                                             const uint8_t *__restrict__ status, uint64_t n,
                                                             const uint32_t *__restrict__ err, StatsView V) {
    if (*err) return;
    __shared__ uint32_t tkey[kStatsSlots];
    __shared__ uint32_t tcnt[2 * kStatsSlots];
    __shared__ uint32_t part[2][kStatsBlock / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t ntiles = (n + kStatsTile - 1) / kStatsTile;
    // 16-byte key loads and 4-byte status loads where the caller's pointers allow them
    const bool aligned = (((uintptr_t)keys & 15u) | ((uintptr_t)status & 3u)) == 0;
    uint32_t n_ok = 0, n_failed = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (uint32_t s = tid; s < kStatsSlots; s += kStatsBlock) {
            tkey[s] = kStatsEmpty;
            tcnt[s] = 0;
            tcnt[kStatsSlots + s] = 0;
        }
        __syncthreads();
        const uint64_t base = tile * kStatsTile;
        const bool full = aligned && base + kStatsTile <= n;
#pragma unroll 1
        for (int r = 0; r < kStatsTile / (kStatsBlock * 4); ++r) {
            const uint64_t i0 = base + ((uint64_t)r * kStatsBlock + tid) * 4;
            if (full) {
                const ulonglong2 ka = *reinterpret_cast<const ulonglong2 *>(keys + i0);
                const ulonglong2 kb = *reinterpret_cast<const ulonglong2 *>(keys + i0 + 2);
                const uint32_t s4 = *reinterpret_cast<const uint32_t *>(status + i0);
                stats_count(tkey, tcnt, ka.x, s4 & 0xFFu, V, n_ok, n_failed);
                stats_count(tkey, tcnt, ka.y, (s4 >> 8) & 0xFFu, V, n_ok, n_failed);
                stats_count(tkey, tcnt, kb.x, (s4 >> 16) & 0xFFu, V, n_ok, n_failed);
                stats_count(tkey, tcnt, kb.y, s4 >> 24, V, n_ok, n_failed);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i0 + j < n) stats_count(tkey, tcnt, keys[i0 + j], status[i0 + j], V, n_ok, n_failed);
            }
        }
        __syncthreads();
        for (uint32_t s = tid; s < kStatsSlots; s += kStatsBlock) {
            const uint32_t k = tkey[s];
            if (k == kStatsEmpty) continue;
            const uint32_t a = tcnt[s], b = tcnt[kStatsSlots + s];
            if (a) stats_add(V.ok + k, a);
            if (b) stats_add(V.failed + k, b);
        }
        __syncthreads();   // the flush has read the table before the next tile clears it
    }
    // (a workgroup's tiles hold < 2^32 requests: a batch does)
    const uint32_t t_ok = stats_block_sum(n_ok, part[0]);
    const uint32_t t_failed = stats_block_sum(n_failed, part[1]);
    if (tid == 0) {
        if (t_ok) stats_add(V.tot, t_ok);
        if (t_failed) stats_add(V.tot + 1, t_failed);
    }
}

// Counts a log: the NewestFirst evictions of a wait batch (failed[key], the key being the
// causing request's: keys[cause - ai_base]) or the grants of a drain (ok[keyseq >> 16]).
// *count is the log's device-side counter, `cap` the capacity it was written under; every
// log is sized so that no entry is dropped (the eviction log from the entries queued plus
// the batch, the drain logs from tbe_refresh_bound), so min(*count, cap) entries are all
// there are.  err (may be NULL): the batch's flag, as in k_stats_batch.
__global__ __launch_bounds__(kStatsBlock) void k_stats_log(const uint32_t *__restrict__ count, uint32_t cap,
                                                           const uint32_t *__restrict__ ev_cause,
                                                           const uint64_t *__restrict__ keys, uint64_t n_batch,
                                                           uint32_t ai_base, const uint64_t *__restrict__ keyseq,
                                                           uint64_t n_keys, const uint32_t *__restrict__ err,
                                                           unsigned long long *__restrict__ per_key,
                                                           unsigned long long *__restrict__ total) {
    if (err && *err) return;
    __shared__ uint32_t part[kStatsBlock / 64];
    const uint32_t m = min(*count, cap);
    uint32_t mine = 0;
    const uint32_t stride = gridDim.x * kStatsBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kStatsBlock + threadIdx.x; i < m; i += stride) {
        uint64_t key;
        if (ev_cause) {
            const uint64_t at = (uint64_t)(ev_cause[i] - ai_base);
            if (at >= n_batch) continue;      // (cannot happen: every cause is a request of the batch)
            key = keys[at];
        } else {
            key = keyseq[i] >> 16;
        }
        if (key >= n_keys) continue;          // (cannot happen either; keeps the add in bounds)
        stats_add(per_key + key, 1ull);
        ++mine;
    }
    const uint32_t t = stats_block_sum(mine, part);
    if (threadIdx.x == 0 && t) stats_add(total, t);
}

// The refilled, clamped token count of a row at the time of `rq` (TB:202-221), truncated as
// the reply's new_v is (TB:238): the `remaining` a denied request would be told.  The fold's
// arithmetic (tb_step_ft) without its commit; the row is only read.
__device__ __forceinline__ int32_t stats_available(const Slot &row, const ReqTime &rq, const TbParams &P) {
    const bool had = row.t_us != kAbsent;
    const bool present = had && !(row.t_us < rq.exp_lt);
    const double pv = present ? row.v : P.cap;                          // TB:211-215
    const double pt = present ? new_t_of(row.t_us) : rq.new_t;
    const double delta_t = lua_max(0.0, rq.new_t - pt);                 // TB:218
    const double fill = delta_t * P.rate;                               // TB:221: mul, then add
    const double x = lua_max(0.0, lua_min(P.cap, pv + fill));
    return (int32_t)x;
}

// The batched query's validating pass: *bad when any key is >= n_keys.
__global__ void k_stats_check(const uint64_t *__restrict__ keys, uint64_t n, uint64_t n_keys,
                              uint32_t *__restrict__ bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (keys[i] >= n_keys) *bad = 1u;
}

// The batched query (tbe_stats_batch_device): gathers the counters, evaluates `available`
// (clocked kinds: stats_available with the key's class; approximate kind: AvailableTokens,
// A:37) and reads the queued permits from the queue header (_queueCount).  Any output may be
// NULL.  Writes no engine state; an invalid call (k_stats_check) writes nothing at all and
// raises the sticky flag.  table == NULL: the approximate kind (alocal); qhdr only on the
// queueing kind; a ClsView only on a classed engine.
template <typename HW, typename... CV>
__global__ __launch_bounds__(kBlock) void k_stats_read(const uint64_t *__restrict__ keys, uint64_t n, int64_t ts_us,
                                                       const Slot *__restrict__ table, TbParams P0,
                                                       const HW *__restrict__ qhdr,
                                                       const ALocal *__restrict__ alocal, StatsView V,
                                                       unsigned long long *__restrict__ out_ok,
                                                       unsigned long long *__restrict__ out_failed,
                                                       int32_t *__restrict__ out_avail,
                                                       uint32_t *__restrict__ out_queued,
                                                       const uint32_t *__restrict__ bad,
                                                       uint32_t *__restrict__ sticky, CV... C) {
    static_assert(sizeof...(CV) <= 1, "at most one class view");
    if (*bad) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *sticky = 1u;
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint64_t k = keys[i];
        if (out_ok) out_ok[i] = V.ok[k];
        if (out_failed) out_failed[i] = V.failed[k];
        if (out_avail) {
            if (table) {
                TbParams P = P0;
                if constexpr (sizeof...(CV) == 1) {
                    const ClsView &cv = (C, ...);
                    P = cv.par[cv.cls[k]];
                }
                out_avail[i] = stats_available(table[k], req_time(ts_us, P.ttl_ms), P);
            } else {
                out_avail[i] = avail_of(alocal[k]);
            }
        }
        if (out_queued)
            out_queued[i] = qhdr ? (uint32_t)(qh_widen(qhdr[k]) >> 32) : (alocal ? (uint32_t)alocal[k].qsum : 0u);
    }
}

// A reused id starts at zero: both counters of every flagged key of [first, first + count).
// The engine totals stay (they count leases, not keys).
__global__ __launch_bounds__(kBlock) void k_stats_zero(const uint8_t *__restrict__ flags, uint64_t first,
                                                       uint64_t count, StatsView V) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count || !flags[i]) return;
    V.ok[first + i] = 0;
    V.failed[first + i] = 0;
}
