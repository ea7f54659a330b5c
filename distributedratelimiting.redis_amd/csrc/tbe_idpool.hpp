// tbe_idpool.hpp -- what the device u64 key directory (tbe_cluster.hip) and the device
// string directory (tbe_strdir.hip) share: the id pool ("The id rule"), the
// CAS probes of their slot tables, and the front half of a reclaim.  Both files link into
// one library, so everything here has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/tbe.h"
#include "tbe_device.hpp"
#include "tbe_hash.hpp"

namespace tbe {
namespace {

constexpr uint32_t kNoId = 0xFFFFFFFFu;
constexpr int kPoolBlock = 256;
constexpr int kPoolTile = 1024;      // ids (or requests) per counting block, 4 per thread
constexpr int kScanThreads = 1024;

unsigned grid_for(uint64_t n, unsigned block, unsigned cap = 8192) {
    const uint64_t g = (n + block - 1) / block;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(g, cap));
}

// ---------------------------------------------------------------- the id pool
// A fresh counter and a LIFO stack of freed ids (free_ids).  A batch's new keys, in arrival
// order of their first requests, pop the stack first and then take scramble_walk(fresh++);
// a reclaim pushes its victims in ascending id order.  Room for new keys = nfree +
// capacity - fresh; keys held = fresh - nfree.
//
// Each directory keeps eight state[] words; these sit at the same index in both.  Words
// 0, 3 and 4 are the directory's own (kDir* in tbe_cluster.hip, kSd* in tbe_strdir.hip).
enum : int {
    kStErr = 1,      // sticky error bits
    kStFresh0 = 2,   // the fresh counter before the current batch
    kStFresh = 5,    // fresh counters used
    kStNfree = 6,    // ids on the free stack
    kStNfree0 = 7,   // the stack's height before the current batch
    kStateWords = 8,
};

// A batch brings `tot` new keys: as many as there is room for are taken (beyond it:
// range_bit, sticky), freed ids first.  One thread, before the batch's ids are handed out.
__device__ __forceinline__ unsigned long long pool_take(unsigned long long *__restrict__ state,
                                                        unsigned long long tot, uint64_t capacity,
                                                        unsigned long long range_bit) {
    const unsigned long long fresh = state[kStFresh], nfree = state[kStNfree];
    const unsigned long long room = nfree + capacity - fresh;
    unsigned long long take = tot;
    if (take > room) {
        take = room;
        state[kStErr] |= range_bit;
    }
    const unsigned long long pop = take < nfree ? take : nfree;
    state[kStFresh0] = fresh;
    state[kStNfree0] = nfree;
    state[kStNfree] = nfree - pop;
    state[kStFresh] = fresh + (take - pop);
    return take;
}

// Id of the batch's new key of rank `rank` (fresh0 / nfree0: state[kStFresh0] and
// state[kStNfree0]): the stack's rank-th id from the top, then the bijection of the
// counter fresh0 + rank - nfree0; beyond capacity, none.  free_ids is null until the first
// reclaim, and nfree0 is 0 until then.
__device__ __forceinline__ uint32_t pool_id(uint64_t rank, uint64_t fresh0, uint64_t nfree0, uint64_t capacity,
                                            uint64_t imask, uint32_t ish, const uint32_t *__restrict__ free_ids) {
    if (rank < nfree0) return free_ids[nfree0 - 1 - rank];
    const uint64_t counter = fresh0 + (rank - nfree0);
    return counter < capacity ? (uint32_t)scramble_walk(counter, capacity, imask, ish) : kNoId;
}

// A reclaim pushed `victims` ids.
__device__ __forceinline__ void pool_reclaimed(unsigned long long *__restrict__ state, uint32_t victims) {
    state[kStNfree] += victims;
}

// Exclusive scan of per-block counts in place by one workgroup of kScanThreads: each thread
// sums a contiguous run of blocks (blocks_sum), the sums are scanned over the workgroup,
// and the carry runs through the thread's blocks (blocks_write).  also(j) rides along in a
// loop for a caller that carries a second array through the same passes (the string
// directory's bytes); these loops wait for every load, so a pass of its own would cost as
// much again.
template <class F>
__device__ __forceinline__ uint32_t blocks_sum(const uint32_t *__restrict__ v, uint32_t nblk, F also) {
    const uint32_t per = (nblk + kScanThreads - 1) / kScanThreads;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < per; ++k) {
        const uint32_t j = threadIdx.x * per + k;
        if (j < nblk) {
            sum += v[j];
            also(j);
        }
    }
    return sum;
}

template <class F>
__device__ __forceinline__ void blocks_write(uint32_t *__restrict__ v, uint32_t nblk, uint32_t run, F also) {
    const uint32_t per = (nblk + kScanThreads - 1) / kScanThreads;
    for (uint32_t k = 0; k < per; ++k) {
        const uint32_t j = threadIdx.x * per + k;
        if (j < nblk) {
            const uint32_t c = v[j];
            v[j] = run;
            run += c;
            also(j);
        }
    }
}

// The whole scan of one array; returns the sum of the counts to every thread.
__device__ __forceinline__ uint32_t scan_blocks(uint32_t *__restrict__ v, uint32_t nblk, uint32_t *wsum) {
    const auto nothing = [](uint32_t) {};
    uint32_t tot;
    const uint32_t run = block_excl_scan<kScanThreads>(blocks_sum(v, nblk, nothing), wsum, &tot);
    blocks_write(v, nblk, run, nothing);
    return tot;
}

__global__ __launch_bounds__(kScanThreads) void k_scan_blocks(uint32_t *__restrict__ v, uint32_t nblk,
                                                              uint32_t *__restrict__ total) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    const uint32_t tot = scan_blocks(v, nblk, wsum);
    if (threadIdx.x == 0) *total = tot;
}

// ---------------------------------------------------------------- slot table
// Open addressing with linear probing over u64 words, `empty` marking a free slot.
//
// The slot that holds `w`, claimed by CAS if no slot does; kNoId for a full table.
__device__ __forceinline__ uint32_t probe_find_or_claim(uint64_t *__restrict__ tab, uint64_t smask, uint64_t w,
                                                        uint64_t empty) {
    uint64_t h = mix64(w) & smask;
    for (uint64_t probe = 0; probe <= smask; ++probe) {
        const uint64_t cur = tab[h];
        if (cur == w) return (uint32_t)h;
        if (cur == empty) {
            const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(&tab[h]), empty, w);
            if (prev == empty || prev == w) return (uint32_t)h;
        }
        h = (h + 1) & smask;
    }
    return kNoId;
}

// Claim a slot for a word no slot holds: the slot, or kNoId when `w` is in the table
// already (or the table is full).
__device__ __forceinline__ uint32_t probe_insert(uint64_t *__restrict__ tab, uint64_t smask, uint64_t w,
                                                 uint64_t empty) {
    uint64_t h = mix64(w) & smask;
    for (uint64_t probe = 0; probe <= smask; ++probe) {
        const uint64_t cur = tab[h];
        if (cur == w) return kNoId;
        if (cur == empty) {
            const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(&tab[h]), empty, w);
            if (prev == empty) return (uint32_t)h;
            if (prev == w) return kNoId;
        }
        h = (h + 1) & smask;
    }
    return kNoId;
}

// Request i is the first one of a slot claimed in this batch: it brings a new key.
__device__ __forceinline__ bool is_new(const uint32_t *slot_of, const uint32_t *sid, const uint32_t *sfirst,
                                       uint64_t i) {
    const uint32_t sl = slot_of[i];
    return sl != kNoId && sid[sl] == kNoId && sfirst[sl] == (uint32_t)i;
}

__global__ void k_table_init(uint64_t *__restrict__ tab, uint32_t *__restrict__ sid, uint32_t *__restrict__ sfirst,
                             uint64_t nslots, uint64_t empty) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nslots; j += stride) {
        tab[j] = empty;
        sid[j] = kNoId;
        sfirst[j] = kNoId;
    }
}

// ids[i] of every request (or of the listed ones: list / list_n) out of its slot.
__global__ void k_gather(const uint32_t *__restrict__ slot_of, uint64_t n, const uint32_t *__restrict__ sid,
                         uint64_t *__restrict__ ids, const uint32_t *__restrict__ list = nullptr,
                         const uint32_t *__restrict__ list_n = nullptr) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t count = list ? *list_n : n;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += stride) {
        const uint64_t i = list ? list[t] : t;
        const uint32_t sl = slot_of[i];
        const uint32_t id = sl == kNoId ? kNoId : sid[sl];
        ids[i] = id == kNoId ? ~0ull : (uint64_t)id;
    }
}

// ---------------------------------------------------------------- reclaim, front half
// vict[id] = 1 marks a victim (each directory flags them its own way); the keep ids are
// no victims.
__global__ void k_pool_keep(const uint64_t *__restrict__ keep, uint64_t n_keep, uint64_t capacity,
                            uint8_t *__restrict__ vict) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_keep; j += stride)
        if (keep[j] < capacity) vict[keep[j]] = 0;
}

// Victims per block of kPoolTile ids (thread-contiguous).
__global__ __launch_bounds__(kPoolBlock) void k_pool_vcount(uint64_t capacity, const uint8_t *__restrict__ vict,
                                                            uint32_t *__restrict__ bv) {
    __shared__ uint32_t wsum[kPoolBlock / 64];
    constexpr int PER = kPoolTile / kPoolBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kPoolTile + (uint64_t)threadIdx.x * PER;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) c += base + k < capacity && vict[base + k];
    uint32_t tot;
    (void)block_excl_scan<kPoolBlock>(c, wsum, &tot);
    if (threadIdx.x == 0) bv[blockIdx.x] = tot;
}

// The victims onto the free stack in ascending id order (bv scanned; state[kStNfree] is
// still the stack's height before the reclaim).  forget(id): the directory drops what it
// keeps per id.  The stack holds distinct ids, so it never passes capacity.
template <class Forget>
__global__ __launch_bounds__(kPoolBlock) void k_pool_vpush(uint64_t capacity, const uint8_t *__restrict__ vict,
                                                           const uint32_t *__restrict__ bv,
                                                           const unsigned long long *__restrict__ state,
                                                           uint32_t *__restrict__ free_ids, Forget forget) {
    __shared__ uint32_t wsum[kPoolBlock / 64];
    constexpr int PER = kPoolTile / kPoolBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kPoolTile + (uint64_t)threadIdx.x * PER;
    bool v[PER];
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        v[k] = base + k < capacity && vict[base + k];
        c += v[k];
    }
    uint32_t tot;
    uint64_t at = (uint64_t)state[kStNfree] + bv[blockIdx.x] + block_excl_scan<kPoolBlock>(c, wsum, &tot);
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (v[k] && at < capacity) {
            free_ids[at++] = (uint32_t)(base + k);
            forget(base + k);
        }
}

// The pool's part of a directory's reclaim memory.  The first reclaim allocates vict,
// rc_bv, rc_n and free_ids (the directory's own buffers before them, free_ids last: it
// marks the set complete, and the assign kernels take it as null until then); the
// synchronous reclaim adds rc_dead, rc_keep and rc_count.
struct PoolScratch {
    uint32_t *free_ids = nullptr;          // the free stack, capacity ids
    uint8_t *vict = nullptr;               // [capacity]
    uint32_t *rc_bv = nullptr, *rc_n = nullptr;   // victims per block; {victims, survivors, ...}
    uint8_t *rc_dead = nullptr;            // the engine's flags, the caller's keep list, the count
    uint64_t *rc_keep = nullptr, *rc_count = nullptr;
    uint64_t rc_keep_cap = 0;
};

inline bool pool_scratch_alloc(PoolScratch &s, uint64_t capacity) {
    const uint64_t nbi = (capacity + kPoolTile - 1) / kPoolTile;
    return hipMalloc(&s.vict, capacity) == hipSuccess && hipMalloc(&s.rc_bv, nbi * sizeof(uint32_t)) == hipSuccess &&
           hipMalloc(&s.rc_n, 4 * sizeof(uint32_t)) == hipSuccess &&
           hipMalloc(&s.free_ids, capacity * sizeof(uint32_t)) == hipSuccess;
}

inline void pool_scratch_free(PoolScratch &s) {
    for (void *p : {(void *)s.free_ids, (void *)s.vict, (void *)s.rc_bv, (void *)s.rc_n, (void *)s.rc_dead,
                    (void *)s.rc_keep, (void *)s.rc_count})
        if (p) (void)hipFree(p);
    s = PoolScratch{};
}

// The synchronous reclaim of a directory on `device` with `capacity` ids: the engine's
// expired rows (cleared) are the dead flags of reclaim_device(d_dead, d_keep, n_keep,
// d_count), the directory's device-form reclaim on the null stream.
template <class F>
tbe_status pool_reclaim_sync(PoolScratch &s, int device, uint64_t capacity, tbe_engine *engine, int64_t ts_us,
                             const uint64_t *keep_ids, uint64_t n_keep, uint64_t *n_reclaimed, F reclaim_device) {
    if (!engine || !n_reclaimed || (n_keep && !keep_ids)) return TBE_EINVAL;
    *n_reclaimed = 0;
    // The engine must live on the directory's device: a read of one of its rows makes its
    // device current (and changes nothing).
    double v, t;
    int32_t present;
    int edev = -1;
    if (tbe_query(engine, 0, -1, &v, &t, &present) != TBE_OK || hipGetDevice(&edev) != hipSuccess) return TBE_EINVAL;
    // after every assign and engine batch, whatever its stream
    if (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return TBE_EDEVICE;
    if (edev != device) return TBE_EINVAL;
    if ((!s.rc_dead && hipMalloc(&s.rc_dead, capacity) != hipSuccess) ||
        (!s.rc_count && hipMalloc(&s.rc_count, sizeof(uint64_t)) != hipSuccess))
        return TBE_ENOMEM;
    if (n_keep > s.rc_keep_cap) {
        if (s.rc_keep) (void)hipFree(s.rc_keep);
        s.rc_keep = nullptr;
        s.rc_keep_cap = 0;
        if (hipMalloc(&s.rc_keep, n_keep * sizeof(uint64_t)) != hipSuccess) return TBE_ENOMEM;
        s.rc_keep_cap = n_keep;
    }
    if (n_keep && hipMemcpy(s.rc_keep, keep_ids, n_keep * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess)
        return TBE_EDEVICE;
    // refuses the approximate kind and an engine with fewer rows than the directory has ids
    tbe_status rc = tbe_expired_device(engine, ts_us, 0, capacity, s.rc_dead, 1, nullptr);
    if (rc != TBE_OK) return rc;
    if (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return TBE_EDEVICE;
    rc = reclaim_device(s.rc_dead, s.rc_keep, n_keep, s.rc_count);
    if (rc != TBE_OK) return rc;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(n_reclaimed, s.rc_count, sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
        return TBE_EDEVICE;
    return TBE_OK;
}

}  // namespace
}  // namespace tbe
