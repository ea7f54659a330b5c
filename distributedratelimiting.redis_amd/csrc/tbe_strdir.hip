// tbe_strdir.hip -- device string-key directory (include/tbe_strdir.h, SURVEY.md §8(f)
// row 2): InstanceName + resourceID (PartitionedRedisTokenBucketRateLimiter.cs:42) ->
// dense key id, exact byte comparison, ids by first occurrence.
//
// Layout in HBM (nslots = pow2 >= 2 * capacity, load <= 1/2):
//   stag[s]   u64  the slot's tag (below), ~0 = empty
//   sid[s]    u32  the key's id once assigned (kNoId before)
//   sfirst[s] u32  arrival index of the key's first request in the batch that claimed it
//   sloc[s]   u64  bit 63 | (arena offset << 17) | length of the key's text, once assigned
//   iloc[id]  u64  the same per id (tbe_sdir_key_of)
//   arena     key text (resourceID bytes), each key at an 8-byte aligned offset
//   free_ids  u32  stack of ids a reclaim took back, popped before fresh counters (tbe_idpool.hpp)
//
// A string's tag in probe round k (0..3) is (k << 62) | (H_k(string) & hmask), H_k a
// 64-bit hash seeded from the prefix and k.  Tags are unique in the table: a batch's
// requests with equal tags land on one slot (CAS), and its representative -- the stored
// text of an assigned key, else the batch's first request that landed there -- is
// compared byte for byte with every request.  Requests whose text differs (different
// strings, equal tags) move to the next round's tag; round k's tags only ever meet
// round k's claims, so a slot's first request is settled within the round that claims
// it.  Lookups follow the same rounds: the first slot tagged like the string whose text
// matches is its key; an empty slot before any tagged one means "never assigned".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/tbe_strdir.h"
#include "tbe_device.hpp"
#include "tbe_hash.hpp"
#include "tbe_idpool.hpp"
#include "tbe_text.hpp"

using namespace tbe;

namespace {

constexpr uint64_t kEmptyTag = ~0ull;
constexpr uint32_t kMaxLen = 1u << 16;
constexpr int kRounds = 4;
constexpr int kSdBlock = 256;
constexpr int kSdTile = 1024;            // requests per count/assign block (4 per thread)
constexpr unsigned kListGrid = 1024;     // workgroups of a probe round over the collided list
constexpr uint64_t kLocValid = 1ull << 63;
constexpr double kWarmShare = 0.5;       // warm path while the last batch's new keys stay below this share

__device__ __host__ __forceinline__ uint32_t loc_len(uint64_t loc) { return (uint32_t)(loc & (2 * kMaxLen - 1)); }
__device__ __host__ __forceinline__ uint64_t loc_off(uint64_t loc) { return (loc >> 17) & ((1ull << 46) - 1); }

// The directory's own state[] words, beside the id pool's (tbe_idpool.hpp): new keys ever
// assigned (only grows: the warm-path choice reads its deltas), arena bytes used, this
// batch's arena base.
enum : int { kSdEver = 0, kSdArena = 3, kSdArenaBase = 4 };
// error bits (state[kStErr])
constexpr unsigned long long kErrBatch = 1, kErrRange = 2, kErrRounds = 4, kErrArena = 8, kErrFull = 16;

struct SdParams {
    uint64_t seed[kRounds];
    uint64_t hmask;
};

__device__ __forceinline__ uint64_t sd_tag(uint32_t round, uint64_t h, uint64_t hmask) {
    const uint64_t t = ((uint64_t)round << 62) | (h & hmask);
    return t == kEmptyTag ? t - 1 : t;
}

__device__ __forceinline__ bool sd_equal(const uint8_t *__restrict__ a, uint64_t asafe, uint64_t aoff,
                                         const uint8_t *__restrict__ b, uint64_t bsafe, uint64_t boff,
                                         uint32_t len) {
    for (uint32_t k = 0; 8u * k < len; ++k)
        if (sd_word(a, asafe, aoff, len, k) != sd_word(b, bsafe, boff, len, k)) return false;
    return true;
}

// Offsets of string i, validated (false: malformed).
__device__ __forceinline__ bool sd_span(const uint64_t *__restrict__ offs, uint64_t i, uint64_t n_bytes,
                                        uint64_t &off, uint32_t &len) {
    const uint64_t a = offs[i], b = offs[i + 1];
    if (b < a || b > n_bytes || b - a > kMaxLen) return false;
    off = a;
    len = (uint32_t)(b - a);
    return true;
}

struct SdBatch {
    const uint8_t *bytes;
    const uint64_t *offs;
    uint64_t n_bytes;
    uint64_t safe;         // n_bytes rounded down to 8
};
struct SdArena {
    const uint8_t *bytes;
    uint64_t safe;
};

// Probe round `round`: find or claim the slot tagged like each request's string (over
// all requests in round 0, over the collided list after).  A slot claimed in this batch
// records the arrival index of its first request (atomicMin).
__global__ __launch_bounds__(kSdBlock) void k_sd_claim(SdBatch B, uint64_t n, const uint32_t *__restrict__ list,
                                                       const uint32_t *__restrict__ list_n, uint32_t round,
                                                       SdParams P, uint64_t *__restrict__ stag,
                                                       const uint32_t *__restrict__ sid,
                                                       uint32_t *__restrict__ sfirst, uint64_t smask,
                                                       uint32_t *__restrict__ slot_of,
                                                       unsigned long long *__restrict__ err) {
    const uint64_t count = list ? *list_n : n;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += stride) {
        const uint64_t i = list ? list[t] : t;
        uint64_t off;
        uint32_t len;
        if (!sd_span(B.offs, i, B.n_bytes, off, len)) {
            slot_of[i] = kNoId;
            atomicOr(err, kErrBatch);
            continue;
        }
        const uint64_t tag = sd_tag(round, sd_hash(B.bytes, B.safe, off, len, P.seed[round]), P.hmask);
        const uint32_t found = probe_find_or_claim(stag, smask, tag, kEmptyTag);
        slot_of[i] = found;
        if (found == kNoId) atomicOr(err, kErrFull);
        else if (sid[found] == kNoId) atomicMin(&sfirst[found], (uint32_t)i);
    }
}

// Compare every request of the round with its slot's representative; a mismatch clears
// the request's slot and lists it for the next round (wave-aggregated appends).
__global__ __launch_bounds__(kSdBlock) void k_sd_verify(SdBatch B, uint64_t n, const uint32_t *__restrict__ list,
                                                        const uint32_t *__restrict__ list_n, SdArena A,
                                                        const uint32_t *__restrict__ sid,
                                                        const uint32_t *__restrict__ sfirst,
                                                        const uint64_t *__restrict__ sloc,
                                                        uint32_t *__restrict__ slot_of,
                                                        uint32_t *__restrict__ next, uint32_t *__restrict__ next_n,
                                                        unsigned long long *__restrict__ err) {
    const uint64_t count = list ? *list_n : n;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x; t0 < count; t0 += stride) {
        const uint64_t t = t0 + threadIdx.x;
        bool moved = false;
        uint64_t i = 0;
        if (t < count) {
            i = list ? list[t] : t;
            const uint32_t s = slot_of[i];
            if (s != kNoId) {
                const uint64_t off = B.offs[i];
                const uint32_t len = (uint32_t)(B.offs[i + 1] - off);
                const uint32_t id = sid[s];
                bool eq;
                if (id != kNoId) {
                    const uint64_t loc = sloc[s];
                    eq = loc_len(loc) == len && sd_equal(A.bytes, A.safe, loc_off(loc), B.bytes, B.safe, off, len);
                } else {
                    const uint32_t j = sfirst[s];
                    if (j == (uint32_t)i) {
                        eq = true;
                    } else {
                        const uint64_t jo = B.offs[j];
                        eq = (uint32_t)(B.offs[j + 1] - jo) == len && sd_equal(B.bytes, B.safe, jo, B.bytes, B.safe, off, len);
                    }
                }
                if (!eq) {
                    slot_of[i] = kNoId;
                    moved = true;
                }
            }
        }
        const uint64_t m = __ballot(moved);
        if (m) {
            if (!next) {
                if (moved) atomicOr(err, kErrRounds);
                continue;
            }
            const int leader = __ffsll((long long)m) - 1;
            uint32_t base = 0;
            if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(next_n, (uint32_t)__popcll(m));
            base = __shfl(base, leader, 64);
            if (moved) next[base + __popcll(m & lanemask_lt())] = (uint32_t)i;
        }
    }
}

__device__ __forceinline__ uint32_t sd_room(const uint64_t *offs, uint64_t i) {
    return (uint32_t)((offs[i + 1] - offs[i] + 7) & ~7ull);
}

// Request at position t of a pass over the batch: t itself, or list[t] when the pass
// runs over an ordered list of requests (the warm path's misses, in arrival order).
__device__ __forceinline__ bool sd_at(const uint32_t *__restrict__ list, uint64_t count, uint64_t t, uint64_t &i) {
    if (t >= count) return false;
    i = list ? list[t] : t;
    return true;
}

// New keys and their arena bytes per block of kSdTile requests (of the batch, or of the
// ordered list: list / list_n).
__global__ __launch_bounds__(kSdBlock) void k_sd_count(const uint64_t *__restrict__ offs, uint64_t n,
                                                       const uint32_t *__restrict__ slot_of,
                                                       const uint32_t *__restrict__ sid,
                                                       const uint32_t *__restrict__ sfirst,
                                                       uint32_t *__restrict__ bsum, uint32_t *__restrict__ bbytes,
                                                       const uint32_t *__restrict__ list = nullptr,
                                                       const uint32_t *__restrict__ list_n = nullptr) {
    __shared__ uint32_t wsum[kSdBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kSdTile;
    const uint64_t count = list ? *list_n : n;
    uint32_t c = 0, nb = 0;
    for (int k = 0; k < kSdTile / kSdBlock; ++k) {
        uint64_t i;
        if (sd_at(list, count, base + (uint64_t)threadIdx.x * (kSdTile / kSdBlock) + k, i) &&
            is_new(slot_of, sid, sfirst, i)) {
            ++c;
            nb += sd_room(offs, i);
        }
    }
    uint32_t tc, tb;
    (void)block_excl_scan<kSdBlock>(c, wsum, &tc);
    __syncthreads();
    (void)block_excl_scan<kSdBlock>(nb, wsum, &tb);
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = tc;
        bbytes[blockIdx.x] = tb;
    }
}

// Exclusive scans of per-block counts (in place) and bytes (into u64 bbase) by one block of
// kScanThreads threads.  Returns the sum of the counts; thread kScanThreads - 1 gets the sum
// of the bytes in *bytes.
__device__ __forceinline__ uint32_t sd_scan_blocks(uint32_t *__restrict__ bsum, const uint32_t *__restrict__ bbytes,
                                                   uint64_t *__restrict__ bbase, uint32_t nblk, uint32_t *wsum,
                                                   unsigned long long *part, unsigned long long *bytes) {
    const uint32_t t = threadIdx.x;
    unsigned long long bs = 0;
    const uint32_t sum = blocks_sum(bsum, nblk, [&](uint32_t j) { bs += bbytes[j]; });
    uint32_t tot;
    const uint32_t run = block_excl_scan<kScanThreads>(sum, wsum, &tot);
    // bytes: u64 scan through LDS (one thread per 1024 partials; nblk is small)
    part[t] = bs;
    __syncthreads();
    if (t == 0) {
        unsigned long long acc = 0;
        for (uint32_t k = 0; k < kScanThreads; ++k) {
            const unsigned long long v = part[k];
            part[k] = acc;
            acc += v;
        }
    }
    __syncthreads();
    unsigned long long brun = part[t];
    blocks_write(bsum, nblk, run, [&](uint32_t j) {
        bbase[j] = brun;
        brun += bbytes[j];
    });
    *bytes = brun;
    return tot;
}

// The batch's block scans; the pool takes the batch's new keys, and the arena their text
// (beyond it: sticky error).
__global__ __launch_bounds__(kScanThreads) void k_sd_scan(uint32_t *__restrict__ bsum, const uint32_t *__restrict__ bbytes,
                                                          uint64_t *__restrict__ bbase, uint32_t nblk,
                                                          unsigned long long *__restrict__ state, uint64_t capacity,
                                                          uint64_t arena_bytes) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    __shared__ unsigned long long part[kScanThreads];
    unsigned long long brun;
    const uint32_t tot = sd_scan_blocks(bsum, bbytes, bbase, nblk, wsum, part, &brun);
    if (threadIdx.x == kScanThreads - 1) {
        state[kSdEver] += pool_take(state, tot, capacity, kErrRange);
        const unsigned long long abefore = state[kSdArena];
        state[kSdArenaBase] = abefore;
        unsigned long long aafter = abefore + brun;
        if (aafter > arena_bytes) {
            aafter = arena_bytes;
            state[kStErr] |= kErrArena | kErrRange;
        }
        state[kSdArena] = aafter;
    }
}

// Assign ids (pool_id of the rank among the batch's new keys) and store the new keys'
// text; beyond capacity or arena, none.
__global__ __launch_bounds__(kSdBlock) void k_sd_assign(SdBatch B, uint64_t n, const uint32_t *__restrict__ slot_of,
                                                        uint32_t *__restrict__ sid, const uint32_t *__restrict__ sfirst,
                                                        uint64_t *__restrict__ sloc, uint64_t *__restrict__ iloc,
                                                        uint8_t *__restrict__ arena, const uint32_t *__restrict__ bsum,
                                                        const uint64_t *__restrict__ bbase,
                                                        const unsigned long long *__restrict__ state,
                                                        uint64_t capacity, uint64_t arena_bytes, uint64_t imask,
                                                        uint32_t ish, const uint32_t *__restrict__ free_ids,
                                                        const uint32_t *__restrict__ list = nullptr,
                                                        const uint32_t *__restrict__ list_n = nullptr) {
    __shared__ uint32_t wsum[kSdBlock / 64];
    constexpr int PER = kSdTile / kSdBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kSdTile;
    const uint64_t count = list ? *list_n : n;
    bool nw[PER];
    uint64_t iv[PER];
    uint32_t c = 0, nb = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        nw[k] = sd_at(list, count, base + (uint64_t)threadIdx.x * PER + k, iv[k]) &&
                is_new(slot_of, sid, sfirst, iv[k]);
        c += nw[k];
        nb += nw[k] ? sd_room(B.offs, iv[k]) : 0u;
    }
    uint32_t tc, tb;
    uint32_t r = block_excl_scan<kSdBlock>(c, wsum, &tc);   // every thread has read sid before it returns
    __syncthreads();
    uint32_t rb = block_excl_scan<kSdBlock>(nb, wsum, &tb);
    const uint64_t fresh = state[kStFresh0], nfree = state[kStNfree0];
    const uint64_t r0 = bsum[blockIdx.x];
    const uint64_t a0 = (uint64_t)state[kSdArenaBase] + bbase[blockIdx.x];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (!nw[k]) continue;
        const uint64_t i = iv[k];
        const uint32_t id = pool_id(r0 + r++, fresh, nfree, capacity, imask, ish, free_ids);
        const uint64_t off = B.offs[i];
        const uint32_t len = (uint32_t)(B.offs[i + 1] - off);
        const uint64_t aoff = a0 + rb;
        rb += (len + 7) & ~7u;
        if (id == kNoId || aoff + ((len + 7) & ~7u) > arena_bytes) continue;
        for (uint32_t w = 0; 8u * w < len; ++w)
            *reinterpret_cast<uint64_t *>(arena + aoff + 8ull * w) = sd_word(B.bytes, B.safe, off, len, w);
        const uint64_t loc = kLocValid | (aoff << 17) | len;
        sloc[slot_of[i]] = loc;
        iloc[id] = loc;
        sid[slot_of[i]] = id;
    }
}

__global__ __launch_bounds__(kSdBlock) void k_sd_lookup(SdBatch B, uint64_t n, SdParams P,
                                                        const uint64_t *__restrict__ stag,
                                                        const uint32_t *__restrict__ sid,
                                                        const uint64_t *__restrict__ sloc, uint64_t smask, SdArena A,
                                                        uint64_t *__restrict__ ids) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t id = ~0ull;
        uint64_t off;
        uint32_t len;
        if (sd_span(B.offs, i, B.n_bytes, off, len)) {
            bool done = false;
            for (uint32_t round = 0; round < (uint32_t)kRounds && !done; ++round) {
                const uint64_t tag = sd_tag(round, sd_hash(B.bytes, B.safe, off, len, P.seed[round]), P.hmask);
                uint64_t h = mix64(tag) & smask;
                for (uint64_t probe = 0; probe <= smask; ++probe) {
                    const uint64_t cur = stag[h];
                    if (cur == kEmptyTag) {
                        done = true;   // no slot carries this tag: never assigned
                        break;
                    }
                    if (cur == tag) {
                        const uint32_t s_id = sid[h];
                        const uint64_t loc = sloc[h];
                        if (s_id != kNoId && loc_len(loc) == len &&
                            sd_equal(A.bytes, A.safe, loc_off(loc), B.bytes, B.safe, off, len)) {
                            id = s_id;
                            done = true;
                        }
                        break;         // tags are unique: try the next round's
                    }
                    h = (h + 1) & smask;
                }
            }
        }
        ids[i] = id;
    }
}

// ---------------------------------------------------------------- warm path
// Most strings of a steady-state batch are already known.  k_sd_resolve answers them the
// way a lookup does (every probe round, byte compare with the stored text) and leaves
// UINT64_MAX for the misses; a stable compaction lists the misses in arrival order, and
// the assign machinery (claim / verify rounds, count, scan, assign, gather) runs over that
// list only.  Ids are unchanged: the known strings keep theirs, and the new ones get
// counters in arrival order, exactly as a full pass assigns them.
__device__ __forceinline__ uint64_t sd_find(const SdBatch &B, uint64_t i, const SdParams &P,
                                            const uint64_t *__restrict__ stag, const uint32_t *__restrict__ sid,
                                            const uint64_t *__restrict__ sloc, uint64_t smask, const SdArena &A) {
    uint64_t off;
    uint32_t len;
    if (!sd_span(B.offs, i, B.n_bytes, off, len)) return ~0ull;   // the claim round flags it
    for (uint32_t round = 0; round < (uint32_t)kRounds; ++round) {
        const uint64_t tag = sd_tag(round, sd_hash(B.bytes, B.safe, off, len, P.seed[round]), P.hmask);
        uint64_t h = mix64(tag) & smask;
        for (uint64_t probe = 0; probe <= smask; ++probe) {
            const uint64_t cur = stag[h];
            if (cur == kEmptyTag) return ~0ull;       // never assigned
            if (cur == tag) {
                const uint32_t s_id = sid[h];
                const uint64_t loc = sloc[h];
                if (s_id != kNoId && loc_len(loc) == len &&
                    sd_equal(A.bytes, A.safe, loc_off(loc), B.bytes, B.safe, off, len))
                    return s_id;
                break;                                // tags are unique: the next round's
            }
            h = (h + 1) & smask;
        }
    }
    return ~0ull;
}

// ids[i] = the id of a known string, UINT64_MAX for a miss; bmiss[block] = its misses.
// Requests are thread-contiguous within a block (as k_sd_count), kSdTile per block.
__global__ __launch_bounds__(kSdBlock) void k_sd_resolve(SdBatch B, uint64_t n, SdParams P,
                                                         const uint64_t *__restrict__ stag,
                                                         const uint32_t *__restrict__ sid,
                                                         const uint64_t *__restrict__ sloc, uint64_t smask, SdArena A,
                                                         uint64_t *__restrict__ ids, uint32_t *__restrict__ bmiss) {
    __shared__ uint32_t wsum[kSdBlock / 64];
    constexpr int PER = kSdTile / kSdBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kSdTile;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const uint64_t i = base + (uint64_t)threadIdx.x * PER + k;
        if (i < n) {
            const uint64_t id = sd_find(B, i, P, stag, sid, sloc, smask, A);
            ids[i] = id;
            c += id == ~0ull;
        }
    }
    uint32_t tot;
    (void)block_excl_scan<kSdBlock>(c, wsum, &tot);
    if (threadIdx.x == 0) bmiss[blockIdx.x] = tot;
}

// The misses in arrival order: list[bmiss[block] + rank in block] = i.
__global__ __launch_bounds__(kSdBlock) void k_sd_compact(uint64_t n, const uint64_t *__restrict__ ids,
                                                         const uint32_t *__restrict__ bmiss,
                                                         uint32_t *__restrict__ list) {
    __shared__ uint32_t wsum[kSdBlock / 64];
    constexpr int PER = kSdTile / kSdBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kSdTile;
    bool miss[PER];
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const uint64_t i = base + (uint64_t)threadIdx.x * PER + k;
        miss[k] = i < n && ids[i] == ~0ull;
        c += miss[k];
    }
    uint32_t tot;
    uint32_t at = bmiss[blockIdx.x] + block_excl_scan<kSdBlock>(c, wsum, &tot);
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (miss[k]) list[at++] = (uint32_t)(base + (uint64_t)threadIdx.x * PER + k);
}

// ---------------------------------------------------------------- reclaim
// Removing a key in place would break the probe rounds: a key sits in round k because its
// earlier rounds' tags were taken, so an emptied slot ends other keys' lookups early, and a
// slot left tagged without an id is claimed again by the first string that hashes to it.
// A reclaim therefore rebuilds the table from its survivors (tbe_sdir_reclaim_device):
//   1. vict[id] = assigned, flagged dead and not kept; the victims, in ascending id
//      order (block counts + scan), go onto the free stack and lose their iloc;
//   2. the surviving slots are compacted in slot order: their text moves to the second
//      arena at offsets from a scan of the rounded lengths, their {tag, id, new loc} to a
//      record list, and the ones that sat in a round > 0 to the list of movers;
//   3. the slot table is reset and the survivors are put back.  A survivor may always
//      return to its own tag (tags were unique), and a mover first tries the earlier
//      rounds' tags, which removals may have freed: it takes the first round whose tag no
//      one holds, exactly the rule an assign places a new string by.  Round 0's owners
//      go in first (k_rc_place0); k_rc_place(j) then lets every unplaced mover try round
//      j and, failing that, puts round j + 1's owners back, so a try at round j + 1 (the
//      next launch) finds all of them.  No survivor ends in a later round than before.
__global__ void k_rc_flag(uint64_t capacity, const uint64_t *__restrict__ iloc, const uint8_t *__restrict__ dead,
                          uint8_t *__restrict__ vict) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < capacity; id += stride)
        vict[id] = (iloc[id] & kLocValid) && dead[id];
}

// A victim's id reads as never assigned from here on.
struct IlocForget {
    uint64_t *iloc;
    __device__ void operator()(uint64_t id) const { iloc[id] = 0; }
};

__device__ __forceinline__ bool rc_survives(const uint32_t *__restrict__ sid, const uint8_t *__restrict__ vict,
                                            uint64_t s, uint64_t nslots) {
    if (s >= nslots) return false;
    const uint32_t id = sid[s];
    return id != kNoId && !vict[id];
}

// Surviving keys and their arena bytes per block of kSdTile slots.
__global__ __launch_bounds__(kSdBlock) void k_rc_scount(uint64_t nslots, const uint32_t *__restrict__ sid,
                                                        const uint64_t *__restrict__ sloc,
                                                        const uint8_t *__restrict__ vict, uint32_t *__restrict__ bs,
                                                        uint32_t *__restrict__ bb) {
    __shared__ uint32_t wsum[kSdBlock / 64];
    constexpr int PER = kSdTile / kSdBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kSdTile + (uint64_t)threadIdx.x * PER;
    uint32_t c = 0, nb = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (rc_survives(sid, vict, base + k, nslots)) {
            ++c;
            nb += (loc_len(sloc[base + k]) + 7) & ~7u;
        }
    uint32_t tc, tb;
    (void)block_excl_scan<kSdBlock>(c, wsum, &tc);
    __syncthreads();
    (void)block_excl_scan<kSdBlock>(nb, wsum, &tb);
    if (threadIdx.x == 0) {
        bs[blockIdx.x] = tc;
        bb[blockIdx.x] = tb;
    }
}

// Scans of the survivors' block counts and bytes, and the counters after the reclaim:
// rc_n[0] victims (k_scan_blocks), [1] survivors, [2] movers listed so far.
__global__ __launch_bounds__(kScanThreads) void k_rc_scan(uint32_t *__restrict__ bs, const uint32_t *__restrict__ bb,
                                                     uint64_t *__restrict__ base, uint32_t nblk,
                                                     unsigned long long *__restrict__ state,
                                                     uint32_t *__restrict__ rc_n, uint64_t *__restrict__ n_reclaimed) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    __shared__ unsigned long long part[kScanThreads];
    unsigned long long bytes;
    const uint32_t tot = sd_scan_blocks(bs, bb, base, nblk, wsum, part, &bytes);
    if (threadIdx.x == kScanThreads - 1) {
        rc_n[1] = tot;
        rc_n[2] = 0;
        state[kSdArena] = bytes;   // the arena holds the survivors' text only
        pool_reclaimed(state, rc_n[0]);
        if (n_reclaimed) *n_reclaimed = rc_n[0];
    }
}

// The survivors, in slot order: text to the second arena, {tag, id, new loc} to the record
// list (rank = bs[block] + rank in block), the new loc to iloc; a survivor of a round > 0
// is listed as a mover (wave-aggregated appends).
__global__ __launch_bounds__(kSdBlock) void k_rc_move(uint64_t nslots, const uint64_t *__restrict__ stag,
                                                      const uint32_t *__restrict__ sid,
                                                      const uint64_t *__restrict__ sloc,
                                                      const uint8_t *__restrict__ vict,
                                                      const uint32_t *__restrict__ bs,
                                                      const uint64_t *__restrict__ bbase,
                                                      const uint8_t *__restrict__ arena, uint8_t *__restrict__ arena2,
                                                      uint64_t *__restrict__ sv_tag, uint32_t *__restrict__ sv_id,
                                                      uint64_t *__restrict__ sv_loc, uint64_t *__restrict__ iloc,
                                                      uint32_t *__restrict__ movers, uint32_t *__restrict__ rc_n) {
    __shared__ uint32_t wsum[kSdBlock / 64];
    constexpr int PER = kSdTile / kSdBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kSdTile + (uint64_t)threadIdx.x * PER;
    bool sv[PER];
    uint32_t c = 0, nb = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        sv[k] = rc_survives(sid, vict, base + k, nslots);
        c += sv[k];
        nb += sv[k] ? (loc_len(sloc[base + k]) + 7) & ~7u : 0u;
    }
    uint32_t tc, tb;
    uint32_t r = bs[blockIdx.x] + block_excl_scan<kSdBlock>(c, wsum, &tc);
    __syncthreads();
    uint64_t at = bbase[blockIdx.x] + block_excl_scan<kSdBlock>(nb, wsum, &tb);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        bool mover = false;
        uint32_t rank = 0;
        if (sv[k]) {
            const uint64_t s = base + k;
            const uint64_t loc = sloc[s], tag = stag[s];
            const uint32_t id = sid[s], len = loc_len(loc);
            const uint64_t from = loc_off(loc);
            for (uint32_t w = 0; 8u * w < len; ++w)
                *reinterpret_cast<uint64_t *>(arena2 + at + 8ull * w) =
                    *reinterpret_cast<const uint64_t *>(arena + from + 8ull * w);
            const uint64_t nloc = kLocValid | (at << 17) | len;
            at += (len + 7) & ~7u;
            rank = r++;
            sv_tag[rank] = tag;
            sv_id[rank] = id;
            sv_loc[rank] = nloc;
            iloc[id] = nloc;
            mover = (tag >> 62) != 0;
        }
        const uint64_t m = __ballot(mover);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            uint32_t mb = 0;
            if ((int)(threadIdx.x & 63) == leader) mb = atomicAdd(&rc_n[2], (uint32_t)__popcll(m));
            mb = __shfl(mb, leader, 64);
            if (mover) movers[mb + __popcll(m & lanemask_lt())] = rank;
        }
    }
}

// Round 0's owners back to their tags.
__global__ __launch_bounds__(kSdBlock) void k_rc_place0(const uint32_t *__restrict__ rc_n,
                                                        const uint64_t *__restrict__ sv_tag,
                                                        const uint32_t *__restrict__ sv_id,
                                                        const uint64_t *__restrict__ sv_loc,
                                                        uint64_t *__restrict__ stag, uint32_t *__restrict__ sid,
                                                        uint64_t *__restrict__ sloc, uint64_t smask,
                                                        unsigned long long *__restrict__ err) {
    const uint64_t count = rc_n[1];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < count; r += stride) {
        const uint64_t tag = sv_tag[r];
        if (tag >> 62) continue;
        const uint32_t h = probe_insert(stag, smask, tag, kEmptyTag);
        if (h == kNoId) {
            atomicOr(err, kErrRounds);
            continue;
        }
        sloc[h] = sv_loc[r];
        sid[h] = sv_id[r];
    }
}

// Every unplaced mover tries round j's tag of its string; one that fails and owned a tag
// of round j + 1 returns to it.  A placed mover's record tag is set to kEmptyTag.
__global__ __launch_bounds__(kSdBlock) void k_rc_place(uint32_t j, const uint32_t *__restrict__ rc_n,
                                                       const uint32_t *__restrict__ movers,
                                                       uint64_t *__restrict__ sv_tag,
                                                       const uint32_t *__restrict__ sv_id,
                                                       const uint64_t *__restrict__ sv_loc, SdArena A, SdParams P,
                                                       uint64_t *__restrict__ stag, uint32_t *__restrict__ sid,
                                                       uint64_t *__restrict__ sloc, uint64_t smask,
                                                       unsigned long long *__restrict__ err) {
    const uint64_t count = rc_n[2];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += stride) {
        const uint32_t r = movers[t];
        const uint64_t own = sv_tag[r];
        if (own == kEmptyTag) continue;
        const uint64_t loc = sv_loc[r];
        const uint64_t tag = sd_tag(j, sd_hash(A.bytes, A.safe, loc_off(loc), loc_len(loc), P.seed[j]), P.hmask);
        uint32_t h = probe_insert(stag, smask, tag, kEmptyTag);
        if (h == kNoId) {
            if ((own >> 62) != j + 1) continue;
            h = probe_insert(stag, smask, own, kEmptyTag);
            if (h == kNoId) {
                atomicOr(err, kErrRounds);
                continue;
            }
        }
        sloc[h] = loc;
        sid[h] = sv_id[r];
        sv_tag[r] = kEmptyTag;
    }
}

// Key text by id (tbe_sdir_text_lengths_device / tbe_sdir_text_device): the length from
// iloc, 0 for an id that is not held; then the bytes out of the arena into the caller's
// Arrow layout, never more than the span its offsets give the string.
__global__ void k_sd_text_len(const uint64_t *__restrict__ ids, uint64_t n, const uint64_t *__restrict__ iloc,
                              uint64_t capacity, uint64_t *__restrict__ lens,
                              unsigned long long *__restrict__ n_missing) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t id = ids[i];
        const uint64_t loc = id < capacity ? iloc[id] : 0ull;
        const bool held = (loc & kLocValid) != 0;
        lens[i] = held ? loc_len(loc) : 0u;
        if (!held && n_missing) atomicAdd(n_missing, 1ull);
    }
}

__global__ void k_sd_text(const uint64_t *__restrict__ ids, uint64_t n, const uint64_t *__restrict__ iloc,
                          uint64_t capacity, const uint8_t *__restrict__ arena, const uint64_t *__restrict__ offs,
                          uint8_t *__restrict__ bytes) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t id = ids[i];
        const uint64_t loc = id < capacity ? iloc[id] : 0ull;
        const uint64_t a = offs[i], b = offs[i + 1];
        if (!(loc & kLocValid) || b <= a) continue;
        const uint64_t len = min((uint64_t)loc_len(loc), b - a);
        const uint8_t *src = arena + loc_off(loc);
        for (uint64_t j = 0; j < len; ++j) bytes[a + j] = src[j];
    }
}

// Routing key of every held id (tbe_sdir_route_keys_device): keys[i] = sd_hash of the text id
// first + i holds, seeded as tbe_route_text_keys_device seeds the sender's copy of the same
// text; kNoKey for an id that is not held.  One id per thread: iloc is read coalesced, the
// text straight out of the arena, where every key starts on an 8-byte boundary and its last
// word is stored zero-padded, so sd_hash takes its aligned one-load path for every word
// (A.safe covers the arena's 16 spare bytes).  The trip count is uniform in a block, so the
// ballot sees whole waves: one atomic per wave and round for *n_held.
constexpr uint64_t kNoKey = ~0ull;
__global__ __launch_bounds__(kSdBlock) void k_sd_route_keys(const uint64_t *__restrict__ iloc, SdArena A,
                                                            uint64_t first, uint64_t count, uint64_t seed,
                                                            uint64_t *__restrict__ keys,
                                                            unsigned long long *__restrict__ n_held) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x; t0 < count; t0 += stride) {
        const uint64_t i = t0 + threadIdx.x;
        bool held = false;
        if (i < count) {
            const uint64_t loc = iloc[first + i];
            held = (loc & kLocValid) != 0;
            keys[i] = held ? sd_hash(A.bytes, A.safe, loc_off(loc), loc_len(loc), seed) : kNoKey;
        }
        const uint64_t m = __ballot(held);
        if (n_held && m && (threadIdx.x & 63) == 0) atomicAdd(n_held, (unsigned long long)__popcll(m));
    }
}

// Host hash of the prefix (the seeds of the four rounds derive from it).
uint64_t host_hash(const uint8_t *p, uint32_t len) {
    uint64_t h = mix64(0x243F6A8885A308D3ull ^ ((uint64_t)len * 0x9E3779B97F4A7C15ull));
    for (uint32_t k = 0; 8u * k < len; ++k) {
        uint64_t w = 0;
        for (uint32_t b = 0; b < 8 && 8u * k + b < len; ++b) w |= (uint64_t)p[8u * k + b] << (8 * b);
        h = mix64(h ^ w);
    }
    return h;
}

}  // namespace

struct tbe_string_directory {
    uint64_t capacity = 0, nslots = 0, arena_bytes = 0, arena_alloc = 0;
    int device = 0;
    uint64_t imask = 0;
    uint32_t ish = 0;
    bool used = false;
    SdParams P{};
    uint64_t *stag = nullptr;
    uint32_t *sid = nullptr;
    uint32_t *sfirst = nullptr;
    uint64_t *sloc = nullptr;
    uint64_t *iloc = nullptr;
    uint8_t *arena = nullptr;
    unsigned long long *state = nullptr;   // kStateWords counters (tbe_idpool.hpp, kSd*)
    // reclaim (allocated by the first one, sd_reclaim_scratch)
    PoolScratch pool;
    uint8_t *arena2 = nullptr;             // the arena the next reclaim compacts into
    uint64_t *sv_tag = nullptr, *sv_loc = nullptr;
    uint32_t *sv_id = nullptr, *movers = nullptr;   // survivor records / movers, capacity each
    uint32_t *rc_bs = nullptr, *rc_bb = nullptr;
    uint64_t *rc_base = nullptr;
    // per-batch scratch
    uint64_t tmp_cap = 0;
    uint32_t *slot_of = nullptr;
    uint32_t *list[2] = {nullptr, nullptr};
    uint32_t *list_n = nullptr;            // [kRounds]
    uint32_t *bsum = nullptr, *bbytes = nullptr;
    uint64_t *bbase = nullptr;
    uint32_t *miss = nullptr;              // warm path: the batch's misses, arrival order
    uint32_t *bmiss = nullptr;             // warm path: misses per block (scanned)
    // warm-path choice: 0 auto (the last observed batch's new-key share), 1 full pass, 2 warm
    int mode = 0;
    unsigned long long *h_state = nullptr; // pinned: state[kSdEver] after the last assign (async copy)
    hipEvent_t ev_state = nullptr;
    bool state_pending = false;
    unsigned long long last_ids = 0;       // ids at the previous observed copy
    uint64_t since_n = 0;                  // requests assigned since the last copy was enqueued
    uint64_t last_n = 0;                   // requests between the previous copy and the one in flight
    double new_share = 1.0;                // new keys / requests between the last two observed copies
    // host-buffer staging
    uint64_t st_bytes = 0, st_n = 0;
    uint8_t *d_bytes = nullptr;
    uint64_t *d_offs = nullptr, *d_ids = nullptr;
};

namespace {

void sd_free_scratch(tbe_string_directory *d) {
    for (void *p : {(void *)d->slot_of, (void *)d->list[0], (void *)d->list[1], (void *)d->bsum, (void *)d->bbytes,
                    (void *)d->bbase, (void *)d->miss, (void *)d->bmiss})
        if (p) (void)hipFree(p);
    d->slot_of = d->list[0] = d->list[1] = d->bsum = d->bbytes = d->miss = d->bmiss = nullptr;
    d->bbase = nullptr;
    d->tmp_cap = 0;
}

tbe_status sd_scratch(tbe_string_directory *d, uint64_t n) {
    if (n <= d->tmp_cap) return TBE_OK;
    if (hipDeviceSynchronize() != hipSuccess) return TBE_EDEVICE;   // the previous batch may use them
    sd_free_scratch(d);
    const uint64_t cap = std::max<uint64_t>(n, 1u << 16);
    const uint64_t nblk = (cap + kSdTile - 1) / kSdTile;
    if (hipMalloc(&d->slot_of, cap * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&d->list[0], cap * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&d->list[1], cap * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&d->bsum, nblk * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&d->bbytes, nblk * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&d->bbase, nblk * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&d->miss, cap * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&d->bmiss, nblk * sizeof(uint32_t)) != hipSuccess) {
        sd_free_scratch(d);
        return TBE_ENOMEM;
    }
    d->tmp_cap = cap;
    return TBE_OK;
}

void sd_free_reclaim_scratch(tbe_string_directory *d) {
    for (void *p : {(void *)d->arena2, (void *)d->sv_tag, (void *)d->sv_loc, (void *)d->sv_id, (void *)d->movers,
                    (void *)d->rc_bs, (void *)d->rc_bb, (void *)d->rc_base})
        if (p) (void)hipFree(p);
    d->arena2 = nullptr;
    d->sv_tag = d->sv_loc = d->rc_base = nullptr;
    d->sv_id = d->movers = d->rc_bs = d->rc_bb = nullptr;
    pool_scratch_free(d->pool);
}

tbe_status sd_reclaim_scratch(tbe_string_directory *d) {
    if (d->pool.free_ids) return TBE_OK;
    const uint64_t cap = d->capacity, nbs = (d->nslots + kSdTile - 1) / kSdTile;
    if (hipMalloc(&d->arena2, d->arena_alloc) == hipSuccess &&
        hipMalloc(&d->sv_tag, cap * sizeof(uint64_t)) == hipSuccess &&
        hipMalloc(&d->sv_loc, cap * sizeof(uint64_t)) == hipSuccess &&
        hipMalloc(&d->sv_id, cap * sizeof(uint32_t)) == hipSuccess &&
        hipMalloc(&d->movers, cap * sizeof(uint32_t)) == hipSuccess &&
        hipMalloc(&d->rc_bs, nbs * sizeof(uint32_t)) == hipSuccess &&
        hipMalloc(&d->rc_bb, nbs * sizeof(uint32_t)) == hipSuccess &&
        hipMalloc(&d->rc_base, nbs * sizeof(uint64_t)) == hipSuccess &&
        hipMemset(d->arena2, 0, d->arena_alloc) == hipSuccess && pool_scratch_alloc(d->pool, cap))
        return TBE_OK;
    sd_free_reclaim_scratch(d);
    return TBE_ENOMEM;
}

bool batch_ok(const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *d_offs, uint64_t n) {
    if (!d_offs || n >= (1ull << 32)) return false;
    if (n_bytes && !d_bytes) return false;
    return (reinterpret_cast<uintptr_t>(d_bytes) & 7u) == 0;
}

}  // namespace

extern "C" {

tbe_status tbe_sdir_create(uint64_t capacity, uint64_t arena_bytes, const char *prefix, uint32_t prefix_len,
                           int32_t device, tbe_string_directory **out) {
    if (!out) return TBE_EINVAL;
    *out = nullptr;
    if (capacity == 0 || capacity > 0xFFFFFFFEull || arena_bytes > (1ull << 46) || (prefix_len && !prefix))
        return TBE_EINVAL;
    tbe_string_directory *d = new (std::nothrow) tbe_string_directory();
    if (!d) return TBE_ENOMEM;
    if (device >= 0) {
        if (hipSetDevice(device) != hipSuccess) { delete d; return TBE_EDEVICE; }
        d->device = device;
    } else if (hipGetDevice(&d->device) != hipSuccess) {
        delete d;
        return TBE_EDEVICE;
    }
    d->capacity = capacity;
    d->arena_bytes = arena_bytes & ~7ull;
    d->arena_alloc = d->arena_bytes + 16;
    uint64_t ns = 1;
    while (ns < 2 * capacity) ns <<= 1;
    d->nslots = ns;
    scramble_params(capacity, d->imask, d->ish);
    const uint64_t ph = host_hash(reinterpret_cast<const uint8_t *>(prefix), prefix_len);
    for (int k = 0; k < kRounds; ++k) d->P.seed[k] = mix64(ph + (uint64_t)(k + 1) * 0x9E3779B97F4A7C15ull);
    d->P.hmask = (1ull << 62) - 1;
    bool ok = hipMalloc(&d->stag, ns * sizeof(uint64_t)) == hipSuccess &&
              hipMalloc(&d->sid, ns * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc(&d->sfirst, ns * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc(&d->sloc, ns * sizeof(uint64_t)) == hipSuccess &&
              hipMalloc(&d->iloc, capacity * sizeof(uint64_t)) == hipSuccess &&
              hipMalloc(&d->arena, d->arena_alloc) == hipSuccess &&
              hipMalloc(&d->state, kStateWords * sizeof(unsigned long long)) == hipSuccess &&
              hipMalloc(&d->list_n, (kRounds + 1) * sizeof(uint32_t)) == hipSuccess &&
              hipHostMalloc(&d->h_state, sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess &&
              hipEventCreateWithFlags(&d->ev_state, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        tbe_sdir_destroy(d);
        return TBE_ENOMEM;
    }
    k_table_init<<<grid_for(ns, 256), 256>>>(d->stag, d->sid, d->sfirst, ns, kEmptyTag);
    if (hipMemset(d->state, 0, kStateWords * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(d->arena, 0, d->arena_alloc) != hipSuccess ||
        hipMemset(d->iloc, 0, capacity * sizeof(uint64_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        tbe_sdir_destroy(d);
        return TBE_EDEVICE;
    }
    *out = d;
    return TBE_OK;
}

void tbe_sdir_destroy(tbe_string_directory *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    sd_free_scratch(d);
    sd_free_reclaim_scratch(d);
    if (d->h_state) (void)hipHostFree(d->h_state);
    if (d->ev_state) (void)hipEventDestroy(d->ev_state);
    for (void *p : {(void *)d->stag, (void *)d->sid, (void *)d->sfirst, (void *)d->sloc, (void *)d->iloc,
                    (void *)d->arena, (void *)d->state, (void *)d->list_n, (void *)d->d_bytes, (void *)d->d_offs,
                    (void *)d->d_ids})
        if (p) (void)hipFree(p);
    delete d;
}

tbe_status tbe_sdir_set_hash_bits(tbe_string_directory *d, uint32_t bits) {
    if (!d || bits == 0 || bits > 62 || d->used) return TBE_EINVAL;
    d->P.hmask = (bits == 62) ? (1ull << 62) - 1 : (1ull << bits) - 1;
    return TBE_OK;
}

tbe_status tbe_sdir_assign_device(tbe_string_directory *d, const uint8_t *d_bytes, uint64_t n_bytes,
                                  const uint64_t *d_offs, uint64_t n, uint64_t *d_ids, void *stream) {
    if (!d) return TBE_EINVAL;
    if (n == 0) return TBE_OK;
    if (!d_ids || !batch_ok(d_bytes, n_bytes, d_offs, n)) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    tbe_status rc = sd_scratch(d, n);
    if (rc != TBE_OK) return rc;
    d->used = true;
    hipStream_t st = (hipStream_t)stream;
    const SdBatch B{d_bytes, d_offs, n_bytes, n_bytes & ~7ull};
    const SdArena A{d->arena, d->arena_alloc & ~7ull};
    unsigned long long *err = d->state + kStErr;
    if (hipMemsetAsync(d->list_n, 0, (kRounds + 1) * sizeof(uint32_t), st) != hipSuccess) return TBE_EDEVICE;
    const uint64_t smask = d->nslots - 1;
    const uint32_t nblk = (uint32_t)((n + kSdTile - 1) / kSdTile);
    // The warm path pays one lookup pass over the batch to run the assign machinery over
    // its misses only: chosen while the last observed batch brought few new keys (its id
    // count is copied back asynchronously; the choice never waits for it).
    // The copy in flight holds the id count after the batch it followed; last_n counts every
    // request assigned between that copy and the previous one (several batches when copies
    // were still pending), so the share is new ids per request over exactly those batches.
    if (d->state_pending) {
        const hipError_t q = hipEventQuery(d->ev_state);
        if (q == hipSuccess) {
            d->new_share = d->last_n ? (double)(*d->h_state - d->last_ids) / (double)d->last_n : 1.0;
            d->last_ids = *d->h_state;
            d->state_pending = false;
        } else if (q != hipErrorNotReady) {
            // an unreadable copy: forget it, take the full path, and copy again below
            (void)hipGetLastError();
            d->new_share = 1.0;
            d->state_pending = false;
        }
    }
    const bool warm = d->mode == 2 || (d->mode == 0 && d->new_share < kWarmShare);
    const uint32_t *miss = warm ? d->miss : nullptr;
    const uint32_t *miss_n = warm ? d->list_n + kRounds : nullptr;
    if (warm) {
        k_sd_resolve<<<nblk, kSdBlock, 0, st>>>(B, n, d->P, d->stag, d->sid, d->sloc, smask, A, d_ids, d->bmiss);
        k_scan_blocks<<<1, kScanThreads, 0, st>>>(d->bmiss, nblk, d->list_n + kRounds);
        k_sd_compact<<<nblk, kSdBlock, 0, st>>>(n, d_ids, d->bmiss, d->miss);
    }
    for (int round = 0; round < kRounds; ++round) {
        const uint32_t *in = round ? d->list[(round - 1) & 1] : miss;
        const uint32_t *in_n = round ? d->list_n + (round - 1) : miss_n;
        uint32_t *nx = (round + 1 < kRounds) ? d->list[round & 1] : nullptr;
        uint32_t *nx_n = (round + 1 < kRounds) ? d->list_n + round : nullptr;
        const unsigned g = in ? (round ? kListGrid : grid_for(n, kSdBlock)) : grid_for(n, kSdBlock);
        k_sd_claim<<<g, kSdBlock, 0, st>>>(B, n, in, in_n, (uint32_t)round, d->P, d->stag, d->sid, d->sfirst, smask,
                                           d->slot_of, err);
        k_sd_verify<<<g, kSdBlock, 0, st>>>(B, n, in, in_n, A, d->sid, d->sfirst, d->sloc, d->slot_of, nx, nx_n, err);
    }
    k_sd_count<<<nblk, kSdBlock, 0, st>>>(d_offs, n, d->slot_of, d->sid, d->sfirst, d->bsum, d->bbytes, miss,
                                          miss_n);
    k_sd_scan<<<1, kScanThreads, 0, st>>>(d->bsum, d->bbytes, d->bbase, nblk, d->state, d->capacity, d->arena_bytes);
    k_sd_assign<<<nblk, kSdBlock, 0, st>>>(B, n, d->slot_of, d->sid, d->sfirst, d->sloc, d->iloc, d->arena, d->bsum,
                                           d->bbase, d->state, d->capacity, d->arena_bytes, d->imask, d->ish,
                                           d->pool.free_ids, miss, miss_n);
    k_gather<<<grid_for(n, 256), 256, 0, st>>>(d->slot_of, n, d->sid, d_ids, miss, miss_n);
    d->since_n += n;
    if (!d->state_pending) {
        // the id count after this batch, for a later call's choice
        if (hipMemcpyAsync(d->h_state, d->state + kSdEver, sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipEventRecord(d->ev_state, st) != hipSuccess)
            return TBE_EDEVICE;
        d->state_pending = true;
        d->last_n = d->since_n;
        d->since_n = 0;
    }
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_sdir_set_mode(tbe_string_directory *d, int32_t mode) {
    if (!d || mode < 0 || mode > 2) return TBE_EINVAL;
    d->mode = mode;
    return TBE_OK;
}

tbe_status tbe_sdir_lookup_device(tbe_string_directory *d, const uint8_t *d_bytes, uint64_t n_bytes,
                                  const uint64_t *d_offs, uint64_t n, uint64_t *d_ids, void *stream) {
    if (!d) return TBE_EINVAL;
    if (n == 0) return TBE_OK;
    if (!d_ids || !batch_ok(d_bytes, n_bytes, d_offs, n)) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    const SdBatch B{d_bytes, d_offs, n_bytes, n_bytes & ~7ull};
    const SdArena A{d->arena, d->arena_alloc & ~7ull};
    k_sd_lookup<<<grid_for(n, kSdBlock), kSdBlock, 0, (hipStream_t)stream>>>(B, n, d->P, d->stag, d->sid, d->sloc,
                                                                            d->nslots - 1, A, d_ids);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_sdir_assign(tbe_string_directory *d, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *offs,
                           uint64_t n, uint64_t *ids) {
    if (!d) return TBE_EINVAL;
    if (n == 0) return TBE_OK;
    if (!offs || !ids || (n_bytes && !bytes) || n >= (1ull << 32)) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    if (n_bytes > d->st_bytes || n > d->st_n) {
        if (hipDeviceSynchronize() != hipSuccess) return TBE_EDEVICE;
        for (void *p : {(void *)d->d_bytes, (void *)d->d_offs, (void *)d->d_ids})
            if (p) (void)hipFree(p);
        d->d_bytes = nullptr;
        d->d_offs = d->d_ids = nullptr;
        d->st_bytes = d->st_n = 0;
        const uint64_t nb = std::max<uint64_t>(n_bytes, 1u << 16), nn = std::max<uint64_t>(n, 1u << 12);
        if (hipMalloc(&d->d_bytes, nb + 8) != hipSuccess || hipMalloc(&d->d_offs, (nn + 1) * sizeof(uint64_t)) != hipSuccess ||
            hipMalloc(&d->d_ids, nn * sizeof(uint64_t)) != hipSuccess)
            return TBE_ENOMEM;
        d->st_bytes = nb;
        d->st_n = nn;
    }
    if ((n_bytes && hipMemcpy(d->d_bytes, bytes, n_bytes, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(d->d_offs, offs, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess)
        return TBE_EDEVICE;
    tbe_status rc = tbe_sdir_assign_device(d, d->d_bytes, n_bytes, d->d_offs, n, d->d_ids, nullptr);
    if (rc != TBE_OK) return rc;
    return hipMemcpy(ids, d->d_ids, n * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_sdir_size(tbe_string_directory *d, uint64_t *n_ids) {
    if (!d || !n_ids) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return TBE_EDEVICE;
    unsigned long long st[kStateWords] = {0};
    if (hipMemcpy(st, d->state, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) return TBE_EDEVICE;
    *n_ids = st[kStFresh] - st[kStNfree];   // counters handed out less the ids waiting on the free stack
    if (st[kStErr] & (kErrRange | kErrRounds | kErrArena | kErrFull)) return TBE_ERANGE;
    return (st[kStErr] & kErrBatch) ? TBE_EINVAL : TBE_OK;
}

tbe_status tbe_sdir_usage(tbe_string_directory *d, uint64_t out[3]) {
    if (!d || !out) return TBE_EINVAL;
    const tbe_status rc = tbe_sdir_size(d, &out[0]);
    if (rc == TBE_EDEVICE) return rc;
    unsigned long long used = 0;
    if (hipMemcpy(&used, d->state + kSdArena, sizeof used, hipMemcpyDeviceToHost) != hipSuccess) return TBE_EDEVICE;
    out[1] = used;
    out[2] = d->arena_bytes;
    return rc;
}

tbe_status tbe_sdir_route_keys_device(tbe_string_directory *d, uint64_t seed, uint64_t first, uint64_t count,
                                      uint64_t *d_keys, uint64_t *d_n_held, void *stream) {
    if (!d || !d_keys || first > d->capacity || count > d->capacity - first) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (d_n_held && hipMemsetAsync(d_n_held, 0, sizeof(uint64_t), st) != hipSuccess) return TBE_EDEVICE;
    if (count == 0) return TBE_OK;
    const SdArena A{d->arena, d->arena_alloc & ~7ull};
    k_sd_route_keys<<<grid_for(count, kSdBlock), kSdBlock, 0, st>>>(d->iloc, A, first, count, seed, d_keys,
                                                                   reinterpret_cast<unsigned long long *>(d_n_held));
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_sdir_reclaim_device(tbe_string_directory *d, const uint8_t *d_dead, const uint64_t *d_keep_ids,
                                   uint64_t n_keep, uint64_t *d_n_reclaimed, void *stream) {
    if (!d || !d_dead || (n_keep && !d_keep_ids)) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    const tbe_status rc = sd_reclaim_scratch(d);
    if (rc != TBE_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t cap = d->capacity, ns = d->nslots, smask = ns - 1;
    const uint32_t nbi = (uint32_t)((cap + kPoolTile - 1) / kPoolTile), nbs = (uint32_t)((ns + kSdTile - 1) / kSdTile);
    unsigned long long *err = d->state + kStErr;
    const PoolScratch &p = d->pool;
    k_rc_flag<<<grid_for(cap, 256), 256, 0, st>>>(cap, d->iloc, d_dead, p.vict);
    if (n_keep) k_pool_keep<<<grid_for(n_keep, 256), 256, 0, st>>>(d_keep_ids, n_keep, cap, p.vict);
    k_pool_vcount<<<nbi, kPoolBlock, 0, st>>>(cap, p.vict, p.rc_bv);
    k_scan_blocks<<<1, kScanThreads, 0, st>>>(p.rc_bv, nbi, p.rc_n);
    k_pool_vpush<<<nbi, kPoolBlock, 0, st>>>(cap, p.vict, p.rc_bv, d->state, p.free_ids, IlocForget{d->iloc});
    k_rc_scount<<<nbs, kSdBlock, 0, st>>>(ns, d->sid, d->sloc, p.vict, d->rc_bs, d->rc_bb);
    k_rc_scan<<<1, kScanThreads, 0, st>>>(d->rc_bs, d->rc_bb, d->rc_base, nbs, d->state, p.rc_n, d_n_reclaimed);
    k_rc_move<<<nbs, kSdBlock, 0, st>>>(ns, d->stag, d->sid, d->sloc, p.vict, d->rc_bs, d->rc_base, d->arena,
                                        d->arena2, d->sv_tag, d->sv_id, d->sv_loc, d->iloc, d->movers, p.rc_n);
    k_table_init<<<grid_for(ns, 256), 256, 0, st>>>(d->stag, d->sid, d->sfirst, ns, kEmptyTag);
    std::swap(d->arena, d->arena2);   // every later call reads the compacted arena
    const SdArena A{d->arena, d->arena_alloc & ~7ull};
    k_rc_place0<<<grid_for(cap, kSdBlock), kSdBlock, 0, st>>>(p.rc_n, d->sv_tag, d->sv_id, d->sv_loc, d->stag, d->sid,
                                                            d->sloc, smask, err);
    for (uint32_t j = 0; j + 1 < (uint32_t)kRounds; ++j)
        k_rc_place<<<kListGrid, kSdBlock, 0, st>>>(j, p.rc_n, d->movers, d->sv_tag, d->sv_id, d->sv_loc, A, d->P,
                                                   d->stag, d->sid, d->sloc, smask, err);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_sdir_reclaim(tbe_string_directory *d, tbe_engine *engine, int64_t ts_us, const uint64_t *keep_ids,
                            uint64_t n_keep, uint64_t *n_reclaimed) {
    if (!d) return TBE_EINVAL;
    return pool_reclaim_sync(d->pool, d->device, d->capacity, engine, ts_us, keep_ids, n_keep, n_reclaimed,
                             [d](const uint8_t *dead, const uint64_t *keep, uint64_t nk, uint64_t *count) {
                                 return tbe_sdir_reclaim_device(d, dead, keep, nk, count, nullptr);
                             });
}

tbe_status tbe_sdir_text_lengths_device(tbe_string_directory *d, const uint64_t *d_ids, uint64_t n, uint64_t *d_lens,
                                        uint64_t *d_n_missing, void *stream) {
    if (!d) return TBE_EINVAL;
    if (n && (!d_ids || !d_lens)) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (d_n_missing && hipMemsetAsync(d_n_missing, 0, sizeof(uint64_t), st) != hipSuccess) return TBE_EDEVICE;
    if (n == 0) return TBE_OK;
    k_sd_text_len<<<grid_for(n, 256), 256, 0, st>>>(d_ids, n, d->iloc, d->capacity, d_lens,
                                                   reinterpret_cast<unsigned long long *>(d_n_missing));
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_sdir_text_device(tbe_string_directory *d, const uint64_t *d_ids, uint64_t n, const uint64_t *d_offs,
                                uint8_t *d_bytes, void *stream) {
    if (!d) return TBE_EINVAL;
    if (n == 0) return TBE_OK;
    if (!d_ids || !d_offs || !d_bytes) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    k_sd_text<<<grid_for(n, 256), 256, 0, (hipStream_t)stream>>>(d_ids, n, d->iloc, d->capacity, d->arena, d_offs,
                                                                d_bytes);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_sdir_key_of(tbe_string_directory *d, uint64_t id, uint8_t *buf, uint64_t cap, uint64_t *len) {
    if (!d || !len || (cap && !buf) || id >= d->capacity) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return TBE_EDEVICE;
    uint64_t loc = 0;   // iloc is zero for ids never assigned
    if (hipMemcpy(&loc, d->iloc + id, sizeof loc, hipMemcpyDeviceToHost) != hipSuccess) return TBE_EDEVICE;
    if (!(loc & kLocValid)) return TBE_EINVAL;
    *len = loc_len(loc);
    const uint64_t m = std::min<uint64_t>(loc_len(loc), cap);
    if (m && hipMemcpy(buf, d->arena + loc_off(loc), m, hipMemcpyDeviceToHost) != hipSuccess) return TBE_EDEVICE;
    return TBE_OK;
}

}  // extern "C"
