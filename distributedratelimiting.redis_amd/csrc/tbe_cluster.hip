// tbe_cluster.hip -- multi-GPU data path (include/tbe_cluster.h): stable
// routing partition of request batches by owner GPU and the per-GPU key directory.
//
// Routing: the reference serialises every client's script calls in one Redis (README:1-9),
// so any order in which a key's requests reach it is a valid serial order.  A batch that
// arrives at one GPU is grouped by owner with a stable partition (arrival order kept per
// owner); the all-to-all concatenates the groups by source rank, so each owner applies a
// key's requests in (source rank, arrival) order.
//
// Directory: InstanceName + resourceID is an exact string in Redis (PTB:42), never a
// hash; the directory keeps whole keys, so two keys never share a bucket.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "../../include/tbe_cluster.h"
#include "tbe_device.hpp"
#include "tbe_hash.hpp"
#include "tbe_idpool.hpp"
#include "tbe_text.hpp"

using namespace tbe;

namespace {

constexpr int kRtBlock = 512;
constexpr int kRtItems = 8;
constexpr int kRtTile = kRtBlock * kRtItems;   // 4096 requests per routing tile
constexpr uint32_t kMaxOwners = 256;

// Owner of a key: the hash partition, or the owner map's entry for its virtual node
// (`m` = the workgroup's LDS copy of the map, filled by load_owner_map).
__device__ __forceinline__ uint32_t route_owner(uint64_t key, uint32_t G, const uint8_t *m) {
    return m ? (uint32_t)m[key_vnode(key)] : key_owner(key, G);
}
// Entries >= G are clamped to G - 1 on the way into LDS, so a malformed map (the header
// requires every entry < n_owners; cluster.py validates before calling) misroutes requests
// but can never index the per-owner arrays out of bounds.
__device__ __forceinline__ const uint8_t *load_owner_map(const uint8_t *__restrict__ omap, uint8_t *lds,
                                                         uint32_t G) {
    if (!omap) return nullptr;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(omap);
    uint32_t *dst = reinterpret_cast<uint32_t *>(lds);
    const uint32_t top = G - 1u;
    for (uint32_t j = threadIdx.x; j < kOwnerMapSize / 4; j += blockDim.x) {
        const uint32_t w = src[j];
        uint32_t o = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) o |= min((w >> (8 * b)) & 0xFFu, top) << (8 * b);
        dst[j] = o;
    }
    __syncthreads();
    return lds;
}

// Per-tile request count of every owner.
__global__ __launch_bounds__(kRtBlock) void k_route_count(const uint64_t *__restrict__ keys, uint64_t n,
                                                          uint32_t G, const uint8_t *__restrict__ omap,
                                                          uint32_t *__restrict__ tile_counts) {
    __shared__ uint32_t c[kMaxOwners];
    __shared__ __attribute__((aligned(16))) uint8_t mlds[kOwnerMapSize];
    const int tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kRtTile;
    for (uint32_t j = tid; j < G; j += kRtBlock) c[j] = 0;
    const uint8_t *m = load_owner_map(omap, mlds, G);   // (its barrier also publishes c[])
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kRtItems; ++it) {
        const uint64_t i = base + (uint64_t)it * kRtBlock + tid;
        if (i < n) atomicAdd(&c[route_owner(keys[i], G, m)], 1u);
    }
    __syncthreads();
    for (uint32_t j = tid; j < G; j += kRtBlock) tile_counts[(uint64_t)blockIdx.x * G + j] = c[j];
}

// One workgroup: per owner, the exclusive scan of its tile counts (in place) and its
// total; then owner bases (exclusive scan over owners).
__global__ __launch_bounds__(kScanThreads) void k_route_scan(uint32_t *__restrict__ tile_counts, uint32_t ntiles,
                                                             uint32_t G, uint64_t *__restrict__ owner_counts,
                                                             uint32_t *__restrict__ owner_base) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    __shared__ uint32_t totals[kMaxOwners];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (ntiles + kScanThreads - 1) / kScanThreads;
    for (uint32_t o = 0; o < G; ++o) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < per; ++k) {
            const uint32_t tile = t * per + k;
            if (tile < ntiles) sum += tile_counts[(uint64_t)tile * G + o];
        }
        uint32_t tot;
        uint32_t run = block_excl_scan<kScanThreads>(sum, wsum, &tot);
        for (uint32_t k = 0; k < per; ++k) {
            const uint32_t tile = t * per + k;
            if (tile < ntiles) {
                const uint32_t c = tile_counts[(uint64_t)tile * G + o];
                tile_counts[(uint64_t)tile * G + o] = run;
                run += c;
            }
        }
        if (t == 0) totals[o] = tot;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t acc = 0;
        for (uint32_t o = 0; o < G; ++o) {
            owner_base[o] = acc;
            owner_counts[o] = totals[o];
            acc += totals[o];
        }
    }
}

// Position of every request in the owner-grouped order: owner base + the tile's offset
// in that owner's group + the request's stable rank among the tile's requests of that
// owner (wave ballot-match ranking, as the partition passes use).
__global__ __launch_bounds__(kRtBlock) void k_route_pos(const uint64_t *__restrict__ keys, uint64_t n, uint32_t G,
                                                        const uint8_t *__restrict__ omap,
                                                        const uint32_t *__restrict__ tile_off,
                                                        const uint32_t *__restrict__ owner_base,
                                                        uint32_t *__restrict__ pos) {
    __shared__ RankLds<kRtBlock> L;
    __shared__ uint16_t cnt[kRtItems * (kRtBlock / 64) * kDigits];
    __shared__ __attribute__((aligned(16))) uint8_t mlds[kOwnerMapSize];
    const int tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kRtTile;
    const int nvalid = (int)min<uint64_t>(kRtTile, n - base);
    const uint8_t *m = load_owner_map(omap, mlds, G);
    uint32_t own[kRtItems], lpos[kRtItems];
#pragma unroll
    for (int it = 0; it < kRtItems; ++it) {
        const int e = it * kRtBlock + tid;
        own[it] = e < nvalid ? route_owner(keys[base + e], G, m) : 0u;
    }
    rank_tile<kRtBlock, kRtItems>(own, 0, nvalid, L, cnt, lpos);
#pragma unroll
    for (int it = 0; it < kRtItems; ++it) {
        const int e = it * kRtBlock + tid;
        if (e < nvalid) {
            const uint32_t o = own[it];
            pos[base + e] = owner_base[o] + tile_off[(uint64_t)blockIdx.x * G + o] + lpos[it] - L.lstart[o];
        }
    }
}

// Requests per virtual node (owner-map balancing): an LDS histogram per workgroup over a
// grid-stride range, added to the 4096 global counters once.
__global__ __launch_bounds__(kRtBlock) void k_vnode_count(const uint64_t *__restrict__ keys, uint64_t n,
                                                          unsigned long long *__restrict__ counts) {
    __shared__ uint32_t h[kOwnerMapSize];
    for (uint32_t j = threadIdx.x; j < kOwnerMapSize; j += kRtBlock) h[j] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * kRtBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kRtBlock + threadIdx.x; i < n; i += stride)
        atomicAdd(&h[key_vnode(keys[i])], 1u);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < kOwnerMapSize; j += kRtBlock)
        if (h[j]) atomicAdd(&counts[j], (unsigned long long)h[j]);
}

__global__ void k_route_pack(const uint32_t *__restrict__ pos, uint64_t n, const uint64_t *__restrict__ keys,
                             const int32_t *__restrict__ permits, const int64_t *__restrict__ ts,
                             int64_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t q = (uint64_t)pos[i] * 3;
        out[q] = (int64_t)keys[i];
        out[q + 1] = ts[i];
        out[q + 2] = permits[i];
    }
}

__global__ void k_route_gather(const uint32_t *__restrict__ pos, uint64_t n, const int64_t *__restrict__ in,
                               uint32_t cols, int64_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t q = (uint64_t)pos[i] * cols;
        for (uint32_t c = 0; c < cols; ++c) out[i * cols + c] = in[q + c];
    }
}

// ---------------------------------------------------------------- routing text
// A batch keyed by text (include/tbe_cluster.h "Routing text") is grouped by the owner of
// H(text, seed), and each string travels with its bytes: the send buffer holds the strings
// of owner 0, 1, ... tightly packed, arrival order inside an owner, so string i lands at
// send_offs[pos[i]], the exclusive scan of the lengths in grouped order.  The scan is three
// launches (block sums, one workgroup over the sums, write), as the directories' scans are.
constexpr uint32_t kRtMaxLen = 1u << 16;   // a key's longest text (sd_span, tbe_strdir.hip)
constexpr int kTxBlock = 256;
constexpr int kTxTile = 1024;              // lengths per scan block (4 per thread)

// Span of string i by sd_span's rules; a malformed one reads as the empty string (false).
__device__ __forceinline__ bool rt_span(const uint64_t *__restrict__ offs, uint64_t i, uint64_t n_bytes,
                                        uint64_t &off, uint32_t &len) {
    const uint64_t a = offs[i], b = offs[i + 1];
    const bool ok = b >= a && b <= n_bytes && b - a <= kRtMaxLen;
    off = ok ? a : 0ull;
    len = ok ? (uint32_t)(b - a) : 0u;
    return ok;
}

__global__ __launch_bounds__(kTxBlock) void k_rt_text_keys(const uint8_t *__restrict__ bytes, uint64_t n_bytes,
                                                           const uint64_t *__restrict__ offs, uint64_t n,
                                                           uint64_t seed, uint64_t *__restrict__ keys,
                                                           unsigned long long *__restrict__ n_bad) {
    const uint64_t safe = n_bytes & ~7ull;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t off;
        uint32_t len;
        if (!rt_span(offs, i, n_bytes, off, len)) atomicAdd(n_bad, 1ull);
        keys[i] = sd_hash(bytes, safe, off, len, seed);
    }
}

// lens[pos[i]] = length of string i: the lengths in owner-grouped order.
__global__ __launch_bounds__(kTxBlock) void k_rt_len_scatter(const uint64_t *__restrict__ offs, uint64_t n,
                                                             uint64_t n_bytes, const uint32_t *__restrict__ pos,
                                                             uint32_t *__restrict__ lens) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t off;
        uint32_t len;
        (void)rt_span(offs, i, n_bytes, off, len);
        const uint32_t p = pos[i];
        if (p < n) lens[p] = len;
    }
}

// Where the scan reads length j: the scattered lengths of the sender, column 0 of the
// receiver's rows (a length outside 0..65536 counts as 65536: the directory then refuses the
// batch, whose offsets pass its bytes).
struct LenOfList {
    const uint32_t *lens;
    __device__ uint32_t operator()(uint64_t j) const { return lens[j]; }
};
struct LenOfRows {
    const int64_t *rows;
    __device__ uint32_t operator()(uint64_t j) const {
        const uint64_t v = (uint64_t)rows[3 * j];
        return v > kRtMaxLen ? kRtMaxLen : (uint32_t)v;
    }
};

// Bytes per block of kTxTile lengths (thread-contiguous; at most 2^26).
template <class Len>
__global__ __launch_bounds__(kTxBlock) void k_rt_len_count(Len len_of, uint64_t n, uint32_t *__restrict__ bsum) {
    __shared__ uint32_t wsum[kTxBlock / 64];
    constexpr int PER = kTxTile / kTxBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kTxTile + (uint64_t)threadIdx.x * PER;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) c += base + k < n ? len_of(base + k) : 0u;
    uint32_t tot;
    (void)block_excl_scan<kTxBlock>(c, wsum, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// One workgroup: bbase[b] (u64) = bytes before block b; offs_out[n] = all bytes.
__global__ __launch_bounds__(kScanThreads) void k_rt_len_scan(const uint32_t *__restrict__ bsum, uint32_t nblk,
                                                              uint64_t *__restrict__ bbase,
                                                              uint64_t *__restrict__ total) {
    __shared__ unsigned long long part[kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nblk + kScanThreads - 1) / kScanThreads;
    unsigned long long s = 0;
    for (uint32_t k = 0; k < per; ++k) {
        const uint32_t j = t * per + k;
        if (j < nblk) s += bsum[j];
    }
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        unsigned long long acc = 0;
        for (uint32_t k = 0; k < kScanThreads; ++k) {
            const unsigned long long v = part[k];
            part[k] = acc;
            acc += v;
        }
        *total = acc;
    }
    __syncthreads();
    unsigned long long run = part[t];
    for (uint32_t k = 0; k < per; ++k) {
        const uint32_t j = t * per + k;
        if (j < nblk) {
            bbase[j] = run;
            run += bsum[j];
        }
    }
}

// offs_out[j] = bytes before length j.
template <class Len>
__global__ __launch_bounds__(kTxBlock) void k_rt_len_write(Len len_of, uint64_t n, const uint64_t *__restrict__ bbase,
                                                           uint64_t *__restrict__ offs_out) {
    __shared__ uint32_t wsum[kTxBlock / 64];
    constexpr int PER = kTxTile / kTxBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kTxTile + (uint64_t)threadIdx.x * PER;
    uint32_t l[PER], c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        l[k] = base + k < n ? len_of(base + k) : 0u;
        c += l[k];
    }
    uint32_t tot;
    uint64_t at = bbase[blockIdx.x] + block_excl_scan<kTxBlock>(c, wsum, &tot);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (base + k < n) offs_out[base + k] = at;
        at += l[k];
    }
}

// Bytes per owner: the span of its group in the send offsets (counts: tbe_route_plan_map_device's).
__global__ __launch_bounds__(kMaxOwners) void k_rt_owner_bytes(const uint64_t *__restrict__ counts, uint32_t G,
                                                               uint64_t n, const uint64_t *__restrict__ send_offs,
                                                               uint64_t *__restrict__ byte_counts) {
    const uint32_t o = threadIdx.x;
    if (o >= G) return;
    uint64_t start = 0;
    for (uint32_t j = 0; j < o; ++j) start += counts[j];
    const uint64_t a = min(start, n), b = min(start + counts[o], n);
    byte_counts[o] = send_offs[b] - send_offs[a];
}

// String i to out_bytes[send_offs[pos[i]] ..) and its record {len, ts_us, permits} to row
// pos[i].  Neighbouring strings share the 8-byte granules of the destination, so a thread
// stores whole words only where all eight bytes are its own string's: the bytes up to the
// first 8-byte boundary and those after the last one go out one by one.  The source is
// read through sd_word (8 bytes at any alignment, never outside [0, n_bytes)).  A string
// that would pass out_cap is left out (a malformed batch's spans may overlap).
__global__ __launch_bounds__(kTxBlock) void k_rt_text_pack(const uint8_t *__restrict__ bytes, uint64_t n_bytes,
                                                           const uint64_t *__restrict__ offs, uint64_t n,
                                                           const uint32_t *__restrict__ pos,
                                                           const uint64_t *__restrict__ send_offs,
                                                           const int32_t *__restrict__ permits,
                                                           const int64_t *__restrict__ ts,
                                                           uint8_t *__restrict__ out, uint64_t out_cap,
                                                           int64_t *__restrict__ rows) {
    const uint64_t safe = n_bytes & ~7ull;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t off;
        uint32_t len;
        (void)rt_span(offs, i, n_bytes, off, len);
        const uint64_t p = pos[i];
        if (p >= n) continue;
        rows[3 * p] = len;
        rows[3 * p + 1] = ts[i];
        rows[3 * p + 2] = permits[i];
        const uint64_t d = send_offs[p];
        if (len == 0 || d > out_cap || out_cap - d < len) continue;
        const uint32_t lead = min(len, (uint32_t)((8u - (uint32_t)(d & 7)) & 7u));
        if (lead) {
            const uint64_t w = sd_word(bytes, safe, off, len, 0);
            for (uint32_t b = 0; b < lead; ++b) out[d + b] = (uint8_t)(w >> (8 * b));
        }
        const uint64_t o2 = off + lead, d2 = d + lead;   // d2 is 8-byte aligned (or the string has ended)
        const uint32_t l2 = len - lead;
        for (uint32_t k = 0; 8u * k < l2; ++k) {
            const uint64_t w = sd_word(bytes, safe, o2, l2, k);
            const uint32_t rem = l2 - 8u * k;
            if (rem >= 8) {
                *reinterpret_cast<uint64_t *>(out + d2 + 8ull * k) = w;
            } else {
                for (uint32_t b = 0; b < rem; ++b) out[d2 + 8ull * k + b] = (uint8_t)(w >> (8 * b));
            }
        }
    }
}

// The exclusive scan of n lengths into d_offs[n + 1] (n > 0); bbase and bsum: nblk entries each.
template <class Len>
void text_scan(Len len_of, uint64_t n, uint64_t *bbase, uint32_t *bsum, uint64_t *d_offs, hipStream_t st) {
    const uint32_t nblk = (uint32_t)((n + kTxTile - 1) / kTxTile);
    k_rt_len_count<<<nblk, kTxBlock, 0, st>>>(len_of, n, bsum);
    k_rt_len_scan<<<1, kScanThreads, 0, st>>>(bsum, nblk, bbase, d_offs + n);
    k_rt_len_write<<<nblk, kTxBlock, 0, st>>>(len_of, n, bbase, d_offs);
}

// ---------------------------------------------------------------- directory
constexpr uint64_t kEmptyKey = ~0ull;
constexpr int kDirBlock = 256;
constexpr int kDirTile = 1024;   // requests per flag block (4 per thread)
// The directory's own state[] words, beside the id pool's (tbe_idpool.hpp): keys held =
// fresh - nfree; the value of kDirEver that the id -> key table covers; ids ever handed out
// (only grows).
enum : int { kDirHeld = 0, kDirRevCovers = 3, kDirEver = 4 };
// state[kStErr]: a UINT64_MAX key or a full table; more new keys than room
constexpr unsigned long long kErrTable = 1, kErrRange = 2;

// Find or claim the slot of every key (linear probing on the whole key); a slot claimed
// in this batch records the arrival index of its first request (atomicMin).
__global__ __launch_bounds__(kDirBlock) void k_dir_claim(const uint64_t *__restrict__ keys, uint64_t n,
                                                         uint64_t *__restrict__ skey,
                                                         const uint32_t *__restrict__ sid,
                                                         uint32_t *__restrict__ sfirst, uint64_t smask,
                                                         uint32_t *__restrict__ slot_of,
                                                         unsigned long long *__restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t key = keys[i];
        const uint32_t found = key != kEmptyKey ? probe_find_or_claim(skey, smask, key, kEmptyKey) : kNoId;
        slot_of[i] = found;
        if (found == kNoId) {
            atomicOr(err, kErrTable);
        } else if (sid[found] == kNoId) {
            atomicMin(&sfirst[found], (uint32_t)i);
        }
    }
}

// New keys per block of kDirTile requests.
__global__ __launch_bounds__(kDirBlock) void k_dir_count(const uint32_t *__restrict__ slot_of, uint64_t n,
                                                         const uint32_t *__restrict__ sid,
                                                         const uint32_t *__restrict__ sfirst,
                                                         uint32_t *__restrict__ bsum) {
    __shared__ uint32_t wsum[kDirBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kDirTile;
    uint32_t c = 0;
    for (int k = 0; k < kDirTile / kDirBlock; ++k) {
        const uint64_t i = base + (uint64_t)threadIdx.x * (kDirTile / kDirBlock) + k;
        if (i < n && is_new(slot_of, sid, sfirst, i)) ++c;
    }
    uint32_t tot;
    (void)block_excl_scan<kDirBlock>(c, wsum, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// Exclusive scan of the block counts (in place), and the pool takes the batch's new keys.
// Without a reclaim the stack stays empty and keys held = fresh advances by the new keys,
// clamped at capacity.
__global__ __launch_bounds__(kScanThreads) void k_dir_scan(uint32_t *__restrict__ bsum, uint32_t nblk,
                                                           unsigned long long *__restrict__ state,
                                                           uint64_t capacity) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    const uint32_t tot = scan_blocks(bsum, nblk, wsum);
    if (threadIdx.x == 0) {
        state[kDirEver] += pool_take(state, tot, capacity, kErrRange);
        state[kDirHeld] = state[kStFresh] - state[kStNfree];
    }
}

// Assign ids to the new keys: rank among the batch's new keys = block prefix + rank in
// block, id by pool_id.
__global__ __launch_bounds__(kDirBlock) void k_dir_assign(const uint32_t *__restrict__ slot_of, uint64_t n,
                                                          uint32_t *__restrict__ sid,
                                                          const uint32_t *__restrict__ sfirst,
                                                          const uint32_t *__restrict__ bsum,
                                                          const unsigned long long *__restrict__ state,
                                                          uint64_t capacity, uint64_t imask, uint32_t ish,
                                                          const uint32_t *__restrict__ free_ids) {
    __shared__ uint32_t wsum[kDirBlock / 64];
    constexpr int PER = kDirTile / kDirBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kDirTile;
    bool nw[PER];
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const uint64_t i = base + (uint64_t)threadIdx.x * PER + k;
        nw[k] = i < n && is_new(slot_of, sid, sfirst, i);
        c += nw[k];
    }
    uint32_t tot;
    uint32_t r = block_excl_scan<kDirBlock>(c, wsum, &tot);   // every thread has read sid before it returns
    const uint64_t fresh = state[kStFresh0], nfree = state[kStNfree0];
    const uint64_t r0 = bsum[blockIdx.x];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (!nw[k]) continue;
        const uint64_t i = base + (uint64_t)threadIdx.x * PER + k;
        const uint32_t id = pool_id(r0 + r++, fresh, nfree, capacity, imask, ish, free_ids);
        if (id != kNoId) sid[slot_of[i]] = id;
    }
}

// Read-only lookup: id, or UINT64_MAX for a key the directory has never assigned.
__global__ __launch_bounds__(kDirBlock) void k_dir_lookup(const uint64_t *__restrict__ keys, uint64_t n,
                                                          const uint64_t *__restrict__ skey,
                                                          const uint32_t *__restrict__ sid, uint64_t smask,
                                                          uint64_t *__restrict__ ids) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t key = keys[i];
        uint64_t id = ~0ull;
        if (key != kEmptyKey) {
            uint64_t h = mix64(key) & smask;
            for (uint64_t probe = 0; probe <= smask; ++probe) {
                const uint64_t cur = skey[h];
                if (cur == key) {
                    if (sid[h] != kNoId) id = sid[h];
                    break;
                }
                if (cur == kEmptyKey) break;
                h = (h + 1) & smask;
            }
        }
        ids[i] = id;
    }
}

// Reverse lookup (tbe_dir_keys_of_device): rev[id] = the key holding id, built from the
// slots whenever ids have been handed out since the last build (state[kDirRevCovers] = the
// value of state[kDirEver], ids ever handed out, that the table covers; the keys held would not do, since
// a reclaim and an assign can bring them back to the same number).  A build only adds
// entries to the table, which starts as all UINT64_MAX; ids are taken back by a reclaim
// alone, which clears its victims' entries itself (RevForget) and sets state[kDirRevCovers]
// to UINT64_MAX, so the next call builds again whether or not an assign came in between.
__global__ void k_dir_rev_build(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sid,
                                uint64_t nslots, const unsigned long long *__restrict__ state, uint64_t capacity,
                                uint64_t *__restrict__ rev) {
    if (state[kDirRevCovers] == state[kDirEver]) return;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nslots; j += stride) {
        const uint32_t id = sid[j];
        if (id != kNoId && id < capacity) rev[id] = skey[j];
    }
}

// (runs after k_dir_rev_build on the same stream, so it also records what the table covers)
__global__ void k_dir_keys_of(const uint64_t *__restrict__ ids, uint64_t n, const uint64_t *__restrict__ rev,
                              uint64_t capacity, unsigned long long *__restrict__ state,
                              uint64_t *__restrict__ keys) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[kDirRevCovers] = state[kDirEver];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t id = ids[i];
        keys[i] = id < capacity ? rev[id] : kEmptyKey;
    }
}

// ---------------------------------------------------------------- directory reclaim
// Emptying a victim's slot in place would cut the probe chains that run through it, and a
// tombstone per victim would fill the table of a churning key space.  A reclaim
// (tbe_dir_reclaim_device) therefore rebuilds the table from its survivors:
//   1. vict[id] = 1 for every slot's id that is flagged dead (one pass over the slots: only
//      they know which ids are assigned), then 0 again for the keep ids;
//   2. the victims, in ascending id order (block counts, scan, write over the ids), go
//      onto the free stack and lose their id -> key entry;
//   3. the surviving slots' (key, id) are compacted in slot order (block counts, scan,
//      write over the slots) into a record list; a slot that holds a key without an id (an
//      overflowed batch left it) is no survivor;
//   4. the slot table is reset and every record claims a slot again by CAS, probing from
//      its key's home slot as an assign does.
// Every index is bounded by what it indexes: ids by capacity, slots by nslots, records by
// the survivors (distinct ids, so at most capacity), the stack by the distinct ids not held.
__global__ void k_dr_flag(const uint32_t *__restrict__ sid, uint64_t nslots, uint64_t capacity,
                          const uint8_t *__restrict__ dead, uint8_t *__restrict__ vict) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nslots; s += stride) {
        const uint32_t id = sid[s];
        if (id != kNoId && id < capacity && dead[id]) vict[id] = 1;
    }
}

// Exclusive scan of the survivors' block counts in place (rc_n[1] = their sum), which runs
// after the victims (rc_n[0] of them) were pushed: the counters after the reclaim, and
// the caller's count.
__global__ __launch_bounds__(kScanThreads) void k_dr_scan(uint32_t *__restrict__ v, uint32_t nblk,
                                                          unsigned long long *__restrict__ state,
                                                          uint32_t *__restrict__ rc_n,
                                                          uint64_t *__restrict__ n_reclaimed) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    const uint32_t tot = scan_blocks(v, nblk, wsum);
    if (threadIdx.x == 0) {
        rc_n[1] = tot;
        pool_reclaimed(state, rc_n[0]);
        state[kDirHeld] = state[kStFresh] - state[kStNfree];
        state[kDirRevCovers] = ~0ull;      // the id -> key table is built again
        if (n_reclaimed) *n_reclaimed = rc_n[0];
    }
}

// A victim loses its id -> key entry (once the table exists).
struct RevForget {
    uint64_t *rev;
    __device__ void operator()(uint64_t id) const {
        if (rev) rev[id] = kEmptyKey;
    }
};

__device__ __forceinline__ bool dr_survives(const uint32_t *__restrict__ sid, const uint8_t *__restrict__ vict,
                                            uint64_t s, uint64_t nslots, uint64_t capacity) {
    if (s >= nslots) return false;
    const uint32_t id = sid[s];
    return id != kNoId && id < capacity && !vict[id];
}

// Surviving keys per block of kDirTile slots.
__global__ __launch_bounds__(kDirBlock) void k_dr_scount(uint64_t nslots, uint64_t capacity,
                                                         const uint32_t *__restrict__ sid,
                                                         const uint8_t *__restrict__ vict,
                                                         uint32_t *__restrict__ bs) {
    __shared__ uint32_t wsum[kDirBlock / 64];
    constexpr int PER = kDirTile / kDirBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kDirTile + (uint64_t)threadIdx.x * PER;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) c += dr_survives(sid, vict, base + k, nslots, capacity);
    uint32_t tot;
    (void)block_excl_scan<kDirBlock>(c, wsum, &tot);
    if (threadIdx.x == 0) bs[blockIdx.x] = tot;
}

// The survivors' (key, id) in slot order: record rank = bs[block] + rank in block.
__global__ __launch_bounds__(kDirBlock) void k_dr_move(uint64_t nslots, uint64_t capacity,
                                                       const uint64_t *__restrict__ skey,
                                                       const uint32_t *__restrict__ sid,
                                                       const uint8_t *__restrict__ vict,
                                                       const uint32_t *__restrict__ bs,
                                                       uint64_t *__restrict__ sv_key, uint32_t *__restrict__ sv_id) {
    __shared__ uint32_t wsum[kDirBlock / 64];
    constexpr int PER = kDirTile / kDirBlock;
    const uint64_t base = (uint64_t)blockIdx.x * kDirTile + (uint64_t)threadIdx.x * PER;
    bool sv[PER];
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        sv[k] = dr_survives(sid, vict, base + k, nslots, capacity);
        c += sv[k];
    }
    uint32_t tot;
    uint64_t r = (uint64_t)bs[blockIdx.x] + block_excl_scan<kDirBlock>(c, wsum, &tot);
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (sv[k] && r < capacity) {
            sv_key[r] = skey[base + k];
            sv_id[r] = sid[base + k];
            ++r;
        }
}

// Every survivor back into the reset table: the first empty slot from its key's home
// slot on, claimed by CAS (the keys are distinct, so a lost CAS means "probe on").
__global__ __launch_bounds__(kDirBlock) void k_dr_place(const uint32_t *__restrict__ rc_n,
                                                        const uint64_t *__restrict__ sv_key,
                                                        const uint32_t *__restrict__ sv_id,
                                                        uint64_t *__restrict__ skey, uint32_t *__restrict__ sid,
                                                        uint64_t smask, uint64_t capacity,
                                                        unsigned long long *__restrict__ err) {
    const uint64_t count = min((uint64_t)rc_n[1], capacity);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < count; r += stride) {
        const uint32_t h = probe_insert(skey, smask, sv_key[r], kEmptyKey);
        if (h == kNoId) atomicOr(err, kErrTable);   // cannot happen: survivors <= capacity <= nslots / 2
        else sid[h] = sv_id[r];
    }
}

}  // namespace

struct tbe_directory {
    uint64_t capacity = 0;
    uint64_t nslots = 0;
    int device = 0;
    uint64_t imask = 0;
    uint32_t ish = 0;
    uint64_t *skey = nullptr;
    uint32_t *sid = nullptr;
    uint32_t *sfirst = nullptr;
    unsigned long long *state = nullptr;   // kStateWords counters (tbe_idpool.hpp, kDir*)
    uint64_t *rev = nullptr;               // id -> key, capacity entries (the first tbe_dir_keys_of_device allocates it)
    uint32_t *slot_of = nullptr;           // per-request slot of the current batch
    uint32_t *bsum = nullptr;
    uint64_t tmp_cap = 0;
    // reclaim (allocated by the first one, dir_reclaim_scratch)
    PoolScratch pool;
    uint64_t *sv_key = nullptr;            // survivor records, capacity each
    uint32_t *sv_id = nullptr;
    uint32_t *rc_bs = nullptr;
};

namespace {

tbe_status dir_reclaim_scratch(tbe_directory *d) {
    if (d->pool.free_ids) return TBE_OK;
    const uint64_t cap = d->capacity, nbs = (d->nslots + kDirTile - 1) / kDirTile;
    if (hipMalloc(&d->sv_key, cap * sizeof(uint64_t)) == hipSuccess &&
        hipMalloc(&d->sv_id, cap * sizeof(uint32_t)) == hipSuccess &&
        hipMalloc(&d->rc_bs, nbs * sizeof(uint32_t)) == hipSuccess && pool_scratch_alloc(d->pool, cap))
        return TBE_OK;
    for (void *p : {(void *)d->sv_key, (void *)d->sv_id, (void *)d->rc_bs})
        if (p) (void)hipFree(p);
    d->sv_key = nullptr;
    d->sv_id = d->rc_bs = nullptr;
    pool_scratch_free(d->pool);
    return TBE_ENOMEM;
}

}  // namespace

extern "C" {

uint32_t tbe_key_owner(uint64_t key, uint32_t n_owners) { return n_owners ? key_owner(key, n_owners) : 0u; }

uint64_t tbe_route_workspace_bytes(uint64_t n, uint32_t n_owners) {
    const uint64_t ntiles = (n + kRtTile - 1) / kRtTile;
    return (ntiles * (uint64_t)n_owners + kMaxOwners) * sizeof(uint32_t);
}

tbe_status tbe_route_plan_device(const uint64_t *d_keys, uint64_t n, uint32_t n_owners, void *d_work,
                                 uint32_t *d_pos, uint64_t *d_counts, void *stream) {
    return tbe_route_plan_map_device(d_keys, n, n_owners, nullptr, d_work, d_pos, d_counts, stream);
}

uint32_t tbe_key_vnode(uint64_t key) { return key_vnode(key); }

tbe_status tbe_route_plan_map_device(const uint64_t *d_keys, uint64_t n, uint32_t n_owners,
                                     const uint8_t *d_owner_map, void *d_work, uint32_t *d_pos,
                                     uint64_t *d_counts, void *stream) {
    if (n_owners == 0 || n_owners > kMaxOwners || n >= (1ull << 32) || !d_counts) return TBE_EINVAL;
    if (d_owner_map && (reinterpret_cast<uintptr_t>(d_owner_map) & 3u)) return TBE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return hipMemsetAsync(d_counts, 0, n_owners * sizeof(uint64_t), st) == hipSuccess ? TBE_OK : TBE_EDEVICE;
    if (!d_keys || !d_work || !d_pos) return TBE_EINVAL;
    const uint32_t ntiles = (uint32_t)((n + kRtTile - 1) / kRtTile);
    uint32_t *tile = static_cast<uint32_t *>(d_work);
    uint32_t *obase = tile + (uint64_t)ntiles * n_owners;
    k_route_count<<<ntiles, kRtBlock, 0, st>>>(d_keys, n, n_owners, d_owner_map, tile);
    k_route_scan<<<1, kScanThreads, 0, st>>>(tile, ntiles, n_owners, d_counts, obase);
    k_route_pos<<<ntiles, kRtBlock, 0, st>>>(d_keys, n, n_owners, d_owner_map, tile, obase, d_pos);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_vnode_count_device(const uint64_t *d_keys, uint64_t n, uint64_t *d_counts, void *stream) {
    if (!d_counts || (n && !d_keys)) return TBE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_counts, 0, kOwnerMapSize * sizeof(uint64_t), st) != hipSuccess) return TBE_EDEVICE;
    if (n == 0) return TBE_OK;
    k_vnode_count<<<grid_for(n, kRtBlock, 1024), kRtBlock, 0, st>>>(
        d_keys, n, reinterpret_cast<unsigned long long *>(d_counts));
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_route_pack_device(const uint32_t *d_pos, uint64_t n, const uint64_t *d_keys, const int32_t *d_permits,
                                 const int64_t *d_ts_us, int64_t *d_out, void *stream) {
    if (n == 0) return TBE_OK;
    if (!d_pos || !d_keys || !d_permits || !d_ts_us || !d_out) return TBE_EINVAL;
    k_route_pack<<<grid_for(n, 256), 256, 0, (hipStream_t)stream>>>(d_pos, n, d_keys, d_permits, d_ts_us, d_out);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_route_gather_device(const uint32_t *d_pos, uint64_t n, const int64_t *d_in, uint32_t cols,
                                   int64_t *d_out, void *stream) {
    if (n == 0) return TBE_OK;
    if (!d_pos || !d_in || !d_out || cols == 0 || cols > 8) return TBE_EINVAL;
    k_route_gather<<<grid_for(n, 256), 256, 0, (hipStream_t)stream>>>(d_pos, n, d_in, cols, d_out);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

uint64_t tbe_text_route_key(const uint8_t *text, uint64_t len, uint64_t seed) {
    return text_hash_host(text, text ? len : 0, seed);
}

tbe_status tbe_route_text_keys_device(const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *d_offs, uint64_t n,
                                      uint64_t seed, uint64_t *d_keys, uint64_t *d_n_bad, void *stream) {
    if (!d_n_bad || n >= (1ull << 32) || (reinterpret_cast<uintptr_t>(d_bytes) & 7u)) return TBE_EINVAL;
    if (n && (!d_offs || !d_keys || (n_bytes && !d_bytes))) return TBE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_n_bad, 0, sizeof(uint64_t), st) != hipSuccess) return TBE_EDEVICE;
    if (n == 0) return TBE_OK;
    k_rt_text_keys<<<grid_for(n, kTxBlock), kTxBlock, 0, st>>>(d_bytes, n_bytes, d_offs, n, seed, d_keys,
                                                               reinterpret_cast<unsigned long long *>(d_n_bad));
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

uint64_t tbe_route_text_workspace_bytes(uint64_t n) {
    const uint64_t nblk = (n + kTxTile - 1) / kTxTile;
    return nblk * (sizeof(uint64_t) + sizeof(uint32_t)) + n * sizeof(uint32_t);
}

tbe_status tbe_route_text_offsets_device(const uint64_t *d_offs, uint64_t n_bytes, uint64_t n, const uint32_t *d_pos,
                                         const uint64_t *d_counts, uint32_t n_owners, void *d_work,
                                         uint64_t *d_send_offs, uint64_t *d_byte_counts, void *stream) {
    if (n_owners == 0 || n_owners > kMaxOwners || n >= (1ull << 32) || !d_send_offs || !d_byte_counts)
        return TBE_EINVAL;
    if (n && (!d_offs || !d_pos || !d_counts || !d_work || (reinterpret_cast<uintptr_t>(d_work) & 7u)))
        return TBE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0)
        return hipMemsetAsync(d_send_offs, 0, sizeof(uint64_t), st) == hipSuccess &&
                       hipMemsetAsync(d_byte_counts, 0, n_owners * sizeof(uint64_t), st) == hipSuccess
                   ? TBE_OK
                   : TBE_EDEVICE;
    const uint64_t nblk = (n + kTxTile - 1) / kTxTile;
    uint64_t *bbase = static_cast<uint64_t *>(d_work);
    uint32_t *bsum = reinterpret_cast<uint32_t *>(bbase + nblk);
    uint32_t *lens = bsum + nblk;
    k_rt_len_scatter<<<grid_for(n, kTxBlock), kTxBlock, 0, st>>>(d_offs, n, n_bytes, d_pos, lens);
    text_scan(LenOfList{lens}, n, bbase, bsum, d_send_offs, st);
    k_rt_owner_bytes<<<1, kMaxOwners, 0, st>>>(d_counts, n_owners, n, d_send_offs, d_byte_counts);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_route_text_pack_device(const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *d_offs, uint64_t n,
                                      const uint32_t *d_pos, const uint64_t *d_send_offs, const int32_t *d_permits,
                                      const int64_t *d_ts_us, uint8_t *d_out_bytes, uint64_t out_capacity,
                                      int64_t *d_out_rows, void *stream) {
    if (n >= (1ull << 32) || (reinterpret_cast<uintptr_t>(d_bytes) & 7u) ||
        (reinterpret_cast<uintptr_t>(d_out_bytes) & 7u))
        return TBE_EINVAL;
    if (n == 0) return TBE_OK;
    if (!d_offs || !d_pos || !d_send_offs || !d_permits || !d_ts_us || !d_out_rows || (n_bytes && !d_bytes) ||
        (out_capacity && !d_out_bytes))
        return TBE_EINVAL;
    k_rt_text_pack<<<grid_for(n, kTxBlock), kTxBlock, 0, (hipStream_t)stream>>>(
        d_bytes, n_bytes, d_offs, n, d_pos, d_send_offs, d_permits, d_ts_us, d_out_bytes, out_capacity, d_out_rows);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_route_text_recv_offsets_device(const int64_t *d_rows, uint64_t m, void *d_work, uint64_t *d_offs,
                                              void *stream) {
    if (!d_offs || m >= (1ull << 32)) return TBE_EINVAL;
    if (m && (!d_rows || !d_work || (reinterpret_cast<uintptr_t>(d_work) & 7u))) return TBE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (m == 0) return hipMemsetAsync(d_offs, 0, sizeof(uint64_t), st) == hipSuccess ? TBE_OK : TBE_EDEVICE;
    const uint64_t nblk = (m + kTxTile - 1) / kTxTile;
    uint64_t *bbase = static_cast<uint64_t *>(d_work);
    text_scan(LenOfRows{d_rows}, m, bbase, reinterpret_cast<uint32_t *>(bbase + nblk), d_offs, st);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_dir_create(uint64_t capacity, int32_t device, tbe_directory **out) {
    if (!out) return TBE_EINVAL;
    *out = nullptr;
    if (capacity == 0 || capacity > 0xFFFFFFFEull) return TBE_EINVAL;
    tbe_directory *d = new (std::nothrow) tbe_directory();
    if (!d) return TBE_ENOMEM;
    if (device >= 0) {
        if (hipSetDevice(device) != hipSuccess) { delete d; return TBE_EDEVICE; }
        d->device = device;
    } else if (hipGetDevice(&d->device) != hipSuccess) {
        delete d;
        return TBE_EDEVICE;
    }
    d->capacity = capacity;
    uint64_t ns = 1;
    while (ns < 2 * capacity) ns <<= 1;   // load <= 1/2
    d->nslots = ns;
    scramble_params(capacity, d->imask, d->ish);
    bool ok = hipMalloc(&d->skey, ns * sizeof(uint64_t)) == hipSuccess &&
              hipMalloc(&d->sid, ns * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc(&d->sfirst, ns * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc(&d->state, kStateWords * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
        tbe_dir_destroy(d);
        return TBE_ENOMEM;
    }
    k_table_init<<<grid_for(ns, 256), 256>>>(d->skey, d->sid, d->sfirst, ns, kEmptyKey);
    if (hipMemset(d->state, 0, kStateWords * sizeof(unsigned long long)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        tbe_dir_destroy(d);
        return TBE_EDEVICE;
    }
    *out = d;
    return TBE_OK;
}

void tbe_dir_destroy(tbe_directory *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)d->skey, (void *)d->sid, (void *)d->sfirst, (void *)d->state, (void *)d->slot_of,
                    (void *)d->bsum, (void *)d->rev, (void *)d->sv_key, (void *)d->sv_id, (void *)d->rc_bs})
        if (p) (void)hipFree(p);
    pool_scratch_free(d->pool);
    delete d;
}

tbe_status tbe_dir_assign_device(tbe_directory *d, const uint64_t *d_keys, uint64_t n, uint64_t *d_ids, void *stream) {
    if (!d) return TBE_EINVAL;
    if (n == 0) return TBE_OK;
    if (!d_keys || !d_ids || n >= (1ull << 32)) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (n > d->tmp_cap) {
        // the previous batch may still be using the old buffers
        if (hipDeviceSynchronize() != hipSuccess) return TBE_EDEVICE;
        if (d->slot_of) (void)hipFree(d->slot_of);
        if (d->bsum) (void)hipFree(d->bsum);
        d->slot_of = nullptr;
        d->bsum = nullptr;
        d->tmp_cap = 0;
        const uint64_t cap = std::max<uint64_t>(n, 1u << 16);
        if (hipMalloc(&d->slot_of, cap * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc(&d->bsum, ((cap + kDirTile - 1) / kDirTile) * sizeof(uint32_t)) != hipSuccess)
            return TBE_ENOMEM;
        d->tmp_cap = cap;
    }
    const uint32_t nblk = (uint32_t)((n + kDirTile - 1) / kDirTile);
    k_dir_claim<<<grid_for(n, kDirBlock), kDirBlock, 0, st>>>(d_keys, n, d->skey, d->sid, d->sfirst, d->nslots - 1,
                                                             d->slot_of, d->state + kStErr);
    k_dir_count<<<nblk, kDirBlock, 0, st>>>(d->slot_of, n, d->sid, d->sfirst, d->bsum);
    k_dir_scan<<<1, kScanThreads, 0, st>>>(d->bsum, nblk, d->state, d->capacity);
    k_dir_assign<<<nblk, kDirBlock, 0, st>>>(d->slot_of, n, d->sid, d->sfirst, d->bsum, d->state, d->capacity,
                                             d->imask, d->ish, d->pool.free_ids);
    k_gather<<<grid_for(n, 256), 256, 0, st>>>(d->slot_of, n, d->sid, d_ids);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_dir_lookup_device(tbe_directory *d, const uint64_t *d_keys, uint64_t n, uint64_t *d_ids, void *stream) {
    if (!d) return TBE_EINVAL;
    if (n == 0) return TBE_OK;
    if (!d_keys || !d_ids) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    k_dir_lookup<<<grid_for(n, kDirBlock), kDirBlock, 0, (hipStream_t)stream>>>(d_keys, n, d->skey, d->sid,
                                                                               d->nslots - 1, d_ids);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_dir_keys_of_device(tbe_directory *d, const uint64_t *d_ids, uint64_t n, uint64_t *d_keys,
                                  void *stream) {
    if (!d) return TBE_EINVAL;
    if (n == 0) return TBE_OK;
    if (!d_ids || !d_keys) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (!d->rev) {
        if (hipMalloc(&d->rev, d->capacity * sizeof(uint64_t)) != hipSuccess) return TBE_ENOMEM;
        // every entry UINT64_MAX, and what the table covers too: the first build fills in every id held
        if (hipMemsetAsync(d->rev, 0xFF, d->capacity * sizeof(uint64_t), st) != hipSuccess ||
            hipMemsetAsync(d->state + kDirRevCovers, 0xFF, sizeof(unsigned long long), st) != hipSuccess)
            return TBE_EDEVICE;
    }
    k_dir_rev_build<<<grid_for(d->nslots, 256), 256, 0, st>>>(d->skey, d->sid, d->nslots, d->state, d->capacity,
                                                             d->rev);
    k_dir_keys_of<<<grid_for(n, 256), 256, 0, st>>>(d_ids, n, d->rev, d->capacity, d->state, d_keys);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_dir_state_async(tbe_directory *d, uint64_t *out2, void *stream) {
    if (!d || !out2) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    return hipMemcpyAsync(out2, d->state, 2 * sizeof(uint64_t), hipMemcpyDefault, (hipStream_t)stream) == hipSuccess
               ? TBE_OK
               : TBE_EDEVICE;
}

tbe_status tbe_dir_size(tbe_directory *d, uint64_t *n_ids) {
    if (!d || !n_ids) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return TBE_EDEVICE;
    unsigned long long st[2] = {0, 0};
    if (hipMemcpy(st, d->state, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) return TBE_EDEVICE;
    *n_ids = st[kDirHeld];
    return st[kStErr] ? TBE_ERANGE : TBE_OK;
}

tbe_status tbe_dir_reclaim_device(tbe_directory *d, const uint8_t *d_dead, const uint64_t *d_keep_ids,
                                  uint64_t n_keep, uint64_t *d_n_reclaimed, void *stream) {
    if (!d || !d_dead || (n_keep && !d_keep_ids)) return TBE_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return TBE_EDEVICE;
    const tbe_status rc = dir_reclaim_scratch(d);
    if (rc != TBE_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t cap = d->capacity, ns = d->nslots;
    const uint32_t nbi = (uint32_t)((cap + kPoolTile - 1) / kPoolTile), nbs = (uint32_t)((ns + kDirTile - 1) / kDirTile);
    const PoolScratch &p = d->pool;
    if (hipMemsetAsync(p.vict, 0, cap, st) != hipSuccess) return TBE_EDEVICE;
    k_dr_flag<<<grid_for(ns, 256), 256, 0, st>>>(d->sid, ns, cap, d_dead, p.vict);
    if (n_keep) k_pool_keep<<<grid_for(n_keep, 256), 256, 0, st>>>(d_keep_ids, n_keep, cap, p.vict);
    k_pool_vcount<<<nbi, kPoolBlock, 0, st>>>(cap, p.vict, p.rc_bv);
    k_scan_blocks<<<1, kScanThreads, 0, st>>>(p.rc_bv, nbi, p.rc_n);
    k_pool_vpush<<<nbi, kPoolBlock, 0, st>>>(cap, p.vict, p.rc_bv, d->state, p.free_ids, RevForget{d->rev});
    k_dr_scount<<<nbs, kDirBlock, 0, st>>>(ns, cap, d->sid, p.vict, d->rc_bs);
    k_dr_scan<<<1, kScanThreads, 0, st>>>(d->rc_bs, nbs, d->state, p.rc_n, d_n_reclaimed);
    k_dr_move<<<nbs, kDirBlock, 0, st>>>(ns, cap, d->skey, d->sid, p.vict, d->rc_bs, d->sv_key, d->sv_id);
    k_table_init<<<grid_for(ns, 256), 256, 0, st>>>(d->skey, d->sid, d->sfirst, ns, kEmptyKey);
    k_dr_place<<<grid_for(cap, kDirBlock), kDirBlock, 0, st>>>(p.rc_n, d->sv_key, d->sv_id, d->skey, d->sid, ns - 1, cap,
                                                              d->state + kStErr);
    return hipGetLastError() == hipSuccess ? TBE_OK : TBE_EDEVICE;
}

tbe_status tbe_dir_reclaim(tbe_directory *d, tbe_engine *engine, int64_t ts_us, const uint64_t *keep_ids,
                           uint64_t n_keep, uint64_t *n_reclaimed) {
    if (!d) return TBE_EINVAL;
    return pool_reclaim_sync(d->pool, d->device, d->capacity, engine, ts_us, keep_ids, n_keep, n_reclaimed,
                             [d](const uint8_t *dead, const uint64_t *keep, uint64_t nk, uint64_t *count) {
                                 return tbe_dir_reclaim_device(d, dead, keep, nk, count, nullptr);
                             });
}

}  // extern "C"
