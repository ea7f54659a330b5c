// tbe_text.hpp -- the 64-bit hash of a key's text, shared by the device string directory
// (tbe_strdir.hip: slot tags) and the multi-GPU layer (tbe_cluster.hip: the routing key of
// a string, include/tbe_cluster.h "Routing text"):
//
//   H(text, seed): h = mix64(seed ^ len * 0x9E3779B97F4A7C15), then h = mix64(h ^ w_k) over
//   the little-endian 8-byte words w_k of the text, the last one zero-padded.
//
// sd_word / sd_hash are the device form over an Arrow-style byte buffer, text_hash_host the
// same function over host memory (cluster.py text_route_keys is its numpy mirror).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbe_hash.hpp"

namespace tbe {
namespace {

// 8 bytes of a string starting at its byte 8k (bytes past its end read as 0).  `safe` =
// the largest multiple of 8 such that [0, safe) is readable; words past it are read
// byte by byte up to the string's end.
__device__ __forceinline__ uint64_t sd_word(const uint8_t *__restrict__ base, uint64_t safe, uint64_t off,
                                            uint32_t len, uint32_t k) {
    const uint64_t p = off + 8ull * k;
    const uint32_t rem = len - 8u * k;
    const uint64_t a = p & ~7ull;
    const uint32_t sh = (uint32_t)(p & 7) * 8u;
    uint64_t w;
    if (a + 16 <= safe) {
        const uint64_t lo = *reinterpret_cast<const uint64_t *>(base + a);
        if (sh) {
            const uint64_t hi = *reinterpret_cast<const uint64_t *>(base + a + 8);
            w = (lo >> sh) | (hi << (64 - sh));
        } else {
            w = lo;
        }
    } else {
        w = 0;
        const uint32_t m = rem < 8 ? rem : 8;
        for (uint32_t b = 0; b < m; ++b) w |= (uint64_t)base[p + b] << (8 * b);
    }
    if (rem < 8) w &= (1ull << (8 * rem)) - 1;
    return w;
}

__device__ __forceinline__ uint64_t sd_hash(const uint8_t *__restrict__ base, uint64_t safe, uint64_t off,
                                            uint32_t len, uint64_t seed) {
    uint64_t h = mix64(seed ^ ((uint64_t)len * 0x9E3779B97F4A7C15ull));
    for (uint32_t k = 0; 8u * k < len; ++k) h = mix64(h ^ sd_word(base, safe, off, len, k));
    return h;
}

// H(text, seed) on the host: the same words, read byte by byte.
inline uint64_t text_hash_host(const uint8_t *text, uint64_t len, uint64_t seed) {
    uint64_t h = mix64(seed ^ (len * 0x9E3779B97F4A7C15ull));
    for (uint64_t k = 0; 8 * k < len; ++k) {
        uint64_t w = 0;
        for (uint64_t b = 0; b < 8 && 8 * k + b < len; ++b) w |= (uint64_t)text[8 * k + b] << (8 * b);
        h = mix64(h ^ w);
    }
    return h;
}

}  // namespace
}  // namespace tbe
