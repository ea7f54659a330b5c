// Record formats of the partition passes (PackFmt, FoldFmt) and the packers that turn a
// narrow pass-0 record into a fold record: the generic one, written against run-time field
// widths, and the per-batch codec (Pass1Codec) the last pass uses.  Host and device: the
// stand-alone program tests/host/codec_test.cpp compares the two over every reachable format.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TBE_CODEC_FN __host__ __device__ __forceinline__
#else
#define TBE_CODEC_FN inline
#endif

// Packed request records (token-bucket kind).  When the key, a permit code and a
// 32-bit time offset fit one u64, the partition passes and the fold move one 8-byte
// record per request instead of {key u32, permits i32, ts i64}:
//
//   bits [0, kb)            key (< n_keys <= 2^kb)
//   bits [kb, kb+pb)        permit code min(permits, TokenLimit + 1): x <= TokenLimit
//                           always (TB:221), so every larger request is decided, and
//                           leaves the state, exactly like TokenLimit + 1 (TB:224)
//   bit  kb+pb              escape
//   bits [kb+pb+1, 64)      ts - base  (base = ts[0] of the batch - 2^(wb-1)), or, with
//                           the escape bit, the arrival index: the fold then reads the
//                           request's timestamp from the caller's array
//
// wb = 64 - kb - pb - 1 >= 32, so a batch whose timestamps lie within +-35 minutes of
// its first one never escapes.
struct PackFmt {
    uint64_t kmask;     // (1 << kb) - 1
    int32_t kb;
    int32_t pb;
    int32_t pc_max;     // TokenLimit + 1
    int32_t wb;
    // Narrow pass-0 records (round 5; token bucket, two passes, fold records, digit stream):
    // pass 0 writes a u32 per request -- row within the bucket (rb bits), permit code,
    // escape, ts - base0 (w0 = 32 - rb - pb - 1 bits, base0 = ts[0] - 2^(w0-1)) -- beside
    // the one-byte digit stream that already carries the pass-1 digit; the pass-0 digit is
    // the record's position.  An escaped request (time outside the window) also writes its
    // timestamp to a side array at its pass-0 output position, where the fold finds it.
    // 4 + 1 bytes instead of 8 + 1 written by pass 0 and read by pass 1.
    int32_t n0;         // 1: pass 0 writes narrow records
    int32_t rb;         // row bits (r_bits) of a narrow record
    int32_t w0;         // time-offset bits of a narrow record
};
// A narrow pass-0 record from the partition key (row = its low rb bits); *esc: the time did
// not fit and goes to the side array.
TBE_CODEC_FN uint32_t pack_rec32(uint32_t pkey, int32_t p, int64_t ts, int64_t tbase, const PackFmt &F, bool &esc) {
    const uint32_t pc = (uint32_t)(p < 0 ? 0 : (p > F.pc_max ? F.pc_max : p));
    const uint64_t d = (uint64_t)ts - (uint64_t)tbase;
    const bool fits = ts >= tbase && (d >> F.w0) == 0;
    esc = !fits;
    return (pkey & ((1u << F.rb) - 1u)) | (pc << F.rb) | ((uint32_t)!fits << (F.rb + F.pb)) |
           (fits ? (uint32_t)d << (F.rb + F.pb + 1) : 0u);
}

// Fold records (token-bucket kind, packed, >= 2 partition passes).  The last pass writes,
// instead of a PackFmt record and its permutation, what the fold and the hot runs need:
//
//   bits [0, rb)              row within the bucket (the key field's low r_bits)
//   bits [rb, rb+pb)          permit code (as PackFmt)
//   bit  rb+pb                escape
//   bits [rb+pb+1, +pw)       the request's position in the last pass's INPUT (the previous
//                             pass's output): its reply goes there, so the last pass needs
//                             no permutation and no un-partition pass of its own
//   bits [rb+pb+1+pw, 64)     ts - base1 (tw bits, base1 = ts[0] - 2^(tw-1)); with the
//                             escape bit: unused, and the fold takes the request's time from
//                             the previous pass's record at that position
//
// pw = ceil_log2(batch), tw = 64 - rb - pb - 1 - pw (config B: 22 bits, +-2.1 s around the
// batch's first request; the batch spans 10 ms).  Used when tw >= 8.
struct FoldFmt {
    int32_t on;
    int32_t n0;             // pass 0 wrote narrow records: an escaped record's time is rec0[pos] itself
    int32_t rb, pb, pw, tw;
    uint32_t nb;            // ordinary buckets
    uint32_t region_bits;   // 8 * (passes - 1): buckets with equal low region_bits share a reply region
    uint32_t n_hi;          // ceil(nb / 2^region_bits)
};
// The generic form: decode the narrow record's time, re-base it, test the fold window.
TBE_CODEC_FN uint64_t fold_rec32(uint32_t r32, uint32_t pos, int64_t tbase0, int64_t tbase1, const PackFmt &F,
                           const FoldFmt &G) {
    const uint64_t row = r32 & ((1u << F.rb) - 1u);
    const uint64_t pc = (r32 >> F.rb) & ((1u << F.pb) - 1u);
    const bool esc0 = (r32 >> (F.rb + F.pb)) & 1u;
    const int64_t ts = (int64_t)((uint64_t)tbase0 + (uint64_t)(r32 >> (F.rb + F.pb + 1)));
    const uint64_t d = (uint64_t)ts - (uint64_t)tbase1;
    const bool fits = !esc0 && ts >= tbase1 && (d >> G.tw) == 0;
    return row | (pc << G.rb) | ((uint64_t)!fits << (G.rb + G.pb)) | ((uint64_t)pos << (G.rb + G.pb + 1)) |
           ((fits ? d : 0ull) << (G.rb + G.pb + 1 + G.pw));
}

// Narrow pass-0 record -> fold record with the batch's constants worked out once.
//  - Row, permit code and escape bit occupy bits [0, rb+pb] of both records: one mask copies them.
//  - The fold window never rejects a time the narrow window accepted.  With t0 the narrow
//    record's time field (0 <= t0 < 2^w0), d = ts - base1 = t0 + (base0 - base1) and
//    base0 - base1 = 2^(tw-1) - 2^(w0-1) whatever ts[0] is.  tw = w0 + 32 - pw and pw <= 32 (a
//    batch has fewer than 2^32 requests), so tw >= w0, the constant is >= 0, and
//    0 <= d < 2^w0 + 2^(tw-1) - 2^(w0-1) <= 2^tw: `fits` of fold_rec32 equals !esc0 and the
//    64-bit subtract, compare and shift that test it are dead.  d is t0 plus the constant.
//  - A batch without timestamps (the approximate kind) has both bases 0: the constant is 0.
struct Pass1Codec {
    uint32_t low_mask;   // (1 << (rb+pb+1)) - 1
    uint32_t s_esc;      // rb+pb
    uint32_t s_pos;      // rb+pb+1   (2 .. 24: w0 >= 8)
    uint32_t s_time;     // rb+pb+1+pw
    uint64_t dconst;     // base0 - base1
};
TBE_CODEC_FN bool pass1_codec_ok(const PackFmt &F, const FoldFmt &G) {
    return F.n0 && G.pw >= 1 && G.pw <= 32 && F.rb == G.rb && F.pb == G.pb && F.w0 == 32 - F.rb - F.pb - 1 &&
           F.w0 >= 1 && G.tw == 64 - G.rb - G.pb - 1 - G.pw && G.tw >= F.w0;
}
TBE_CODEC_FN Pass1Codec pass1_codec(const PackFmt &F, const FoldFmt &G, bool have_ts) {
    Pass1Codec C;
    C.s_esc = (uint32_t)(F.rb + F.pb);
    C.s_pos = C.s_esc + 1u;
    C.s_time = C.s_pos + (uint32_t)G.pw;
    C.low_mask = (1u << C.s_pos) - 1u;
    C.dconst = have_ts ? (1ull << (G.tw - 1)) - (1ull << (F.w0 - 1)) : 0ull;
    return C;
}
TBE_CODEC_FN uint64_t fold_rec32_codec(uint32_t r32, uint32_t pos, const Pass1Codec &C) {
    const bool esc0 = (r32 >> C.s_esc) & 1u;
    const uint64_t d = (uint64_t)(r32 >> C.s_pos) + C.dconst;
    // the position field by halves: 1 <= s_pos <= 31
    const uint32_t plo = pos << C.s_pos, phi = pos >> (32u - C.s_pos);
    return ((uint64_t)phi << 32 | ((r32 & C.low_mask) | plo)) | ((esc0 ? 0ull : d) << C.s_time);
}
