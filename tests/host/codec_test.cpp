// The last pass's per-batch record codec (csrc/tbe_codec.hpp: Pass1Codec, fold_rec32_codec)
// against the generic packer fold_rec32, on the host, over every format the engine can reach
// and beyond: row bits 1-16, permit bits and position bits as far as a narrow record has a
// time field at all (w0 >= 1; the engine asks for w0 >= 8 and tw >= 8).  Both directions:
// equal packed bits, and the fields decoded from the packed record (by the documented layout)
// equal to what went in.  Also the claim the codec rests on: a time that fits the narrow
// record's window always fits the fold record's.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../distributedratelimiting.redis_amd/csrc/tbe_codec.hpp"

static long g_fail = 0, g_checks = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        ++g_checks;                                    \
        if (!(c)) {                                    \
            if (++g_fail <= 20) {                      \
                std::printf("FAIL %s: ", #c);          \
                std::printf(__VA_ARGS__);              \
                std::printf("\n");                     \
            }                                          \
        }                                              \
    } while (0)

struct Fmt {
    PackFmt F;
    FoldFmt G;
};

static Fmt make_fmt(int rb, int pb, int pw) {
    Fmt f{};
    f.F.kb = 27;
    f.F.kmask = (1ull << f.F.kb) - 1;
    f.F.pb = pb;
    f.F.pc_max = (int32_t)((1u << pb) - 1u);
    f.F.wb = 64 - f.F.kb - pb - 1;
    f.F.n0 = 1;
    f.F.rb = rb;
    f.F.w0 = 32 - rb - pb - 1;
    f.G.on = 1;
    f.G.n0 = 1;
    f.G.rb = rb;
    f.G.pb = pb;
    f.G.pw = pw;
    f.G.tw = 64 - rb - pb - 1 - pw;
    return f;
}

// one narrow record through both packers, then decoded
static void check_record(const Fmt &f, const Pass1Codec &C, uint32_t r32, uint32_t pos, int64_t tbase0,
                         int64_t tbase1, bool have_in, uint32_t row_in, uint32_t pc_in, bool esc_in, int64_t ts_in) {
    const PackFmt &F = f.F;
    const FoldFmt &G = f.G;
    const uint64_t a = fold_rec32(r32, pos, tbase0, tbase1, F, G);
    const uint64_t b = fold_rec32_codec(r32, pos, C);
    CHECK(a == b, "rb %d pb %d pw %d r32 %08x pos %u: generic %016" PRIx64 " codec %016" PRIx64, F.rb, F.pb, G.pw,
          r32, pos, a, b);
    if (!have_in) return;
    const uint32_t row = (uint32_t)(b & ((1ull << G.rb) - 1));
    const uint32_t pc = (uint32_t)((b >> G.rb) & ((1ull << G.pb) - 1));
    const bool esc = (b >> (G.rb + G.pb)) & 1;
    const uint32_t p2 = (uint32_t)((b >> (G.rb + G.pb + 1)) & ((1ull << G.pw) - 1));
    const uint64_t tf = b >> (G.rb + G.pb + 1 + G.pw);
    CHECK(row == row_in && pc == pc_in && esc == esc_in && p2 == pos,
          "rb %d pb %d pw %d: decoded row %u/%u pc %u/%u esc %d/%d pos %u/%u", F.rb, F.pb, G.pw, row, row_in, pc,
          pc_in, (int)esc, (int)esc_in, p2, pos);
    if (!esc)
        CHECK((int64_t)((uint64_t)tbase1 + tf) == ts_in, "rb %d pb %d pw %d: decoded time %" PRId64 " != %" PRId64,
              F.rb, F.pb, G.pw, (int64_t)((uint64_t)tbase1 + tf), ts_in);
    else
        CHECK(tf == 0, "escaped record carries a time field");
}

int main() {
    std::mt19937_64 rng(0xC0DEC);
    long formats = 0;
    for (int rb = 1; rb <= 16; ++rb)
        for (int pb = 1; pb <= 32; ++pb)
            for (int pw = 1; pw <= 32; ++pw) {
                const int w0 = 32 - rb - pb - 1;
                if (w0 < 1) continue;   // no narrow record: the engine writes 8-byte pass-0 records
                const Fmt f = make_fmt(rb, pb, pw);
                const int tw = f.G.tw;
                ++formats;
                CHECK(pass1_codec_ok(f.F, f.G), "rb %d pb %d pw %d not accepted", rb, pb, pw);
                CHECK(tw >= w0, "tw %d < w0 %d", tw, w0);
                const Pass1Codec C = pass1_codec(f.F, f.G, true);
                const uint32_t pmax = pw == 32 ? 0xFFFFFFFFu : (1u << pw) - 1u;
                const int64_t first[] = {0, 5, (int64_t)1 << (w0 - 1), 1700000000000000ll, ((int64_t)1 << 53) - 1};
                for (int64_t ts0 : first) {
                    const int64_t tbase0 = ts0 - ((int64_t)1 << (w0 - 1));
                    const int64_t tbase1 = ts0 - ((int64_t)1 << (tw - 1));
                    CHECK((uint64_t)tbase0 - (uint64_t)tbase1 == C.dconst, "base difference depends on ts[0]");
                    const int64_t win = (int64_t)1 << w0;
                    // the window's edges, a step outside it on both sides, far outside, and random
                    int64_t tsv[16] = {tbase0,     tbase0 + 1,     tbase0 + win - 1, tbase0 + win - 2, tbase0 + win / 2,
                                       tbase0 - 1, tbase0 + win,   tbase0 + win + 1, ts0,              ts0 + 2400000000ll,
                                       ts0 - 40000, ts0 + 40000};
                    for (int k = 12; k < 16; ++k) tsv[k] = tbase0 + (int64_t)(rng() % (uint64_t)win);
                    for (int64_t ts : tsv) {
                        const uint32_t pkey = (uint32_t)rng();
                        const int32_t pvals[] = {0, 1, f.F.pc_max, -3, (int32_t)(rng() % ((uint64_t)f.F.pc_max + 1))};
                        const int32_t p = pvals[rng() % 5];
                        bool esc = false;
                        const uint32_t r32 = pack_rec32(pkey, p, ts, tbase0, f.F, esc);
                        // the fold window test for a time the narrow window accepted
                        const uint64_t d = (uint64_t)ts - (uint64_t)tbase1;
                        const bool fits1 = ts >= tbase1 && (d >> tw) == 0;
                        CHECK(esc || fits1, "rb %d pb %d pw %d: ts %" PRId64 " fits w0 %d, not tw %d", rb, pb, pw, ts, w0, tw);
                        const uint32_t pc = (uint32_t)(p < 0 ? 0 : p);
                        const uint32_t posv[] = {0u, 1u & pmax, pmax, (uint32_t)rng() & pmax};
                        for (uint32_t pos : posv)
                            check_record(f, C, r32, pos, tbase0, tbase1, true, pkey & ((1u << rb) - 1u), pc, esc, ts);
                    }
                }
                // every time field of a small window; the extreme time fields of the others
                const uint32_t nt = w0 <= 10 ? (1u << w0) : 0u;
                const int64_t ts0 = 1700000000123456ll;
                const int64_t tbase0 = ts0 - ((int64_t)1 << (w0 - 1)), tbase1 = ts0 - ((int64_t)1 << (tw - 1));
                for (uint32_t t0 = 0; t0 < nt; ++t0) {
                    const int64_t ts = tbase0 + t0;
                    const uint64_t d = (uint64_t)ts - (uint64_t)tbase1;
                    CHECK(ts >= tbase1 && (d >> tw) == 0, "t0 %u outside the fold window (w0 %d tw %d)", t0, w0, tw);
                    const uint32_t r32 = (t0 << (rb + pb + 1)) | ((uint32_t)rng() & ((1u << (rb + pb)) - 1u));
                    check_record(f, C, r32, (uint32_t)rng() & pmax, tbase0, tbase1, false, 0, 0, false, 0);
                }
                // raw records: all-ones and random bit patterns, escape bit set and clear
                for (int k = 0; k < 8; ++k) {
                    uint32_t r32 = k == 0 ? 0xFFFFFFFFu : k == 1 ? 0u : (uint32_t)rng();
                    if (r32 >> (rb + pb) & 1u) r32 &= (1u << (rb + pb + 1)) - 1u;   // an escaped record's time field is 0
                    check_record(f, C, r32, (uint32_t)rng() & pmax, tbase0, tbase1, false, 0, 0, false, 0);
                }
                // a batch without timestamps (both bases 0): row | permit code only
                const Pass1Codec C0 = pass1_codec(f.F, f.G, false);
                for (int k = 0; k < 4; ++k)
                    check_record(f, C0, (uint32_t)rng() & ((1u << (rb + pb)) - 1u), (uint32_t)rng() & pmax, 0, 0, false,
                                 0, 0, false, 0);
            }
    std::printf("codec_test: %ld formats, %ld checks, %ld failed\n", formats, g_checks, g_fail);
    return g_fail ? 1 : 0;
}
