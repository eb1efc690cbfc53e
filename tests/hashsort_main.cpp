// Stand-alone host check of reth_amd/csrc/radix.h (built and run by
// tests/test_plain_model_cpu.py): digits and sort keys against byte and bit
// loops, the full-key compare against memcmp, and the tile / histogram
// offset arithmetic against a serial scan and std::stable_sort.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "radix.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static long n_checked = 0, n_failed = 0;
static void expect(bool ok, const char *what)
{
    ++n_checked;
    if (!ok && n_failed++ < 10)
        fprintf(stderr, "FAILED: %s\n", what);
}

// bit i (0 = most significant) of a byte string
static int bit_of(const uint8_t *b, int i)
{
    return (b[i >> 3] >> (7 - (i & 7))) & 1;
}

// the first `width` bits of h as an integer, bits at and after `keep` zeroed
static uint64_t prefix_ref(const uint8_t *h, int width, int keep)
{
    uint64_t v = 0;
    for (int i = 0; i < width; ++i)
        v = (v << 1) | (uint64_t)((keep < 0 || i < keep) ? bit_of(h, i) : 0);
    return v;
}

static void check_keys()
{
    const int gates[] = {-1, 0, 1, 4, 7, 8, 9, 31, 32, 33, 63, 64, 65};
    for (int rep = 0; rep < 2000; ++rep) {
        uint8_t h[32];
        for (int k = 0; k < 4; ++k) {
            uint64_t r = rep == 0 ? 0 : rep == 1 ? ~0ull : rnd();
            memcpy(h + 8 * k, &r, 8);
        }
        uint64_t w[4];
        memcpy(w, h, 32); // little-endian host, like the device
        uint32_t rank = rep == 1 ? 0xFFFFFFFEu : (uint32_t)rnd();
        for (int g : gates) {
            uint64_t ka = hs_account_key(w[0], g);
            expect(ka == prefix_ref(h, 64, g), "hs_account_key");
            uint64_t ks = hs_storage_key(rank, w[0], g);
            expect(ks == (((uint64_t)rank << 32) | prefix_ref(h, 32, g)),
                   "hs_storage_key");
            // digits: pass p is byte 7 - p of the big-endian key
            uint8_t be[8];
            for (int j = 0; j < 8; ++j)
                be[j] = (uint8_t)(ks >> (8 * (7 - j)));
            for (int p = 0; p < HS_PASSES; ++p)
                expect(hs_digit(ks, p) == be[7 - p], "hs_digit");
        }
    }
}

static int sign(int x) { return (x > 0) - (x < 0); }

static void check_compare()
{
    for (int rep = 0; rep < 200000; ++rep) {
        uint8_t a[32], b[32];
        for (int k = 0; k < 4; ++k) {
            uint64_t r = rnd(), q = rnd();
            memcpy(a + 8 * k, &r, 8);
            memcpy(b + 8 * k, &q, 8);
        }
        int share = (int)(rnd() % 34); // 33 = equal
        memcpy(b, a, share > 32 ? 32 : share);
        if (share < 32 && (rep & 1)) { // differ in one bit only
            memcpy(b, a, 32);
            b[share] ^= (uint8_t)(1u << (rnd() & 7));
        }
        uint64_t wa[4], wb[4];
        memcpy(wa, a, 32);
        memcpy(wb, b, 32);
        expect(hs_cmp_words(wa, wb) == sign(memcmp(a, b, 32)), "hs_cmp_words");
        expect(hs_cmp_words(wb, wa) == sign(memcmp(b, a, 32)), "hs_cmp_words rev");
    }
}

// One radix pass over n keys on the host, with exactly the arithmetic the
// kernels use, against std::stable_sort on the digit.
static void check_pass(uint64_t n, int pass, int spread)
{
    std::vector<uint64_t> keys(n);
    for (auto &k : keys)
        k = spread == 0 ? 0x0101010101010101ull * 7 : rnd() % spread * 0x0101010101010101ull;
    const uint64_t ntiles = hs_num_tiles(n);
    expect(ntiles * HS_TILE >= n && (ntiles == 0 || (ntiles - 1) * HS_TILE < n),
           "hs_num_tiles");
    // (tile, wave, round, lane) order is index order
    uint64_t next = 0;
    bool in_order = true;
    for (uint64_t t = 0; t < ntiles; ++t)
        for (uint32_t w = 0; w < HS_WAVES; ++w)
            for (uint32_t r = 0; r < HS_ROUNDS; ++r)
                for (uint32_t l = 0; l < HS_WAVE; ++l)
                    in_order &= hs_item_index(t, w, r, l) == next++;
    expect(in_order && next == ntiles * HS_TILE, "hs_item_index order");

    // stage 1 + 2: histogram matrix and its exclusive scan
    std::vector<uint32_t> hist(ntiles * HS_BINS, 0), offs(ntiles * HS_BINS, 0);
    for (uint64_t i = 0; i < n; ++i)
        hist[hs_hist_slot(hs_digit(keys[i], pass), i / HS_TILE, ntiles)]++;
    uint32_t run = 0;
    for (size_t j = 0; j < hist.size(); ++j) {
        offs[j] = run;
        run += hist[j];
    }
    // stage 3: per-tile, per-wave counts, then rounds with peer masks
    std::vector<uint64_t> out(n, ~0ull);
    std::vector<uint32_t> src(n, ~0u);
    bool in_range = true;
    for (uint64_t t = 0; t < ntiles; ++t) {
        std::vector<uint32_t> wcount(HS_WAVES * HS_BINS, 0);
        for (uint32_t w = 0; w < HS_WAVES; ++w)
            for (uint32_t r = 0; r < HS_ROUNDS; ++r)
                for (uint32_t l = 0; l < HS_WAVE; ++l) {
                    uint64_t i = hs_item_index(t, w, r, l);
                    if (i < n)
                        wcount[w * HS_BINS + hs_digit(keys[i], pass)]++;
                }
        for (uint32_t w = 0; w < HS_WAVES; ++w) {
            std::vector<uint32_t> earlier_rounds(HS_BINS, 0);
            for (uint32_t r = 0; r < HS_ROUNDS; ++r) {
                uint32_t dig[HS_WAVE];
                bool valid[HS_WAVE];
                for (uint32_t l = 0; l < HS_WAVE; ++l) {
                    uint64_t i = hs_item_index(t, w, r, l);
                    valid[l] = i < n;
                    dig[l] = valid[l] ? hs_digit(keys[i], pass) : 0;
                }
                for (uint32_t l = 0; l < HS_WAVE; ++l) {
                    if (!valid[l])
                        continue;
                    uint64_t peers = 0;
                    for (uint32_t m = 0; m < HS_WAVE; ++m)
                        if (valid[m] && dig[m] == dig[l])
                            peers |= 1ull << m;
                    uint32_t earlier_waves = 0;
                    for (uint32_t v = 0; v < w; ++v)
                        earlier_waves += wcount[v * HS_BINS + dig[l]];
                    uint64_t pos = (uint64_t)offs[hs_hist_slot(dig[l], t, ntiles)] +
                                   earlier_waves + earlier_rounds[dig[l]] +
                                   hs_rank_in_mask(peers, l);
                    uint64_t i = hs_item_index(t, w, r, l);
                    if (pos >= n || out[pos] != ~0ull) {
                        in_range = false;
                        continue;
                    }
                    out[pos] = keys[i];
                    src[pos] = (uint32_t)i;
                }
                for (uint32_t l = 0; l < HS_WAVE; ++l)
                    if (valid[l])
                        earlier_rounds[dig[l]]++;
            }
        }
    }
    expect(in_range, "every pair gets its own slot inside [0, n)");
    std::vector<uint32_t> want(n);
    for (uint64_t i = 0; i < n; ++i)
        want[i] = (uint32_t)i;
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) {
        return hs_digit(keys[a], pass) < hs_digit(keys[b], pass);
    });
    expect(in_range && src == want, "scatter equals stable_sort");
}

int main()
{
    check_keys();
    check_compare();
    // around every boundary of the tile arithmetic: the wave (64), the wave
    // span (512), the tile (2048), several tiles
    const uint64_t sizes[] = {0,    1,    2,    63,   64,   65,   511,  512,
                              513,  2047, 2048, 2049, 4095, 4096, 4097, 10000};
    for (uint64_t n : sizes)
        for (int spread : {0, 2, 256})
            check_pass(n, (int)(n % HS_PASSES), spread);
    printf("checked %ld failed %ld\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
