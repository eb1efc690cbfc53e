// Stand-alone host check of reth_amd/csrc/junction.h against a byte-wise
// nibble loop (built and run by tests/test_junction_cpu.py).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "junction.h"

static int nib(const uint8_t *k, int i)
{
    return (i & 1) ? (k[i >> 1] & 0xF) : (k[i >> 1] >> 4);
}

// reference: shared leading nibbles, *gt = a > b (first differing nibble)
static int ref_lcp(const uint8_t *a, const uint8_t *b, bool *gt)
{
    *gt = false;
    for (int i = 0; i < 64; ++i)
        if (nib(a, i) != nib(b, i)) {
            *gt = nib(a, i) > nib(b, i);
            return i;
        }
    return 64;
}

static int ref_junction(const uint8_t *la, const uint8_t *ls, const uint8_t *ra,
                        const uint8_t *rs, bool *bad)
{
    bool gt;
    if (ref_lcp(la, ra, &gt) < 64) {
        *bad = gt;
        return -1;
    }
    int l = ref_lcp(ls, rs, &gt);
    *bad = gt || l == 64;
    return l;
}

// the kernel's view of a key: four u64 loaded little-endian from memory
static void words(const uint8_t *k, uint64_t w[4])
{
    memcpy(w, k, 32); // the host is little-endian, like the device
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static void rnd_key(uint8_t *k)
{
    for (int i = 0; i < 4; ++i) {
        uint64_t r = rnd();
        memcpy(k + 8 * i, &r, 8);
    }
}

static long n_checked = 0, n_failed = 0;

static void check_lcp(const uint8_t *a, const uint8_t *b)
{
    uint64_t wa[4], wb[4];
    words(a, wa);
    words(b, wb);
    bool gt, rgt;
    int l = key_lcp_words(wa, wb, &gt), r = ref_lcp(a, b, &rgt);
    ++n_checked;
    if (l != r || gt != rgt) {
        if (n_failed++ < 10)
            fprintf(stderr, "key_lcp_words: got %d/%d want %d/%d\n", l, gt, r, rgt);
    }
}

static void check_junction(const uint8_t *la, const uint8_t *ls, const uint8_t *ra,
                           const uint8_t *rs)
{
    uint64_t wla[4], wls[4], wra[4], wrs[4];
    words(la, wla);
    words(ls, wls);
    words(ra, wra);
    words(rs, wrs);
    bool bad, rbad;
    int l = storage_junction(wla, wls, wra, wrs, &bad);
    int r = ref_junction(la, ls, ra, rs, &rbad);
    ++n_checked;
    if (l != r || bad != rbad) {
        if (n_failed++ < 10)
            fprintf(stderr, "storage_junction: got %d/%d want %d/%d\n", l, bad, r,
                    rbad);
    }
}

// b = a with nibble p raised or lowered (and everything after it random)
static void differ_at(const uint8_t *a, int p, uint8_t *b)
{
    rnd_key(b);
    memcpy(b, a, p / 2);
    int an = nib(a, p), bn;
    do
        bn = (int)(rnd() & 0xF);
    while (bn == an);
    if (p & 1)
        b[p >> 1] = (uint8_t)((a[p >> 1] & 0xF0) | bn);
    else
        b[p >> 1] = (uint8_t)((bn << 4) | (b[p >> 1] & 0x0F));
}

int main()
{
    uint8_t a[32], b[32], s[32], t[32];
    // every first-differing nibble position, both orders; equal keys; each
    // combined with the same account key and with account keys that differ
    // at every position, again in both orders
    for (int rep = 0; rep < 8; ++rep)
        for (int p = 0; p <= 64; ++p) {
            rnd_key(s);
            if (p < 64)
                differ_at(s, p, t);
            else
                memcpy(t, s, 32); // equal slot keys
            check_lcp(s, t);
            check_lcp(t, s);
            rnd_key(a);
            check_junction(a, s, a, t); // same account
            check_junction(a, t, a, s);
            for (int q = 0; q < 64; ++q) {
                differ_at(a, q, b);
                check_junction(a, s, b, t);
                check_junction(b, s, a, t);
                check_junction(a, t, b, s);
                check_junction(b, t, a, s);
            }
        }
    // extreme bytes around the byte swap
    memset(a, 0x00, 32);
    memset(b, 0xFF, 32);
    check_lcp(a, b);
    check_lcp(b, a);
    check_lcp(a, a);
    check_lcp(b, b);
    for (int p = 0; p < 64; ++p) {
        memset(a, 0x00, 32);
        memset(b, 0x00, 32);
        b[p >> 1] = (p & 1) ? 0x01 : 0x10; // lowest bit of nibble p only
        check_lcp(a, b);
        check_lcp(b, a);
        memset(a, 0xFF, 32);
        memcpy(b, a, 32);
        b[p >> 1] = (p & 1) ? 0xF7 : 0x7F; // highest bit of nibble p only
        check_lcp(a, b);
        check_lcp(b, a);
    }
    // 1M random pairs (half with a shared random-length prefix, so deep
    // positions occur), as keys and as junctions
    for (int k = 0; k < 1000000; ++k) {
        rnd_key(s);
        rnd_key(t);
        rnd_key(a);
        rnd_key(b);
        if (k & 1)
            memcpy(t, s, rnd() % 33);
        if (k & 2)
            memcpy(b, a, (k & 4) ? 32 : rnd() % 33);
        check_lcp(s, t);
        check_junction(a, s, b, t);
    }
    printf("checked %ld failed %ld\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
