// Junction of two adjacent storage entries: the compare the storage leaf
// kernel runs on the key words it already holds. Host-compilable so the
// compare can be tested without a GPU (tests/test_junction_cpu.py).
//
// A 32-byte big-endian key is held as four u64 words loaded little-endian
// from memory (word k = key bytes 8k..8k+7, byte j of the word = key byte
// 8k+j), exactly as the dwordx4 loads of an entry deliver it.
#ifndef SRE_JUNCTION_H
#define SRE_JUNCTION_H

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JUNCTION_HD __host__ __device__ __forceinline__
#else
#define JUNCTION_HD inline
#endif

// Shared leading nibbles of keys a and b (64 = equal); *gt = a > b. Returns
// what key_lcp returns on the same bytes: xor the words, select the first
// nonzero one, byte-swap it, clz >> 2. The first differing bit is set in
// exactly one of the two keys, so a > b iff it is set in a.
JUNCTION_HD int key_lcp_words(const uint64_t a[4], const uint64_t b[4], bool *gt)
{
    uint64_t x0 = a[0] ^ b[0], x1 = a[1] ^ b[1], x2 = a[2] ^ b[2],
             x3 = a[3] ^ b[3];
    uint64_t x = x2 ? x2 : x3, w = x2 ? a[2] : a[3];
    int base = x2 ? 32 : 48;
    x = x1 ? x1 : x; w = x1 ? a[1] : w; base = x1 ? 16 : base;
    x = x0 ? x0 : x; w = x0 ? a[0] : w; base = x0 ? 0 : base;
    if (!x) {
        *gt = false;
        return 64;
    }
    int c = __builtin_clzll(__builtin_bswap64(x));
    *gt = ((__builtin_bswap64(w) << c) >> 63) != 0;
    return base + (c >> 2);
}

// Junction of entry L (left) and its successor R in the sorted storage
// array. Returns the lcp byte stored for R: -1 where the account key
// changes (R starts a segment), else the shared nibbles of the slot keys.
// *bad = the pair violates the input contract: account keys descending, or
// within one account slot keys descending or equal. A bad junction may
// return 64; the caller must not build a leaf from it.
JUNCTION_HD int storage_junction(const uint64_t l_acct[4], const uint64_t l_slot[4],
                                 const uint64_t r_acct[4], const uint64_t r_slot[4],
                                 bool *bad)
{
    bool gt;
    if (key_lcp_words(l_acct, r_acct, &gt) < 64) {
        *bad = gt;
        return -1;
    }
    int l = key_lcp_words(l_slot, r_slot, &gt);
    *bad = gt || l == 64;
    return l;
}

#endif
