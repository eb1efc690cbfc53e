// Arithmetic of the plain-state hash-and-sort path (sre_upload_plain_state):
// digit extraction, the two sort-key constructions with the test gate's
// bit mask, the full 32-byte key compare and the tile / histogram offset
// arithmetic of hs_sort_pairs. No device-only intrinsics, so everything
// here is also checked by a host program (tests/hashsort_main.cpp).
//
// A 32-byte hash is held as four u64 words loaded little-endian from
// memory (word k = bytes 8k..8k+7, byte j of the word = hash byte 8k+j),
// which is also how the Keccak state delivers it.
#ifndef SRE_RADIX_H
#define SRE_RADIX_H

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RADIX_HD __host__ __device__ __forceinline__
#else
#define RADIX_HD inline
#endif

#define HS_RADIX_BITS 8
#define HS_BINS 256u
#define HS_PASSES 8            // 64-bit keys, 8-bit digits
#define HS_WAVE 64u
#define HS_WAVES 4u            // BLOCK / wave
#define HS_ROUNDS 8u           // keys per lane and tile
#define HS_WAVE_SPAN (HS_WAVE * HS_ROUNDS)       // 512 keys per wave
#define HS_TILE (HS_WAVES * HS_WAVE_SPAN)        // 2048 keys per tile

// digit of radix pass p (p = 0 is the least significant byte)
RADIX_HD uint32_t hs_digit(uint64_t key, int pass)
{
    return (uint32_t)(key >> (HS_RADIX_BITS * pass)) & (HS_BINS - 1);
}

// Keep the top `keep` bits of a `width`-bit prefix (width 32 or 64) and
// clear the rest. keep < 0 (gate unset) or keep >= width keeps everything.
RADIX_HD uint64_t hs_keep_top(uint64_t prefix, int width, int keep)
{
    if (keep < 0 || keep >= width)
        return prefix;
    if (keep == 0)
        return 0;
    uint64_t all = width == 64 ? ~0ull : ((1ull << width) - 1);
    return prefix & (all << (width - keep)) & all;
}

// Account sort key: the big-endian first 8 bytes of the hashed address
// (w0 = the hash's first word, little-endian loaded).
RADIX_HD uint64_t hs_account_key(uint64_t w0, int keep)
{
    return hs_keep_top(__builtin_bswap64(w0), 64, keep);
}

// Storage sort key: rank of the row's account in the sorted accounts in the
// high half, the big-endian first 4 bytes of the hashed slot in the low
// half. The gate masks the slot part only.
RADIX_HD uint64_t hs_storage_key(uint32_t rank, uint64_t slot_w0, int keep)
{
    uint32_t pre = __builtin_bswap32((uint32_t)slot_w0);
    return ((uint64_t)rank << 32) | hs_keep_top(pre, 32, keep);
}

// memcmp order of two 32-byte hashes held as LE-loaded words: -1, 0, 1.
RADIX_HD int hs_cmp_words(const uint64_t a[4], const uint64_t b[4])
{
    for (int k = 0; k < 4; ++k)
        if (a[k] != b[k])
            return __builtin_bswap64(a[k]) < __builtin_bswap64(b[k]) ? -1 : 1;
    return 0;
}

// ---- tiles --------------------------------------------------------------
// A block sorts one tile of HS_TILE consecutive pairs per pass. Inside the
// tile wave w owns the HS_WAVE_SPAN consecutive pairs from w * HS_WAVE_SPAN
// and reads them in HS_ROUNDS rounds of 64, so (wave, round, lane) order is
// index order and a stable rank is "pairs of my digit earlier in that
// order".

RADIX_HD uint64_t hs_num_tiles(uint64_t n)
{
    return (n + HS_TILE - 1) / HS_TILE;
}

// index of the pair that (wave, round, lane) of `tile` handles
RADIX_HD uint64_t hs_item_index(uint64_t tile, uint32_t wave, uint32_t round,
                                uint32_t lane)
{
    return tile * HS_TILE + wave * HS_WAVE_SPAN + round * HS_WAVE + lane;
}

// Slot of (digit, tile) in the histogram matrix. Digit-major: the exclusive
// scan of the flattened matrix is then, for every (digit, tile), the number
// of pairs with a smaller digit plus those with the same digit in earlier
// tiles, i.e. the tile's first output slot for that digit. A pair's slot is
// that base plus the pairs of its digit in earlier waves of the tile,
// earlier rounds of its wave and lower lanes of its round.
RADIX_HD uint64_t hs_hist_slot(uint32_t digit, uint64_t tile, uint64_t ntiles)
{
    return (uint64_t)digit * ntiles + tile;
}

// rank of a lane among its peers: set bits of the peer mask below the lane
RADIX_HD uint32_t hs_rank_in_mask(uint64_t peers, uint32_t lane)
{
    return (uint32_t)__builtin_popcountll(peers & ((1ull << lane) - 1));
}

#endif
