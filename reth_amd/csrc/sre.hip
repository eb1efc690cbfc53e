// sre.hip — MI355X-native state-root engine (gfx950 / CDNA4).
//
// From-scratch GPU implementation of the Merkle Patricia Trie commitment
// path behind include/sre.h. NOT a port: the reference
// (/root/reference/crates/trie, Rust, CPU-only) streams leaves through a
// sequential HashBuilder (crates/trie/trie/src/trie.rs:171-374); this engine
// instead builds each trie bottom-up from the sorted leaf stream with
// data-parallel LCP levels:
//
//   1. lcp[i] between adjacent keys (segment-aware; -1 sentinels at segment
//      boundaries = per-account storage tries, matching the per-account
//      independence of StorageRoot::calculate_with_cursors, trie.rs:750-876).
//      The storage leaf kernel computes these junctions itself (junction.h).
//   2. every leaf's parent-branch depth D = max(lcp[i], lcp[i+1]); leaf RLP
//      (hex-prefix short key from D+1 + RLP value) assembled directly in a
//      per-lane LDS slot, hashed by a per-lane Keccak-f[1600] sponge with the
//      5x5 state in VGPRs (all state indices compile-time constant).
//   3. levels d = maxD..0: nodes with parent depth == d grouped into branch
//      nodes (adjacent runs with junction lcp == d), 17-item branch RLP
//      assembled in LDS + hashed; extension wrap when the depth jumps; the
//      new node re-enters the level machinery at its own parent depth.
//   4. nodes reaching parent depth -1 are (per-segment) roots: root hash is
//      always keccak(RLP) (proof_v2/mod.rs:1628 compute_root_hash rule).
//
// Node semantics restated from the reference:
//   leaf  = RLP([HP(short,1), RLP_value])        proof_v2/node.rs:40-66
//   ext   = RLP([HP(shared,0), child_ref])
//   branch= RLP([c0..c15, ""])  (value slot always empty in state tries)
//   ref   = RLP if len<32 else 0xa0||keccak      RlpNode::from_rlp rule
//   storage value = minimal big-endian RLP of U256 (trie.rs:819-825)
//   account value = RLP([nonce,balance,storage_root,code_hash]) <= 110 B
//                   (trie.rs:472-476, root.rs:9-31)
//   empty storage -> EMPTY_ROOT_HASH (trie.rs:771-781)
//
// All hashing and node construction runs on-device; there is no CPU
// fallback. Parity: bit-exact vs oracle/ (tests/test_gpu_parity.py).

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>
#include <map>
#include <array>
#include <memory>
#include <numeric>
#include <optional>

#include "../../include/sre.h"
#include "junction.h"
#include "merge_plan.h" // the E_* bit numbers live there
#include "proof_host.h"
#include "radix.h"
#include "revert_plan.h"
#include "updates_diff.h"

#define BLOCK 256u

// ---------------------------------------------------------------------------
// device keccak-256 (one sponge per lane, state in registers)
// ---------------------------------------------------------------------------

__constant__ uint64_t KRC[24] = {
    0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL,
    0x8000000080008000ULL, 0x000000000000808bULL, 0x0000000080000001ULL,
    0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL,
    0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
    0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
    0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL,
    0x000000000000800aULL, 0x800000008000000aULL, 0x8000000080008081ULL,
    0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL,
};

__constant__ uint8_t D_EMPTY_ROOT[32] = {
    // keccak(rlp("")) — trie.rs:771-781 empty-storage shortcut
    0x56, 0xe8, 0x1f, 0x17, 0x1b, 0xcc, 0x55, 0xa6, 0xff, 0x83, 0x45, 0xe6,
    0x92, 0xc0, 0xf8, 0x6e, 0x5b, 0x48, 0xe0, 0x1b, 0x99, 0x6c, 0xad, 0xc0,
    0x01, 0x62, 0x2f, 0xb5, 0xe3, 0x63, 0xb4, 0x21,
};

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int n)
{
    return (x << n) | (x >> (64 - n));
}

// constant-amount 64-bit rotate as exactly two v_alignbit_b32 (the generic
// shift form compiles to a 64-bit shift + 32-bit shift + or; measured in
// profiles/ this is the keccak round's hottest primitive)
__device__ __forceinline__ uint64_t rotl64c(uint64_t x, int n)
{
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    uint32_t nh, nl;
    if (n == 32) {
        nh = lo;
        nl = hi;
    } else if (n < 32) {
        nh = __builtin_amdgcn_alignbit(hi, lo, 32 - n);
        nl = __builtin_amdgcn_alignbit(lo, hi, 32 - n);
    } else {
        int m = n - 32;
        nh = __builtin_amdgcn_alignbit(lo, hi, 32 - m);
        nl = __builtin_amdgcn_alignbit(hi, lo, 32 - m);
    }
    return ((uint64_t)nh << 32) | nl;
}

// 3-input bitwise ops on 64-bit lanes. gfx950 has v_bitop3_b32 (any boolean
// function of three operands, truth table in the immediate: src0 = 0xF0,
// src1 = 0xCC, src2 = 0xAA); the compiler does not form it from the plain
// expression (it emits v_bfi + v_xor for chi), so it is asked for by name.
__device__ __forceinline__ uint64_t xor3_64(uint64_t a, uint64_t b, uint64_t c)
{
#if defined(__gfx950__)
    uint32_t lo = __builtin_amdgcn_bitop3_b32((uint32_t)a, (uint32_t)b,
                                              (uint32_t)c, 0x96);
    uint32_t hi = __builtin_amdgcn_bitop3_b32((uint32_t)(a >> 32),
                                              (uint32_t)(b >> 32),
                                              (uint32_t)(c >> 32), 0x96);
    return ((uint64_t)hi << 32) | lo;
#else
    return a ^ b ^ c;
#endif
}

// chi: a ^ (~b & c), truth table 0xF0 ^ (~0xCC & 0xAA) = 0xD2
__device__ __forceinline__ uint64_t chi64(uint64_t a, uint64_t b, uint64_t c)
{
#if defined(__gfx950__)
    uint32_t lo = __builtin_amdgcn_bitop3_b32((uint32_t)a, (uint32_t)b,
                                              (uint32_t)c, 0xD2);
    uint32_t hi = __builtin_amdgcn_bitop3_b32((uint32_t)(a >> 32),
                                              (uint32_t)(b >> 32),
                                              (uint32_t)(c >> 32), 0xD2);
    return ((uint64_t)hi << 32) | lo;
#else
    return a ^ (~b & c);
#endif
}

// Keccak-f[1600]. Inner loops unrolled so every s[]/b[] index is a
// compile-time constant (register-resident; dynamic indexing would spill to
// scratch — cdna_hip_programming.md §5.4 rule 20).
__device__ void keccak_f(uint64_t s[25])
{
    #ifndef KECCAK_UNROLL
#define KECCAK_UNROLL 2
#endif
    // rho+pi as the XKCP in-place cycle walk (one temp, no b[25] copy —
    // the copy cost ~15 v_mov_b64 per round) and chi row-wise in place
    // with two saved lanes. Validated bit-exact against FIPS-202 vectors.
    // Theta and chi run on 3-input ops: column parity as two xor3, the
    // theta update s ^= c[x-1] ^ rotl(c[x+1],1) as one xor3 per lane (no
    // d[] array), chi as one op per lane.
    constexpr int PILN[24] = {10, 7,  11, 17, 18, 3, 5,  16, 8,  21, 24, 4,
                              15, 23, 19, 13, 12, 2, 20, 14, 22, 9,  6,  1};
    constexpr int ROTC[24] = {1,  3,  6,  10, 15, 21, 28, 36, 45, 55, 2,  14,
                              27, 41, 56, 8,  25, 43, 62, 18, 39, 61, 20, 44};
#pragma unroll KECCAK_UNROLL
    for (int r = 0; r < 24; ++r) {
        uint64_t c[5], cr[5];
#pragma unroll
        for (int x = 0; x < 5; ++x)
            c[x] = xor3_64(xor3_64(s[x], s[x + 5], s[x + 10]), s[x + 15],
                           s[x + 20]);
#pragma unroll
        for (int x = 0; x < 5; ++x)
            cr[x] = rotl64c(c[x], 1);
#pragma unroll
        for (int i = 0; i < 25; ++i)
            s[i] = xor3_64(s[i], c[(i + 4) % 5], cr[(i + 1) % 5]);
        uint64_t t = s[1], u;
#pragma unroll
        for (int k = 0; k < 24; ++k) {
            const int j = PILN[k];
            u = s[j];
            s[j] = rotl64c(t, ROTC[k]);
            t = u;
        }
#pragma unroll
        for (int y = 0; y < 25; y += 5) {
            uint64_t a0 = s[y], a1 = s[y + 1];
            s[y] = chi64(s[y], a1, s[y + 2]);
            s[y + 1] = chi64(s[y + 1], s[y + 2], s[y + 3]);
            s[y + 2] = chi64(s[y + 2], s[y + 3], s[y + 4]);
            s[y + 3] = chi64(s[y + 3], s[y + 4], a0);
            s[y + 4] = chi64(s[y + 4], a0, a1);
        }
        s[0] ^= KRC[r];
    }
}

// Hash a message in an LDS slot already zero-padded to nblocks*136 bytes
// with the 0x01 / 0x80 domain bytes applied.
__device__ __forceinline__ void keccak_lds(const uint64_t *slot, int nblocks,
                                           uint64_t out[4])
{
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 25; ++i)
        s[i] = 0;
    for (int blk = 0; blk < nblocks; ++blk) {
#pragma unroll
        for (int i = 0; i < 17; ++i)
            s[i] ^= slot[blk * 17 + i];
        keccak_f(s);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        out[i] = s[i];
}

// keccak pad10*1 (domain 0x01) over an LDS slot holding len message bytes
// (slot zeroed beyond len). Returns block count.
__device__ __forceinline__ int keccak_pad(uint8_t *slot, int len)
{
    int nblocks = len / 136 + 1;
    slot[len] = 0x01;
    slot[nblocks * 136 - 1] |= 0x80;
    return nblocks;
}

// ---------------------------------------------------------------------------
// device RLP / hex-prefix / key helpers (assembly goes straight into LDS;
// no dynamically-indexed private arrays -> no scratch spills)
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint8_t nib_of(const uint8_t *key, int i)
{
    return (key[i >> 1] >> ((i & 1) ? 0 : 4)) & 0x0f;
}

__device__ __forceinline__ int rlp_list_hdr_len(int payload)
{
    return payload < 56 ? 1 : (payload <= 255 ? 2 : 3);
}

__device__ __forceinline__ int rlp_list_hdr_write(uint8_t *p, int payload)
{
    if (payload < 56) {
        p[0] = (uint8_t)(0xc0 + payload);
        return 1;
    }
    if (payload <= 255) {
        p[0] = 0xf8;
        p[1] = (uint8_t)payload;
        return 2;
    }
    p[0] = 0xf9;
    p[1] = (uint8_t)(payload >> 8);
    p[2] = (uint8_t)payload;
    return 3;
}

// hex-prefix item length for key nibbles [from,to): HP bytes = 1+floor(n/2);
// the RLP string wrapper adds 1 prefix byte unless it is a single byte <0x80
// (HP first byte is <= 0x3f, so the 1-byte case is always unprefixed).
__device__ __forceinline__ int hp_bytes(int from, int to)
{
    return 1 + ((to - from) >> 1);
}

__device__ __forceinline__ int hp_item_len(int from, int to)
{
    int hb = hp_bytes(from, to);
    return hb == 1 ? 1 : 1 + hb;
}

// write the RLP string item of HP(key[from..to), leaf) at p; returns bytes.
__device__ __forceinline__ int hp_item_write(uint8_t *p, const uint8_t *key,
                                             int from, int to, int leaf)
{
    int n = to - from;
    int odd = n & 1;
    int hb = hp_bytes(from, to);
    int w = 0;
    if (hb > 1)
        p[w++] = (uint8_t)(0x80 + hb);
    uint8_t first = (uint8_t)((leaf ? 0x20 : 0x00) | (odd ? 0x10 : 0x00));
    int i = from;
    if (odd) {
        first |= nib_of(key, i);
        i++;
    }
    p[w++] = first;
    for (; i < to; i += 2)
        p[w++] = (uint8_t)((nib_of(key, i) << 4) | nib_of(key, i + 1));
    return w;
}

__device__ __forceinline__ uint64_t be64_at(const uint8_t *p)
{
    uint64_t v;
    memcpy(&v, p, 8);
    return __builtin_bswap64(v);
}

// Dynamic byte-granular funnels over little-endian-packed byte streams
// (byte k of a word = stream byte 8w+k). v_lshlrev_b64/v_lshrrev_b64 are
// single VOP3 ops on CDNA, so each funnel is ~4 VALU; the double-shift
// avoids the undefined 64-bit shift at tb == 0.
__device__ __forceinline__ uint64_t dn8(uint64_t lo, uint64_t hi, int tb)
{   // stream advanced by tb bytes: out byte k = concat(lo,hi) byte tb+k
    return (lo >> (8 * tb)) | ((hi << (63 - 8 * tb)) << 1);
}
__device__ __forceinline__ uint64_t up8(uint64_t prev, uint64_t cur, int tb)
{   // stream delayed by tb bytes: out byte k = (k>=tb) ? cur byte k-tb : prev tail
    return (cur << (8 * tb)) | ((prev >> (63 - 8 * tb)) >> 1);
}

// lcp in nibbles of two 32-byte keys; sets *gt if a > b.
__device__ __forceinline__ int key_lcp(const uint8_t *a, const uint8_t *b, bool *gt)
{
    *gt = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint64_t wa = be64_at(a + 8 * k);
        uint64_t wb = be64_at(b + 8 * k);
        if (wa != wb) {
            *gt = wa > wb;
            return k * 16 + (__clzll(wa ^ wb) >> 2);
        }
    }
    return 64;
}

// minimal big-endian length of a 32-byte big-endian value (0 for zero)
__device__ __forceinline__ int min_be_len(const uint8_t *v)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint64_t w = be64_at(v + 8 * k);
        if (w)
            return 32 - 8 * k - (__clzll(w) >> 3);
    }
    return 0;
}

// active trie node record, 48 bytes
struct __attribute__((aligned(16))) node_rec {
    uint32_t s, e;    // covered leaf interval [s, e)
    uint32_t seg;     // key word: the big-endian first four bytes of key[s], so
                      // nibble p < 8 is (seg >> (28 - 4p)) & 0xF, the account
                      // shard seg >> 28, the capture cell seg >> 12
    int8_t depth;     // parent branch depth this node waits for (-1 = root)
    uint8_t ref_len;  // 1..33 (0 marks a consumed root record)
    uint8_t ref[33];
    uint8_t pad_;     // child nibble at `depth` (nib(key, depth); 0 for roots)
};
static_assert(sizeof(node_rec) == 48, "node_rec must be 48 bytes");

// 3 x dwordx4: records are 16-B aligned (48-B stride in 256-B-aligned
// allocations); scalar u32 copies were address-throughput bound.
__device__ __forceinline__ void copy_rec(node_rec *dst, const node_rec *src)
{
    const int4 *s4 = (const int4 *)src;
    int4 *d4 = (int4 *)dst;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        d4[i] = s4[i];
}

__device__ __forceinline__ uint32_t key_word(const uint8_t *key)
{
    return ((uint32_t)key[0] << 24) | ((uint32_t)key[1] << 16) |
           ((uint32_t)key[2] << 8) | (uint32_t)key[3];
}

// ref from an LDS-resident rlp + its precomputed hash
__device__ __forceinline__ void make_ref(const uint8_t *rlp, int len,
                                         const uint64_t hash[4], uint8_t *ref,
                                         uint8_t *ref_len)
{
    if (len < 32) {
        *ref_len = (uint8_t)len;
        for (int i = 0; i < len; ++i)
            ref[i] = rlp[i];
    } else {
        *ref_len = 33;
        ref[0] = 0xa0;
        memcpy(ref + 1, hash, 32);
    }
}

// ---------------------------------------------------------------------------
// batch keccak (input generation / hashing-stage offload)
// ---------------------------------------------------------------------------

#define SLOT_KB 136
__global__ void __launch_bounds__(BLOCK) k_keccak_batch(
    const uint8_t *__restrict__ in, uint64_t stride, uint32_t len, uint64_t n,
    uint8_t *__restrict__ out)
{
    __shared__ __align__(16) uint8_t lds[BLOCK * SLOT_KB];
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint8_t *slot = lds + (uint64_t)threadIdx.x * SLOT_KB;
    uint64_t *slot64 = (uint64_t *)slot;
#pragma unroll
    for (int k = 0; k < SLOT_KB / 8; ++k)
        slot64[k] = 0;
    const uint8_t *msg = in + i * stride;
    for (uint32_t b = 0; b < len; ++b)
        slot[b] = msg[b];
    int nblocks = keccak_pad(slot, (int)len);
    uint64_t hash[4];
    keccak_lds(slot64, nblocks, hash);
    uint64_t *o = (uint64_t *)(out + 32 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        o[k] = hash[k];
}

// Any message length: blocks are absorbed straight from global memory, byte
// by byte, with the pad bytes patched in (no LDS slot, so no length limit).
// The multi-block sibling of k_keccak_batch; same keccak_f.
__global__ void __launch_bounds__(BLOCK) k_keccak_long(
    const uint8_t *__restrict__ in, uint64_t stride, uint32_t len, uint64_t n,
    uint8_t *__restrict__ out)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint8_t *msg = in + i * stride;
    const uint32_t nblocks = len / 136 + 1, last = nblocks * 136 - 1;
    uint64_t s[25];
#pragma unroll
    for (int k = 0; k < 25; ++k)
        s[k] = 0;
    for (uint32_t blk = 0; blk < nblocks; ++blk) {
#pragma unroll
        for (int w = 0; w < 17; ++w) {
            uint64_t v = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                uint32_t b = blk * 136 + w * 8 + k;
                uint8_t c = b < len ? msg[b] : (b == len ? 0x01 : 0x00);
                if (b == last)
                    c |= 0x80;
                v |= (uint64_t)c << (8 * k);
            }
            s[w] ^= v;
        }
        keccak_f(s);
    }
    uint64_t *o = (uint64_t *)(out + 32 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        o[k] = s[k];
}

// ---------------------------------------------------------------------------
// segmentation + lcp kernels
// ---------------------------------------------------------------------------

// One pass over adjacent entry pairs produces BOTH the segment-start flags
// (acct_key change) and the slot-key lcp array (with -1 sentinels exactly at
// the segment boundaries) — each 96-byte entry is pulled once.
__global__ void k_seg_flags_lcp(const sre_storage_entry *__restrict__ st,
                                uint64_t ns, uint32_t *__restrict__ flags,
                                int8_t *__restrict__ lcp,
                                uint32_t *__restrict__ err)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > ns)
        return;
    if (i == 0 || i == ns) {
        lcp[i] = -1;
        if (i == 0 && ns)
            flags[0] = 1;
        return;
    }
    bool gt;
    int la = key_lcp(st[i - 1].acct_key, st[i].acct_key, &gt);
    if (gt)
        atomicOr(err, 1u << E_UNSORTED_STORAGE);
    if (la < 64) { // segment boundary
        flags[i] = 1;
        lcp[i] = -1;
        return;
    }
    flags[i] = 0;
    int l = key_lcp(st[i - 1].slot_key, st[i].slot_key, &gt);
    if (gt || l == 64)
        atomicOr(err, 1u << E_UNSORTED_STORAGE);
    lcp[i] = (int8_t)l;
}

// One sweep of the flags and their exclusive scan (computed by the host):
// seg_id = inclusive_scan(flags) - 1, fixed up in place per element
// (excl + flag - 1), and the first entry of every segment.
// With seg_roots (storage pass, after the leaf kernel): a segment whose
// start is also its end (lcp[i + 1] == -1) is a single-slot trie, whose
// root is its leaf's hash: a 64-nibble leaf RLP is >= 35 B, so recs[i].ref
// is always 0xa0 || hash there.
__global__ void k_seg_starts(const uint32_t *__restrict__ flags,
                             uint32_t *__restrict__ seg_id, uint64_t ns,
                             uint32_t *__restrict__ seg_start,
                             const int8_t *__restrict__ lcp,
                             const node_rec *__restrict__ recs,
                             uint8_t *__restrict__ seg_roots)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns)
        return;
    const uint32_t f = flags[i];
    const uint32_t seg = seg_id[i] + f - 1;
    seg_id[i] = seg;
    if (f) {
        seg_start[seg] = (uint32_t)i;
        if (seg_roots && lcp[i + 1] == -1)
            memcpy(seg_roots + 32ull * seg, recs[i].ref + 1, 32);
    }
}

__global__ void k_seg_acct(const sre_storage_entry *__restrict__ st,
                           const uint32_t *__restrict__ seg_start, uint32_t n_seg,
                           const sre_account_entry *__restrict__ acct, uint64_t na,
                           uint32_t *__restrict__ seg_acct, uint32_t *__restrict__ err)
{
    uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg)
        return;
    const uint8_t *key = st[seg_start[s]].acct_key;
    uint64_t lo = 0, hi = na;
    while (lo < hi) {
        uint64_t mid = (lo + hi) / 2;
        bool gt;
        int l = key_lcp(acct[mid].key, key, &gt);
        if (l == 64) {
            seg_acct[s] = (uint32_t)mid;
            return;
        }
        if (gt)
            hi = mid;
        else
            lo = mid + 1;
    }
    atomicOr(err, 1u << E_ORPHAN_STORAGE);
}

__global__ void k_lcp_account(const sre_account_entry *__restrict__ acct, uint64_t na,
                              int subtree, int8_t *__restrict__ lcp,
                              uint32_t *__restrict__ err)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > na)
        return;
    if (i == 0 || i == na) {
        lcp[i] = -1;
        return;
    }
    bool gt;
    int l = key_lcp(acct[i - 1].key, acct[i].key, &gt);
    if (gt || l == 64)
        atomicOr(err, 1u << E_UNSORTED_ACCT);
    if (subtree && l == 0)
        l = -1;
    lcp[i] = (int8_t)l;
}

// ---------------------------------------------------------------------------
// leaf kernels
// ---------------------------------------------------------------------------

// Storage leaf: rlp <= 2 + 34 + 34 = 70 B -> always one keccak block.
//
// Fast path (D <= 13, i.e. the short key starts within the first 8 key
// bytes — always true for real states; 16^14 colliding keys otherwise):
// the hex-prefix packed short key is a byte-aligned SUFFIX of the slot
// key (nibbles from `from` pack into key bytes [(from+1)/2, 32) whether
// `from` is odd or even), so the whole message is three byte-streams —
// head, key suffix, value item — combined into the 17 keccak state words
// by register byte-funnels. No LDS traffic, no per-nibble loads, and the
// keccak pad byte rides the value funnel as a 5th input word. The slow
// path keeps the original byte-wise LDS assembly.
//
// The kernel also computes the junctions (junction.h) the trie shape comes
// from, so no separate pass reads the entries first: lane i loads its whole
// entry and entry i+1's two keys (a second load of lines its neighbour lane
// pulls anyway), computes the right junction and stores lcp[i+1] /
// flags[i+1]; the left junction is lane i-1's finished result, moved across
// with one shuffle. The first lane of a wave computes its left junction
// itself. Lane 0 stores lcp[0] / flags[0], lane ns-1 stores lcp[ns];
// st[-1] and st[ns] are never read. A junction travels as its lcp byte in
// bits 0..7 and the contract violation in bit 8. A lane with a violating
// junction on either side flags it and, like a zero-valued slot, writes
// neither record nor depth byte (a duplicate key's 64 shared nibbles would
// put `from` at 65); the host checks err before any level runs.
// Records carry the key word in seg, not a segment id: the ids exist only
// after this kernel (scan of the flags) and are looked up per entry where
// they are consumed.
#define SLOT_STO 136
__device__ __forceinline__ void words_of(uint4 a, uint4 b, uint64_t w[4])
{
    w[0] = (uint64_t)a.x | ((uint64_t)a.y << 32);
    w[1] = (uint64_t)a.z | ((uint64_t)a.w << 32);
    w[2] = (uint64_t)b.x | ((uint64_t)b.y << 32);
    w[3] = (uint64_t)b.z | ((uint64_t)b.w << 32);
}

// junction of entries l, r (adjacent, both inside the array), packed
__device__ __forceinline__ int packed_junction(const uint64_t l_acct[4],
                                               const uint64_t l_slot[4],
                                               const uint64_t r_acct[4],
                                               const uint64_t r_slot[4])
{
    bool bad;
    int l = storage_junction(l_acct, l_slot, r_acct, r_slot, &bad);
    return (l & 0xFF) | (bad ? 0x100 : 0);
}

__global__ void __launch_bounds__(BLOCK) k_leaf_storage(
    const sre_storage_entry *__restrict__ st, uint64_t ns,
    int8_t *__restrict__ lcp, uint32_t *__restrict__ flags,
    node_rec *__restrict__ recs, uint8_t *__restrict__ depths,
    uint32_t *__restrict__ hist, uint32_t *__restrict__ err)
{
    __shared__ __align__(16) uint8_t lds[BLOCK * SLOT_STO + 66 * 4];
    uint32_t *hist_l = (uint32_t *)(lds + BLOCK * SLOT_STO);
    if (threadIdx.x < 66)
        hist_l[threadIdx.x] = 0;
    __syncthreads();

    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < ns;
    uint64_t A[4], K[6], V[6];
    int jr = 0xFF; // right junction; the array end is a boundary (-1)
    if (live) {
        // entries are 96 B at a 16-B-aligned base -> acct_key/slot_key/value
        // are 16-B aligned; pull each as a dwordx4 pair once.
        const uint4 *e4 = (const uint4 *)&st[i];
        uint4 aa = e4[0], ac = e4[1], ka = e4[2], kc = e4[3], va = e4[4],
              vc = e4[5];
        words_of(aa, ac, A);
        words_of(ka, kc, K);
        words_of(va, vc, V);
        if (i + 1 < ns) {
            const uint4 *n4 = (const uint4 *)&st[i + 1];
            uint64_t NA[4], NK[4];
            words_of(n4[0], n4[1], NA);
            words_of(n4[2], n4[3], NK);
            jr = packed_junction(A, K, NA, NK);
            lcp[i + 1] = (int8_t)jr;
            flags[i + 1] = (jr & 0xFF) == 0xFF ? 1u : 0u;
        } else {
            lcp[ns] = -1;
        }
    }
    // every lane of the wave is here: the shuffle runs in uniform flow
    int jl = __shfl_up(jr, 1);
    if (live && (threadIdx.x & 63) == 0) {
        if (i == 0) {
            jl = 0xFF;
            lcp[0] = -1;
            flags[0] = 1;
        } else {
            const uint4 *p4 = (const uint4 *)&st[i - 1];
            uint64_t PA[4], PK[4];
            words_of(p4[0], p4[1], PA);
            words_of(p4[2], p4[3], PK);
            jl = packed_junction(PA, PK, A, K);
        }
    }
    if (live) {
        int l0 = (int8_t)jl, l1 = (int8_t)jr;
        int D = l0 > l1 ? l0 : l1;
        int from = D + 1;
        const bool bad = ((jl | jr) & 0x100) != 0;

        const uint8_t *key = st[i].slot_key;
        const uint8_t *val = st[i].value;

        K[4] = 0; K[5] = 0;
        V[4] = 0x01; // keccak pad start byte, rides the value funnel
        V[5] = 0;

        // vlen: value is big-endian bytes; first nonzero byte in memory
        // order (= lowest bytes of the LE-loaded words).
        int j0;
        if (V[0])      j0 = __builtin_ctzll(V[0]) >> 3;
        else if (V[1]) j0 = 8 + (__builtin_ctzll(V[1]) >> 3);
        else if (V[2]) j0 = 16 + (__builtin_ctzll(V[2]) >> 3);
        else if (V[3]) j0 = 24 + (__builtin_ctzll(V[3]) >> 3);
        else           j0 = 32;
        int vlen = 32 - j0;
        if (bad)
            atomicOr(err, 1u << E_UNSORTED_STORAGE);
        if (vlen == 0)
            atomicOr(err, 1u << E_ZERO_VALUE);
        if (bad || vlen == 0) {
            // rejected entry: no record, no depth byte
        } else if (D <= 13) {
            // ---- fast register path ----
            int kb = (from + 1) >> 1; // suffix start byte, 0..7
            int rj = j0 & 7, q0 = j0 >> 3;
            // value suffix stream (+pad): VS[j] = F[q0+j]
            uint64_t F0 = dn8(V[0], V[1], rj), F1 = dn8(V[1], V[2], rj),
                     F2 = dn8(V[2], V[3], rj), F3 = dn8(V[3], V[4], rj),
                     F4 = dn8(V[4], V[5], rj);
            uint64_t VS0 = q0 == 0 ? F0 : q0 == 1 ? F1 : q0 == 2 ? F2 : F3;
            uint64_t VS1 = q0 == 0 ? F1 : q0 == 1 ? F2 : q0 == 2 ? F3 : F4;
            uint64_t VS2 = q0 == 0 ? F2 : q0 == 1 ? F3 : q0 == 2 ? F4 : 0;
            uint64_t VS3 = q0 == 0 ? F3 : q0 == 1 ? F4 : 0;
            uint64_t VS4 = q0 == 0 ? F4 : 0;
            int top = (int)(VS0 & 0xFF);
            // storage value = encode_fixed_size(U256) (trie.rs:824) wrapped
            // once more as a string item; both prefix bytes appear together
            int vrlp_len = (vlen == 1 && top < 0x80) ? 1 : 1 + vlen;
            int vitem_len = vrlp_len == 1 ? 1 : 1 + vrlp_len;
            uint64_t VI0, VI1, VI2, VI3, VI4;
            if (vrlp_len == 1) {
                VI0 = VS0; VI1 = VS1; VI2 = VS2; VI3 = VS3; VI4 = VS4;
            } else {
                uint64_t pfx = (uint64_t)(0x80 + vrlp_len) |
                               ((uint64_t)(0x80 + vlen) << 8);
                VI0 = pfx | (VS0 << 16);
                VI1 = (VS1 << 16) | (VS0 >> 48);
                VI2 = (VS2 << 16) | (VS1 >> 48);
                VI3 = (VS3 << 16) | (VS2 >> 48);
                VI4 = (VS4 << 16) | (VS3 >> 48);
            }
            int n = 63 - D;  // short-key nibbles (>= 50 here)
            int odd = n & 1;
            int hb = 1 + (n >> 1);
            int payload = 1 + hb + vitem_len;
            int h = payload < 56 ? 1 : 2;
            int len = h + payload;
            int hl = h + 2;
            uint8_t first = (uint8_t)(0x20 | (odd ? 0x10 |
                ((int)(K[0] >> ((8 * kb - 8) & 63)) & 0xF) : 0));
            uint64_t head;
            if (h == 1)
                head = (uint64_t)(0xc0 + payload) |
                       ((uint64_t)(0x80 + hb) << 8) | ((uint64_t)first << 16);
            else
                head = 0xf8ull | ((uint64_t)payload << 8) |
                       ((uint64_t)(0x80 + hb) << 16) | ((uint64_t)first << 24);
            // key suffix: message byte x (x >= hl) = key byte x - t, t = hl-kb
            int t = hl - kb; // in [-4, 4]
            uint64_t lowmask = (1ull << (8 * hl)) - 1;
            uint64_t m0, m1, m2, m3, m4;
            if (t >= 0) {
                m0 = head | (up8(0, K[0], t) & ~lowmask);
                m1 = up8(K[0], K[1], t);
                m2 = up8(K[1], K[2], t);
                m3 = up8(K[2], K[3], t);
                m4 = up8(K[3], K[4], t);
            } else {
                int u = -t;
                m0 = head | (dn8(K[0], K[1], u) & ~lowmask);
                m1 = dn8(K[1], K[2], u);
                m2 = dn8(K[2], K[3], u);
                m3 = dn8(K[3], K[4], u);
                m4 = 0;
            }
            uint64_t m5 = 0, m6 = 0, m7 = 0, m8 = 0;
            // value item at vo = hl + (32 - kb) = 32 + t (28..36)
            int vo = 32 + t;
            int rv = vo & 7;
            uint64_t G0 = up8(0, VI0, rv), G1 = up8(VI0, VI1, rv),
                     G2 = up8(VI1, VI2, rv), G3 = up8(VI2, VI3, rv),
                     G4 = up8(VI3, VI4, rv), G5 = up8(VI4, 0, rv);
            if (vo < 32) {
                m3 |= G0; m4 |= G1; m5 = G2; m6 = G3; m7 = G4; m8 = G5;
            } else {
                // vi stream <= 35 B + rv <= 4 -> G5 is provably zero here
                m4 |= G0; m5 = G1; m6 = G2; m7 = G3; m8 = G4;
            }
            // single 136-B block; m9..m15 zero, end bit constant in s[16]
            uint64_t s[25];
            s[0] = m0; s[1] = m1; s[2] = m2; s[3] = m3; s[4] = m4;
            s[5] = m5; s[6] = m6; s[7] = m7; s[8] = m8;
#pragma unroll
            for (int k = 9; k < 25; ++k)
                s[k] = 0;
            s[16] = 0x8000000000000000ull;
            keccak_f(s);

            if (len >= 32) {
                // compose the whole 48-B record in registers, store as
                // 3 x dwordx4 (byte-wise ref stores were address-bound)
                uint8_t pb = D >= 0
                    ? (uint8_t)((K[0] >> ((8 * (D >> 1) +
                                           ((D & 1) ? 0 : 4)) & 63)) & 0xF)
                    : 0;
                uint32_t w[12];
                w[0] = (uint32_t)i;
                w[1] = (uint32_t)(i + 1);
                w[2] = __builtin_bswap32((uint32_t)K[0]); // key word
                w[3] = (uint32_t)(uint8_t)(int8_t)D | (33u << 8) |
                       (0xa0u << 16) | ((uint32_t)(s[0] & 0xFF) << 24);
                w[4] = (uint32_t)(s[0] >> 8);
                w[5] = (uint32_t)((s[0] >> 40) | (s[1] << 24));
                w[6] = (uint32_t)(s[1] >> 8);
                w[7] = (uint32_t)((s[1] >> 40) | (s[2] << 24));
                w[8] = (uint32_t)(s[2] >> 8);
                w[9] = (uint32_t)((s[2] >> 40) | (s[3] << 24));
                w[10] = (uint32_t)(s[3] >> 8);
                w[11] = (uint32_t)((s[3] >> 40) & 0xFFFFFF) |
                        ((uint32_t)pb << 24);
                uint4 *r4 = (uint4 *)&recs[i];
                r4[0] = make_uint4(w[0], w[1], w[2], w[3]);
                r4[1] = make_uint4(w[4], w[5], w[6], w[7]);
                r4[2] = make_uint4(w[8], w[9], w[10], w[11]);
            } else {
                // inline (<32 B) leaf ref: rare; message bytes from m0..m3
                node_rec *r = &recs[i];
                r->s = (uint32_t)i;
                r->e = (uint32_t)(i + 1);
                r->seg = key_word(key);
                r->depth = (int8_t)D;
                r->ref_len = (uint8_t)len;
                uint64_t mm[4] = {m0, m1, m2, m3};
                for (int k = 0; k < len; ++k)
                    r->ref[k] = (uint8_t)(mm[k >> 3] >> (8 * (k & 7)));
                r->pad_ = D >= 0 ? nib_of(key, D) : 0;
            }
            depths[i] = (uint8_t)(D + 1);
            // D == -1 (single-slot trie): the record's hash is the segment
            // root; k_seg_starts copies it out once the segment ids exist
            atomicAdd(&hist_l[D + 1], 1u);
        } else {
            // ---- slow LDS path (deep shared prefixes) ----
            uint8_t *slot = lds + (uint64_t)threadIdx.x * SLOT_STO;
            uint64_t *slot64 = (uint64_t *)slot;
#pragma unroll
            for (int k = 0; k < SLOT_STO / 8; ++k)
                slot64[k] = 0;
            // storage value = encode_fixed_size(U256) (trie.rs:824); the leaf
            // stores that RLP as a string item -> wrap once more.
            int vrlp_len = (vlen == 1 && val[31] < 0x80) ? 1 : 1 + vlen;
            int vitem_len = vrlp_len == 1 ? 1 : 1 + vrlp_len;
            int payload = hp_item_len(from, 64) + vitem_len;
            int h = rlp_list_hdr_write(slot, payload);
            int p = h + hp_item_write(slot + h, key, from, 64, 1);
            if (vrlp_len > 1)
                slot[p++] = (uint8_t)(0x80 + vrlp_len);
            if (vlen > 1 || val[31] >= 0x80)
                slot[p++] = (uint8_t)(0x80 + vlen);
            for (int k = 0; k < vlen; ++k)
                slot[p++] = val[32 - vlen + k];
            int len = h + payload;
            int nblocks = keccak_pad(slot, len);
            uint64_t hash[4];
            keccak_lds(slot64, nblocks, hash);

            node_rec *r = &recs[i];
            r->s = (uint32_t)i;
            r->e = (uint32_t)(i + 1);
            r->seg = key_word(key);
            r->depth = (int8_t)D;
            uint8_t rl;
            make_ref(slot, len, hash, r->ref, &rl);
            r->ref_len = rl;
            // child nibble at the parent branch (known now; saves the branch
            // assembler a scattered key gather per member)
            r->pad_ = D >= 0 ? nib_of(key, D) : 0;
            depths[i] = (uint8_t)(D + 1); // D >= 14: never a segment root
            atomicAdd(&hist_l[D + 1], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 66 && hist_l[threadIdx.x])
        atomicAdd(&hist[threadIdx.x], hist_l[threadIdx.x]);
}

// Account leaf. value = RLP([nonce,balance,storage_root,code_hash])
// (trie.rs:472-476); leaf rlp <= 2 + 34 + 2 + 113 = 151 B -> <= 2 blocks.
#define SLOT_ACC 280
__global__ void __launch_bounds__(BLOCK) k_leaf_account(
    const sre_account_entry *__restrict__ acct, uint64_t na,
    const uint8_t *__restrict__ storage_roots, const int8_t *__restrict__ lcp,
    int subtree, node_rec *__restrict__ recs, uint8_t *__restrict__ depths,
    uint32_t *__restrict__ hist, uint8_t *__restrict__ roots,
    uint8_t *__restrict__ child_refs, uint8_t *__restrict__ child_lens,
    const uint8_t *__restrict__ cell_dirty /* incremental: null = all */,
    const uint8_t *__restrict__ covered /* incremental: seeded positions */,
    const uint32_t *__restrict__ pos_list /* sparse launch: recompute set */,
    uint64_t n_list)
{
    __shared__ __align__(16) uint8_t lds[BLOCK * SLOT_ACC + 66 * 4];
    uint32_t *hist_l = (uint32_t *)(lds + BLOCK * SLOT_ACC);
    if (threadIdx.x < 66)
        hist_l[threadIdx.x] = 0;
    __syncthreads();

    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool active;
    if (pos_list) { // sparse launch: the position list IS the recompute set
        active = i < n_list;
        if (active)
            i = pos_list[i];
    } else {
        active = i < na;
        if (active && cell_dirty) {
            uint32_t cell = ((uint32_t)acct[i].key[0] << 12) |
                            ((uint32_t)acct[i].key[1] << 4) |
                            ((uint32_t)acct[i].key[2] >> 4);
            // recompute leaves of dirty cells and of positions no seeded
            // cell-top interval covers; clean covered cells keep their seeds
            active = cell_dirty[cell] != 0 || covered[i] == 0;
        }
    }
    if (active) {
        uint8_t *slot = lds + (uint64_t)threadIdx.x * SLOT_ACC;
        uint64_t *slot64 = (uint64_t *)slot;

        int8_t l0 = lcp[i], l1 = lcp[i + 1];
        int D = l0 > l1 ? l0 : l1;
        const uint8_t *key = acct[i].key;

        // account-value field lengths
        uint64_t nonce = acct[i].nonce;
        int nlen = nonce ? (8 - (__clzll(nonce) >> 3)) : 0;
        int nonce_rlp = (nlen == 0 || (nlen == 1 && nonce < 0x80)) ? 1 : 1 + nlen;
        const uint8_t *bal = acct[i].balance;
        int blen = min_be_len(bal);
        int bal_rlp = (blen == 0 || (blen == 1 && bal[31] < 0x80)) ? 1 : 1 + blen;
        int vw = nonce_rlp + bal_rlp + 33 + 33;      // account list payload
        int vh = rlp_list_hdr_len(vw);               // its list header (1: vw<56? vw>=68 -> 2... see below)
        int vtotal = vh + vw;                        // bytes of account RLP
        int vs = vtotal < 56 ? 1 : 2;                // string wrapper header

        // assemble + hash leaf with short key from `fr`
        auto emit = [&](int fr, uint64_t hash[4]) -> int {
#pragma unroll
            for (int k = 0; k < SLOT_ACC / 8; ++k)
                slot64[k] = 0;
            int payload = hp_item_len(fr, 64) + vs + vtotal;
            int h = rlp_list_hdr_write(slot, payload);
            int p = h + hp_item_write(slot + h, key, fr, 64, 1);
            if (vs == 1) {
                slot[p++] = (uint8_t)(0x80 + vtotal);
            } else {
                slot[p++] = 0xb8;
                slot[p++] = (uint8_t)vtotal;
            }
            p += rlp_list_hdr_write(slot + p, vw);
            if (nlen == 0) {
                slot[p++] = 0x80;
            } else {
                if (nonce_rlp > 1)
                    slot[p++] = (uint8_t)(0x80 + nlen);
                for (int k = nlen - 1; k >= 0; --k)
                    slot[p++] = (uint8_t)(nonce >> (8 * k));
            }
            if (blen == 0) {
                slot[p++] = 0x80;
            } else {
                if (bal_rlp > 1)
                    slot[p++] = (uint8_t)(0x80 + blen);
                for (int k = 0; k < blen; ++k)
                    slot[p++] = bal[32 - blen + k];
            }
            slot[p++] = 0xa0;
            for (int k = 0; k < 32; ++k) // null => accounts-only state
                slot[p++] = storage_roots ? storage_roots[32 * i + k]
                                          : D_EMPTY_ROOT[k];
            slot[p++] = 0xa0;
            for (int k = 0; k < 32; ++k)
                slot[p++] = acct[i].code_hash[k];
            int len = h + payload;
            int nblocks = keccak_pad(slot, len);
            keccak_lds(slot64, nblocks, hash);
            return len;
        };

        uint64_t hash[4];
        int len = emit(D + 1, hash);
        node_rec r;
        r.s = (uint32_t)i;
        r.e = (uint32_t)(i + 1);
        r.seg = key_word(key);
        const uint32_t shard = subtree ? r.seg >> 28 : 0u;
        r.depth = (int8_t)D;
        make_ref(slot, len, hash, r.ref, &r.ref_len);
        r.pad_ = D >= 0 ? nib_of(key, D) : 0;
        copy_rec(&recs[i], &r);
        depths[i] = (uint8_t)(D + 1);
        atomicAdd(&hist_l[D + 1], 1u);
        if (D == -1) {
            if (subtree) {
                uint64_t chash[4];
                int clen = emit(1, chash); // child-of-root-branch form
                uint8_t clens;
                make_ref(slot, clen, chash, child_refs + 33ull * shard, &clens);
                child_lens[shard] = clens;
                len = emit(0, hash); // standalone-root form
            }
            memcpy(roots + 32ull * shard, hash, 32);
        }
    } // active
    __syncthreads();
    if (threadIdx.x < 66 && hist_l[threadIdx.x])
        atomicAdd(&hist[threadIdx.x], hist_l[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// level machinery: selection / partition / merge / grouping
// ---------------------------------------------------------------------------


// parallel exclusive scan of 256 per-thread counts in LDS; returns (excl,
// total) — Hillis-Steele, 8 steps.
__device__ __forceinline__ void block_scan(uint32_t *lds, uint32_t v,
                                           uint32_t *excl, uint32_t *total)
{
    lds[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t off = 1; off < BLOCK; off <<= 1) {
        uint32_t x = threadIdx.x >= off ? lds[threadIdx.x - off] : 0;
        __syncthreads();
        lds[threadIdx.x] += x;
        __syncthreads();
    }
    *excl = threadIdx.x ? lds[threadIdx.x - 1] : 0;
    *total = lds[BLOCK - 1];
    __syncthreads();
}

// Level select over nodes kept IN PLACE: a node with interval [s, e) lives
// at recs[s] for its whole life (leaf i at recs[i]; a branch overwrites its
// first child's slot, branch_tail), and depths[s] = parent depth + 1. The
// input of level d is then "every slot whose depth byte is d+1, in slot
// order": one stable compaction per level, no bucket and no merges.
//
// Group starts fall out of the same sweep. A member at slot s starts a
// branch group exactly when lcp[s] < d: a first child's left neighbour key
// lies outside the branch (lcp[s] < d), every later sibling differs from
// its predecessor's keys first at nibble d (lcp[s] == d).
//
// One wave sweeps LV_SPAN = 1024 slots, 16 depth bytes per lane in one
// dwordx4 load; a wave with no member stops there. Per-wave counts are
// scanned on the device; ranks inside a wave come from ballots, so the
// order is stable and nothing is sorted or merged afterwards.
#define LV_SPAN 1024u

// Lane's 16 slots from `base`: bit k = slot base+k is a level-d member,
// bit 16+k = it also starts a group. Both arrays are 16-B aligned at base.
__device__ __forceinline__ uint32_t level_masks(const uint8_t *__restrict__ depths,
                                                const int8_t *__restrict__ lcp,
                                                uint64_t n, uint64_t base, int d)
{
    if (base >= n)
        return 0;
    const uint32_t key = (uint32_t)(d + 1);
    uint32_t m = 0, g = 0;
    if (base + 16 <= n) {
        uint4 v = *(const uint4 *)(depths + base);
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k)
            m |= (((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) == key) ? 1u << k : 0u;
        if (m) {
            uint4 l = *(const uint4 *)(lcp + base);
            uint32_t lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
            for (int k = 0; k < 16; ++k)
                g |= ((int)(int8_t)(lw[k >> 2] >> (8 * (k & 3))) < d) ? 1u << k
                                                                     : 0u;
            g &= m;
        }
    } else { // the array's last, partial 16 slots
        for (int k = 0; base + k < n; ++k)
            if (depths[base + k] == key) {
                m |= 1u << k;
                if ((int)lcp[base + k] < d)
                    g |= 1u << k;
            }
    }
    return m | (g << 16);
}

// cnts[w] = level-d members in wave w's span, cnts[nw + w] = group starts
// among them (two rows, scanned as one array).
__global__ void __launch_bounds__(BLOCK) k_level_count(
    const uint8_t *__restrict__ depths, const int8_t *__restrict__ lcp,
    uint64_t n, int d, uint32_t nw, uint32_t *__restrict__ cnts)
{
    uint64_t w = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    int lane = threadIdx.x & 63;
    if (w >= nw)
        return;
    uint32_t mg = level_masks(depths, lcp, n, w * LV_SPAN + (uint64_t)lane * 16, d);
    uint32_t c = 0; // members | starts << 16, each <= 1024
    if (__ballot(mg != 0)) {
        c = (uint32_t)__popc(mg & 0xFFFFu) | ((uint32_t)__popc(mg >> 16) << 16);
#pragma unroll
        for (int off = 32; off; off >>= 1)
            c += __shfl_xor(c, off);
    }
    if (lane == 0) {
        cnts[w] = c & 0xFFFFu;
        cnts[(uint64_t)nw + w] = c >> 16;
    }
}

// List level d's members: idx[p] = slot of member p (slot order), and the
// group starts gs[] as positions in that list. The records stay where they
// are; the branch kernels read member p as recs[idx[p]] (and its interval
// start as idx[p] itself: every record sits at its own s). offs = exclusive
// scan of k_level_count's rows, so the second row's entries are offset by
// n_level. The span is walked in 16 rounds of 64 consecutive slots (lane =
// slot, so a round's index stores are one contiguous run); round r's member
// bits sit in lanes 4r..4r+3 of the masks.
__global__ void __launch_bounds__(BLOCK) k_level_gather(
    const uint8_t *__restrict__ depths, const int8_t *__restrict__ lcp,
    uint64_t n, int d, uint32_t nw,
    const uint32_t *__restrict__ offs, uint32_t n_level, uint32_t n_groups,
    uint32_t *__restrict__ idx, uint32_t *__restrict__ gs)
{
    uint64_t w = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    int lane = threadIdx.x & 63;
    if (w >= nw)
        return;
    uint64_t base = w * LV_SPAN;
    uint32_t mg = level_masks(depths, lcp, n, base + (uint64_t)lane * 16, d);
    if (!__ballot(mg != 0))
        return;
    uint32_t pos = offs[w];
    uint32_t gpos = offs[(uint64_t)nw + w] - n_level;
    const uint64_t below = (1ull << lane) - 1;
    for (int r = 0; r < 16; ++r) {
        uint32_t v = __shfl(mg, 4 * r + (lane >> 4)) >> (lane & 15);
        bool hit = v & 1u, start = (v >> 16) & 1u;
        uint64_t mh = __ballot(hit);
        if (!mh)
            continue;
        uint64_t ms = __ballot(start);
        if (hit) {
            uint32_t p = pos + (uint32_t)__popcll(mh & below);
            if (p < n_level) { // always, when counts and host agree
                idx[p] = (uint32_t)(base + (uint64_t)r * 64 + lane);
                if (start) {
                    uint32_t gp = gpos + (uint32_t)__popcll(ms & below);
                    if (gp < n_groups)
                        gs[gp] = p;
                }
            }
        }
        pos += (uint32_t)__popcll(mh);
        gpos += (uint32_t)__popcll(ms);
    }
}

// ---------------------------------------------------------------------------
// branch kernel
// ---------------------------------------------------------------------------

#define SLOT_BR 552 // >= 4*136 zero-padded branch RLP slot in global scratch
// Branch scratch layout: column-major u64 words (word w of group g at
// w * stride + g: per-instruction coalescing). A row-major layout (576-B row
// per group) was tried and measured slower: col 444.7 ms vs row 456.6 ms
// @10Mx64.
#ifndef SRE_BR_CHUNK_MB
#define SRE_BR_CHUNK_MB 16 // branch-pipeline chunk, Mi-groups. Measured:
// 16 beats 8 (382.5 vs 385.0 ms at 10Mx64); 32 OOMs the ping-pong scratch.
#endif


// per-group metadata produced by the assemble kernel
struct br_meta {
    uint32_t s, e, seg;
    uint16_t br_len;   // 0 marks an invariant-violation group (error flagged)
    int8_t P;          // parent depth (-1 = segment root)
    uint8_t d;         // branch depth (level)
    uint8_t flags;     // bit0: stored (hash_mask != 0 — has a hashed-branch child)
    uint8_t pad_[3];
};
static_assert(sizeof(br_meta) == 20, "br_meta must be 20 bytes");


// Assemble one branch node per lane, streaming bytes through a register
// appender straight into the COLUMN-MAJOR u64 scratch (no LDS at all): a
// per-lane LDS slot capped occupancy at 4 waves/CU and left the kernel 99%
// latency-stalled (profiles/r01_2Mx64_sq_pmc.txt); the appender keeps the
// kernel at full occupancy and every scratch store coalesced.
#ifndef BLOCK_A
#define BLOCK_A 256
#endif

struct byte_appender {
    uint64_t cur;
    int pos;      // bytes filled in cur (0..7)
    int widx;     // next column-major word index
    uint64_t *base;
    uint64_t stride;
    uint32_t g;

    __device__ __forceinline__ void init(uint64_t *b, uint64_t s, uint32_t gg)
    {
        cur = 0;
        pos = 0;
        widx = 0;
        base = b;
        stride = s;
        g = gg;
    }
    __device__ __forceinline__ uint64_t *slot64(int w)
    {
        if (stride == 0) // direct row (fused kernel's LDS slot)
            return base + w;
        return base + (uint64_t)w * stride + g;
    }
    __device__ __forceinline__ void put(uint8_t v)
    {
        cur |= (uint64_t)v << (8 * pos);
        if (++pos == 8) {
            *slot64(widx) = cur;
            widx++;
            pos = 0;
            cur = 0;
        }
    }
    // append nbytes (1..33) from the LE-packed word stream R[0..4]
    // (stream byte k = R[k/8] byte k%8): word funnels + predicated flushes
    // instead of per-byte flush checks. Garbage bytes of R beyond nbytes
    // never reach the scratch: flushed words only cover stream bytes
    // < pos+nbytes, and the carried partial word is masked.
    __device__ __forceinline__ void put_bytes33(const uint64_t R[5], int nbytes)
    {
        int total = pos + nbytes;
        uint64_t S0 = cur | (R[0] << (8 * pos));
        uint64_t S1 = up8(R[0], R[1], pos);
        uint64_t S2 = up8(R[1], R[2], pos);
        uint64_t S3 = up8(R[2], R[3], pos);
        uint64_t S4 = up8(R[3], R[4], pos);
        int F = total >> 3;
        if (F > 0) *slot64(widx) = S0;
        if (F > 1) *slot64(widx + 1) = S1;
        if (F > 2) *slot64(widx + 2) = S2;
        if (F > 3) *slot64(widx + 3) = S3;
        if (F > 4) *slot64(widx + 4) = S4;
        widx += F;
        cur = F == 0 ? S0 : F == 1 ? S1 : F == 2 ? S2 : F == 3 ? S3
            : F == 4 ? S4 : 0;
        pos = total & 7;
        cur &= pos ? (1ull << (8 * pos)) - 1 : 0;
    }
    // finish the message with the keccak pad10*1: the start byte 0x01
    // right after the message, zero-fill to the last word of block nb, and
    // the end bit (0x80) in the block's final byte. The start byte goes
    // into `cur` WITHOUT the flush put() would do: when the message ends
    // one byte short of the rate (len % 136 == 135) both pad bytes are the
    // same byte, and a flushed final word would be overwritten below.
    __device__ __forceinline__ void finish(int nb)
    {
        cur |= (uint64_t)0x01 << (8 * pos);
        int last = nb * 17 - 1;
        while (widx < last) {
            *slot64(widx) = cur;
            widx++;
            cur = 0;
            pos = 0;
        }
        cur |= 0x8000000000000000ULL;
        *slot64(last) = cur;
    }
};

// Branch-size class of a group with nmem members: guaranteed RLP block
// count 1/2/3/4 (payload <= 1 + (16-nmem) + 33*nmem, so nmem<=3 -> <=115 B
// -> 1 block, <=7 -> 2, <=11 -> 3, else 4). Groups are partitioned by class
// per chunk so every wave of k_branch_assemble / k_branch_hash is
// block-count uniform: the hash absorb runs lane-sum (not wave-max) keccak,
// and assemble's column-major flush addresses stay within one class's word
// range instead of scattering over 0..68.
__device__ __forceinline__ int nmem_class(uint32_t nmem)
{
    return nmem <= 3 ? 0 : nmem <= 7 ? 1 : nmem <= 11 ? 2 : 3;
}

#define CLS_BLOCK 256
// per-block class histogram, laid out cnts[c*nblk + b] so ONE exclusive
// scan over 4*nblk yields every (class, block) partition offset
__global__ void k_class_hist(const uint32_t *__restrict__ gs, uint32_t n_groups,
                             uint32_t nblk, uint32_t *__restrict__ cnts)
{
    __shared__ uint32_t c_l[4];
    if (threadIdx.x < 4)
        c_l[threadIdx.x] = 0;
    __syncthreads();
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n_groups)
        atomicAdd(&c_l[nmem_class(gs[g + 1] - gs[g])], 1u);
    __syncthreads();
    if (threadIdx.x < 4)
        cnts[threadIdx.x * nblk + blockIdx.x] = c_l[threadIdx.x];
}

// scatter: perm[offs[c*nblk + b] + rank] = g. STABLE (ballot ranks +
// per-wave LDS counts): group order within each class is preserved, so
// the assemble/fused kernels' member gathers stay coalesced — the old
// atomic-bump scatter randomized the order and left the fused kernel
// gather-latency bound.
__global__ void k_class_scatter(const uint32_t *__restrict__ gs,
                                uint32_t n_groups, uint32_t nblk,
                                const uint32_t *__restrict__ offs,
                                uint32_t *__restrict__ perm,
                                uint32_t *__restrict__ inv /* nullable */)
{
    __shared__ uint32_t wh[4][CLS_BLOCK / 64];
    int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < 4)
#pragma unroll
        for (int w = 0; w < CLS_BLOCK / 64; ++w)
            wh[threadIdx.x][w] = 0;
    __syncthreads();
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    int c = (g < n_groups) ? nmem_class(gs[g + 1] - gs[g]) : 255;
    uint32_t rank_in_wave = 0;
    for (int k = 0; k < 4; ++k) {
        uint64_t m = __ballot(c == k);
        if (c == k)
            rank_in_wave = __popcll(m & ((1ull << lane) - 1));
        if (lane == 0 && m)
            wh[k][wid] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (c > 3)
        return;
    uint32_t before = 0;
    for (int w = 0; w < wid; ++w)
        before += wh[c][w];
    uint32_t slot = offs[(uint32_t)c * nblk + blockIdx.x] + before +
                    rank_in_wave;
    perm[slot] = g;
    if (inv)
        inv[g] = slot;
}

#ifndef ASM_MEMBERS
#define ASM_MEMBERS 4 // members whose loads one step of k_branch_assemble issues
#endif
__global__ void __launch_bounds__(BLOCK_A, 8) k_branch_assemble(
    const node_rec *__restrict__ recs, const uint32_t *__restrict__ idx,
    const uint32_t *__restrict__ gs,
    uint32_t n_groups, const int8_t *__restrict__ lcp,
    const uint8_t *__restrict__ keys, uint64_t key_stride, int d,
    uint8_t *__restrict__ scratch, uint64_t scratch_stride,
    br_meta *__restrict__ meta, const uint32_t *__restrict__ perm,
    uint32_t *__restrict__ err)
{
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups)
        return;
    uint32_t gg = perm ? perm[g] : g; // meta/scratch by thread slot g
    uint64_t j = gs[gg], jend = gs[gg + 1];
    br_meta mt;
    mt.s = idx[j]; // a record's slot is its s
    mt.e = recs[idx[jend - 1]].e;
    mt.seg = recs[mt.s].seg;
    mt.d = (uint8_t)d;
    int8_t pl = lcp[mt.s], pr = lcp[mt.e];
    mt.P = pl > pr ? pl : pr;

    int nmem = (int)(jend - j);
    // ONE pass over the members: cache each member's child nibble (4 bits
    // into a u64), validate strictly-ascending nibbles (implies distinct,
    // in-order, and <= 16 of them), accumulate the payload.
    // Members are taken ASM_MEMBERS at a time: their slots (contiguous in
    // idx), then their records, each set of loads issued together, so a
    // step costs two round trips, not two per member. The spare places of
    // a short last step re-read the group's last member.
    uint64_t nibs = 0;
    int payload = 1 + (16 - nmem);
    bool order_ok = nmem >= 2 && nmem <= 16;
    bool stored = false; // this branch gets a TrieUpdates row (hash_mask != 0)
    {
        int prev = -1;
        for (int c0 = 0; c0 < nmem && order_ok; c0 += ASM_MEMBERS) {
            uint32_t sl[ASM_MEMBERS], w3[ASM_MEMBERS], w11[ASM_MEMBERS];
#pragma unroll
            for (int k = 0; k < ASM_MEMBERS; ++k)
                sl[k] = idx[j + (c0 + k < nmem ? c0 + k : nmem - 1)];
#pragma unroll
            for (int k = 0; k < ASM_MEMBERS; ++k) {
                const uint32_t *r32 = (const uint32_t *)&recs[sl[k]];
                w3[k] = r32[3];   // depth, ref_len, ref[0..1]
                w11[k] = r32[11]; // ..., pad_
            }
#pragma unroll
            for (int k = 0; k < ASM_MEMBERS; ++k)
                if (c0 + k < nmem) {
                    uint8_t pb = (uint8_t)(w11[k] >> 24);
                    int nbm = pb & 0xF; // child nibble, stored at node creation
                    order_ok &= nbm > prev;
                    prev = nbm;
                    nibs |= (uint64_t)nbm << (4 * (c0 + k));
                    payload += (w3[k] >> 8) & 0xFF; // ref_len
                    stored |= (pb & 0x20) != 0; // member is a hashed branch
                }
        }
    }
    mt.flags = stored ? 1 : 0;
    if (!order_ok || payload > 529) {
        atomicOr(err, 1u << E_INTERNAL);
        mt.br_len = 0;
        mt.flags = 0;
        meta[g] = mt;
        return;
    }
    int h = rlp_list_hdr_len(payload);
    int br_len = h + payload;
    // NOTE: the keccak pad must land at the message's own rate boundary —
    // absorbing extra zero blocks up to the class bound would change the
    // digest, so block count stays per-lane (waves are still class-uniform
    // in the typical all-hashed-refs case).
    int nb = br_len / 136 + 1;
    // everything in the meta is known: store it now, so that its registers
    // are free while the member records are in flight (64 VGPRs, 8 waves)
    mt.br_len = (uint16_t)br_len;
    meta[g] = mt;

    byte_appender ap;
    ap.init((uint64_t *)scratch, scratch_stride, g);
    if (payload < 56) {
        ap.put((uint8_t)(0xc0 + payload));
    } else if (payload <= 255) {
        ap.put(0xf8);
        ap.put((uint8_t)payload);
    } else {
        ap.put(0xf9);
        ap.put((uint8_t)(payload >> 8));
        ap.put((uint8_t)payload);
    }
    {
        // member by member (ascending nibbles), empty items in the gaps;
        // the same ASM_MEMBERS-wide steps as the validation pass
        int prevnib = -1;
        for (int c0 = 0; c0 < nmem; c0 += ASM_MEMBERS) {
            uint32_t sl[ASM_MEMBERS], w[ASM_MEMBERS][9];
#pragma unroll
            for (int k = 0; k < ASM_MEMBERS; ++k)
                sl[k] = idx[j + (c0 + k < nmem ? c0 + k : nmem - 1)];
#pragma unroll
            for (int k = 0; k < ASM_MEMBERS; ++k) {
                const uint32_t *rec32 = (const uint32_t *)&recs[sl[k]];
#pragma unroll
                for (int q = 0; q < 9; ++q)
                    w[k][q] = rec32[3 + q]; // bytes 12..48 of the record
            }
#pragma unroll
            for (int k = 0; k < ASM_MEMBERS; ++k)
                if (c0 + k < nmem) {
                    int nbm = (int)((nibs >> (4 * (c0 + k))) & 0xF);
                    for (int b = prevnib + 1; b < nbm; ++b)
                        ap.put(0x80);
                    prevnib = nbm;
                    int rl = (w[k][0] >> 8) & 0xFF; // ref_len
                    // ref byte i lives at record byte 14+i: repack into the
                    // LE word stream R and append word-wise
                    const uint32_t *v = w[k];
                    uint64_t R[5];
                    R[0] = ((uint64_t)v[0] >> 16) | ((uint64_t)v[1] << 16) |
                           ((uint64_t)v[2] << 48);
                    R[1] = ((uint64_t)v[2] >> 16) | ((uint64_t)v[3] << 16) |
                           ((uint64_t)v[4] << 48);
                    R[2] = ((uint64_t)v[4] >> 16) | ((uint64_t)v[5] << 16) |
                           ((uint64_t)v[6] << 48);
                    R[3] = ((uint64_t)v[6] >> 16) | ((uint64_t)v[7] << 16) |
                           ((uint64_t)v[8] << 48);
                    R[4] = ((uint64_t)v[8] >> 16) & 0xFF;
                    ap.put_bytes33(R, rl);
                }
        }
        for (int b = prevnib + 1; b < 16; ++b)
            ap.put(0x80);
        ap.put(0x80); // empty value item
    }
    ap.finish(nb); // keccak pad
}

// Everything after a branch's RLP keccak: ref composition, extension/root
// wraps, record/bhash/seg-root emission and the pending-histogram bumps.
// Shared by the split hash kernel and the fused 1-block kernel.
// A non-root node is placed where the next levels look for it: recs[mt.s]
// (its first child's slot) with depth byte P + 1. Roots and error groups
// store no record. The other consumed slots keep a stale depth byte; that
// is harmless: a placed record's byte is <= d and levels only descend, so a
// stale byte (d+1 or more) is never selected again.
//
// The level's members are read from recs too (recs[idx[p]]), while this
// store overwrites one of them. Why no reader sees a record of this level:
// - the groups of a level have disjoint member sets (a member belongs to
//   the one branch its depth byte and position name), and the only slot a
//   group writes is its own first member's. So a group's members are
//   written by that group alone, and only after it has read them:
//   - a fused lane loads every member (validation words, then the emit
//     re-read) before its own branch_tail;
//   - in the split path a chunk's k_branch_assemble, k_proof_grab and
//     k_emit_updates are ordered before that chunk's k_branch_hash (same
//     stream, or the assemble event the hash waits for);
// - chunk k+1's assemble and the stream2 slice of the fused kernel overlap
//   chunk k's hash, but they touch other groups' slots. Records of
//   different groups may share a 128-B line; the stores are whole-record
//   dwordx4 stores and never touch a neighbour's bytes;
// - k_proof_grab's search reads idx (written by the select, not here) and
//   the e of a group's LAST member, which no group of this level writes;
// - k_capture_L runs before any branch kernel of its level, after the
//   previous level's streams have joined;
// - depths[] is written here and read only by the next level's select.
// This holds in every mode (root, subtree, updates, proof, retaining /
// incremental): they differ in which of these kernels run, not in order.
// `inline_src64` points at the branch RLP's word 0 for the <32-B inline
// case, with `inline_stride` u64s between message words (column-major
// scratch: stride = chunk; LDS row: stride = 1). `ext` is a per-lane LDS
// scratch of >= SLOT_EXT bytes (may alias the message slot: the inline
// words are consumed before the first wrap reuses it).
#define SLOT_EXT 88
// hist_l of the branch kernels: [0..65] the pending bumps, [BR_HIST_Q] the
// block's deferred-wrap count, [BR_HIST_Q + 1] its base in the job queue
#define BR_HIST_Q 66
#define BR_HIST 68
#define NO_WRAP_JOB 0xFFFFFFFFu

// Extension node over key0[from..d) around the child ref `refw` (LE word
// stream, ref_len bytes), from < d: RLP built in `ext` (>= SLOT_EXT bytes of
// LDS), one keccak block. Result: the node's hash and its ref.
__device__ __forceinline__ void ext_wrap(uint8_t *ext, const uint8_t *key0,
                                         int from, int d,
                                         const uint64_t refw[5], uint8_t ref_len,
                                         uint64_t whash[4], uint64_t wrefw[5],
                                         uint8_t *wrl)
{
    uint64_t *ext64 = (uint64_t *)ext;
#pragma unroll
    for (int k = 0; k < SLOT_EXT / 8; ++k)
        ext64[k] = 0;
    int pay = hp_item_len(from, d) + ref_len;
    int hh = rlp_list_hdr_write(ext, pay);
    int p = hh + hp_item_write(ext + hh, key0, from, d, 0);
#pragma unroll
    for (int k = 0; k < 33; ++k)
        if (k < ref_len)
            ext[p + k] = (uint8_t)(refw[k >> 3] >> (8 * (k & 7)));
    int len = hh + pay; // <= 69 < SLOT_EXT
    ext[len] = 0x01;    // pad start; end bit lands in lane 16 below
    // single 136-B keccak block: absorb SLOT_EXT bytes + implicit zeros
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 25; ++i)
        s[i] = 0;
#pragma unroll
    for (int i = 0; i < SLOT_EXT / 8; ++i)
        s[i] ^= ext64[i];
    s[16] ^= 0x8000000000000000ULL; // pad end bit of the 136-B block
    keccak_f(s);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        whash[k] = s[k];
    if (len < 32) {
        *wrl = (uint8_t)len;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            wrefw[k] = ext64[k];
        wrefw[4] = 0;
    } else {
        *wrl = 33;
        wrefw[0] = 0xa0ull | (s[0] << 8);
        wrefw[1] = (s[0] >> 56) | (s[1] << 8);
        wrefw[2] = (s[1] >> 56) | (s[2] << 8);
        wrefw[3] = (s[2] >> 56) | (s[3] << 8);
        wrefw[4] = s[3] >> 56;
    }
}

// Whole 48-B record composed in registers, 3 x dwordx4 stores: interval,
// seg, parent depth P, the ref (LE word stream) and the pad byte.
__device__ __forceinline__ void store_rec(node_rec *r, uint32_t s, uint32_t e,
                                          uint32_t seg, int P, uint8_t rl,
                                          const uint64_t refw[5], uint8_t pb)
{
    uint32_t w3 = (uint32_t)(uint8_t)(int8_t)P | ((uint32_t)rl << 8) |
                  ((uint32_t)(refw[0] & 0xFFFF) << 16);
    uint4 *r4 = (uint4 *)r;
    r4[0] = make_uint4(s, e, seg, w3);
    r4[1] = make_uint4((uint32_t)(refw[0] >> 16),
                       (uint32_t)((refw[0] >> 48) | (refw[1] << 16)),
                       (uint32_t)(refw[1] >> 16),
                       (uint32_t)((refw[1] >> 48) | (refw[2] << 16)));
    r4[2] = make_uint4((uint32_t)(refw[2] >> 16),
                       (uint32_t)((refw[2] >> 48) | (refw[3] << 16)),
                       (uint32_t)(refw[3] >> 16),
                       (uint32_t)((refw[3] >> 48) & 0xFFFF) |
                           ((uint32_t)(refw[4] & 0xFF) << 16) |
                           ((uint32_t)pb << 24));
}

// Deferred extension wraps (plain-root mode). A hashed branch at depth d
// under a parent junction P < d - 1 needs an extension node around it: a
// second keccak_f that few lanes of a wave need, but which every lane's
// issue slots pay for when it runs inside the branch kernels. With
// `may_defer` such a lane PARKS its node instead: the final record, except
// that the ref is still the branch's own, goes to recs[mt.s], and the lane
// takes a rank in the block's job count (*wrap_job; NO_WRAP_JOB = not
// parked). The kernel appends the slot to the level's job queue
// (wrap_queue_append) and k_branch_wrap finishes the node before the level
// ends. A parked lane leaves depths[mt.s] and the pending count of depth P
// alone, so no select can see a half-made node; of the keccak blocks it
// counts the branch's own, the wrap kernel adds the extension's.
// recs[mt.s] is free for this: it is the slot the finished record goes to,
// and no other group of the level reads it (below).
__device__ __forceinline__ void branch_tail(
    const br_meta &mt, int subtree, const uint8_t *keys, uint64_t key_stride,
    const uint64_t br_hash[4], const uint64_t *inline_src64,
    uint64_t inline_stride, uint8_t *ext, node_rec *recs, uint8_t *depths,
    uint64_t n, uint8_t *seg_roots, uint8_t *child_refs, uint8_t *child_lens,
    uint32_t *hist_l, uint8_t *bhash_by_s, sre_update_row *urows,
    uint32_t urowidx_val, const uint32_t *seg_by_slot, bool may_defer,
    uint32_t *wrap_job)
{
    int d = mt.d;
    int kblocks = mt.br_len / 136 + 1;
    // branch ref as an LE word stream (bytes beyond br_ref_len are never
    // consumed: the assemble appender masks them, record stores carry them
    // deterministically)
    uint64_t br_refw[5];
    uint8_t br_ref_len;
    if (mt.br_len < 32) { // inline: raw rlp words
        br_ref_len = (uint8_t)mt.br_len;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            br_refw[k] = inline_src64[(uint64_t)k * inline_stride];
        br_refw[4] = 0;
    } else {
        br_ref_len = 33;
        br_refw[0] = 0xa0ull | (br_hash[0] << 8);
        br_refw[1] = (br_hash[0] >> 56) | (br_hash[1] << 8);
        br_refw[2] = (br_hash[1] >> 56) | (br_hash[2] << 8);
        br_refw[3] = (br_hash[2] >> 56) | (br_hash[3] << 8);
        br_refw[4] = br_hash[3] >> 56;
    }
    const uint8_t *key0 = keys + (uint64_t)mt.s * key_stride;

    // extension wrap over key0[from..d): result in whash/wrefw/wrl
    uint64_t whash[4], wrefw[5];
    uint8_t wrl;
    auto wrap = [&](int from) {
        if (d == from) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                whash[k] = br_hash[k];
#pragma unroll
            for (int k = 0; k < 5; ++k)
                wrefw[k] = br_refw[k];
            wrl = br_ref_len;
            return;
        }
        ext_wrap(ext, key0, from, d, br_refw, br_ref_len, whash, wrefw, &wrl);
        kblocks += 1;
    };

    if (bhash_by_s) {
        memcpy(bhash_by_s + 32ull * mt.s, br_hash, 32);
        if (mt.d == 0 && urows && urowidx_val != 0xFFFFFFFFu) {
            // path-[] row: root branch carries its own hash
            sre_update_row *ur = &urows[urowidx_val];
            ur->root_hash_set = 1;
            memcpy(ur->root_hash, br_hash, 32);
        }
    }
    uint8_t upd_bits = (uint8_t)(((mt.flags & 1) << 4) |
                                 ((mt.br_len >= 32 ? 1 : 0) << 5));
    if (mt.P >= 0) {
        // child nibble at P: from the record's key word while it reaches
        // (P < 8), else one byte of the entry's key
        uint8_t pb = (uint8_t)((mt.P < 8 ? (mt.seg >> (28 - 4 * mt.P)) & 0xF
                                         : nib_of(key0, mt.P)) |
                               upd_bits);
        if (may_defer && d > mt.P + 1 && mt.br_len >= 32 && mt.s < n) {
            store_rec(&recs[mt.s], mt.s, mt.e, mt.seg, mt.P, br_ref_len, br_refw,
                      pb);
            *wrap_job = atomicAdd(&hist_l[BR_HIST_Q], 1u);
        } else {
            wrap(mt.P + 1);
            if (mt.s < n) {
                store_rec(&recs[mt.s], mt.s, mt.e, mt.seg, mt.P, wrl, wrefw, pb);
                depths[mt.s] = (uint8_t)(mt.P + 1);
            }
            atomicAdd(&hist_l[mt.P + 1], 1u);
        }
    } else {
        // storage pass: records carry no segment id; a root looks its own up
        // by its first entry (one load per segment root, off the group path).
        // Account pass: the shard (top nibble) in subtree mode, else 0
        const uint32_t seg = seg_by_slot ? seg_by_slot[mt.s]
                                         : (subtree ? mt.seg >> 28 : 0u);
        if (subtree) {
            wrap(1);
            uint8_t *cr = child_refs + 33ull * seg;
#pragma unroll
            for (int k = 0; k < 33; ++k)
                if (k < wrl)
                    cr[k] = (uint8_t)(wrefw[k >> 3] >> (8 * (k & 7)));
            child_lens[seg] = wrl;
        }
        wrap(0); // standalone form: only the hash matters
        memcpy(seg_roots + 32ull * seg, whash, 32);
    }
    atomicAdd(&hist_l[65], (uint32_t)kblocks);
}

// A level's deferred-wrap jobs: the slots of the parked nodes, in no
// particular order. jobs == nullptr: every wrap runs inline.
struct wrap_queue {
    uint32_t *jobs = nullptr;
    uint32_t *count = nullptr; // device word: jobs appended so far
    uint32_t cap = 0;
};

// Append the block's parked slots to the queue, one global atomic per block
// (as for pending[]). Called by every thread of the block, after the
// __syncthreads() that follows branch_tail.
__device__ __forceinline__ void wrap_queue_append(const wrap_queue &q,
                                                  uint32_t *hist_l,
                                                  uint32_t wrap_job,
                                                  uint32_t slot, uint32_t *err)
{
    if (!q.jobs || !hist_l[BR_HIST_Q]) // uniform over the block
        return;
    if (threadIdx.x == 0)
        hist_l[BR_HIST_Q + 1] = atomicAdd(q.count, hist_l[BR_HIST_Q]);
    __syncthreads();
    if (wrap_job == NO_WRAP_JOB)
        return;
    uint32_t pos = hist_l[BR_HIST_Q + 1] + wrap_job;
    if (pos < q.cap) // always: cap = the level's groups, one job per group
        q.jobs[pos] = slot;
    else
        atomicOr(err, 1u << E_INTERNAL);
}

// Hash one branch per lane: absorb the padded slot straight from global,
// then do extension/root wraps in a small LDS slot (88 B -> high occupancy).
__global__ void __launch_bounds__(BLOCK) k_branch_hash(
    const uint8_t *__restrict__ scratch, uint64_t scratch_stride,
    const br_meta *__restrict__ meta,
    uint32_t n_groups, const uint8_t *__restrict__ keys, uint64_t key_stride,
    int subtree, node_rec *__restrict__ recs, uint8_t *__restrict__ depths,
    uint64_t n, uint8_t *__restrict__ seg_roots,
    uint8_t *__restrict__ child_refs, uint8_t *__restrict__ child_lens,
    uint32_t *__restrict__ pending, uint32_t *__restrict__ err,
    uint8_t *__restrict__ bhash_by_s, /* updates mode: branch hash by
                                         interval start; null otherwise */
    sre_update_row *__restrict__ urows, /* updates mode: this level's rows */
    const uint32_t *__restrict__ urowidx,
    const uint32_t *__restrict__ seg_by_slot /* storage pass: segment id per
                                                entry; null = account pass */,
    wrap_queue wq)
{
    // pending[] updates are LDS-aggregated: one global atomic per counter
    // per block instead of per group (a single hot counter word saturates at
    // ~88 atomics/us chip-wide and was the dominant cost of this kernel).
    __shared__ __align__(16) uint8_t lds[BLOCK * SLOT_EXT + BR_HIST * 4];
    uint32_t *hist_l = (uint32_t *)(lds + BLOCK * SLOT_EXT);
    if (threadIdx.x < BR_HIST)
        hist_l[threadIdx.x] = 0;
    __syncthreads();
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    bool active = g < n_groups;
    uint32_t wrap_job = NO_WRAP_JOB;
    br_meta mt{};
    if (active) {
        mt = meta[g]; // meta/scratch by thread slot
        if (mt.br_len == 0) // error group: no node (err already flagged)
            active = false;
    }
    if (active) {
    int d = mt.d;
    const uint64_t *scr64 = (const uint64_t *)scratch; // column-major
    int nblocks = mt.br_len / 136 + 1;
    uint64_t br_hash[4];
    {
        uint64_t s[25];
#pragma unroll
        for (int i = 0; i < 25; ++i)
            s[i] = 0;
        for (int blk = 0; blk < nblocks; ++blk) {
#pragma unroll
            for (int i = 0; i < 17; ++i)
                s[i] ^= scr64[(uint64_t)(blk * 17 + i) * scratch_stride + g];
            keccak_f(s);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            br_hash[i] = s[i];
    }
    const uint64_t *inl = scr64 + g;
    const uint64_t inl_stride = scratch_stride;
    branch_tail(mt, subtree, keys, key_stride, br_hash, inl, inl_stride,
                lds + (uint64_t)threadIdx.x * SLOT_EXT, recs, depths, n,
                seg_roots, child_refs, child_lens, hist_l, bhash_by_s, urows,
                urowidx ? urowidx[g] : 0xFFFFFFFFu, seg_by_slot,
                wq.jobs != nullptr, &wrap_job);
    } // active
    __syncthreads();
    if (threadIdx.x < 66 && hist_l[threadIdx.x])
        atomicAdd(&pending[threadIdx.x], hist_l[threadIdx.x]);
    wrap_queue_append(wq, hist_l, wrap_job, mt.s, err);
}


// Fused assemble+hash for the 1-block branch class (nmem <= 3, the
// majority of groups at uniform keys): the branch RLP is built in a
// per-lane 136-B LDS slot and hashed in the same kernel — no global
// scratch round trip, no meta array, no second kernel pass. Runs on the
// main stream concurrently with the split pipeline's assemble (stream2)
// handling classes 1-3. Not used in updates/proof mode (those read meta/
// scratch across kernels).
#define SLOT_F1 136
__global__ void __launch_bounds__(BLOCK) k_branch_fused1(
    const uint32_t *__restrict__ idx, const uint32_t *__restrict__ gs,
    uint32_t n_groups /* class-0 groups of this chunk */,
    const int8_t *__restrict__ lcp, const uint8_t *__restrict__ keys,
    uint64_t key_stride, int d, int subtree, node_rec *__restrict__ recs,
    uint8_t *__restrict__ depths, uint64_t n,
    const uint32_t *__restrict__ perm /* class-0 slice */,
    uint8_t *__restrict__ seg_roots, uint8_t *__restrict__ child_refs,
    uint8_t *__restrict__ child_lens, uint32_t *__restrict__ pending,
    uint32_t *__restrict__ err,
    const uint32_t *__restrict__ seg_by_slot /* as in k_branch_hash */,
    wrap_queue wq)
{
    __shared__ __align__(16) uint8_t lds[BLOCK * SLOT_F1 + BR_HIST * 4];
    uint32_t *hist_l = (uint32_t *)(lds + BLOCK * SLOT_F1);
    if (threadIdx.x < BR_HIST)
        hist_l[threadIdx.x] = 0;
    __syncthreads();
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t wrap_job = NO_WRAP_JOB, wrap_slot = 0;
    if (g < n_groups) {
        uint32_t gg = perm[g];
        uint64_t j = gs[gg], jend = gs[gg + 1];
        int nmem = (int)(jend - j);
        bool sized_ok = nmem >= 2 && nmem <= 3;
        // validation words of all members issued up front (2 u32 each:
        // ref_len word + pad word). This both validates and WARMS the
        // records' cache lines, so the emit pass re-reads them from L1 —
        // caching the full 48-B records in registers measured as scratch
        // spills instead.
        // The members' slots come first, all at once (they are contiguous
        // in idx): the record loads hang on them, and mt.s is member 0's
        // slot itself, so word 0 of the records is never loaded.
        uint32_t im[3];
#pragma unroll
        for (int m = 0; m < 3; ++m)
            im[m] = idx[(sized_ok && m < nmem) ? j + m : j];
        uint32_t w3[3], w11[3], w1[3], w2[3];
#pragma unroll
        for (int m = 0; m < 3; ++m)
            if (sized_ok && m < nmem) {
                const uint32_t *r32 = (const uint32_t *)&recs[im[m]];
                w1[m] = r32[1];
                w2[m] = r32[2];
                w3[m] = r32[3];
                w11[m] = r32[11];
            }
        br_meta mt;
        mt.s = im[0];
        // select, not w1[nmem - 1]: a run-time index puts w1 in scratch.
        // An ill-sized group is an error group: its e/seg are never used.
        mt.e = sized_ok ? (nmem == 3 ? w1[2] : w1[1]) : mt.s;
        mt.seg = sized_ok ? w2[0] : 0;
        mt.d = (uint8_t)d;
        int8_t pl = lcp[mt.s], pr = lcp[mt.e];
        mt.P = pl > pr ? pl : pr;
        uint64_t nibs = 0;
        int payload = 1 + (16 - nmem);
        bool order_ok = sized_ok;
        bool stored = false;
        if (sized_ok) {
            int prev = -1;
#pragma unroll
            for (int m = 0; m < 3; ++m)
                if (m < nmem) {
                    uint8_t pb = (uint8_t)(w11[m] >> 24);
                    int nbm = pb & 0xF;
                    order_ok &= nbm > prev;
                    prev = nbm;
                    nibs |= (uint64_t)nbm << (4 * m);
                    payload += (w3[m] >> 8) & 0xFF;
                    stored |= (pb & 0x20) != 0;
                }
        }
        mt.flags = stored ? 1 : 0;
        if (!order_ok || payload > 116) { // error group: no node
            atomicOr(err, 1u << E_INTERNAL);
        } else {
            int h = rlp_list_hdr_len(payload);
            mt.br_len = (uint16_t)(h + payload);
            uint8_t *slot = lds + (uint64_t)threadIdx.x * SLOT_F1;
            uint64_t *slot64 = (uint64_t *)slot;
            byte_appender ap;
            ap.init(slot64, 0 /* direct row */, 0);
            if (payload < 56) {
                ap.put((uint8_t)(0xc0 + payload));
            } else {
                ap.put(0xf8);
                ap.put((uint8_t)payload);
            }
            {
                int prevnib = -1;
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    if (m < nmem) {
                        int nbm = (int)((nibs >> (4 * m)) & 0xF);
                        for (int b = prevnib + 1; b < nbm; ++b)
                            ap.put(0x80);
                        prevnib = nbm;
                        int rl = (w3[m] >> 8) & 0xFF;
                        const uint32_t *rec32 =
                            (const uint32_t *)&recs[im[m]]; // L1-hot re-read
                        uint32_t v[9];
#pragma unroll
                        for (int k = 0; k < 9; ++k)
                            v[k] = rec32[3 + k];
                        uint64_t R[5];
                        R[0] = ((uint64_t)v[0] >> 16) | ((uint64_t)v[1] << 16) |
                               ((uint64_t)v[2] << 48);
                        R[1] = ((uint64_t)v[2] >> 16) | ((uint64_t)v[3] << 16) |
                               ((uint64_t)v[4] << 48);
                        R[2] = ((uint64_t)v[4] >> 16) | ((uint64_t)v[5] << 16) |
                               ((uint64_t)v[6] << 48);
                        R[3] = ((uint64_t)v[6] >> 16) | ((uint64_t)v[7] << 16) |
                               ((uint64_t)v[8] << 48);
                        R[4] = ((uint64_t)v[8] >> 16) & 0xFF;
                        ap.put_bytes33(R, rl);
                    }
                for (int b = prevnib + 1; b < 16; ++b)
                    ap.put(0x80);
                ap.put(0x80); // empty value item
            }
            ap.finish(1); // keccak pad
            uint64_t s[25];
#pragma unroll
            for (int i = 0; i < 17; ++i)
                s[i] = slot64[i];
#pragma unroll
            for (int i = 17; i < 25; ++i)
                s[i] = 0;
            keccak_f(s);
            uint64_t br_hash[4] = {s[0], s[1], s[2], s[3]};
            // ext scratch aliases the message slot: branch_tail reads the
            // inline words before any wrap reuses it
            branch_tail(mt, subtree, keys, key_stride, br_hash, slot64, 1,
                        slot, recs, depths, n, seg_roots, child_refs,
                        child_lens, hist_l,
                        nullptr, nullptr, 0xFFFFFFFFu, seg_by_slot,
                        wq.jobs != nullptr, &wrap_job);
            wrap_slot = mt.s;
        }
    }
    __syncthreads();
    if (threadIdx.x < 66 && hist_l[threadIdx.x])
        atomicAdd(&pending[threadIdx.x], hist_l[threadIdx.x]);
    wrap_queue_append(wq, hist_l, wrap_job, wrap_slot, err);
}

// Finish the level's parked nodes (branch_tail), one job per lane: wrap the
// extension over key[P+1..d) around the branch ref the record holds, store
// the finished record, and only then make the node visible to the selects
// (depths[s], pending[P+1]). Grid-strides over the queue, whose length it
// reads on the device. Runs after every branch kernel of the level.
__global__ void __launch_bounds__(BLOCK) k_branch_wrap(
    wrap_queue wq, int d, const uint8_t *__restrict__ keys, uint64_t key_stride,
    node_rec *__restrict__ recs, uint8_t *__restrict__ depths, uint64_t n,
    uint32_t *__restrict__ pending, uint32_t *__restrict__ err)
{
    __shared__ __align__(16) uint8_t lds[BLOCK * SLOT_EXT + 66 * 4];
    uint32_t *hist_l = (uint32_t *)(lds + BLOCK * SLOT_EXT);
    if (threadIdx.x < 66)
        hist_l[threadIdx.x] = 0;
    __syncthreads();
    uint32_t cnt = *wq.count;
    if (cnt > wq.cap) // the appender has flagged it
        cnt = wq.cap;
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < cnt;
         j += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t s = wq.jobs[j];
        if (s >= n) {
            atomicOr(err, 1u << E_INTERNAL);
            continue;
        }
        const uint4 *r4 = (const uint4 *)&recs[s];
        const uint4 a = r4[0], b = r4[1], c = r4[2];
        const int P = (int)(int8_t)(a.w & 0xFF);
        const uint8_t rl = (uint8_t)(a.w >> 8);
        if (P < 0 || P + 1 >= d || rl != 33 || a.x != s) { // not a parked node
            atomicOr(err, 1u << E_INTERNAL);
            continue;
        }
        // ref byte i lives at record byte 14+i: back to the LE word stream
        uint64_t refw[5];
        refw[0] = ((uint64_t)a.w >> 16) | ((uint64_t)b.x << 16) |
                  ((uint64_t)b.y << 48);
        refw[1] = ((uint64_t)b.y >> 16) | ((uint64_t)b.z << 16) |
                  ((uint64_t)b.w << 48);
        refw[2] = ((uint64_t)b.w >> 16) | ((uint64_t)c.x << 16) |
                  ((uint64_t)c.y << 48);
        refw[3] = ((uint64_t)c.y >> 16) | ((uint64_t)c.z << 16) |
                  ((uint64_t)c.w << 48);
        refw[4] = ((uint64_t)c.w >> 16) & 0xFF;
        uint64_t whash[4], wrefw[5];
        uint8_t wrl;
        ext_wrap(lds + (uint64_t)threadIdx.x * SLOT_EXT,
                 keys + (uint64_t)s * key_stride, P + 1, d, refw, rl, whash,
                 wrefw, &wrl);
        store_rec(&recs[s], a.x, a.y, a.z, P, wrl, wrefw, (uint8_t)(c.w >> 24));
        depths[s] = (uint8_t)(P + 1);
        atomicAdd(&hist_l[P + 1], 1u);
        atomicAdd(&hist_l[65], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 66 && hist_l[threadIdx.x])
        atomicAdd(&pending[threadIdx.x], hist_l[threadIdx.x]);
}

// TrieUpdates emission (updates mode): one row per STORED branch
// (hash_mask != 0 — semantics in sre.h, pinned by the reference tests).
// Runs per level chunk after k_branch_hash; row slots via LDS-aggregated
// atomic bump. kind: 0 account trie, 1 storage trie (acct_key patched on
// host from the stashed seg id).
__global__ void __launch_bounds__(BLOCK) k_emit_updates(
    const node_rec *__restrict__ recs, const uint32_t *__restrict__ idx,
    const uint32_t *__restrict__ gs,
    uint32_t n_groups, const br_meta *__restrict__ meta,
    const uint8_t *__restrict__ keys, uint64_t key_stride,
    const uint8_t *__restrict__ bhash_by_s, int kind,
    sre_update_row *__restrict__ rows, uint32_t *__restrict__ row_counter,
    const uint32_t *__restrict__ perm,
    uint32_t *__restrict__ rowidx /* per thread slot: row slot or ~0 */,
    const uint32_t *__restrict__ seg_by_slot /* storage pass: segment id per
                                                entry; null = account pass */)
{
    __shared__ uint32_t lds[BLOCK];
    __shared__ uint32_t base;
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    bool stored = g < n_groups && meta[g].br_len != 0 && (meta[g].flags & 1);
    uint32_t excl, total;
    block_scan(lds, stored ? 1u : 0u, &excl, &total);
    if (threadIdx.x == 0)
        base = total ? atomicAdd(row_counter, total) : 0;
    __syncthreads();
    if (g < n_groups)
        rowidx[g] = stored ? base + excl : 0xFFFFFFFFu;
    if (!stored)
        return;
    br_meta mt = meta[g];
    sre_update_row *row = &rows[base + excl];
    uint32_t gg = perm ? perm[g] : g;
    uint64_t j = gs[gg], jend = gs[gg + 1];
    uint16_t state = 0, tree = 0, hashm = 0;
    int nh = 0;
    for (uint64_t m = j; m < jend; ++m) {
        const uint32_t ms = idx[m]; // the member's slot, and its s
        uint8_t pb = recs[ms].pad_;
        int b = pb & 0xF;
        state |= (uint16_t)(1u << b);
        if (pb & 0x20) { // child subtree top is a hashed branch
            hashm |= (uint16_t)(1u << b);
            memcpy(row->hashes[nh++], bhash_by_s + 32ull * ms, 32);
        }
        if (pb & 0x10) // child branch is itself stored
            tree |= (uint16_t)(1u << b);
    }
    for (int k = nh; k < 16; ++k)
        for (int q = 0; q < 32; ++q)
            row->hashes[k][q] = 0;
    row->state_mask = state;
    row->tree_mask = tree;
    row->hash_mask = hashm;
    row->num_hashes = (uint8_t)nh;
    row->kind = (uint8_t)kind;
    int d = mt.d;
    row->path_len = (uint8_t)d;
    const uint8_t *key0 = keys + (uint64_t)mt.s * key_stride;
    for (int k = 0; k < 32; ++k) {
        uint8_t hi = (2 * k < d) ? nib_of(key0, 2 * k) : 0;
        uint8_t lo = (2 * k + 1 < d) ? nib_of(key0, 2 * k + 1) : 0;
        row->path[k] = (uint8_t)((hi << 4) | lo);
    }
    // root_hash (d == 0 rows) is patched by k_branch_hash afterwards: this
    // kernel runs BEFORE the level's hashing so the children's bhash_by_s
    // entries are not yet overwritten by ancestors sharing the same
    // leftmost interval start.
    row->root_hash_set = 0;
    for (int q = 0; q < 32; ++q)
        row->root_hash[q] = 0;
    // stash seg for the host-side acct_key patch; zero the rest
    for (int q = 0; q < 32; ++q)
        row->acct_key[q] = 0;
    const uint32_t seg = seg_by_slot ? seg_by_slot[mt.s] : 0u;
    memcpy(row->pad_, &seg, 4);
    row->pad_[4] = 0;
    row->removed = 0;
}

// ---------------------------------------------------------------------------
// overlay-delta merge (sre_apply_delta): post-state wins, zero deletes,
// deleted accounts wipe storage (post_state.rs:89,313,355 semantics)
// ---------------------------------------------------------------------------

__device__ __forceinline__ int cmp_key32(const uint8_t *a, const uint8_t *b)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint64_t wa = be64_at(a + 8 * k), wb = be64_at(b + 8 * k);
        if (wa != wb)
            return wa < wb ? -1 : 1;
    }
    return 0;
}

__device__ __forceinline__ int cmp_key64(const uint8_t *a, const uint8_t *b)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint64_t wa = be64_at(a + 8 * k), wb = be64_at(b + 8 * k);
        if (wa != wb)
            return wa < wb ? -1 : 1;
    }
    return 0;
}

// lower_bound over keys at `stride`, comparing `klen` (32 or 64) bytes
__device__ __forceinline__ uint64_t lb_keys(const uint8_t *base, uint64_t stride,
                                            uint64_t n, const uint8_t *key,
                                            int klen)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        uint64_t mid = (lo + hi) / 2;
        int c = klen == 32 ? cmp_key32(base + mid * stride, key)
                           : cmp_key64(base + mid * stride, key);
        if (c < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// ---- account multiproof capture (sre_account_proof; proof/mod.rs:59-137
// semantics). A path node for target index ti is exactly the branch group
// whose member interval contains ti, so per level chunk one thread per
// target binary-searches the groups and, on containment, copies the
// assembled branch RLP out of the scratch slot before it is reused, into a
// proof_row (proof_host.h).

// target key -> index in the sorted account array (+ presence flag)
__global__ void k_proof_ti(const sre_account_entry *__restrict__ acct,
                           uint64_t na, const uint8_t *__restrict__ targets,
                           uint32_t n_t, uint32_t *__restrict__ ti,
                           uint32_t *__restrict__ present)
{
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_t)
        return;
    const uint8_t *key = targets + 32ull * t;
    uint64_t lo = 0, hi = na;
    while (lo < hi) {
        uint64_t mid = (lo + hi) / 2;
        if (cmp_key32(acct[mid].key, key) < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    ti[t] = (uint32_t)lo;
    present[t] = (lo < na && cmp_key32(acct[lo].key, key) == 0) ? 1u : 0u;
}

// (acct_key, slot_key) -> index in the sorted storage array (+ presence)
__global__ void k_proof_ti64(const sre_storage_entry *__restrict__ st,
                             uint64_t ns, const uint8_t *__restrict__ targets,
                             uint32_t n_t, uint32_t *__restrict__ ti,
                             uint32_t *__restrict__ present)
{
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_t)
        return;
    const uint8_t *key = targets + 64ull * t;
    uint64_t lo = 0, hi = ns;
    while (lo < hi) {
        uint64_t mid = (lo + hi) / 2;
        if (cmp_key64((const uint8_t *)&st[mid], key) < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    ti[t] = (uint32_t)lo;
    present[t] = (lo < ns && cmp_key64((const uint8_t *)&st[lo], key) == 0)
                     ? 1u
                     : 0u;
}

__device__ __forceinline__ void proof_grab_one(
    const br_meta *meta,
    const uint8_t *scratch, uint64_t scratch_stride, const uint32_t *inv,
    const uint8_t *keys, uint64_t key_stride, uint32_t t, uint32_t g,
    proof_row *rows, uint32_t *cnt, uint32_t cap, uint32_t *err)
{
    uint32_t slot = inv ? inv[g] : g;
    br_meta mt = meta[slot];
    if (mt.br_len == 0)
        return;
    uint32_t r = atomicAdd(cnt, 1u);
    if (r >= cap) {
        atomicOr(err, 1u << E_INTERNAL);
        return;
    }
    rows[r].target = t;
    rows[r].d = (int16_t)mt.d;
    rows[r].P = (int16_t)mt.P;
    rows[r].br_len = mt.br_len;
    rows[r].s = mt.s;
    rows[r].e = mt.e;
    const uint8_t *k0 = keys + (uint64_t)mt.s * key_stride;
    for (int k = 0; k < 32; ++k)
        rows[r].key0[k] = k0[k];
    const uint64_t *scr64 = (const uint64_t *)scratch;
    uint64_t *dst = (uint64_t *)rows[r].rlp;
    int nw = (mt.br_len + 7) / 8;
    for (int w = 0; w < nw; ++w)
        dst[w] = scr64[(uint64_t)w * scratch_stride + slot];
}

// find the chunk-local group covering leaf index pos, or ~0u
__device__ __forceinline__ uint32_t proof_find_group(const node_rec *recs,
                                                     const uint32_t *idx,
                                                     const uint32_t *gs,
                                                     uint32_t n_groups,
                                                     uint32_t pos)
{
    uint32_t lo = 0, hi = n_groups;
    while (lo < hi) {
        uint32_t mid = (lo + hi) / 2;
        if (idx[gs[mid]] <= pos) // first member's slot = the group's s
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo == 0)
        return ~0u;
    uint32_t g = lo - 1;
    if (pos >= recs[idx[gs[g + 1] - 1]].e)
        return ~0u;
    return g;
}

__global__ void k_proof_grab(const node_rec *__restrict__ recs,
                             const uint32_t *__restrict__ idx,
                             const uint32_t *__restrict__ gs, uint32_t n_groups,
                             const br_meta *__restrict__ meta,
                             const uint8_t *__restrict__ scratch,
                             uint64_t scratch_stride,
                             const uint32_t *__restrict__ inv,
                             const uint8_t *__restrict__ keys,
                             uint64_t key_stride,
                             const uint32_t *__restrict__ ti,
                             const uint32_t *__restrict__ ti2, uint32_t n_t,
                             proof_row *__restrict__ rows,
                             uint32_t *__restrict__ cnt, uint32_t cap,
                             uint32_t *__restrict__ err)
{
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_t)
        return;
    uint32_t g1 = proof_find_group(recs, idx, gs, n_groups, ti[t]);
    uint32_t g2 = ti2 ? proof_find_group(recs, idx, gs, n_groups, ti2[t]) : g1;
    if (g1 != ~0u)
        proof_grab_one(meta, scratch, scratch_stride, inv, keys,
                       key_stride, t, g1, rows, cnt, cap, err);
    if (g2 != ~0u && g2 != g1)
        proof_grab_one(meta, scratch, scratch_stride, inv, keys,
                       key_stride, t, g2, rows, cnt, cap, err);
}

// old->new position map for interval rebasing: map[i] = the new index of
// base entry i (or of its successor when i was dropped); map[nb] = new_na.
__global__ void k_ovl_posmap(const sre_account_entry *__restrict__ base,
                             uint64_t nb, const uint32_t *__restrict__ bexcl,
                             const sre_account_delta *__restrict__ dl,
                             uint64_t nd, const uint32_t *__restrict__ dexcl,
                             uint32_t *__restrict__ map)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nb)
        return;
    if (i == nb) {
        map[i] = bexcl[nb] + dexcl[nd];
        return;
    }
    uint64_t p = lb_keys((const uint8_t *)dl, sizeof(sre_account_delta), nd,
                         base[i].key, 32);
    map[i] = bexcl[i] + dexcl[p];
}

// carry surviving accounts' retained storage roots into the merged
// positions (accounts replaced by a non-deleting delta row KEEP their
// storage — hashed_state.rs:425-440 wipes only on destruction)
__global__ void k_ovl_carry_roots(const sre_account_entry *__restrict__ base,
                                  uint64_t nb,
                                  const uint32_t *__restrict__ bexcl,
                                  const sre_account_delta *__restrict__ dl,
                                  uint64_t nd,
                                  const uint32_t *__restrict__ dexcl,
                                  const uint8_t *__restrict__ old_roots,
                                  uint8_t *__restrict__ new_roots)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb)
        return;
    uint64_t p = lb_keys((const uint8_t *)dl, sizeof(sre_account_delta), nd,
                         base[i].key, 32);
    if (p < nd && cmp_key32(dl[p].key, base[i].key) == 0 && dl[p].deleted)
        return; // destroyed: no root to carry
    uint64_t j = bexcl[i] + dexcl[p]; // new index (posmap formula)
    const uint64_t *s = (const uint64_t *)(old_roots + 32 * i);
    uint64_t *d = (uint64_t *)(new_roots + 32 * j);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        d[k] = s[k];
}


// per touched account: segment bounds in the merged storage array, the
// account's index in the merged account array, and an EMPTY_ROOT reset
// (recomputed segments are scattered over it afterwards)
__global__ void k_touched_bounds(const sre_storage_entry *__restrict__ st,
                                 uint64_t ns,
                                 const sre_account_entry *__restrict__ acct,
                                 uint64_t na,
                                 const uint8_t *__restrict__ tkeys, uint32_t nt,
                                 uint32_t *__restrict__ lo,
                                 uint32_t *__restrict__ hi,
                                 uint32_t *__restrict__ aidx,
                                 uint8_t *__restrict__ roots,
                                 uint32_t *__restrict__ err)
{
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt)
        return;
    const uint8_t *key = tkeys + 32ull * t;
    // storage range [lo, hi) of this account
    uint64_t l = 0, h = ns;
    while (l < h) {
        uint64_t m = (l + h) / 2;
        if (cmp_key32(st[m].acct_key, key) < 0)
            l = m + 1;
        else
            h = m;
    }
    lo[t] = (uint32_t)l;
    h = ns;
    uint64_t l2 = l;
    while (l2 < h) {
        uint64_t m = (l2 + h) / 2;
        if (cmp_key32(st[m].acct_key, key) <= 0)
            l2 = m + 1;
        else
            h = m;
    }
    hi[t] = (uint32_t)l2;
    uint64_t p = lb_keys((const uint8_t *)acct, sizeof(sre_account_entry), na,
                         key, 32);
    if (p >= na || cmp_key32(acct[p].key, key) != 0) {
        if (lo[t] != hi[t])
            atomicOr(err, 1u << E_INTERNAL); // slots for an absent account
        aidx[t] = 0xFFFFFFFFu;
        return;
    }
    aidx[t] = (uint32_t)p;
    for (int k = 0; k < 32; ++k)
        roots[32ull * p + k] = D_EMPTY_ROOT[k];
}

// gather the touched accounts' storage entries into a compact array
__global__ void k_gather_touched(const sre_storage_entry *__restrict__ st,
                                 const uint32_t *__restrict__ lo,
                                 const uint32_t *__restrict__ hi,
                                 const uint32_t *__restrict__ offs, uint32_t nt,
                                 uint64_t total,
                                 sre_storage_entry *__restrict__ out)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total)
        return;
    // locate the touched account owning compact position j
    uint32_t l = 0, h = nt;
    while (l < h) {
        uint32_t m = (l + h) / 2;
        if ((uint64_t)offs[m + 1] <= j)
            l = m + 1;
        else
            h = m;
    }
    const uint8_t *s = (const uint8_t *)&st[lo[l] + (j - offs[l])];
    uint8_t *d = (uint8_t *)&out[j];
    for (int k = 0; k < (int)sizeof(sre_storage_entry); k += 8)
        *(uint64_t *)(d + k) = *(const uint64_t *)(s + k);
}

// base account survives iff its key is absent from the delta
__global__ void k_ovl_base_acct_flags(const sre_account_entry *__restrict__ base,
                                      uint64_t nb,
                                      const sre_account_delta *__restrict__ dl,
                                      uint64_t nd, uint32_t *__restrict__ flags)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nb)
        return;
    if (i == nb) { // scan sentinel
        flags[i] = 0;
        return;
    }
    uint64_t p = lb_keys((const uint8_t *)dl, sizeof(sre_account_delta), nd,
                         base[i].key, 32);
    flags[i] = (p < nd && cmp_key32(dl[p].key, base[i].key) == 0) ? 0u : 1u;
}

// delta account row materializes iff not deleted (+ order validation)
__global__ void k_ovl_delta_acct_flags(const sre_account_delta *__restrict__ dl,
                                       uint64_t nd, uint32_t *__restrict__ flags,
                                       uint32_t *__restrict__ del_flags,
                                       uint32_t *__restrict__ err)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nd)
        return;
    if (j == nd) {
        flags[j] = 0;
        del_flags[j] = 0;
        return;
    }
    if (j > 0 && cmp_key32(dl[j - 1].key, dl[j].key) >= 0)
        atomicOr(err, 1u << E_UNSORTED_ACCT);
    flags[j] = dl[j].deleted ? 0u : 1u;
    del_flags[j] = dl[j].deleted ? 1u : 0u;
}

__global__ void k_ovl_scatter_acct(const sre_account_entry *__restrict__ base,
                                   uint64_t nb, const uint32_t *__restrict__ bexcl,
                                   const sre_account_delta *__restrict__ dl,
                                   uint64_t nd, const uint32_t *__restrict__ dexcl,
                                   sre_account_entry *__restrict__ out)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb && bexcl[i] != bexcl[i + 1]) { // base survivor
        uint64_t p = lb_keys((const uint8_t *)dl, sizeof(sre_account_delta), nd,
                             base[i].key, 32);
        out[bexcl[i] + dexcl[p]] = base[i];
    }
    uint64_t j = i; // reuse the same grid for the (smaller) delta side
    if (j < nd && dexcl[j] != dexcl[j + 1]) {
        uint64_t p = lb_keys((const uint8_t *)base, sizeof(sre_account_entry), nb,
                             dl[j].key, 32);
        sre_account_entry e;
        memcpy(e.key, dl[j].key, 32);
        e.nonce = dl[j].nonce;
        memcpy(e.balance, dl[j].balance, 32);
        memcpy(e.code_hash, dl[j].code_hash, 32);
        out[dexcl[j] + bexcl[p]] = e;
    }
}

// gather the keys of deleted accounts (sorted subset of the sorted delta)
__global__ void k_ovl_gather_deleted(const sre_account_delta *__restrict__ dl,
                                     uint64_t nd,
                                     const uint32_t *__restrict__ delexcl,
                                     uint8_t *__restrict__ out_keys)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nd || delexcl[j] == delexcl[j + 1])
        return;
    memcpy(out_keys + 32ull * delexcl[j], dl[j].key, 32);
}

// base storage survives iff acct not deleted and (acct,slot) not in delta
__global__ void k_ovl_base_st_flags(const sre_storage_entry *__restrict__ base,
                                    uint64_t nb,
                                    const sre_storage_entry *__restrict__ dl,
                                    uint64_t nd,
                                    const uint8_t *__restrict__ del_keys,
                                    uint64_t ndel, uint32_t *__restrict__ flags)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nb)
        return;
    if (i == nb) {
        flags[i] = 0;
        return;
    }
    uint64_t q = lb_keys(del_keys, 32, ndel, base[i].acct_key, 32);
    if (q < ndel && cmp_key32(del_keys + 32 * q, base[i].acct_key) == 0) {
        flags[i] = 0; // wiped with its account
        return;
    }
    uint64_t p = lb_keys((const uint8_t *)dl, sizeof(sre_storage_entry), nd,
                         base[i].acct_key, 64);
    flags[i] = (p < nd && cmp_key64(dl[p].acct_key, base[i].acct_key) == 0)
                   ? 0u
                   : 1u;
}

// A nonzero delta storage row needs an owner after the merge: an upsert of
// the same delta or a base account. (A base account the delta deletes is
// flagged through del_keys by the callers; a zero value for an unknown
// account is a no-op deletion.) Both account arrays are sorted — the
// account delta's order is validated before any storage work starts.
__device__ __forceinline__ bool
st_row_orphan(const sre_storage_entry *__restrict__ row,
              const sre_account_entry *__restrict__ acct, uint64_t na,
              const sre_account_delta *__restrict__ dl_a, uint64_t n_acct)
{
    if (!min_be_len(row->value))
        return false;
    uint64_t q = lb_keys((const uint8_t *)dl_a, sizeof(sre_account_delta),
                         n_acct, row->acct_key, 32);
    if (q < n_acct && cmp_key32(dl_a[q].key, row->acct_key) == 0)
        return dl_a[q].deleted != 0;
    uint64_t p = lb_keys((const uint8_t *)acct, sizeof(sre_account_entry), na,
                         row->acct_key, 32);
    return !(p < na && cmp_key32(acct[p].key, row->acct_key) == 0);
}

// delta storage row materializes iff value != 0; a row for a deleted
// account, or a nonzero row for an account that is neither resident nor
// upserted, is an input error (+ order validation)
__global__ void k_ovl_delta_st_flags(const sre_storage_entry *__restrict__ dl,
                                     uint64_t nd,
                                     const uint8_t *__restrict__ del_keys,
                                     uint64_t ndel,
                                     const sre_account_entry *__restrict__ acct,
                                     uint64_t na,
                                     const sre_account_delta *__restrict__ dl_a,
                                     uint64_t n_acct,
                                     uint32_t *__restrict__ flags,
                                     uint32_t *__restrict__ err)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nd)
        return;
    if (j == nd) {
        flags[j] = 0;
        return;
    }
    if (j > 0 && cmp_key64(dl[j - 1].acct_key, dl[j].acct_key) >= 0)
        atomicOr(err, 1u << E_UNSORTED_STORAGE);
    uint64_t q = lb_keys(del_keys, 32, ndel, dl[j].acct_key, 32);
    if ((q < ndel && cmp_key32(del_keys + 32 * q, dl[j].acct_key) == 0) ||
        st_row_orphan(&dl[j], acct, na, dl_a, n_acct))
        atomicOr(err, 1u << E_ORPHAN_STORAGE);
    flags[j] = min_be_len(dl[j].value) ? 1u : 0u; // zero value = delete
}

__global__ void k_ovl_scatter_st(const sre_storage_entry *__restrict__ base,
                                 uint64_t nb, const uint32_t *__restrict__ bexcl,
                                 const sre_storage_entry *__restrict__ dl,
                                 uint64_t nd, const uint32_t *__restrict__ dexcl,
                                 sre_storage_entry *__restrict__ out)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb && bexcl[i] != bexcl[i + 1]) {
        uint64_t p = lb_keys((const uint8_t *)dl, sizeof(sre_storage_entry), nd,
                             base[i].acct_key, 64);
        out[bexcl[i] + dexcl[p]] = base[i];
    }
    uint64_t j = i;
    if (j < nd && dexcl[j] != dexcl[j + 1]) {
        uint64_t p = lb_keys((const uint8_t *)base, sizeof(sre_storage_entry), nb,
                             dl[j].acct_key, 64);
        out[dexcl[j] + bexcl[p]] = dl[j];
    }
}

// ---------------------------------------------------------------------------
// small-delta account merge (dirty-path incremental, accounts-only):
// ONE pass over the base replaces the flags + two scans + scatter + posmap
// passes of the general overlay merge. All delta-side rank arrays are tiny
// (L2-resident); per base row the ranks are closed-form:
//   p      = lower_bound(delta, base[i].key)
//   map[i] = i - m_excl[p] + eff_excl[p]
// where m_excl counts MATCHED delta rows (they drop/replace the base row)
// and eff_excl counts EFFECTIVE (non-deleted) delta rows (they produce an
// output entry). Identical to the general bexcl/dexcl formula.
// ---------------------------------------------------------------------------

__global__ void k_sd_marks(const sre_account_entry *__restrict__ base,
                           uint64_t nb,
                           const sre_account_delta *__restrict__ dl,
                           uint64_t nd, uint32_t *__restrict__ bpos,
                           uint32_t *__restrict__ match)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nd)
        return;
    uint64_t p = lb_keys((const uint8_t *)base, sizeof(sre_account_entry), nb,
                         dl[k].key, 32);
    bpos[k] = (uint32_t)p;
    match[k] = (p < nb && cmp_key32(base[p].key, dl[k].key) == 0) ? 1u : 0u;
}

// merge scatter: survivors copied to their new position; map written for
// EVERY old index (+ sentinel at nb)
__global__ void k_sd_scatter(const sre_account_entry *__restrict__ base,
                             uint64_t nb,
                             const sre_account_delta *__restrict__ dl,
                             uint64_t nd,
                             const uint32_t *__restrict__ m_excl, /* nd+1 */
                             const uint32_t *__restrict__ eff_excl, /* nd+1 */
                             sre_account_entry *__restrict__ out,
                             uint32_t *__restrict__ map)
{
    // the delta rank p is monotone in the base key, so the whole block
    // shares a tiny search window computed once from its first/last row
    // (usually width 0-2: 5k delta positions spread over 200M rows) —
    // the full log2(nd) probe loop per row was half the scatter's cost
    __shared__ uint32_t plo_s, phi_s;
    uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x;
    if (threadIdx.x == 0) {
        uint64_t a = i0 < nb ? i0 : (nb ? nb - 1 : 0);
        plo_s = nb ? (uint32_t)lb_keys((const uint8_t *)dl,
                                       sizeof(sre_account_delta), nd,
                                       base[a].key, 32)
                   : 0;
        uint64_t b = i0 + blockDim.x - 1;
        if (b >= nb)
            b = nb ? nb - 1 : 0;
        phi_s = nb ? (uint32_t)lb_keys((const uint8_t *)dl,
                                       sizeof(sre_account_delta), nd,
                                       base[b].key, 32)
                   : 0;
    }
    __syncthreads();
    uint64_t i = i0 + threadIdx.x;
    // fast path: a full block whose span contains no delta key shifts by
    // a constant — copy flat u64s, fully coalesced on both sides (at a
    // 5k delta over 200M rows this is ~99.99% of blocks)
    if (plo_s == phi_s && i0 + blockDim.x <= nb) {
        uint32_t p = plo_s;
        bool lastmatch =
            p < nd &&
            cmp_key32(dl[p].key, base[i0 + blockDim.x - 1].key) == 0;
        if (!lastmatch) {
            uint64_t j0 = merged_pos(i0, m_excl[p], eff_excl[p]);
            const uint64_t *s8 = (const uint64_t *)&base[i0];
            uint64_t *d8 = (uint64_t *)&out[j0];
            // static trip count: issue all 13 loads before any store
            uint64_t v[13];
#pragma unroll
            for (int w = 0; w < 13; ++w)
                v[w] = s8[threadIdx.x + (uint32_t)w * BLOCK];
#pragma unroll
            for (int w = 0; w < 13; ++w)
                d8[threadIdx.x + (uint32_t)w * BLOCK] = v[w];
            map[i] = (uint32_t)merged_pos(i, m_excl[p], eff_excl[p]);
            return;
        }
    }
    if (i > nb)
        return;
    if (i == nb) {
        map[nb] = (uint32_t)merged_pos(nb, m_excl[nd], eff_excl[nd]);
        return;
    }
    uint64_t lo = plo_s, hi = phi_s;
    // lb within [lo, hi+1): first delta key >= base key
    uint64_t hh = hi < nd ? hi + 1 : nd;
    while (lo < hh) {
        uint64_t mid = (lo + hh) / 2;
        if (cmp_key32(dl[mid].key, base[i].key) < 0)
            lo = mid + 1;
        else
            hh = mid;
    }
    uint64_t p = lo;
    bool m = p < nd && cmp_key32(dl[p].key, base[i].key) == 0;
    uint32_t j = (uint32_t)merged_pos(i, m_excl[p], eff_excl[p]);
    map[i] = j;
    if (!m) {
        // 13 u64 copies (entries are 8-B aligned at the 104-B stride)
        const uint64_t *s8 = (const uint64_t *)&base[i];
        uint64_t *d8 = (uint64_t *)&out[j];
#pragma unroll
        for (int w = 0; w < 13; ++w)
            d8[w] = s8[w];
    }
}

// place effective delta rows; newpos[k] = output position of delta row k
// (for deleted rows: the junction position — the slot where its successor
// now sits — recorded for the lcp boundary patch)
__global__ void k_sd_place(const sre_account_delta *__restrict__ dl,
                           uint64_t nd,
                           const uint32_t *__restrict__ bpos,
                           const uint32_t *__restrict__ m_excl,
                           const uint32_t *__restrict__ eff_excl,
                           sre_account_entry *__restrict__ out,
                           uint32_t *__restrict__ newpos)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nd)
        return;
    uint32_t j = (uint32_t)merged_pos(bpos[k], m_excl[k], eff_excl[k]);
    newpos[k] = j;
    if (!dl[k].deleted) {
        sre_account_entry e;
        memcpy(e.key, dl[k].key, 32);
        e.nonce = dl[k].nonce;
        memcpy(e.balance, dl[k].balance, 32);
        memcpy(e.code_hash, dl[k].code_hash, 32);
        out[j] = e;
    }
}

// lcp repair: an adjacent old pair (i-1, i) that stays adjacent in the
// merge keeps its lcp (keys of matched rows are unchanged — a modify
// replaces the value, not the key). Every other new-pair lcp is a delta
// boundary and is recomputed exactly by k_sd_lcp_patch.
__global__ void k_sd_lcp_copy(const uint32_t *__restrict__ map, uint64_t nb,
                              const int8_t *__restrict__ lcp_old,
                              int8_t *__restrict__ lcp_new)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 1 || i >= nb)
        return;
    uint32_t j = map[i];
    if (j == map[i - 1] + 1)
        lcp_new[j] = lcp_old[i];
}

__global__ void k_sd_lcp_patch(const sre_account_entry *__restrict__ out,
                               uint64_t new_nb,
                               const uint32_t *__restrict__ patch, uint64_t np,
                               int8_t *__restrict__ lcp_new,
                               uint32_t *__restrict__ err)
{
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= np)
        return;
    uint32_t j = patch[t];
    if (j > new_nb)
        return;
    if (j == 0 || j == new_nb) {
        lcp_new[j] = -1;
        return;
    }
    bool gt;
    int l = key_lcp(out[j - 1].key, out[j].key, &gt);
    if (gt || l == 64)
        atomicOr(err, 1u << E_UNSORTED_ACCT);
    lcp_new[j] = (int8_t)l;
}

// ---- closed-form STORAGE merge for small deltas (dirty-path): the same
// rank trick as the account side plus destroyed-account WIPE RANGES —
// each destroyed account's base rows form one contiguous (acct-key
// prefixed) range; removed-rows-before-i is then a prefix sum over at
// most a few thousand ranges, all L1/L2-resident. Replaces the O(ns)
// flags + scans + posmap of the general storage merge; what remains is
// the irreducible array rewrite.

__global__ void k_sds_marks(const sre_storage_entry *__restrict__ base,
                            uint64_t ns,
                            const sre_storage_entry *__restrict__ dl,
                            uint64_t nst,
                            const sre_account_entry *__restrict__ acct,
                            uint64_t na,
                            const sre_account_delta *__restrict__ dl_a,
                            uint64_t n_acct, uint32_t *__restrict__ bpos,
                            uint32_t *__restrict__ match)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nst)
        return;
    uint64_t p = lb_keys((const uint8_t *)base, sizeof(sre_storage_entry), ns,
                         (const uint8_t *)&dl[k], 64);
    bpos[k] = (uint32_t)p;
    uint32_t m = (p < ns && cmp_key64((const uint8_t *)&base[p],
                                      (const uint8_t *)&dl[k]) == 0)
                     ? SDS_MATCH
                     : 0u;
    // the host reads match[] back anyway: the owner check rides along
    // instead of costing a kernel and a copy of its own
    if (st_row_orphan(&dl[k], acct, na, dl_a, n_acct))
        m |= SDS_ORPHAN;
    match[k] = m;
}

// wipe range of each destroyed account: [first row with this acct_key,
// first row past it)
__global__ void k_sds_wipes(const sre_storage_entry *__restrict__ base,
                            uint64_t ns, const uint8_t *__restrict__ sdel,
                            uint32_t ndel, uint32_t *__restrict__ wlo,
                            uint32_t *__restrict__ whi)
{
    uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= ndel)
        return;
    const uint8_t *key = sdel + 32ull * a;
    uint64_t lo = 0, hi = ns;
    while (lo < hi) { // first i with acct_key >= key
        uint64_t mid = (lo + hi) / 2;
        if (cmp_key32(base[mid].acct_key, key) < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    wlo[a] = (uint32_t)lo;
    uint64_t lo2 = lo;
    hi = ns;
    while (lo2 < hi) { // first i with acct_key > key
        uint64_t mid = (lo2 + hi) / 2;
        if (cmp_key32(base[mid].acct_key, key) <= 0)
            lo2 = mid + 1;
        else
            hi = mid;
    }
    whi[a] = (uint32_t)lo2;
}

// ---- revert capture (sre_set_revert_capture) --------------
// One pass over the DELTA rows, before any merge and whichever merge runs
// afterwards: what every delta row overwrites or removes is read out of the
// resident arrays into a delta that undoes it. Row decisions and output
// positions: revert_plan.h. Runs on unvalidated storage rows (the merges
// validate), so every index below is bounded for any input; the account
// delta's order is checked by the host before the pass starts.

__constant__ uint8_t D_KECCAK_EMPTY[32] = {
    0xc5, 0xd2, 0x46, 0x01, 0x86, 0xf7, 0x23, 0x3c, 0x92, 0x7e, 0x7d, 0xb2,
    0xdc, 0xc7, 0x03, 0xc0, 0xe5, 0x00, 0xb6, 0x53, 0xca, 0x82, 0x27, 0x3b,
    0x7b, 0xfa, 0xd8, 0x04, 0x5d, 0x85, 0xa4, 0x70};

// account delta row k: its decision, the resident row it reads, and the
// resident storage segment [seglo, seglo + seglen) it wipes (as k_sds_wipes)
__global__ void k_rv_acct(const sre_account_entry *__restrict__ acct, uint64_t na,
                          const sre_storage_entry *__restrict__ st, uint64_t ns,
                          const sre_account_delta *__restrict__ dl, uint64_t nd,
                          uint32_t *__restrict__ kind, /* nd */
                          uint32_t *__restrict__ flag, /* nd + 1 */
                          uint32_t *__restrict__ src,  /* nd */
                          uint32_t *__restrict__ seglo,
                          uint32_t *__restrict__ seglen /* nd + 1 */)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nd)
        return;
    if (k == nd) { // scan sentinels
        flag[k] = 0;
        seglen[k] = 0;
        return;
    }
    const uint8_t *key = dl[k].key;
    uint64_t p = lb_keys((const uint8_t *)acct, sizeof(sre_account_entry), na,
                         key, 32);
    bool resident = p < na && cmp_key32(acct[p].key, key) == 0;
    bool deleted = dl[k].deleted != 0;
    uint32_t kd = rv_acct_row(resident, deleted);
    kind[k] = kd;
    flag[k] = kd != RV_NONE;
    src[k] = (uint32_t)p;
    uint64_t lo = 0, lo2 = 0;
    if (resident && deleted) {
        uint64_t hi = ns;
        while (lo < hi) { // first i with acct_key >= key
            uint64_t mid = (lo + hi) / 2;
            if (cmp_key32(st[mid].acct_key, key) < 0)
                lo = mid + 1;
            else
                hi = mid;
        }
        lo2 = lo;
        hi = ns;
        while (lo2 < hi) { // first i with acct_key > key
            uint64_t mid = (lo2 + hi) / 2;
            if (cmp_key32(st[mid].acct_key, key) <= 0)
                lo2 = mid + 1;
            else
                hi = mid;
        }
    }
    seglo[k] = (uint32_t)lo;
    seglen[k] = (uint32_t)(lo2 - lo);
}

// storage delta row j: its decision, the resident row it reads, and the
// lower bound of its account among the account delta keys (the owner
// lookup of st_row_orphan, kept for the position formula)
__global__ void k_rv_st(const sre_storage_entry *__restrict__ st, uint64_t ns,
                        const sre_account_entry *__restrict__ acct, uint64_t na,
                        const sre_account_delta *__restrict__ dl_a, uint64_t n_acct,
                        const sre_storage_entry *__restrict__ dl, uint64_t nd,
                        uint32_t *__restrict__ kind, /* nd */
                        uint32_t *__restrict__ flag, /* nd + 1 */
                        uint32_t *__restrict__ src,  /* nd */
                        uint32_t *__restrict__ owner /* nd */)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nd)
        return;
    if (j == nd) {
        flag[j] = 0;
        return;
    }
    const uint8_t *akey = dl[j].acct_key;
    uint64_t q = lb_keys((const uint8_t *)dl_a, sizeof(sre_account_delta),
                         n_acct, akey, 32);
    bool destroyed = q < n_acct && cmp_key32(dl_a[q].key, akey) == 0 &&
                     dl_a[q].deleted != 0;
    uint64_t a = lb_keys((const uint8_t *)acct, sizeof(sre_account_entry), na,
                         akey, 32);
    bool owner_resident = a < na && cmp_key32(acct[a].key, akey) == 0;
    uint64_t p = lb_keys((const uint8_t *)st, sizeof(sre_storage_entry), ns,
                         (const uint8_t *)&dl[j], 64);
    bool slot_resident = p < ns && cmp_key64((const uint8_t *)&st[p],
                                             (const uint8_t *)&dl[j]) == 0;
    uint32_t kd = rv_st_row(owner_resident, destroyed, slot_resident,
                            min_be_len(dl[j].value) != 0);
    kind[j] = kd;
    flag[j] = kd != RV_NONE;
    src[j] = (uint32_t)p;
    owner[j] = (uint32_t)q;
}

// emitted account rows, compacted in delta order
__global__ void k_rv_emit_acct(const sre_account_entry *__restrict__ acct,
                               const sre_account_delta *__restrict__ dl,
                               uint64_t nd, const uint32_t *__restrict__ kind,
                               const uint32_t *__restrict__ ea,
                               const uint32_t *__restrict__ src,
                               sre_account_delta *__restrict__ out)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nd || kind[k] == RV_NONE)
        return;
    sre_account_delta r;
    memset(&r, 0, sizeof(r));
    memcpy(r.key, dl[k].key, 32);
    if (kind[k] == RV_OLD) {
        const sre_account_entry *o = &acct[src[k]];
        r.nonce = o->nonce;
        memcpy(r.balance, o->balance, 32);
        memcpy(r.code_hash, o->code_hash, 32);
    } else {
        for (int b = 0; b < 32; ++b)
            r.code_hash[b] = D_KECCAK_EMPTY[b];
        r.deleted = 1;
    }
    out[ea[k]] = r;
}

// emitted storage delta rows, at rv_delta_row_pos
__global__ void k_rv_emit_st(const sre_storage_entry *__restrict__ st,
                             const sre_storage_entry *__restrict__ dl,
                             uint64_t nd, const uint32_t *__restrict__ kind,
                             const uint32_t *__restrict__ es,
                             const uint32_t *__restrict__ src,
                             const uint32_t *__restrict__ owner,
                             const uint32_t *__restrict__ segsum,
                             sre_storage_entry *__restrict__ out)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nd || kind[j] == RV_NONE)
        return;
    const uint64_t *s = (const uint64_t *)&dl[j];
    uint64_t *d = (uint64_t *)&out[rv_delta_row_pos(es, j, segsum, owner[j])];
#pragma unroll
    for (int w = 0; w < 8; ++w) // (acct_key, slot_key)
        d[w] = s[w];
    uint64_t v[4] = {0, 0, 0, 0}; // RV_GONE: a zero value deletes the slot
    if (kind[j] == RV_OLD) {
        const uint64_t *o = (const uint64_t *)st[src[j]].value;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            v[w] = o[w];
    }
#pragma unroll
    for (int w = 0; w < 4; ++w)
        d[8 + w] = v[w];
}

// per account delta row: emitted storage delta rows with a smaller account
// key (the second term of rv_segment_row_pos)
__global__ void k_rv_seg_base(const sre_account_delta *__restrict__ dl_a,
                              uint64_t n_acct,
                              const uint32_t *__restrict__ seglen,
                              const sre_storage_entry *__restrict__ dl,
                              uint64_t nd, uint32_t *__restrict__ segp)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_acct)
        return;
    segp[k] = seglen[k] ? (uint32_t)lb_keys((const uint8_t *)dl,
                                            sizeof(sre_storage_entry), nd,
                                            dl_a[k].key, 32)
                        : 0u;
}

// The destroyed accounts' resident rows, flat over ALL wiped rows (segment
// sizes are as skewed as contract storage; a pass per segment would run as
// long as its largest one). V = uint4: six lanes move one 96-byte row as
// 16-byte loads and stores; V = uint64_t (twelve lanes) serves a borrowed
// storage array that is only 8-byte aligned.
template <typename V>
__global__ void k_rv_copy_segs(const sre_storage_entry *__restrict__ st,
                               const uint32_t *__restrict__ segsum,
                               const uint32_t *__restrict__ seglo,
                               const uint32_t *__restrict__ segp,
                               uint64_t nseg, uint64_t wiped,
                               const uint32_t *__restrict__ es,
                               sre_storage_entry *__restrict__ out)
{
    constexpr uint64_t LANES = sizeof(sre_storage_entry) / sizeof(V);
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t w = t / LANES, part = t % LANES;
    if (w >= wiped)
        return;
    uint64_t k = rv_segment_of(segsum, nseg, w);
    uint64_t from = seglo[k] + (w - segsum[k]);
    uint64_t to = rv_segment_row_pos(w, es, segp[k]);
    ((V *)&out[to])[part] = ((const V *)&st[from])[part];
}

// wipes_before / merged_pos: merge_plan.h
__global__ void k_sds_scatter(const sre_storage_entry *__restrict__ base,
                              uint64_t ns,
                              const sre_storage_entry *__restrict__ dl,
                              uint64_t nst,
                              const uint32_t *__restrict__ m_excl, /* nst+1 */
                              const uint32_t *__restrict__ eff_excl,
                              const uint32_t *__restrict__ wlo,
                              const uint32_t *__restrict__ whi,
                              const uint32_t *__restrict__ wsum, /* ndel+1 */
                              uint32_t ndel,
                              sre_storage_entry *__restrict__ out)
{
    // block-shared rank window (see k_sd_scatter)
    __shared__ uint32_t plo_s, phi_s;
    uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x;
    if (threadIdx.x == 0) {
        uint64_t a = i0 < ns ? i0 : ns - 1;
        plo_s = (uint32_t)lb_keys((const uint8_t *)dl,
                                  sizeof(sre_storage_entry), nst,
                                  (const uint8_t *)&base[a], 64);
        uint64_t b = i0 + blockDim.x - 1;
        if (b >= ns)
            b = ns - 1;
        phi_s = (uint32_t)lb_keys((const uint8_t *)dl,
                                  sizeof(sre_storage_entry), nst,
                                  (const uint8_t *)&base[b], 64);
    }
    __syncthreads();
    uint64_t i = i0 + threadIdx.x;
    // fast path: full block, no delta key in span, no wipe-range overlap
    // -> constant shift, flat coalesced copy
    if (plo_s == phi_s && i0 + blockDim.x <= ns) {
        uint32_t p = plo_s;
        uint64_t last = i0 + blockDim.x - 1;
        bool w0, w1;
        uint64_t wb0 = wipes_before(wlo, whi, wsum, ndel, i0, &w0);
        uint64_t wb1 = wipes_before(wlo, whi, wsum, ndel, last, &w1);
        bool lastmatch = p < nst &&
                         cmp_key64((const uint8_t *)&dl[p],
                                   (const uint8_t *)&base[last]) == 0;
        if (!lastmatch && !w0 && !w1 && wb0 == wb1) {
            uint64_t j0 = merged_pos(i0, m_excl[p], eff_excl[p], wb0);
            const uint64_t *s8 = (const uint64_t *)&base[i0];
            uint64_t *d8 = (uint64_t *)&out[j0];
            uint64_t v[12];
#pragma unroll
            for (int w = 0; w < 12; ++w)
                v[w] = s8[threadIdx.x + (uint32_t)w * BLOCK];
#pragma unroll
            for (int w = 0; w < 12; ++w)
                d8[threadIdx.x + (uint32_t)w * BLOCK] = v[w];
            return;
        }
    }
    if (i >= ns)
        return;
    bool wiped;
    uint64_t wb = wipes_before(wlo, whi, wsum, ndel, i, &wiped);
    uint64_t lo = plo_s, hh = phi_s < nst ? (uint64_t)phi_s + 1 : nst;
    while (lo < hh) {
        uint64_t mid = (lo + hh) / 2;
        if (cmp_key64((const uint8_t *)&dl[mid],
                      (const uint8_t *)&base[i]) < 0)
            lo = mid + 1;
        else
            hh = mid;
    }
    uint64_t p = lo;
    bool matched = p < nst && cmp_key64((const uint8_t *)&dl[p],
                                        (const uint8_t *)&base[i]) == 0;
    if (matched || wiped)
        return;
    uint64_t j = merged_pos(i, m_excl[p], eff_excl[p], wb);
    const uint64_t *s8 = (const uint64_t *)&base[i];
    uint64_t *d8 = (uint64_t *)&out[j];
#pragma unroll
    for (int w = 0; w < 12; ++w) // 96 B
        d8[w] = s8[w];
}

__global__ void k_sds_place(const sre_storage_entry *__restrict__ dl,
                            uint64_t nst, const uint32_t *__restrict__ bpos,
                            const uint32_t *__restrict__ m_excl,
                            const uint32_t *__restrict__ eff_excl,
                            const uint32_t *__restrict__ wlo,
                            const uint32_t *__restrict__ whi,
                            const uint32_t *__restrict__ wsum, uint32_t ndel,
                            sre_storage_entry *__restrict__ out)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nst)
        return;
    // zero value = slot deletion: no output row
    const uint8_t *v = dl[k].value;
    bool nz = false;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        nz |= ((const uint64_t *)v)[q] != 0;
    if (!nz)
        return;
    bool wiped;
    uint64_t wb = wipes_before(wlo, whi, wsum, ndel, bpos[k], &wiped);
    uint64_t j = merged_pos(bpos[k], m_excl[k], eff_excl[k], wb);
    const uint64_t *s8 = (const uint64_t *)&dl[k];
    uint64_t *d8 = (uint64_t *)&out[j];
#pragma unroll
    for (int w = 0; w < 12; ++w)
        d8[w] = s8[w];
}

// sparse-leaf support: compact the positions no seed covers (dirty cells
// leave covered == 0 too, so this is exactly the recompute set)
__global__ void k_active_hist(const uint8_t *__restrict__ covered, uint64_t n,
                              uint32_t *__restrict__ cnts)
{
    __shared__ uint32_t c_l;
    if (threadIdx.x == 0)
        c_l = 0;
    __syncthreads();
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t m = __ballot(i < n && covered[i] == 0);
    if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(&c_l, (uint32_t)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0)
        cnts[blockIdx.x] = c_l;
}

__global__ void k_active_scatter(const uint8_t *__restrict__ covered,
                                 uint64_t n,
                                 const uint32_t *__restrict__ offs,
                                 uint32_t *__restrict__ list)
{
    __shared__ uint32_t wh[BLOCK / 64];
    int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < BLOCK / 64)
        wh[threadIdx.x] = 0;
    __syncthreads();
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool act = i < n && covered[i] == 0;
    uint64_t m = __ballot(act);
    uint32_t rank = __popcll(m & ((1ull << lane) - 1));
    if (lane == 0)
        wh[wid] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!act)
        return;
    uint32_t before = 0;
    for (int w = 0; w < wid; ++w)
        before += wh[w];
    list[offs[blockIdx.x] + before + rank] = (uint32_t)i;
}

// ---------------------------------------------------------------------------
// dirty-path incremental: cell-top capture (CELL_NIBBLES-prefix cells)
// ---------------------------------------------------------------------------

#define CELL_NIBBLES 5
#define N_CELLS (1u << (4 * CELL_NIBBLES))

struct cap_row {
    node_rec rec;     // interval, parent depth, ref — as of capture
    uint32_t cell;    // 5-nibble prefix of the cell's keys
    uint32_t pad_[3];
    uint8_t bhash[32]; // updates mode: bhash_by_s[rec.s] at capture time
                       // (the keccak of the subtree-top BRANCH below any
                       // extension — what ancestor TrieUpdates rows embed)
};
static_assert(sizeof(cap_row) == 96, "cap_row must be 96 bytes");

__device__ __forceinline__ uint32_t cell_of_key(const uint8_t *key)
{
    return ((uint32_t)key[0] << 12) | ((uint32_t)key[1] << 4) |
           ((uint32_t)key[2] >> 4);
}

// append every level-input record (the active nodes consumed at this level)
// to the capture buffer: at levels < CELL_NIBBLES these are exactly the
// cell-top nodes. Runs before any branch kernel of its level, so the
// members are still as the previous levels left them.
__global__ void k_capture_L(const node_rec *__restrict__ recs,
                            const uint32_t *__restrict__ idx, uint64_t n,
                            cap_row *__restrict__ out,
                            uint32_t *__restrict__ cnt, uint64_t capacity,
                            uint32_t *__restrict__ err,
                            const uint8_t *__restrict__ bhash_by_s /* null
                            unless updates mode */)
{
    __shared__ uint32_t lds[BLOCK];
    __shared__ uint32_t base;
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool act = j < n;
    uint32_t excl, total;
    block_scan(lds, act ? 1u : 0u, &excl, &total);
    if (threadIdx.x == 0)
        base = total ? atomicAdd(cnt, total) : 0;
    __syncthreads();
    if (!act)
        return;
    uint64_t slot = base + excl;
    if (slot >= capacity) {
        atomicOr(err, 1u << E_INTERNAL);
        return;
    }
    cap_row r;
    const uint32_t s = idx[j]; // the member's slot, and its s
    copy_rec(&r.rec, &recs[s]);
    r.cell = r.rec.seg >> 12; // cell_of_key of the record's first key
    r.pad_[0] = r.pad_[1] = r.pad_[2] = 0;
    if (bhash_by_s)
        memcpy(r.bhash, bhash_by_s + 32ull * s, 32);
    else
        memset(r.bhash, 0, 32);
    out[slot] = r;
}

// Revalidate retained cell-top rows against the merged state. Every row is
// a depth-(CELL_NIBBLES-1) record: its keys share >= CELL_NIBBLES nibbles,
// so any delta key inside (or joining) its interval lands in the SAME cell
// and k_mark_delta_cells already dirtied it. A clean cell therefore has
// unchanged interval content; only the junction can move, which the fresh
// boundary-lcp check catches. Rebase: ns = map[s]; ne = map[e-1]+1 — the
// latter excludes keys inserted between the interval and its right
// neighbour (they share < CELL_NIBBLES nibbles, i.e. live outside the
// subtree). Valid rows are seeded (recs[ns]+depths[ns]+hist) and mark
// covered[ns..ne); invalid rows dirty their cell so their leaves rebuild.
__global__ void k_revalidate_rows(const cap_row *__restrict__ rows, uint64_t n,
                                  const uint32_t *__restrict__ old2new,
                                  const int8_t *__restrict__ lcp,
                                  uint8_t *__restrict__ cell_dirty,
                                  node_rec *__restrict__ recs,
                                  uint8_t *__restrict__ depths,
                                  uint8_t *__restrict__ covered,
                                  uint32_t *__restrict__ hist,
                                  uint8_t *__restrict__ bhash_out /* updates
                                  mode: seed bhash_by_s at the new pos */)
{
    __shared__ uint32_t hist_l[66];
    if (threadIdx.x < 66)
        hist_l[threadIdx.x] = 0;
    __syncthreads();
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) {
        cap_row r = rows[j];
        // one captured row per cell (disjoint): no other thread reads or
        // writes this cell's flag concurrently
        if (cell_dirty[r.cell] == 0) {
            uint32_t ns_ = old2new[r.rec.s];
            uint32_t ne_ = old2new[r.rec.e - 1] + 1;
            int8_t l0 = lcp[ns_], l1 = lcp[ne_];
            int8_t nd = l0 > l1 ? l0 : l1;
            if (nd == r.rec.depth) {
                r.rec.s = ns_;
                r.rec.e = ne_;
                copy_rec(&recs[ns_], &r.rec);
                depths[ns_] = (uint8_t)(nd + 1);
                atomicAdd(&hist_l[nd + 1], 1u);
                for (uint32_t p = ns_; p < ne_; ++p)
                    covered[p] = 1;
                if (bhash_out)
                    memcpy(bhash_out + 32ull * ns_, r.bhash, 32);
            } else {
                cell_dirty[r.cell] = 1; // junction moved: rebuild the cell
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 66 && hist_l[threadIdx.x])
        atomicAdd(&hist[threadIdx.x], hist_l[threadIdx.x]);
}

// sre_root_from_nodes: per storage segment, either seed the account's
// storage root from a supplied stored path-[] row (untouched trie) or
// flag the segment for rebuild (no row, or touched by the delta).
__global__ void k_seg_need(const sre_storage_entry *__restrict__ st,
                           const uint32_t *__restrict__ seg_start,
                           uint32_t n_seg,
                           const uint8_t *__restrict__ root_kv, /* nr x 64:
                           acct_key || root, key-sorted */
                           uint64_t nr,
                           const uint8_t *__restrict__ touched, /* nt x 32 */
                           uint64_t nt,
                           const uint32_t *__restrict__ seg_acct,
                           uint8_t *__restrict__ acct_roots,
                           uint32_t *__restrict__ need)
{
    uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg)
        return;
    const uint8_t *key = st[seg_start[s]].acct_key;
    uint64_t t = lb_keys(touched, 32, nt, key, 32);
    if (!(t < nt && cmp_key32(touched + 32 * t, key) == 0)) {
        uint64_t rp = lb_keys(root_kv, 64, nr, key, 32);
        if (rp < nr && cmp_key32(root_kv + 64 * rp, key) == 0) {
            memcpy(acct_roots + 32ull * seg_acct[s], root_kv + 64 * rp + 32,
                   32);
            need[s] = 0;
            return;
        }
    }
    need[s] = 1;
}

// dirty-cell marking from STORAGE delta rows (the account's leaf changes)
__global__ void k_mark_delta_cells_st(const sre_storage_entry *__restrict__ dl,
                                      uint64_t nd,
                                      uint8_t *__restrict__ cell_dirty)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nd)
        return;
    cell_dirty[cell_of_key(dl[j].acct_key)] = 1;
}

// mark cells touched by delta keys
__global__ void k_mark_delta_cells(const sre_account_delta *__restrict__ dl,
                                   uint64_t nd, uint8_t *__restrict__ cell_dirty)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nd)
        return;
    cell_dirty[cell_of_key(dl[j].key)] = 1;
}

// ---------------------------------------------------------------------------
// misc kernels
// ---------------------------------------------------------------------------

__global__ void k_scatter_roots(const uint8_t *__restrict__ seg_roots,
                                const uint32_t *__restrict__ seg_acct, uint32_t n_seg,
                                uint8_t *__restrict__ acct_roots)
{
    uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg)
        return;
    const uint64_t *src = (const uint64_t *)(seg_roots + 32ull * s);
    uint64_t *dst = (uint64_t *)(acct_roots + 32ull * seg_acct[s]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        dst[k] = src[k];
}

__global__ void k_fill_empty_roots(uint8_t *__restrict__ acct_roots, uint64_t na)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= na)
        return;
    for (int k = 0; k < 32; ++k)
        acct_roots[32 * i + k] = D_EMPTY_ROOT[k];
}

__global__ void k_nibble_counts(const sre_account_entry *__restrict__ acct,
                                uint64_t na, uint64_t *__restrict__ counts)
{
    __shared__ uint32_t cnt_l[16];
    if (threadIdx.x < 16)
        cnt_l[threadIdx.x] = 0;
    __syncthreads();
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < na)
        atomicAdd(&cnt_l[acct[i].key[0] >> 4], 1u);
    __syncthreads();
    if (threadIdx.x < 16 && cnt_l[threadIdx.x])
        atomicAdd((unsigned long long *)&counts[threadIdx.x],
                  (unsigned long long)cnt_l[threadIdx.x]);
}

// root-branch assembly from gathered child refs (single thread; O(1) work)
__global__ void k_finish_top(const uint8_t *__restrict__ child_refs,
                             const uint8_t *__restrict__ child_lens,
                             uint8_t *__restrict__ out_root)
{
    __shared__ __align__(16) uint8_t slot[SLOT_BR];
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    uint64_t *slot64 = (uint64_t *)slot;
    for (int k = 0; k < SLOT_BR / 8; ++k)
        slot64[k] = 0;
    int payload = 1;
    for (int b = 0; b < 16; ++b)
        payload += child_lens[b] ? child_lens[b] : 1;
    int h = rlp_list_hdr_write(slot, payload);
    int p = h;
    for (int b = 0; b < 16; ++b) {
        if (child_lens[b]) {
            for (int k = 0; k < child_lens[b]; ++k)
                slot[p++] = child_refs[33 * b + k];
        } else {
            slot[p++] = 0x80;
        }
    }
    slot[p++] = 0x80;
    int len = h + payload;
    int nblocks = keccak_pad(slot, len);
    uint64_t hash[4];
    keccak_lds(slot64, nblocks, hash);
    memcpy(out_root, hash, 32);
}

// ---------------------------------------------------------------------------
// scan utilities (exclusive u32, recursive)
// ---------------------------------------------------------------------------

#define SCAN_ITEMS 8

__global__ void k_scan_block(const uint32_t *__restrict__ in, uint64_t n,
                             uint32_t *__restrict__ out, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t lds[BLOCK];
    uint64_t base = (uint64_t)blockIdx.x * BLOCK * SCAN_ITEMS +
                    (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    uint32_t tsum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        uint64_t i = base + k;
        v[k] = i < n ? in[i] : 0;
        tsum += v[k];
    }
    uint32_t excl, total;
    block_scan(lds, tsum, &excl, &total);
    if (threadIdx.x == 0 && sums)
        sums[blockIdx.x] = total;
    uint32_t run = excl;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        uint64_t i = base + k;
        if (i < n)
            out[i] = run;
        run += v[k];
    }
}

__global__ void k_scan_add(uint32_t *__restrict__ out, uint64_t n,
                           const uint32_t *__restrict__ sums_scanned)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    out[i] += sums_scanned[i / (BLOCK * SCAN_ITEMS)];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

#define HIP_CHECK(ctx, call)                                                     \
    do {                                                                         \
        hipError_t _e = (call);                                                  \
        if (_e != hipSuccess) {                                                  \
            set_err(ctx, std::string(#call) + ": " + hipGetErrorString(_e));     \
            return -1;                                                           \
        }                                                                        \
    } while (0)

// Launch a kernel (no dynamic LDS) and check the launch, like HIP_CHECK.
#define LAUNCH(ctx, kernel, grid, block, stream, ...)                            \
    do {                                                                         \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream,           \
                           __VA_ARGS__);                                         \
        HIP_CHECK(ctx, hipGetLastError());                                       \
    } while (0)

struct sre_ctx;
struct DBuf;

// One resident input array (accounts or storage): borrowed from the caller,
// or owned and then either hipMalloc'd (upload) or a pool buffer (adopt).
template <typename T> struct resident {
    const T *d = nullptr;
    uint64_t n = 0;
    bool own = false;
    // nonzero when the owned array came from the pool (a delta merge
    // replaces the state every call; pooling avoids a 21 GB hipMalloc+Free
    // per delta at the 200M-account config)
    size_t pool_bytes = 0;
    void release(sre_ctx *ctx);
    void adopt(sre_ctx *ctx, DBuf &buf, uint64_t count);
    int borrow(sre_ctx *ctx, const void *d_entries, uint64_t count);
    int upload(sre_ctx *ctx, const T *entries, uint64_t count);
};

// A retained (non-pool) device buffer and its capacity in elements.
struct retained_buf {
    void *p = nullptr;
    uint64_t cap = 0;
    int grow(sre_ctx *ctx, uint64_t want, uint64_t elem_bytes = 1);
};

struct sre_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr; // branch-assemble pipeline stage
    std::string err;
    resident<sre_account_entry> acct;
    resident<sre_storage_entry> st;
    sre_stats stats{};
    // branch-pipeline path counters (sre_get_path_counters): [0] levels that
    // used the class partition, [1] groups sent to k_branch_fused1,
    // [2] chunks launched, [3] levels that ran the two-stream ping-pong.
    // Reset at the start of every root-type call.
    uint64_t path_cnt[4] = {0, 0, 0, 0};
    // dirty-path reuse counters (sre_get_incremental_counters): [0] retained
    // cell-top rows examined, [1] rows revalidated and seeded, [2] account
    // leaves rehashed, [3] one-pass small account merge ran, [4] closed-form
    // storage merge ran, [5] rows captured for the next call. Reset with
    // path_cnt; filled by incremental_root_impl.
    uint64_t inc_cnt[6] = {0, 0, 0, 0, 0, 0};
    // hash-and-sort counters of the last plain-state upload that installed a
    // state (sre_get_hash_sort_counters): [0] keccak-f invocations, [1] radix
    // passes executed, [2] passes skipped, [3] rows in tie runs, [4] tie
    // runs, [5] address hashes reused (always 0: not built).
    uint64_t hs_cnt[6] = {0, 0, 0, 0, 0, 0};
    // TrieUpdates retention (sre_root_with_updates)
    bool retain_updates = false;
    std::vector<sre_update_row> updates;
    // Incremental TrieUpdates: current stored-row set, sorted like
    // TrieUpdatesSorted (armed by sre_root_retaining_with_updates)
    std::vector<snap_row> snap;
    bool snap_valid = false;
    // Dirty-path incremental retention (sre_root_retaining /
    // sre_incremental_root): "cell-top" node records — the unique active
    // node of each 5-nibble key-prefix cell, captured from the level inputs
    // at depths < CELL_NIBBLES during a full account pass.
    bool retain_cells = false;   // capture on the next root computation
    bool cells_valid = false;    // retained rows match the resident state
    retained_buf cap_rows;       // cap_row[cap_count]
    uint64_t cap_count = 0;
    retained_buf roots_ret;  // retained per-account storage roots (na x 32)
    retained_buf roots_ret2; // ping-pong partner (incremental updates)
    // retained account-lcp (na+1 i8) for small-delta repair: chained
    // deltas patch O(delta) boundary lcps instead of recomputing all na
    retained_buf lcp_ret, lcp_ret2;
    bool lcp_valid = false; // lcp_ret matches the resident accounts
    // revert capture (sre_set_revert_capture): the revert of the LAST
    // adopted delta, device-resident in pool buffers, and what its capture
    // did (sre_get_revert_counters). Nothing is held while rv_have is false.
    bool rv_on = false;
    bool rv_have = false;
    resident<sre_account_delta> rv_acct;
    resident<sre_storage_entry> rv_st;
    uint64_t rv_cnt[4] = {0, 0, 0, 0};
    // size-class buffer pool: the level machinery allocates/frees dozens of
    // transient arrays per level; hipMalloc latency would dominate small
    // jobs. Freed buffers are cached by power-of-2 class and reused (also
    // across bench steps). Freed for real in sre_destroy.
    std::vector<std::pair<size_t, void *>> pool;
};

// Size classes: power-of-two up to 256 MiB (transient level-machinery
// buffers — reuse across wildly varying level sizes), then 256 MiB-step
// quantization. Pure pow2 would round the two giant state arrays (e.g.
// ~61 GB of storage entries) up to the next power of two and, with the
// apply_delta ping-pong partner, hold ~2x their footprint in dead
// rounding at near-capacity configs; the step classes bound the waste at
// 256 MiB per huge buffer while keeping exact-class reuse.
static size_t pool_class(size_t bytes)
{
    const size_t STEP = 256ull << 20;
    if (bytes > STEP)
        return (bytes + STEP - 1) / STEP * STEP;
    size_t c = 256;
    while (c < bytes)
        c <<= 1;
    return c;
}

static void *pool_get(sre_ctx *ctx, size_t bytes)
{
    size_t cls = pool_class(bytes);
    for (size_t i = 0; i < ctx->pool.size(); ++i) {
        if (ctx->pool[i].first == cls) {
            void *p = ctx->pool[i].second;
            ctx->pool[i] = ctx->pool.back();
            ctx->pool.pop_back();
            return p;
        }
    }
    void *p = nullptr;
    if (hipMalloc(&p, cls) != hipSuccess) {
        // pool pressure: drop every cached buffer and retry once (a big
        // storage merge after a full-root pass can need the HBM the pool
        // is hoarding)
        (void)hipDeviceSynchronize();
        for (auto &e : ctx->pool)
            (void)hipFree(e.second);
        ctx->pool.clear();
        if (hipMalloc(&p, cls) != hipSuccess)
            return nullptr;
        // the failed first attempt left a sticky hipErrorOutOfMemory in
        // the per-thread last-error slot; consume it so the next launch's
        // hipGetLastError() check doesn't report a phantom OOM
        (void)hipGetLastError();
    }
    return p;
}

static void pool_put(sre_ctx *ctx, size_t bytes, void *p)
{
    if (p)
        ctx->pool.emplace_back(pool_class(bytes), p);
}

static std::string g_err;

static void clear_revert(sre_ctx *ctx);

static void set_err(sre_ctx *ctx, const std::string &msg)
{
    if (ctx)
        ctx->err = msg;
    else
        g_err = msg;
}

extern "C" const char *sre_last_error(const sre_ctx *ctx)
{
    return ctx ? ctx->err.c_str() : g_err.c_str();
}

extern "C" sre_ctx *sre_create(int device)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= device) {
        set_err(nullptr, "sre_create: no HIP device " + std::to_string(device) +
                             " (this engine is GPU-only by design)");
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        set_err(nullptr, "sre_create: hipSetDevice failed");
        return nullptr;
    }
    sre_ctx *ctx = new sre_ctx();
    ctx->device = device;
    if (hipStreamCreate(&ctx->stream) != hipSuccess ||
        hipStreamCreate(&ctx->stream2) != hipSuccess) {
        set_err(nullptr, "sre_create: hipStreamCreate failed");
        delete ctx;
        return nullptr;
    }
    return ctx;
}

extern "C" void sre_destroy(sre_ctx *ctx)
{
    if (!ctx)
        return;
    ctx->acct.release(ctx);
    ctx->st.release(ctx);
    clear_revert(ctx);
    for (retained_buf *b : {&ctx->cap_rows, &ctx->roots_ret, &ctx->roots_ret2,
                            &ctx->lcp_ret, &ctx->lcp_ret2})
        if (b->p)
            (void)hipFree(b->p);
    for (auto &e : ctx->pool)
        (void)hipFree(e.second);
    ctx->pool.clear();
    if (ctx->stream)
        (void)hipStreamDestroy(ctx->stream);
    if (ctx->stream2)
        (void)hipStreamDestroy(ctx->stream2);
    delete ctx;
}

// leaf intervals are u32 (node_rec.s/e) — reject, never truncate (sre.h
// capacity contract)
static int check_cap(sre_ctx *ctx, uint64_t n)
{
    if (!count_fits(n)) {
        set_err(ctx, "entry count exceeds the 2^32-1 per-GPU limit "
                     "(u32 leaf intervals); shard across GPUs");
        return -1;
    }
    return 0;
}

// The resident state changed (or is about to): nothing retained for the
// incremental modes matches it any more.
static void invalidate_retention(sre_ctx *ctx)
{
    ctx->cells_valid = false;
    ctx->snap_valid = false;
    ctx->lcp_valid = false;
}

// Start of a root-type call: select the device, reset the path counters
// and (for the calls that publish them) the stats.
static int begin_call(sre_ctx *ctx, bool zero_stats)
{
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    memset(ctx->path_cnt, 0, sizeof(ctx->path_cnt));
    memset(ctx->inc_cnt, 0, sizeof(ctx->inc_cnt));
    if (zero_stats)
        memset(&ctx->stats, 0, sizeof(ctx->stats));
    return 0;
}

// Replace the array with an engine-owned copy of host entries.
template <typename T>
int resident<T>::upload(sre_ctx *ctx, const T *entries, uint64_t count)
{
    if (check_cap(ctx, count))
        return -1;
    invalidate_retention(ctx);
    clear_revert(ctx);
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    release(ctx);
    void *p = nullptr;
    if (count) {
        HIP_CHECK(ctx, hipMalloc(&p, count * sizeof(T)));
        HIP_CHECK(ctx, hipMemcpy(p, entries, count * sizeof(T), hipMemcpyHostToDevice));
    }
    d = (const T *)p;
    n = count;
    own = true;
    return 0;
}

// Borrow device-resident inputs (zero-copy; caller keeps them alive).
template <typename T>
int resident<T>::borrow(sre_ctx *ctx, const void *d_entries, uint64_t count)
{
    if (check_cap(ctx, count))
        return -1;
    invalidate_retention(ctx);
    clear_revert(ctx);
    release(ctx);
    d = (const T *)d_entries;
    n = count;
    own = false;
    return 0;
}

extern "C" int sre_upload_accounts(sre_ctx *ctx, const sre_account_entry *entries,
                                   uint64_t n)
{
    return ctx->acct.upload(ctx, entries, n);
}

extern "C" int sre_upload_storage(sre_ctx *ctx, const sre_storage_entry *entries,
                                  uint64_t n)
{
    return ctx->st.upload(ctx, entries, n);
}

extern "C" int sre_set_accounts_device(sre_ctx *ctx, const void *d_entries, uint64_t n)
{
    return ctx->acct.borrow(ctx, d_entries, n);
}

extern "C" int sre_set_storage_device(sre_ctx *ctx, const void *d_entries, uint64_t n)
{
    return ctx->st.borrow(ctx, d_entries, n);
}

extern "C" int sre_keccak_batch_device(sre_ctx *ctx, const void *d_in, uint64_t stride,
                                       uint32_t len, uint64_t n, void *d_out)
{
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (len > 135) {
        set_err(ctx, "sre_keccak_batch_device: len > 135 unsupported");
        return -1;
    }
    if (n == 0)
        return 0;
    uint64_t blocks = (n + BLOCK - 1) / BLOCK;
    LAUNCH(ctx, k_keccak_batch, (uint32_t)blocks, BLOCK, ctx->stream,
           (const uint8_t *)d_in, stride, len, n, (uint8_t *)d_out);
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// Messages of any length (sre_keccak_batch_device is one block, <= 135 B).
extern "C" int sre_keccak_long_device(sre_ctx *ctx, const void *d_in, uint64_t stride,
                                      uint32_t len, uint64_t n, void *d_out)
{
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (len > stride) {
        set_err(ctx, "sre_keccak_long_device: len > stride");
        return -1;
    }
    if (n == 0)
        return 0;
    uint64_t blocks = (n + BLOCK - 1) / BLOCK;
    LAUNCH(ctx, k_keccak_long, (uint32_t)blocks, BLOCK, ctx->stream,
           (const uint8_t *)d_in, stride, len, n, (uint8_t *)d_out);
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// Pool-backed transient device buffer (stream-ordered reuse is safe: all
// work runs on ctx->stream).
struct DBuf {
    sre_ctx *ctx = nullptr;
    void *p = nullptr;
    size_t sz = 0;
    DBuf() = default;
    explicit DBuf(sre_ctx *c) : ctx(c) {}
    ~DBuf() { release(); }
    void release()
    {
        if (p) {
            if (ctx)
                pool_put(ctx, sz, p);
            else
                (void)hipFree(p);
            p = nullptr;
        }
    }
    hipError_t alloc(size_t bytes)
    {
        release();
        sz = bytes ? bytes : 16;
        if (ctx) {
            p = pool_get(ctx, sz);
            return p ? hipSuccess : hipErrorOutOfMemory;
        }
        return hipMalloc(&p, sz);
    }
    // hand the buffer out (sz stays: its size class); the DBuf is empty after
    void *take()
    {
        void *q = p;
        p = nullptr;
        return q;
    }
    template <typename T> T *as() { return (T *)p; }
};

// Free or return to the pool whatever the engine owns; n and own stay until
// the caller installs the next array.
template <typename T> void resident<T>::release(sre_ctx *ctx)
{
    if (own && d) {
        if (pool_bytes) {
            DBuf back(ctx); // its destructor returns the buffer to the pool
            back.p = (void *)d;
            back.sz = pool_bytes;
        } else {
            (void)hipFree((void *)d);
        }
    }
    d = nullptr;
    pool_bytes = 0;
}

// Install a merged or sorted array built in a pool buffer (reused across
// repeated deltas). Until this runs the DBuf owns it, so a failed build
// returns the buffer on whatever path it leaves by.
template <typename T> void resident<T>::adopt(sre_ctx *ctx, DBuf &buf, uint64_t count)
{
    release(ctx);
    pool_bytes = buf.sz;
    d = (const T *)buf.take();
    n = count;
    own = true;
}

// Drop the stored revert: counts 0, buffers back to the pool.
static void clear_revert(sre_ctx *ctx)
{
    ctx->rv_acct.release(ctx);
    ctx->rv_st.release(ctx);
    ctx->rv_acct.n = ctx->rv_st.n = 0;
    ctx->rv_have = false;
    memset(ctx->rv_cnt, 0, sizeof(ctx->rv_cnt));
}

// Owning HIP event. A failed create leaves a null event, which the first
// checked record/wait on it reports.
struct Event {
    hipEvent_t ev = nullptr;
    explicit Event(unsigned flags = hipEventDefault)
    {
        (void)hipEventCreateWithFlags(&ev, flags);
    }
    ~Event()
    {
        if (ev)
            (void)hipEventDestroy(ev);
    }
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
};

// Start/stop event pair. Adds no synchronisation: ms() is valid only after
// the caller has synchronised the stream stop() was recorded on.
struct EvTimer {
    Event t0, t1;
    hipError_t start(hipStream_t s) { return hipEventRecord(t0.ev, s); }
    hipError_t stop(hipStream_t s) { return hipEventRecord(t1.ev, s); }
    hipError_t ms(float *out) { return hipEventElapsedTime(out, t0.ev, t1.ev); }
};

static inline uint32_t grid_for(uint64_t n)
{
    return (uint32_t)((n + BLOCK - 1) / BLOCK);
}

// The 4-byte device error flag every pass ORs its E_* bits into.
static int alloc_err_flag(sre_ctx *ctx, DBuf &err)
{
    HIP_CHECK(ctx, err.alloc(4));
    HIP_CHECK(ctx, hipMemsetAsync(err.p, 0, 4, ctx->stream));
    return 0;
}

// Grow to `want` elements; contents are not preserved. The bigger buffer
// is allocated, and the stream drained, before the old one is freed:
// queued work may still read it.
int retained_buf::grow(sre_ctx *ctx, uint64_t want, uint64_t elem_bytes)
{
    if (cap >= want)
        return 0;
    void *bigger = nullptr;
    HIP_CHECK(ctx, hipMalloc(&bigger, want * elem_bytes));
    if (p) {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess)
            (void)hipFree(bigger);
        HIP_CHECK(ctx, e);
        (void)hipFree(p);
    }
    p = bigger;
    cap = want;
    return 0;
}

// Allocate b for n elements and queue their upload on ctx->stream; n == 0
// allocates the minimum and copies nothing.
template <typename T>
static int to_device(sre_ctx *ctx, DBuf &b, const T *src, uint64_t n)
{
    HIP_CHECK(ctx, b.alloc(n * sizeof(T)));
    if (n)
        HIP_CHECK(ctx, hipMemcpyAsync(b.p, src, n * sizeof(T),
                                      hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

// Blocking read-back of b's first n elements.
template <typename T>
static int to_host(sre_ctx *ctx, std::vector<T> &dst, const DBuf &b, uint64_t n)
{
    dst.resize(n);
    if (n)
        HIP_CHECK(ctx, hipMemcpy(dst.data(), b.p, n * sizeof(T),
                                 hipMemcpyDeviceToHost));
    return 0;
}

// exclusive scan of u32 in[n] -> out[n]; total returned synchronously.
static int scan_u32(sre_ctx *ctx, const uint32_t *d_in, uint32_t *d_out, uint64_t n,
                    uint32_t *total)
{
    if (n == 0) {
        if (total)
            *total = 0;
        return 0;
    }
    uint64_t per_block = (uint64_t)BLOCK * SCAN_ITEMS;
    uint64_t nblocks = (n + per_block - 1) / per_block;
    DBuf sums(ctx), sums_scanned(ctx);
    HIP_CHECK(ctx, sums.alloc(nblocks * 4));
    LAUNCH(ctx, k_scan_block, (uint32_t)nblocks, BLOCK, ctx->stream, d_in, n,
           d_out, sums.as<uint32_t>());
    if (nblocks > 1) {
        HIP_CHECK(ctx, sums_scanned.alloc(nblocks * 4));
        if (scan_u32(ctx, sums.as<uint32_t>(), sums_scanned.as<uint32_t>(), nblocks,
                     total))
            return -1;
        LAUNCH(ctx, k_scan_add, grid_for(n), BLOCK, ctx->stream, d_out, n,
               sums_scanned.as<uint32_t>());
    } else if (total) {
        HIP_CHECK(ctx, hipMemcpyAsync(total, sums.as<uint32_t>(), 4,
                                      hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

// ---------------------------------------------------------------------------
// level machinery driver
// ---------------------------------------------------------------------------

struct pass_out {
    double leaf_ms = 0, branch_ms = 0;
    uint64_t leaf_count = 0, leaf_blocks = 0, branch_count = 0, branch_blocks = 0;
    uint64_t levels = 0;
};

static int check_err(sre_ctx *ctx, uint32_t *d_err);

// Test gates for the size-gated branch pipeline (read per call; unset =
// production values). SRE_CLS_MIN: minimum groups per level for the class
// partition (and therefore the fused kernel) — below the default the win is
// noise. SRE_BR_CHUNK: branch-pipeline chunk in GROUPS (floor 256); tests
// lower both so small states run the chunked two-stream path.
static uint64_t cls_min_groups()
{
    const char *e = getenv("SRE_CLS_MIN");
    return e ? (uint64_t)atoll(e) : (1ull << 14);
}

static uint64_t br_chunk_groups()
{
    const char *e = getenv("SRE_BR_CHUNK");
    if (!e)
        return (uint64_t)(SRE_BR_CHUNK_MB) << 20;
    long long v = atoll(e);
    return v < 256 ? 256 : (uint64_t)v;
}

// Required inputs of run_levels: the leaf records of one trie family (every
// storage trie, or the account trie) and where its roots go.
struct level_in {
    uint64_t n = 0;
    node_rec *recs = nullptr;
    uint8_t *depths = nullptr;
    const int8_t *lcp = nullptr;
    const uint8_t *keys = nullptr; // entry i's key at keys + i * key_stride
    uint64_t key_stride = 0;
    const uint32_t *hist_host = nullptr; // records per depth bucket [66]
    int subtree = 0;
    uint8_t *seg_roots = nullptr, *child_refs = nullptr, *child_lens = nullptr;
    // storage pass: segment id per entry. Records carry the key word, not an
    // id (the ids are scanned after the leaf kernel); the id is read as
    // seg_by_slot[s] where it is consumed. Null in the account pass, whose
    // shard is the key word's top nibble.
    const uint32_t *seg_by_slot = nullptr;
    uint32_t *err = nullptr;
    // -1 = off; 0/1 = retain TrieUpdates rows of this trie kind (bhash then
    // holds 32 B per underlying entry for branch-hash lookups)
    int updates_kind = -1;
    uint8_t *bhash = nullptr;
};

// Cell-top capture (dirty-path incremental): when depth > 0, every level
// input at depth depth-1 is appended to rows (each such record's keys share
// >= depth nibbles: exactly one cell, disjoint from every other captured
// row). Default: off.
struct cell_capture {
    int depth = 0;
    cap_row *rows = nullptr;
    uint32_t *count = nullptr;
    uint64_t capacity = 0;
};

// Multiproof capture (sre_account_proof / sre_storage_proof): the path-node
// RLPs of the n targets at entry indices pti / pti2. Default (n == 0): off.
struct proof_capture {
    const uint32_t *pti = nullptr, *pti2 = nullptr;
    uint32_t n = 0;
    proof_row *rows = nullptr;
    uint32_t *row_count = nullptr;
    uint32_t row_cap = 0;
};

// What run_levels carries from one level to the next. The nodes themselves
// wait in place (recs[s] / depths[s]); only their per-depth counts travel.
struct level_carry {
    DBuf pend; // device counters: [p+1] nodes produced for depth p, [65] blocks
    uint32_t pending_host[66] = {0};
    explicit level_carry(sre_ctx *c) : pend(c) {}
};

// Transient buffers every level re-allocates (pool-backed, so a level
// usually gets its predecessor's buffer back). lcnt/loff (the per-wave
// select counts and their scan) are sized once per pass.
struct level_bufs {
    DBuf Lbuf, lcnt, loff, gs, scratch, meta, urows, urow_cnt, urowidx;
    explicit level_bufs(sre_ctx *c)
        : Lbuf(c), lcnt(c), loff(c), gs(c), scratch(c), meta(c),
          urows(c), urow_cnt(c), urowidx(c)
    {
    }
};

// One level's working set, released when the level ends.
struct level_work {
    int d = 0;
    uint64_t n_level = 0;
    uint32_t n_level32 = 0; // H2D source of gs[n_groups]: outlives the copy
    const uint32_t *idx = nullptr; // level input: the members' slots, sorted
    uint32_t n_groups = 0;
    uint64_t chunk = 0; // branch-pipeline chunk, in groups
    bool use_cls = false, use_fused = false, pipe2 = false;
    DBuf perm, ccnt, coff, scratch2, meta2, cinv;
    DBuf wq_jobs, wq_count; // deferred extension wraps (wrap_queue)
    std::vector<uint32_t> c0s; // per chunk: class-0 group count (fused)
    explicit level_work(sre_ctx *c)
        : perm(c), ccnt(c), coff(c), scratch2(c), meta2(c), cinv(c),
          wq_jobs(c), wq_count(c)
    {
    }
};

// Level d's input and groups in one select over the in-place nodes: count
// per wave span, scan, list the members' slots (idx) + group starts gs. Also
// sizes the buffers of the branch pipeline, which runs in chunks of w.chunk
// groups so the 552-B scratch slots stay bounded. w.n_level is the host's
// own count (leaf histogram + pending counters); the device count must
// agree.
static int select_level(sre_ctx *ctx, const level_in &in, level_bufs &bufs,
                        level_work &w)
{
    const uint32_t nw = (uint32_t)((in.n + LV_SPAN - 1) / LV_SPAN);
    const uint32_t grid = (nw + BLOCK / 64 - 1) / (BLOCK / 64);
    uint32_t *cnt = bufs.lcnt.as<uint32_t>(), *off = bufs.loff.as<uint32_t>();
    LAUNCH(ctx, k_level_count, grid, BLOCK, ctx->stream, in.depths, in.lcp, in.n,
           w.d, nw, cnt);
    uint32_t total = 0, n_level_dev = 0;
    if (scan_u32(ctx, cnt, off, 2ull * nw, &total))
        return -1;
    HIP_CHECK(ctx, hipMemcpy(&n_level_dev, off + nw, 4, hipMemcpyDeviceToHost));
    if (n_level_dev != w.n_level) {
        set_err(ctx, "input/engine error: internal-group-invariant");
        return -1;
    }
    w.n_groups = total - n_level_dev;
    w.n_level32 = n_level_dev;
    if (bufs.Lbuf.sz < w.n_level * 4)
        HIP_CHECK(ctx, bufs.Lbuf.alloc(w.n_level * 4));
    w.idx = bufs.Lbuf.as<uint32_t>();
    const uint64_t BR_CHUNK = br_chunk_groups();
    HIP_CHECK(ctx, bufs.gs.alloc(((uint64_t)w.n_groups + 1) * 4));
    w.chunk = w.n_groups < BR_CHUNK ? w.n_groups : BR_CHUNK;
    HIP_CHECK(ctx, bufs.scratch.alloc(w.chunk * SLOT_BR));
    HIP_CHECK(ctx, bufs.meta.alloc(w.chunk * sizeof(br_meta)));
    if (in.updates_kind >= 0) {
        // per-level: capacity must cover THIS level's chunk
        HIP_CHECK(ctx, bufs.urows.alloc(w.chunk * sizeof(sre_update_row)));
        HIP_CHECK(ctx, bufs.urow_cnt.alloc(4));
        HIP_CHECK(ctx, bufs.urowidx.alloc(w.chunk * 4));
    }
    LAUNCH(ctx, k_level_gather, grid, BLOCK, ctx->stream, in.depths, in.lcp,
           in.n, w.d, nw, off, n_level_dev, w.n_groups,
           bufs.Lbuf.as<uint32_t>(), bufs.gs.as<uint32_t>());
    HIP_CHECK(ctx, hipMemcpyAsync(bufs.gs.as<uint32_t>() + w.n_groups,
                                  &w.n_level32, 4, hipMemcpyHostToDevice,
                                  ctx->stream));
    return 0;
}

// Class partition (see nmem_class): one perm per chunk makes
// assemble/hash waves block-count uniform. All chunks' perms are
// built upfront on the main stream; the per-chunk assemble (memory
// heavy, stream2) is then pipelined against the hash (VALU heavy,
// main stream) with ping-pong scratch/meta buffers.
static int partition_classes(sre_ctx *ctx, const level_in &in, uint32_t n_pt,
                             level_bufs &bufs, level_work &w)
{
    const uint64_t CLS_MIN = cls_min_groups();
    w.use_cls = w.n_groups >= CLS_MIN;
    // fused 1-block kernel handles the class-0 slice of each chunk on
    // the main stream (classes 1-3 keep the split assemble/hash
    // pipeline); meta/scratch are produced inside the fused kernel, so
    // updates/proof modes (which read them across kernels) disable it
    w.use_fused = w.use_cls && n_pt == 0 && in.updates_kind < 0 &&
                  getenv("SRE_NO_FUSED") == nullptr;
    if (w.use_cls && n_pt)
        HIP_CHECK(ctx, w.cinv.alloc((uint64_t)w.n_groups * 4));
    if (w.use_cls) {
        HIP_CHECK(ctx, w.perm.alloc((uint64_t)w.n_groups * 4));
        uint32_t nblk_max = (uint32_t)((w.chunk + CLS_BLOCK - 1) / CLS_BLOCK);
        HIP_CHECK(ctx, w.ccnt.alloc((uint64_t)4 * nblk_max * 4));
        HIP_CHECK(ctx, w.coff.alloc((uint64_t)4 * nblk_max * 4));
        for (uint64_t g0 = 0; g0 < w.n_groups; g0 += w.chunk) {
            uint32_t gc = (uint32_t)(w.n_groups - g0 < w.chunk ? w.n_groups - g0
                                                               : w.chunk);
            uint32_t nblk = (gc + CLS_BLOCK - 1) / CLS_BLOCK;
            LAUNCH(ctx, k_class_hist, nblk, CLS_BLOCK, ctx->stream,
                   bufs.gs.as<uint32_t>() + g0, gc, nblk, w.ccnt.as<uint32_t>());
            uint32_t tot = 0;
            if (scan_u32(ctx, w.ccnt.as<uint32_t>(), w.coff.as<uint32_t>(),
                         (uint64_t)4 * nblk, &tot))
                return -1;
            LAUNCH(ctx, k_class_scatter, nblk, CLS_BLOCK, ctx->stream,
                   bufs.gs.as<uint32_t>() + g0, gc, nblk, w.coff.as<uint32_t>(),
                   w.perm.as<uint32_t>() + g0,
                   n_pt ? w.cinv.as<uint32_t>() + g0 : nullptr);
            if (w.use_fused) { // class-0 count = start offset of class 1
                uint32_t c0 = 0;
                HIP_CHECK(ctx, hipMemcpy(&c0, w.coff.as<uint32_t>() + nblk, 4,
                                         hipMemcpyDeviceToHost));
                w.c0s.push_back(c0);
            }
        }
    }
    w.pipe2 = w.n_groups > w.chunk; // >1 chunk: overlap pays for 2nd buf
    if (w.pipe2) {
        HIP_CHECK(ctx, w.scratch2.alloc(w.chunk * SLOT_BR));
        HIP_CHECK(ctx, w.meta2.alloc(w.chunk * sizeof(br_meta)));
    }
    ctx->path_cnt[0] += w.use_cls;
    ctx->path_cnt[3] += w.pipe2;
    return 0;
}

// Branch pipeline over the level's groups, chunk by chunk: assemble ->
// (proof grab, update rows) -> hash, the fused kernel taking the class-0
// slice. Records timer start/stop around it on the main stream; the caller
// synchronises.
static int run_branch_chunks(sre_ctx *ctx, const level_in &in,
                             const proof_capture &proof, level_carry &carry,
                             level_bufs &bufs, level_work &w, EvTimer &timer)
{
    const int d = w.d;
    const uint64_t chunk = w.chunk;
    const bool pipe2 = w.pipe2, updates = in.updates_kind >= 0;
    uint32_t *gs = bufs.gs.as<uint32_t>();
    uint32_t *pend = carry.pend.as<uint32_t>();
    Event ev_asm[2] = {Event(hipEventDisableTiming), Event(hipEventDisableTiming)};
    Event ev_hash[2] = {Event(hipEventDisableTiming),
                        Event(hipEventDisableTiming)};
    // Plain-root calls defer the extension wraps of hashed non-root branches
    // to one k_branch_wrap at the end of the level (branch_tail). A wrap
    // needs d > P + 1 >= 1, so levels 0 and 1 have none. Only levels wide
    // enough for the class partition defer: below that gate a level is a
    // few waves, and the queue's memset and launch cost more than the
    // keccak_f they save (with the queue on every level the storage-bearing
    // incremental workload measured +0.15 ms per step). Updates
    // and proof calls keep every wrap inline; SRE_NO_DEFER_WRAP=1 forces
    // that (test gate, read per call). One job per group at most: 4 B per
    // group.
    wrap_queue wq;
    if (d >= 2 && w.use_cls && !updates && proof.n == 0 &&
        getenv("SRE_NO_DEFER_WRAP") == nullptr) {
        HIP_CHECK(ctx, w.wq_jobs.alloc((uint64_t)w.n_groups * 4));
        HIP_CHECK(ctx, w.wq_count.alloc(4));
        HIP_CHECK(ctx, hipMemsetAsync(w.wq_count.p, 0, 4, ctx->stream));
        wq.jobs = w.wq_jobs.as<uint32_t>();
        wq.count = w.wq_count.as<uint32_t>();
        wq.cap = w.n_groups;
    }
    // stream2 must not outrun state main-stream work this level depends
    // on (idx, gs, perm are ready once the partition above completes)
    HIP_CHECK(ctx, hipEventRecord(ev_hash[0].ev, ctx->stream));
    HIP_CHECK(ctx, hipEventRecord(ev_hash[1].ev, ctx->stream));
    HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream2, ev_hash[0].ev, 0));
    int chunk_i = 0;
    HIP_CHECK(ctx, timer.start(ctx->stream));
    for (uint64_t g0 = 0; g0 < w.n_groups; g0 += chunk, ++chunk_i) {
        uint32_t gc = (uint32_t)(w.n_groups - g0 < chunk ? w.n_groups - g0
                                                         : chunk);
        int buf = chunk_i & 1;
        uint8_t *scr = (pipe2 && buf) ? w.scratch2.as<uint8_t>()
                                      : bufs.scratch.as<uint8_t>();
        br_meta *mt = (pipe2 && buf) ? w.meta2.as<br_meta>()
                                     : bufs.meta.as<br_meta>();
        // class-0 slice -> fused kernel (main stream); classes 1-3 ->
        // split assemble (stream2) / hash (main), overlapped
        uint32_t c0 = w.use_fused ? w.c0s[chunk_i] : 0;
        uint32_t gsplit = gc - c0;
        // split the fused class-0 work across both streams so it
        // overlaps the split hash instead of serializing on main:
        // main runs fused[0,c0m) then (after the assemble event) the
        // split hash; stream2 runs assemble then fused[c0m,c0)
        uint32_t c0m = (pipe2 && gsplit) ? (uint32_t)((uint64_t)c0 * 55 / 100)
                                         : c0;
        uint32_t c0t = c0 - c0m;
        ctx->path_cnt[1] += c0;
        ctx->path_cnt[2]++;
        uint32_t *d_perm = w.use_cls ? w.perm.as<uint32_t>() + g0 + c0 : nullptr;
        hipStream_t s_asm = pipe2 ? ctx->stream2 : ctx->stream;
        if (pipe2) // wait until the hash consuming this buffer finished
            HIP_CHECK(ctx, hipStreamWaitEvent(s_asm, ev_hash[buf].ev, 0));
        if (gsplit)
            LAUNCH(ctx, k_branch_assemble, (gsplit + BLOCK_A - 1) / BLOCK_A,
                   BLOCK_A, s_asm, in.recs, w.idx, gs + g0, gsplit, in.lcp, in.keys,
                   in.key_stride, d, scr, chunk, mt, d_perm, in.err);
        if (pipe2)
            HIP_CHECK(ctx, hipEventRecord(ev_asm[buf].ev, s_asm));
        if (c0m)
            LAUNCH(ctx, k_branch_fused1, grid_for(c0m), BLOCK, ctx->stream, w.idx,
                   gs + g0, c0m, in.lcp, in.keys, in.key_stride, d, in.subtree,
                   in.recs, in.depths, in.n, w.perm.as<uint32_t>() + g0,
                   in.seg_roots,
                   in.child_refs, in.child_lens, pend, in.err, in.seg_by_slot,
                   wq);
        if (c0t)
            LAUNCH(ctx, k_branch_fused1, grid_for(c0t), BLOCK, s_asm, w.idx,
                   gs + g0, c0t, in.lcp, in.keys, in.key_stride, d, in.subtree,
                   in.recs, in.depths, in.n,
                   w.perm.as<uint32_t>() + g0 + c0m, in.seg_roots,
                   in.child_refs, in.child_lens, pend, in.err, in.seg_by_slot,
                   wq);
        if (pipe2)
            HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, ev_asm[buf].ev, 0));
        if (proof.n) // multiproof: copy path-node RLPs out of scratch
            LAUNCH(ctx, k_proof_grab, (proof.n + BLOCK - 1) / BLOCK, BLOCK,
                   ctx->stream, in.recs, w.idx, gs + g0, gc, mt, scr, chunk,
                   w.use_cls ? w.cinv.as<uint32_t>() + g0 : nullptr, in.keys,
                   in.key_stride, proof.pti, proof.pti2, proof.n, proof.rows,
                   proof.row_count, proof.row_cap, in.err);
        if (updates) {
            // emit BEFORE hashing: children's bhash entries must not yet
            // be overwritten by this level's nodes (shared leftmost s)
            HIP_CHECK(ctx, hipMemsetAsync(bufs.urow_cnt.p, 0, 4, ctx->stream));
            LAUNCH(ctx, k_emit_updates, grid_for(gc), BLOCK, ctx->stream,
                   in.recs, w.idx, gs + g0, gc, mt, in.keys, in.key_stride, in.bhash,
                   in.updates_kind, bufs.urows.as<sre_update_row>(),
                   bufs.urow_cnt.as<uint32_t>(), d_perm,
                   bufs.urowidx.as<uint32_t>(), in.seg_by_slot);
        }
        if (gsplit)
            LAUNCH(ctx, k_branch_hash, grid_for(gsplit), BLOCK, ctx->stream, scr,
                   chunk, mt, gsplit, in.keys, in.key_stride, in.subtree,
                   in.recs, in.depths, in.n, in.seg_roots, in.child_refs,
                   in.child_lens, pend, in.err, in.bhash,
                   updates ? bufs.urows.as<sre_update_row>() : nullptr,
                   updates ? bufs.urowidx.as<uint32_t>() : nullptr,
                   in.seg_by_slot, wq);
        if (pipe2)
            HIP_CHECK(ctx, hipEventRecord(ev_hash[buf].ev, ctx->stream));
        if (updates) {
            uint32_t nrows = 0;
            HIP_CHECK(ctx, hipMemcpy(&nrows, bufs.urow_cnt.p, 4,
                                     hipMemcpyDeviceToHost));
            if (nrows) {
                size_t old_sz = ctx->updates.size();
                ctx->updates.resize(old_sz + nrows);
                HIP_CHECK(ctx, hipMemcpy(ctx->updates.data() + old_sz,
                                         bufs.urows.p,
                                         (uint64_t)nrows * sizeof(sre_update_row),
                                         hipMemcpyDeviceToHost));
            }
        }
    }
    if (pipe2) { // trailing stream2 fused work must land before the
                 // level's outputs are consumed
        HIP_CHECK(ctx, hipEventRecord(ev_asm[0].ev, ctx->stream2));
        HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, ev_asm[0].ev, 0));
    }
    if (wq.jobs && w.n_groups) { // every producer of the queue is ordered before this
        const uint32_t grid = grid_for(w.n_groups);
        LAUNCH(ctx, k_branch_wrap, grid < 2048 ? grid : 2048, BLOCK, ctx->stream,
               wq, d, in.keys, in.key_stride, in.recs, in.depths, in.n, pend,
               in.err);
    }
    HIP_CHECK(ctx, timer.stop(ctx->stream));
    return 0;
}

static int run_levels(sre_ctx *ctx, const level_in &in, pass_out *po,
                      const cell_capture &cap = {},
                      const proof_capture &proof = {})
{
    const uint32_t *hist_host = in.hist_host;
    int maxd = -1;
    for (int d = 63; d >= 0; --d)
        if (hist_host[d + 1]) {
            maxd = d;
            break;
        }
    if (maxd < 0)
        return 0; // every leaf was already a segment root

    level_carry carry(ctx);
    level_bufs bufs(ctx);
    HIP_CHECK(ctx, carry.pend.alloc(66 * 4));
    HIP_CHECK(ctx, hipMemsetAsync(carry.pend.p, 0, 66 * 4, ctx->stream));
    const uint64_t nw = (in.n + LV_SPAN - 1) / LV_SPAN;
    HIP_CHECK(ctx, bufs.lcnt.alloc(2 * nw * 4));
    HIP_CHECK(ctx, bufs.loff.alloc(2 * nw * 4));
    uint64_t branch_blocks_base = po->branch_blocks;
    EvTimer timer;

    for (int d = maxd; d >= 0; --d) {
        // fresh leaves of depth d plus the branches placed for depth d
        uint64_t n_level = (uint64_t)hist_host[d + 1] + carry.pending_host[d + 1];
        if (n_level == 0)
            continue;
        po->levels++;
        level_work w(ctx);
        w.d = d;
        w.n_level = n_level;
        if (select_level(ctx, in, bufs, w))
            return -1;
        if (cap.depth > 0 && d == cap.depth - 1)
            LAUNCH(ctx, k_capture_L, grid_for(w.n_level), BLOCK, ctx->stream,
                   in.recs, w.idx, w.n_level, cap.rows, cap.count,
                   cap.capacity, in.err,
                   in.updates_kind >= 0 ? in.bhash : nullptr);
        if (partition_classes(ctx, in, proof.n, bufs, w) ||
            run_branch_chunks(ctx, in, proof, carry, bufs, w, timer))
            return -1;
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0;
        HIP_CHECK(ctx, timer.ms(&ms));
        po->branch_ms += ms;
        po->branch_count += w.n_groups;

        // pend[p+1] = nodes produced so far for depth p (complete for every
        // p the loop has yet to reach: parents lie strictly above), [65] =
        // keccak blocks
        HIP_CHECK(ctx, hipMemcpy(carry.pending_host, carry.pend.p, 66 * 4,
                                 hipMemcpyDeviceToHost));
        po->branch_blocks = branch_blocks_base + carry.pending_host[65];
    }
    return 0;
}

// ---------------------------------------------------------------------------
// passes
// ---------------------------------------------------------------------------

// A sorted storage array cut into per-account segments (one storage trie
// each): seg_id[i] = segment of entry i, lcp = neighbour common prefixes
// (segment-aware), seg_start / seg_acct = first entry / account index per
// segment.
struct storage_segs {
    DBuf flags, seg_id, lcp, seg_start, seg_acct;
    uint32_t n_seg = 0;
    explicit storage_segs(sre_ctx *c)
        : flags(c), seg_id(c), lcp(c), seg_start(c), seg_acct(c)
    {
    }
};

// sg.flags / sg.lcp are written: scan them into seg_id, seg_start and
// seg_acct. With `recs` (the storage pass, whose leaf kernel has run) also
// allocates seg_roots, n_seg being known only here, and stores the roots of
// the single-slot tries. An orphan segment is flagged in d_err; the stream
// is left unsynchronised.
static int segment_ids(sre_ctx *ctx, const sre_storage_entry *d_st, uint64_t ns,
                       uint32_t *d_err, storage_segs &sg,
                       const node_rec *recs = nullptr, DBuf *seg_roots = nullptr)
{
    // seg_id[i] = inclusive_scan(flags)[i] - 1 (segment index of entry i):
    // the exclusive scan here, the fix-up in k_seg_starts
    if (scan_u32(ctx, sg.flags.as<uint32_t>(), sg.seg_id.as<uint32_t>(), ns,
                 &sg.n_seg))
        return -1;
    HIP_CHECK(ctx, sg.seg_start.alloc((uint64_t)sg.n_seg * 4));
    HIP_CHECK(ctx, sg.seg_acct.alloc((uint64_t)sg.n_seg * 4));
    if (seg_roots)
        HIP_CHECK(ctx, seg_roots->alloc((uint64_t)sg.n_seg * 32));
    LAUNCH(ctx, k_seg_starts, grid_for(ns), BLOCK, ctx->stream,
           sg.flags.as<uint32_t>(), sg.seg_id.as<uint32_t>(), ns,
           sg.seg_start.as<uint32_t>(), sg.lcp.as<int8_t>(), recs,
           seg_roots ? seg_roots->as<uint8_t>() : nullptr);
    LAUNCH(ctx, k_seg_acct, grid_for(sg.n_seg), BLOCK, ctx->stream, d_st,
           sg.seg_start.as<uint32_t>(), sg.n_seg, ctx->acct.d, ctx->acct.n,
           sg.seg_acct.as<uint32_t>(), d_err);
    return 0;
}

static int alloc_segs(sre_ctx *ctx, uint64_t ns, storage_segs &sg)
{
    HIP_CHECK(ctx, sg.flags.alloc(ns * 4));
    HIP_CHECK(ctx, sg.seg_id.alloc(ns * 4));
    HIP_CHECK(ctx, sg.lcp.alloc(ns + 1));
    return 0;
}

// Segmentation on its own, for a caller that hashes no leaf
// (sre_root_from_nodes picks the tries to rebuild from it). Input-contract
// violations (unsorted/orphan entries) are flagged in d_err; nothing is
// synchronised here.
static int segment_storage(sre_ctx *ctx, const sre_storage_entry *d_st,
                           uint64_t ns, uint32_t *d_err, storage_segs &sg)
{
    if (alloc_segs(ctx, ns, sg))
        return -1;
    LAUNCH(ctx, k_seg_flags_lcp, grid_for(ns + 1), BLOCK, ctx->stream, d_st, ns,
           sg.flags.as<uint32_t>(), sg.lcp.as<int8_t>(), d_err);
    return segment_ids(ctx, d_st, ns, d_err, sg);
}

// Explicit storage entries for run_storage_pass's subset mode (incremental):
// the pass runs over them instead of the resident array and scatters roots
// into d_acct_roots WITHOUT resetting it first.
struct storage_subset {
    const sre_storage_entry *entries = nullptr;
    uint64_t n = 0;
};

static int run_storage_pass(sre_ctx *ctx, uint8_t *d_acct_roots, pass_out *po,
                            uint32_t *d_err, const proof_capture &proof = {},
                            const storage_subset &sub = {})
{
    const bool subset = sub.entries != nullptr;
    uint64_t ns = subset ? sub.n : ctx->st.n, na = ctx->acct.n;
    const sre_storage_entry *d_st = subset ? sub.entries : ctx->st.d;
    if (!subset)
        LAUNCH(ctx, k_fill_empty_roots, grid_for(na), BLOCK, ctx->stream,
               d_acct_roots, na);
    if (ns == 0)
        return 0;

    DBuf recs(ctx), depths(ctx), hist(ctx), seg_roots(ctx);
    HIP_CHECK(ctx, recs.alloc(ns * sizeof(node_rec)));
    HIP_CHECK(ctx, depths.alloc(ns));
    HIP_CHECK(ctx, hist.alloc(66 * 4));
    HIP_CHECK(ctx, hipMemsetAsync(hist.p, 0, 66 * 4, ctx->stream));
    storage_segs sg(ctx);
    if (alloc_segs(ctx, ns, sg))
        return -1;

    // the leaf kernel computes lcp and the segment flags itself; the ids
    // are scanned from the flags while nothing waits for them
    EvTimer leaf;
    HIP_CHECK(ctx, leaf.start(ctx->stream));
    LAUNCH(ctx, k_leaf_storage, grid_for(ns), BLOCK, ctx->stream, d_st, ns,
           sg.lcp.as<int8_t>(), sg.flags.as<uint32_t>(), recs.as<node_rec>(),
           depths.as<uint8_t>(), hist.as<uint32_t>(), d_err);
    HIP_CHECK(ctx, leaf.stop(ctx->stream));
    if (segment_ids(ctx, d_st, ns, d_err, sg, recs.as<node_rec>(), &seg_roots))
        return -1;
    const uint32_t n_seg = sg.n_seg;
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIP_CHECK(ctx, leaf.ms(&ms));
    po->leaf_ms += ms;
    po->leaf_count += ns;
    po->leaf_blocks += ns;
    // input-contract violations (unsorted/duplicate/orphan/zero-valued
    // entries) are flagged by the kernels above, and a rejected entry wrote
    // neither record nor depth byte: stop before any level selects over
    // unwritten slots
    if (check_err(ctx, d_err))
        return -1;

    uint32_t hist_host[66];
    HIP_CHECK(ctx, hipMemcpy(hist_host, hist.p, 66 * 4, hipMemcpyDeviceToHost));

    DBuf bhash(ctx);
    if (ctx->retain_updates)
        HIP_CHECK(ctx, bhash.alloc(ns * 32));
    size_t upd_start = ctx->updates.size();
    level_in in;
    in.n = ns;
    in.recs = recs.as<node_rec>();
    in.depths = depths.as<uint8_t>();
    in.lcp = sg.lcp.as<int8_t>();
    in.keys = (const uint8_t *)d_st + offsetof(sre_storage_entry, slot_key);
    in.key_stride = sizeof(sre_storage_entry);
    in.hist_host = hist_host;
    in.seg_roots = seg_roots.as<uint8_t>();
    in.seg_by_slot = sg.seg_id.as<uint32_t>();
    in.err = d_err;
    in.updates_kind = ctx->retain_updates ? 1 : -1;
    in.bhash = bhash.as<uint8_t>();
    if (run_levels(ctx, in, po, cell_capture{}, proof))
        return -1;
    if (ctx->retain_updates && ctx->updates.size() > upd_start) {
        // patch acct_key from the stashed seg ids: seg -> account index ->
        // 32-byte hashed key
        std::vector<uint32_t> seg_acct_h;
        if (to_host(ctx, seg_acct_h, sg.seg_acct, n_seg))
            return -1;
        std::vector<uint8_t> keys_h;
        // sparse incremental subset: fetch only the touched accounts' keys
        // instead of all na x 32 B
        bool sparse = subset && (uint64_t)n_seg * 8 <= na;
        if (!sparse) {
            // full pass (or dense subset): strided D2H of the key column
            keys_h.resize((uint64_t)na * 32);
            HIP_CHECK(ctx, hipMemcpy2D(keys_h.data(), 32, ctx->acct.d,
                                       sizeof(sre_account_entry), 32, na,
                                       hipMemcpyDeviceToHost));
        } else {
            keys_h.resize((uint64_t)n_seg * 32);
            for (uint32_t s2 = 0; s2 < n_seg; ++s2)
                HIP_CHECK(ctx, hipMemcpy(keys_h.data() + 32ull * s2,
                                         (const uint8_t *)&ctx->acct.d
                                             [seg_acct_h[s2]],
                                         32, hipMemcpyDeviceToHost));
        }
        for (size_t r = upd_start; r < ctx->updates.size(); ++r) {
            sre_update_row &row = ctx->updates[r];
            uint32_t seg;
            memcpy(&seg, row.pad_, 4);
            memset(row.pad_, 0, sizeof(row.pad_));
            memcpy(row.acct_key,
                   keys_h.data() + 32ull * (sparse ? seg : seg_acct_h[seg]),
                   32);
        }
    }

    LAUNCH(ctx, k_scatter_roots, grid_for(n_seg), BLOCK, ctx->stream,
           seg_roots.as<uint8_t>(), sg.seg_acct.as<uint32_t>(), n_seg,
           d_acct_roots);
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// Gather the [lo[t], hi[t]) intervals of the resident storage (n_iv of
// them; offs_host[t] = interval t's offset in the gathered array, [n_iv] =
// the total, nonzero) into a compact array and run the subset storage pass
// over it: fresh roots for exactly those tries, scattered into d_acct_roots.
static int run_storage_intervals(sre_ctx *ctx, const uint32_t *d_lo,
                                 const uint32_t *d_hi,
                                 const std::vector<uint32_t> &offs_host,
                                 uint8_t *d_acct_roots, pass_out *po,
                                 uint32_t *d_err)
{
    uint32_t n_iv = (uint32_t)offs_host.size() - 1;
    uint64_t total = offs_host[n_iv];
    DBuf doffs(ctx), compact(ctx);
    if (to_device(ctx, doffs, offs_host.data(), (uint64_t)n_iv + 1))
        return -1;
    HIP_CHECK(ctx, compact.alloc(total * sizeof(sre_storage_entry)));
    LAUNCH(ctx, k_gather_touched, grid_for(total), BLOCK, ctx->stream, ctx->st.d,
           d_lo, d_hi, doffs.as<uint32_t>(), n_iv, total,
           compact.as<sre_storage_entry>());
    return run_storage_pass(ctx, d_acct_roots, po, d_err, proof_capture{},
                            {compact.as<sre_storage_entry>(), total});
}

// Everything after the account leaf kernel: read the device histogram back,
// run the account trie's levels and clear the segment stash of the rows they
// emit (account rows carry no acct_key). bhash is allocated here when updates
// are retained, unless the caller seeded it. n_inputs: the histogram's total.
static int run_account_levels(sre_ctx *ctx, DBuf &recs, DBuf &depths,
                              const int8_t *lcp, DBuf &hist, DBuf &bhash,
                              int subtree, uint8_t *d_roots, uint8_t *d_child_refs,
                              uint8_t *d_child_lens, pass_out *po, uint32_t *d_err,
                              const cell_capture &cap = {},
                              const proof_capture &proof = {},
                              uint64_t *n_inputs = nullptr)
{
    uint64_t na = ctx->acct.n;
    uint32_t hist_host[66];
    HIP_CHECK(ctx, hipMemcpy(hist_host, hist.p, 66 * 4, hipMemcpyDeviceToHost));
    if (n_inputs)
        *n_inputs = std::accumulate(hist_host, hist_host + 66, (uint64_t)0);
    if (ctx->retain_updates && !bhash.p)
        HIP_CHECK(ctx, bhash.alloc(na * 32));
    size_t upd_start = ctx->updates.size();
    level_in in;
    in.n = na;
    in.recs = recs.as<node_rec>();
    in.depths = depths.as<uint8_t>();
    in.lcp = lcp;
    in.keys = (const uint8_t *)ctx->acct.d + offsetof(sre_account_entry, key);
    in.key_stride = sizeof(sre_account_entry);
    in.hist_host = hist_host;
    in.subtree = subtree;
    in.seg_roots = d_roots;
    in.child_refs = d_child_refs;
    in.child_lens = d_child_lens;
    in.err = d_err;
    in.updates_kind = ctx->retain_updates ? 0 : -1;
    in.bhash = bhash.as<uint8_t>();
    if (run_levels(ctx, in, po, cap, proof))
        return -1;
    if (ctx->retain_updates) {
        for (size_t r = upd_start; r < ctx->updates.size(); ++r)
            memset(ctx->updates[r].pad_, 0, sizeof(ctx->updates[r].pad_));
    }
    return 0;
}

static int run_account_pass(sre_ctx *ctx, const uint8_t *d_storage_roots, int subtree,
                            uint8_t *d_roots, uint8_t *d_child_refs,
                            uint8_t *d_child_lens, pass_out *po, uint32_t *d_err,
                            const cell_capture &cap = {},
                            const proof_capture &proof = {})
{
    uint64_t na = ctx->acct.n;
    DBuf lcp(ctx), recs(ctx), depths(ctx), hist(ctx);
    HIP_CHECK(ctx, lcp.alloc(na + 1));
    HIP_CHECK(ctx, recs.alloc(na * sizeof(node_rec)));
    HIP_CHECK(ctx, depths.alloc(na));
    HIP_CHECK(ctx, hist.alloc(66 * 4));
    HIP_CHECK(ctx, hipMemsetAsync(hist.p, 0, 66 * 4, ctx->stream));

    LAUNCH(ctx, k_lcp_account, grid_for(na + 1), BLOCK, ctx->stream, ctx->acct.d,
           na, subtree, lcp.as<int8_t>(), d_err);
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (check_err(ctx, d_err))
        return -1;

    EvTimer leaf;
    HIP_CHECK(ctx, leaf.start(ctx->stream));
    LAUNCH(ctx, k_leaf_account, grid_for(na), BLOCK, ctx->stream, ctx->acct.d, na,
           d_storage_roots, lcp.as<int8_t>(), subtree, recs.as<node_rec>(),
           depths.as<uint8_t>(), hist.as<uint32_t>(), d_roots, d_child_refs,
           d_child_lens, nullptr, nullptr, nullptr, 0);
    HIP_CHECK(ctx, leaf.stop(ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIP_CHECK(ctx, leaf.ms(&ms));
    po->leaf_ms += ms;
    po->leaf_count += na;
    po->leaf_blocks += 2 * na;
    // as in the storage pass: no level runs once an error is flagged
    if (check_err(ctx, d_err))
        return -1;

    DBuf bhash(ctx);
    return run_account_levels(ctx, recs, depths, lcp.as<int8_t>(), hist, bhash,
                              subtree, d_roots, d_child_refs, d_child_lens, po,
                              d_err, cap, proof);
}

// A cell-top capture armed for one account pass (dirty-path retention):
// rows go to ctx->cap_rows, grown to fit na accounts, their count to cnt.
struct armed_capture {
    sre_ctx *ctx;
    DBuf cnt{ctx};
    cell_capture cap;
    int arm(uint64_t na);
    int read(); // after the pass: the captured row count, into ctx->cap_count
};

// capture-row capacity for a state of na accounts
static uint64_t cap_rows_for(uint64_t na)
{
    return 2 * (na < (uint64_t)N_CELLS ? na : (uint64_t)N_CELLS) + 8192;
}

int armed_capture::arm(uint64_t na)
{
    if (ctx->cap_rows.grow(ctx, cap_rows_for(na), sizeof(cap_row)))
        return -1;
    HIP_CHECK(ctx, cnt.alloc(4));
    HIP_CHECK(ctx, hipMemsetAsync(cnt.p, 0, 4, ctx->stream));
    cap = {CELL_NIBBLES, (cap_row *)ctx->cap_rows.p, cnt.as<uint32_t>(),
           ctx->cap_rows.cap};
    return 0;
}

int armed_capture::read()
{
    uint32_t n = 0;
    HIP_CHECK(ctx, hipMemcpy(&n, cnt.p, 4, hipMemcpyDeviceToHost));
    ctx->cap_count = n;
    return 0;
}

// What a root-type entry point carries through its passes: the device error
// flag, the pass totals and the whole-call timer. start_timer() and arm_err()
// stand where each entry point starts its clock and first needs its flag.
struct root_call {
    sre_ctx *ctx;
    DBuf err{ctx};
    pass_out po;
    std::optional<EvTimer> whole; // created by start_timer(), on ctx->device
    uint32_t *flag() { return err.as<uint32_t>(); }
    int begin(bool zero_stats) { return begin_call(ctx, zero_stats); }
    int start_timer()
    {
        HIP_CHECK(ctx, whole.emplace().start(ctx->stream));
        return 0;
    }
    int arm_err() { return alloc_err_flag(ctx, err); }
    int publish() // stop the clock, drain the stream, publish the stats
    {
        HIP_CHECK(ctx, whole->stop(ctx->stream));
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        float total = 0;
        HIP_CHECK(ctx, whole->ms(&total));
        ctx->stats.total_ms = total;
        ctx->stats.leaf_hash_ms = po.leaf_ms;
        ctx->stats.leaf_count = po.leaf_count;
        ctx->stats.leaf_blocks = po.leaf_blocks;
        ctx->stats.branch_hash_ms = po.branch_ms;
        ctx->stats.branch_count = po.branch_count;
        ctx->stats.branch_blocks = po.branch_blocks;
        ctx->stats.levels = po.levels;
        return 0;
    }
    // the flag must be clean
    int finish() { return check_err(ctx, flag()) ? -1 : publish(); }
};

// The one vocabulary of validation failures (sre.h "Failed calls"): device
// flags and host-side checks both report through here, so one kind of bad
// input reads the same whichever merge path caught it.
static int fail_flags(sre_ctx *ctx, uint32_t e)
{
    std::string msg = "input/engine error:";
    if (e & (1u << E_UNSORTED_ACCT))
        msg += " accounts-not-sorted";
    if (e & (1u << E_UNSORTED_STORAGE))
        msg += " storage-not-sorted-or-duplicate";
    if (e & (1u << E_ORPHAN_STORAGE))
        msg += " storage-for-unknown-account";
    if (e & (1u << E_ZERO_VALUE))
        msg += " zero-storage-value";
    if (e & (1u << E_DUP_ADDRESS))
        msg += " duplicate-address";
    if (e & (1u << E_DUP_STORAGE))
        msg += " duplicate-storage-slot";
    if (e & (1u << E_INTERNAL))
        msg += " internal-group-invariant";
    set_err(ctx, msg);
    return -1;
}

static int check_err(sre_ctx *ctx, uint32_t *d_err)
{
    uint32_t e = 0;
    HIP_CHECK(ctx, hipMemcpy(&e, d_err, 4, hipMemcpyDeviceToHost));
    return e ? fail_flags(ctx, e) : 0;
}

static const uint8_t EMPTY_ROOT_H[32] = {
    0x56, 0xe8, 0x1f, 0x17, 0x1b, 0xcc, 0x55, 0xa6, 0xff, 0x83, 0x45, 0xe6,
    0x92, 0xc0, 0xf8, 0x6e, 0x5b, 0x48, 0xe0, 0x1b, 0x99, 0x6c, 0xad, 0xc0,
    0x01, 0x62, 0x2f, 0xb5, 0xe3, 0x63, 0xb4, 0x21,
};

// No accounts: the empty root, or an error when storage rows are resident.
static int empty_state_root(sre_ctx *ctx, uint8_t out_root[32])
{
    if (ctx->st.n != 0) {
        set_err(ctx, "storage entries without accounts");
        return -1;
    }
    memcpy(out_root, EMPTY_ROOT_H, 32);
    return 0;
}

// ---------------------------------------------------------------------------
// multiproofs (sre_account_proof / sre_storage_proof). The device side
// captures each target's path branches during an ordinary pass; the node
// lists are assembled on the host (proof_host.h).
// ---------------------------------------------------------------------------
// Target keys -> index in a resident sorted array + presence flag: 32-byte
// keys against the accounts, 64-byte (account || slot) pairs against the
// storage rows.
struct proof_lookup {
    uint32_t n = 0;
    DBuf dkeys, dti, dpres;
    std::vector<uint32_t> ti, pres;
    explicit proof_lookup(sre_ctx *c) : dkeys(c), dti(c), dpres(c) {}
};

static int proof_lookup_launch(sre_ctx *ctx, proof_lookup &l,
                               const uint8_t *keys, uint32_t klen, uint32_t n_t)
{
    l.n = n_t;
    if (to_device(ctx, l.dkeys, keys, (uint64_t)klen * n_t))
        return -1;
    HIP_CHECK(ctx, l.dti.alloc(4ull * n_t));
    HIP_CHECK(ctx, l.dpres.alloc(4ull * n_t));
    if (klen == 32)
        LAUNCH(ctx, k_proof_ti, grid_for(n_t), BLOCK, ctx->stream, ctx->acct.d,
               ctx->acct.n, l.dkeys.as<uint8_t>(), n_t, l.dti.as<uint32_t>(),
               l.dpres.as<uint32_t>());
    else
        LAUNCH(ctx, k_proof_ti64, grid_for(n_t), BLOCK, ctx->stream, ctx->st.d,
               ctx->st.n, l.dkeys.as<uint8_t>(), n_t, l.dti.as<uint32_t>(),
               l.dpres.as<uint32_t>());
    return 0;
}

static int proof_lookup_fetch(sre_ctx *ctx, proof_lookup &l)
{
    if (to_host(ctx, l.ti, l.dti, l.n) || to_host(ctx, l.pres, l.dpres, l.n))
        return -1;
    return 0;
}

// What both proof calls do around their pass: arm() sets up the row capture
// for the looked-up targets, collect() brings the captured rows back grouped
// per target, emit() assembles one target's proof into the caller's buffers.
struct proof_call {
    sre_ctx *ctx;
    const std::string name; // the entry point, for its error messages
    const std::string full = name + ": output capacity exceeded";
    DBuf err, acct_roots; // the pass's error flag and storage roots
    proof_lookup tgt;
    DBuf dti2, drows, dcount;
    proof_capture cap;
    std::vector<proof_row> rows;
    std::vector<std::vector<const proof_row *>> per; // root-first
    proof_sink out;

    proof_call(sre_ctx *c, const char *fn, uint8_t *out_nodes,
               uint64_t cap_nodes, uint32_t *out_lens, uint64_t cap_lens)
        : ctx(c), name(fn), err(c), acct_roots(c), tgt(c), dti2(c), drows(c),
          dcount(c),
          out{out_nodes, cap_nodes, out_lens, cap_lens, full.c_str()}
    {
    }

    int begin()
    {
        if (alloc_err_flag(ctx, err))
            return -1;
        HIP_CHECK(ctx, acct_roots.alloc(ctx->acct.n * 32));
        return 0;
    }

    int arm()
    {
        uint32_t n_t = tgt.n;
        // exclusion targets also need the LEFT neighbour's path: a target
        // that sorts after every key of the divergent subtree has its lookup
        // path under index ti-1, not ti
        {
            std::vector<uint32_t> ti2(n_t);
            for (uint32_t t = 0; t < n_t; ++t)
                ti2[t] = (!tgt.pres[t] && tgt.ti[t] > 0) ? tgt.ti[t] - 1
                                                         : tgt.ti[t];
            if (to_device(ctx, dti2, ti2.data(), n_t))
                return -1;
        }
        uint32_t cap_rows = n_t * 260 + 64;
        HIP_CHECK(ctx, drows.alloc((uint64_t)cap_rows * sizeof(proof_row)));
        HIP_CHECK(ctx, dcount.alloc(4));
        HIP_CHECK(ctx, hipMemsetAsync(dcount.p, 0, 4, ctx->stream));
        cap.pti = tgt.dti.as<uint32_t>();
        cap.pti2 = dti2.as<uint32_t>();
        cap.n = n_t;
        cap.rows = drows.as<proof_row>();
        cap.row_count = dcount.as<uint32_t>();
        cap.row_cap = cap_rows;
        return 0;
    }

    int collect()
    {
        if (check_err(ctx, err.as<uint32_t>()))
            return -1;
        uint32_t nrows = 0;
        HIP_CHECK(ctx, hipMemcpy(&nrows, dcount.p, 4, hipMemcpyDeviceToHost));
        if (to_host(ctx, rows, drows, nrows))
            return -1;
        per.resize(tgt.n);
        for (const auto &r : rows)
            per[r.target].push_back(&r);
        for (auto &v : per)
            std::sort(v.begin(), v.end(),
                      [](const proof_row *a, const proof_row *b) {
                          return a->d < b->d;
                      });
        return 0;
    }

    // nibble at which the leaf at entry index idx starts on target t's path:
    // one below the deepest captured branch that has idx among its members
    int leaf_from(uint32_t t, uint32_t idx) const
    {
        int dmax = -1;
        for (const proof_row *r : per[t])
            if (r->s <= idx && idx < r->e && r->d > dmax)
                dmax = r->d;
        return dmax + 1;
    }

    int emit(uint32_t t, const uint8_t root[32], const uint8_t *key,
             const std::vector<std::vector<uint8_t>> &leaves,
             uint32_t *out_counts)
    {
        uint32_t cnt = 0;
        const char *why = nullptr;
        int rc = proof_assemble(root, key, per[t], leaves, out, &cnt, &why);
        if (rc < 0) {
            set_err(ctx, why);
            return -1;
        }
        if ((rc == 0) != (tgt.pres[t] != 0)) {
            set_err(ctx, name + ": internal presence mismatch");
            return -1;
        }
        out_counts[t] = cnt;
        return 0;
    }
};

extern "C" int sre_account_proof(sre_ctx *ctx, const uint8_t *targets,
                                 uint64_t n_targets, uint8_t *out_nodes,
                                 uint64_t cap_nodes, uint32_t *out_lens,
                                 uint64_t cap_lens, uint32_t *out_counts)
{
    if (begin_call(ctx, false))
        return -1;
    if (n_targets == 0 || n_targets > 4096) {
        set_err(ctx, "sre_account_proof: 1..4096 targets");
        return -1;
    }
    if (ctx->acct.n == 0) { // empty trie: every proof is the empty node list
        for (uint64_t t = 0; t < n_targets; ++t)
            out_counts[t] = 0;
        return 0;
    }
    uint32_t n_t = (uint32_t)n_targets;
    proof_call pc(ctx, "sre_account_proof", out_nodes, cap_nodes, out_lens,
                  cap_lens);
    DBuf root(ctx);
    if (pc.begin())
        return -1;
    HIP_CHECK(ctx, root.alloc(32));
    if (proof_lookup_launch(ctx, pc.tgt, targets, 32, n_t) ||
        proof_lookup_fetch(ctx, pc.tgt) || pc.arm())
        return -1;
    uint8_t *acct_roots = pc.acct_roots.as<uint8_t>();
    uint32_t *d_err = pc.err.as<uint32_t>();

    // the capture rides on the account pass
    pass_out po;
    if (run_storage_pass(ctx, acct_roots, &po, d_err))
        return -1;
    if (run_account_pass(ctx, acct_roots, 0, root.as<uint8_t>(), nullptr,
                         nullptr, &po, d_err, cell_capture{}, pc.cap))
        return -1;
    if (pc.collect())
        return -1;
    uint8_t engine_root[32];
    HIP_CHECK(ctx, hipMemcpy(engine_root, root.p, 32, hipMemcpyDeviceToHost));

    const std::vector<uint32_t> &ti = pc.tgt.ti, &pres = pc.tgt.pres;
    for (uint32_t t = 0; t < n_t; ++t) {
        // candidate leaves: the accounts at ti / ti-1
        uint32_t cands[2];
        int ncand = 0;
        cands[ncand++] = ti[t] < ctx->acct.n ? ti[t] : (uint32_t)(ctx->acct.n - 1);
        if (!pres[t] && ti[t] > 0 && ti[t] - 1 != cands[0])
            cands[ncand++] = ti[t] - 1;
        std::vector<std::vector<uint8_t>> leaves;
        for (int c = 0; c < ncand; ++c) {
            uint32_t idx = cands[c];
            sre_account_entry ae;
            uint8_t sroot[32];
            HIP_CHECK(ctx,
                      hipMemcpy(&ae,
                                (const uint8_t *)ctx->acct.d +
                                    (uint64_t)idx * sizeof(sre_account_entry),
                                sizeof(ae), hipMemcpyDeviceToHost));
            HIP_CHECK(ctx, hipMemcpy(sroot, acct_roots + 32ull * idx, 32,
                                     hipMemcpyDeviceToHost));
            leaves.emplace_back(200);
            leaves.back().resize(h_leaf_node(leaves.back().data(), ae.key,
                                             pc.leaf_from(t, idx), &ae, sroot));
        }
        if (pc.emit(t, engine_root, targets + 32ull * t, leaves, out_counts))
            return -1;
    }
    return 0;
}

/* Storage multiproof: per (acct_key, slot_key) PRESENT pair, the storage
 * root and the root-first node list of that account's storage trie —
 * StorageProof::storage_multiproof (crates/trie/trie/src/proof/mod.rs)
 * restricted to present slots, same v1 limits as sre_account_proof. */
extern "C" int sre_storage_proof(sre_ctx *ctx, const uint8_t *acct_keys,
                                 const uint8_t *slot_keys, uint64_t n_targets,
                                 uint8_t *out_roots, uint8_t *out_nodes,
                                 uint64_t cap_nodes, uint32_t *out_lens,
                                 uint64_t cap_lens, uint32_t *out_counts)
{
    if (begin_call(ctx, false))
        return -1;
    if (ctx->acct.n == 0 || ctx->st.n == 0) {
        set_err(ctx, "sre_storage_proof: no storage resident");
        return -1;
    }
    if (n_targets == 0 || n_targets > 4096) {
        set_err(ctx, "sre_storage_proof: 1..4096 targets");
        return -1;
    }
    uint32_t n_t = (uint32_t)n_targets;
    std::vector<uint8_t> pairs(64ull * n_t);
    for (uint32_t t = 0; t < n_t; ++t) {
        memcpy(pairs.data() + 64ull * t, acct_keys + 32ull * t, 32);
        memcpy(pairs.data() + 64ull * t + 32, slot_keys + 32ull * t, 32);
    }
    proof_call pc(ctx, "sre_storage_proof", out_nodes, cap_nodes, out_lens,
                  cap_lens);
    proof_lookup owner(ctx); // account indices (for the per-target storage root)
    if (pc.begin() ||
        proof_lookup_launch(ctx, pc.tgt, pairs.data(), 64, n_t) ||
        proof_lookup_launch(ctx, owner, acct_keys, 32, n_t) ||
        proof_lookup_fetch(ctx, pc.tgt) || proof_lookup_fetch(ctx, owner) ||
        pc.arm())
        return -1;

    // the capture rides on the storage pass
    pass_out po;
    if (run_storage_pass(ctx, pc.acct_roots.as<uint8_t>(), &po,
                         pc.err.as<uint32_t>(), pc.cap))
        return -1;
    if (pc.collect())
        return -1;

    const std::vector<uint32_t> &ti = pc.tgt.ti, &pres = pc.tgt.pres;
    for (uint32_t t = 0; t < n_t; ++t) {
        uint8_t sroot[32];
        // absent accounts are NOT an error: storage_multiproof returns
        // StorageMultiProof::empty() for them (proof/mod.rs storage_multiproof
        // short-circuits on an empty storage cursor), i.e. EMPTY_ROOT_HASH +
        // an empty node list — same as a present storage-less account.
        if (!owner.pres[t]) {
            memcpy(out_roots + 32ull * t, EMPTY_ROOT_H, 32);
            out_counts[t] = 0;
            continue;
        }
        HIP_CHECK(ctx, hipMemcpy(sroot,
                                 pc.acct_roots.as<uint8_t>() +
                                     32ull * owner.ti[t],
                                 32, hipMemcpyDeviceToHost));
        memcpy(out_roots + 32ull * t, sroot, 32);
        if (memcmp(sroot, EMPTY_ROOT_H, 32) == 0) {
            // account has no storage: the empty node list proves absence
            if (pres[t]) {
                set_err(ctx, "sre_storage_proof: internal presence mismatch");
                return -1;
            }
            out_counts[t] = 0;
            continue;
        }
        // candidate slot leaves at ti / ti-1, guarded to THIS account's
        // segment (a neighbour index may belong to another storage trie)
        uint32_t cands[2];
        int ncand = 0;
        if (ti[t] < ctx->st.n)
            cands[ncand++] = ti[t];
        if (!pres[t] && ti[t] > 0)
            cands[ncand++] = ti[t] - 1;
        std::vector<std::vector<uint8_t>> leaves;
        for (int c = 0; c < ncand; ++c) {
            uint32_t idx = cands[c];
            sre_storage_entry se;
            HIP_CHECK(ctx,
                      hipMemcpy(&se,
                                (const uint8_t *)ctx->st.d +
                                    (uint64_t)idx * sizeof(sre_storage_entry),
                                sizeof(se), hipMemcpyDeviceToHost));
            if (memcmp(se.acct_key, acct_keys + 32ull * t, 32) != 0)
                continue; // other account's segment
            leaves.emplace_back(96);
            leaves.back().resize(h_storage_leaf(leaves.back().data(),
                                                se.slot_key,
                                                pc.leaf_from(t, idx), se.value));
        }
        if (pc.emit(t, sroot, slot_keys + 32ull * t, leaves, out_counts))
            return -1;
    }
    return 0;
}

extern "C" int sre_root(sre_ctx *ctx, uint8_t out_root[32])
{
    root_call f{ctx};
    if (f.begin(true))
        return -1;
    if (ctx->acct.n == 0)
        return empty_state_root(ctx, out_root);
    DBuf acct_roots(ctx), root(ctx);
    if (f.start_timer() || f.arm_err())
        return -1;
    HIP_CHECK(ctx, acct_roots.alloc(ctx->acct.n * 32));
    HIP_CHECK(ctx, root.alloc(32));

    if (run_storage_pass(ctx, acct_roots.as<uint8_t>(), &f.po, f.flag()) ||
        run_account_pass(ctx, acct_roots.as<uint8_t>(), 0, root.as<uint8_t>(),
                         nullptr, nullptr, &f.po, f.flag()) ||
        f.finish())
        return -1;
    HIP_CHECK(ctx, hipMemcpy(out_root, root.p, 32, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sre_storage_roots(sre_ctx *ctx, uint8_t *out, uint64_t n)
{
    root_call f{ctx}; // untimed, and the previous call's stats stay
    if (f.begin(false))
        return -1;
    if (n != ctx->acct.n) {
        set_err(ctx, "sre_storage_roots: n != uploaded account count");
        return -1;
    }
    if (n == 0)
        return 0;
    DBuf acct_roots(ctx);
    if (f.arm_err())
        return -1;
    HIP_CHECK(ctx, acct_roots.alloc(ctx->acct.n * 32));
    if (run_storage_pass(ctx, acct_roots.as<uint8_t>(), &f.po, f.flag()) ||
        check_err(ctx, f.flag()))
        return -1;
    HIP_CHECK(ctx, hipMemcpy(out, acct_roots.p, ctx->acct.n * 32, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sre_subtree_roots(sre_ctx *ctx, uint8_t out_child_refs[16][33],
                                 uint8_t out_child_lens[16],
                                 uint8_t out_root_hash[16][32], uint64_t out_counts[16])
{
    root_call f{ctx};
    if (f.begin(true))
        return -1;
    memset(out_child_lens, 0, 16);
    memset(out_counts, 0, 16 * 8);
    if (ctx->acct.n == 0)
        return 0;
    DBuf acct_roots(ctx), roots(ctx), crefs(ctx), clens(ctx), counts(ctx);
    if (f.start_timer() || f.arm_err())
        return -1;
    HIP_CHECK(ctx, acct_roots.alloc(ctx->acct.n * 32));
    HIP_CHECK(ctx, roots.alloc(16 * 32));
    HIP_CHECK(ctx, crefs.alloc(16 * 33));
    HIP_CHECK(ctx, clens.alloc(16));
    HIP_CHECK(ctx, counts.alloc(16 * 8));
    HIP_CHECK(ctx, hipMemsetAsync(clens.p, 0, 16, ctx->stream));
    HIP_CHECK(ctx, hipMemsetAsync(counts.p, 0, 16 * 8, ctx->stream));
    // zero refs/roots too: pool-recycled buffers hold stale bytes, and rows
    // for absent nibbles must come back deterministically zeroed
    HIP_CHECK(ctx, hipMemsetAsync(crefs.p, 0, 16 * 33, ctx->stream));
    HIP_CHECK(ctx, hipMemsetAsync(roots.p, 0, 16 * 32, ctx->stream));

    if (run_storage_pass(ctx, acct_roots.as<uint8_t>(), &f.po, f.flag()) ||
        run_account_pass(ctx, acct_roots.as<uint8_t>(), 1, roots.as<uint8_t>(),
                         crefs.as<uint8_t>(), clens.as<uint8_t>(), &f.po,
                         f.flag()))
        return -1;
    LAUNCH(ctx, k_nibble_counts, grid_for(ctx->acct.n), BLOCK, ctx->stream,
           ctx->acct.d, ctx->acct.n, counts.as<uint64_t>());
    if (f.finish())
        return -1;
    HIP_CHECK(ctx, hipMemcpy(out_child_refs, crefs.p, 16 * 33, hipMemcpyDeviceToHost));
    HIP_CHECK(ctx, hipMemcpy(out_child_lens, clens.p, 16, hipMemcpyDeviceToHost));
    HIP_CHECK(ctx, hipMemcpy(out_root_hash, roots.p, 16 * 32, hipMemcpyDeviceToHost));
    HIP_CHECK(ctx, hipMemcpy(out_counts, counts.p, 16 * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sre_finish_top(sre_ctx *ctx, const uint8_t child_refs[16][33],
                              const uint8_t child_lens[16],
                              const uint8_t root_hash[16][32],
                              const uint64_t counts[16], uint8_t out_root[32])
{
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    (void)counts;
    int populated = 0, last = -1;
    for (int b = 0; b < 16; ++b)
        if (child_lens[b]) {
            populated++;
            last = b;
        }
    if (populated == 0) {
        memcpy(out_root, EMPTY_ROOT_H, 32);
        return 0;
    }
    if (populated == 1) {
        memcpy(out_root, root_hash[last], 32);
        return 0;
    }
    DBuf crefs(ctx), clens(ctx), root(ctx);
    HIP_CHECK(ctx, crefs.alloc(16 * 33));
    HIP_CHECK(ctx, clens.alloc(16));
    HIP_CHECK(ctx, root.alloc(32));
    HIP_CHECK(ctx, hipMemcpy(crefs.p, child_refs, 16 * 33, hipMemcpyHostToDevice));
    HIP_CHECK(ctx, hipMemcpy(clens.p, child_lens, 16, hipMemcpyHostToDevice));
    LAUNCH(ctx, k_finish_top, 1, 64, ctx->stream, crefs.as<uint8_t>(),
           clens.as<uint8_t>(), root.as<uint8_t>());
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_CHECK(ctx, hipMemcpy(out_root, root.p, 32, hipMemcpyDeviceToHost));
    return 0;
}

// minimum resident ns for the closed-form small-delta storage merge;
// SRE_ST_SMALL_MIN overrides (tests lower it to cover the path on small
// states — the default keeps tiny states on the trivially-fast general
// path)
static uint64_t sds_min_ns()
{
    const char *e = getenv("SRE_ST_SMALL_MIN");
    return e ? (uint64_t)atoll(e) : (1ull << 20);
}

// Optional extras of a delta merge, and what it reports back.
struct merge_io {
    DBuf *map_out = nullptr; // old->new positions, (old na)+1 u32
    // carry retained storage roots across the merge (d_new_roots: new-na x
    // 32, pre-filled EMPTY by the caller)
    const uint8_t *d_old_roots = nullptr;
    uint8_t *d_new_roots = nullptr;
    bool st_closed_form = false; // result: the closed-form storage merge ran
};

// What the steps of the general delta merge share: the uploaded delta, the
// error flag, the destroyed accounts' keys and the merged arrays, which
// stay the DBufs' (so any failing return gives them back) until
// adopt_merged installs them.
struct delta_merge {
    sre_ctx *ctx;
    const sre_account_delta *acct_delta;
    uint64_t n_acct;
    const sre_storage_entry *st_delta;
    uint64_t n_st;
    DBuf dl_a{ctx}, dl_s{ctx}, err{ctx}, sdel{ctx}, new_acct{ctx}, new_st{ctx};
    uint32_t n_del = 0; // destroyed accounts (keys in sdel)
    uint64_t new_na = 0, new_ns = 0;
};

// Pool buffer for a merged array of n rows. The count meets the u32
// capacity contract (check_cap) before anything is allocated.
static int alloc_merged(sre_ctx *ctx, DBuf &out, uint64_t n, size_t row_bytes,
                        const char *oom)
{
    if (check_cap(ctx, n))
        return -1;
    if (out.alloc((n ? n : 1) * row_bytes) != hipSuccess) {
        set_err(ctx, oom);
        return -1;
    }
    return 0;
}

// The revert of the delta being merged, in temporaries until adopt_merged
// installs it (a rejected delta leaves the stored revert alone).
struct revert_tmp {
    sre_ctx *ctx;
    DBuf acct{ctx}, st{ctx};
    uint64_t na = 0, ns = 0;
    uint64_t cnt[4] = {0, 0, 0, 0};
    bool valid = false;
};

// Revert capture: read out of the resident arrays, before they are merged,
// the delta that undoes (dl_a, dl_s) — DESIGN.md §15, revert_plan.h. The
// same pass serves every merge path. The storage rows are not validated
// yet (the merges do that; on rejection rv is dropped): every index is
// bounded for any storage input. An unsorted account delta would let
// destroyed segments repeat and their u32 prefix sums wrap, so the host
// checks its order first and skips the pass; the merge then rejects.
static int capture_revert(sre_ctx *ctx, const sre_account_delta *acct_delta,
                          const sre_account_delta *dl_a, uint64_t n_acct,
                          const sre_storage_entry *dl_s, uint64_t n_st,
                          revert_tmp &rv)
{
    if (acct_delta_order(acct_delta, n_acct))
        return 0;
    uint64_t na = ctx->acct.n, ns = ctx->st.n;
    DBuf ka(ctx), fa(ctx), ea(ctx), sa(ctx), seglo(ctx), seglen(ctx), segsum(ctx),
        segp(ctx), ks(ctx), fs(ctx), es(ctx), ss(ctx), owner(ctx);
    HIP_CHECK(ctx, ka.alloc(n_acct * 4));
    HIP_CHECK(ctx, fa.alloc((n_acct + 1) * 4));
    HIP_CHECK(ctx, ea.alloc((n_acct + 1) * 4));
    HIP_CHECK(ctx, sa.alloc(n_acct * 4));
    HIP_CHECK(ctx, seglo.alloc(n_acct * 4));
    HIP_CHECK(ctx, seglen.alloc((n_acct + 1) * 4));
    HIP_CHECK(ctx, segsum.alloc((n_acct + 1) * 4));
    HIP_CHECK(ctx, segp.alloc(n_acct * 4));
    HIP_CHECK(ctx, ks.alloc(n_st * 4));
    HIP_CHECK(ctx, fs.alloc((n_st + 1) * 4));
    HIP_CHECK(ctx, es.alloc((n_st + 1) * 4));
    HIP_CHECK(ctx, ss.alloc(n_st * 4));
    HIP_CHECK(ctx, owner.alloc(n_st * 4));
    LAUNCH(ctx, k_rv_acct, grid_for(n_acct + 1), BLOCK, ctx->stream, ctx->acct.d,
           na, ctx->st.d, ns, dl_a, n_acct, ka.as<uint32_t>(), fa.as<uint32_t>(),
           sa.as<uint32_t>(), seglo.as<uint32_t>(), seglen.as<uint32_t>());
    LAUNCH(ctx, k_rv_st, grid_for(n_st + 1), BLOCK, ctx->stream, ctx->st.d, ns,
           ctx->acct.d, na, dl_a, n_acct, dl_s, n_st, ks.as<uint32_t>(),
           fs.as<uint32_t>(), ss.as<uint32_t>(), owner.as<uint32_t>());
    uint32_t ta = 0, ts = 0, wiped = 0;
    if (scan_u32(ctx, fa.as<uint32_t>(), ea.as<uint32_t>(), n_acct + 1, &ta) ||
        scan_u32(ctx, seglen.as<uint32_t>(), segsum.as<uint32_t>(), n_acct + 1,
                 &wiped) ||
        scan_u32(ctx, fs.as<uint32_t>(), es.as<uint32_t>(), n_st + 1, &ts))
        return -1;
    rv.na = ta;
    rv.ns = (uint64_t)ts + wiped;
    if (rv.acct.alloc(rv.na * sizeof(sre_account_delta)) != hipSuccess ||
        rv.st.alloc(rv.ns * sizeof(sre_storage_entry)) != hipSuccess) {
        set_err(ctx, "revert capture: out of memory");
        return -1;
    }
    if (ta)
        LAUNCH(ctx, k_rv_emit_acct, grid_for(n_acct), BLOCK, ctx->stream,
               ctx->acct.d, dl_a, n_acct, ka.as<uint32_t>(), ea.as<uint32_t>(),
               sa.as<uint32_t>(), rv.acct.as<sre_account_delta>());
    if (ts)
        LAUNCH(ctx, k_rv_emit_st, grid_for(n_st), BLOCK, ctx->stream, ctx->st.d,
               dl_s, n_st, ks.as<uint32_t>(), es.as<uint32_t>(),
               ss.as<uint32_t>(), owner.as<uint32_t>(), segsum.as<uint32_t>(),
               rv.st.as<sre_storage_entry>());
    if (wiped) {
        LAUNCH(ctx, k_rv_seg_base, grid_for(n_acct), BLOCK, ctx->stream, dl_a,
               n_acct, seglen.as<uint32_t>(), dl_s, n_st, segp.as<uint32_t>());
        bool wide = ((uintptr_t)ctx->st.d & 15) == 0;
        uint64_t lanes = sizeof(sre_storage_entry) / (wide ? 16 : 8);
        if (wide)
            LAUNCH(ctx, k_rv_copy_segs<uint4>, grid_for(wiped * lanes), BLOCK,
                   ctx->stream, ctx->st.d, segsum.as<uint32_t>(),
                   seglo.as<uint32_t>(), segp.as<uint32_t>(), n_acct,
                   (uint64_t)wiped, es.as<uint32_t>(),
                   rv.st.as<sre_storage_entry>());
        else
            LAUNCH(ctx, k_rv_copy_segs<uint64_t>, grid_for(wiped * lanes), BLOCK,
                   ctx->stream, ctx->st.d, segsum.as<uint32_t>(),
                   seglo.as<uint32_t>(), segp.as<uint32_t>(), n_acct,
                   (uint64_t)wiped, es.as<uint32_t>(),
                   rv.st.as<sre_storage_entry>());
    }
    // the index arrays above go back to the pool when this returns
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    rv.cnt[0] = ta;
    rv.cnt[1] = ts;
    rv.cnt[2] = wiped;
    rv.cnt[3] = (n_acct - ta) + (n_st - ts);
    rv.valid = true;
    return 0;
}

// Tail of every delta merge: the merged arrays become the resident state,
// and the captured revert (if any) the stored one.
// An empty st means the storage array was not merged and stays in place.
static void adopt_merged(sre_ctx *ctx, DBuf &acct, uint64_t na, DBuf &st,
                         uint64_t ns, revert_tmp &rv)
{
    if (rv.valid) {
        ctx->rv_acct.adopt(ctx, rv.acct, rv.na);
        ctx->rv_st.adopt(ctx, rv.st, rv.ns);
        memcpy(ctx->rv_cnt, rv.cnt, sizeof(rv.cnt));
        ctx->rv_have = true;
    }
    const size_t adopted[2] = {acct.sz, st.p ? st.sz : 0};
    ctx->acct.adopt(ctx, acct, na);
    if (st.p)
        ctx->st.adopt(ctx, st, ns);
    // prewarm the ping-pong partner buffers: the NEXT delta would otherwise
    // pay a multi-hundred-ms first-time hipMalloc of this size class inside
    // the caller's timed region
    for (size_t b : adopted) {
        DBuf spare(ctx);
        if (b)
            (void)spare.alloc(b);
    }
}

static int merge_accounts_general(delta_merge &m, const merge_io &io)
{
    sre_ctx *ctx = m.ctx;
    uint64_t nb = ctx->acct.n, n_acct = m.n_acct;
    const sre_account_delta *dl_a = m.dl_a.as<sre_account_delta>();
    uint32_t *d_err = m.err.as<uint32_t>();
    DBuf fa(ctx), fd(ctx), fdel(ctx), ea(ctx), ed(ctx), edel(ctx);
    HIP_CHECK(ctx, fa.alloc((nb + 1) * 4));
    HIP_CHECK(ctx, fd.alloc((n_acct + 1) * 4));
    HIP_CHECK(ctx, fdel.alloc((n_acct + 1) * 4));
    LAUNCH(ctx, k_ovl_base_acct_flags, grid_for(nb + 1), BLOCK, ctx->stream,
           ctx->acct.d, nb, dl_a, n_acct, fa.as<uint32_t>());
    LAUNCH(ctx, k_ovl_delta_acct_flags, grid_for(n_acct + 1), BLOCK, ctx->stream,
           dl_a, n_acct, fd.as<uint32_t>(), fdel.as<uint32_t>(), d_err);
    uint32_t Bk = 0, Dk = 0;
    HIP_CHECK(ctx, ea.alloc((nb + 1) * 4));
    HIP_CHECK(ctx, ed.alloc((n_acct + 1) * 4));
    HIP_CHECK(ctx, edel.alloc((n_acct + 1) * 4));
    if (scan_u32(ctx, fa.as<uint32_t>(), ea.as<uint32_t>(), nb + 1, &Bk) ||
        scan_u32(ctx, fd.as<uint32_t>(), ed.as<uint32_t>(), n_acct + 1, &Dk) ||
        scan_u32(ctx, fdel.as<uint32_t>(), edel.as<uint32_t>(), n_acct + 1,
                 &m.n_del) ||
        check_err(ctx, d_err))
        return -1;
    m.new_na = merged_count(Bk, Dk);
    if (alloc_merged(ctx, m.new_acct, m.new_na, sizeof(sre_account_entry),
                     "apply_delta: out of memory (accounts)"))
        return -1;
    uint64_t gmax = nb > n_acct ? nb : n_acct;
    if (gmax)
        LAUNCH(ctx, k_ovl_scatter_acct, grid_for(gmax), BLOCK, ctx->stream,
               ctx->acct.d, nb, ea.as<uint32_t>(), dl_a, n_acct,
               ed.as<uint32_t>(), m.new_acct.as<sre_account_entry>());
    if (io.map_out) {
        HIP_CHECK(ctx, io.map_out->alloc((nb + 1) * 4));
        LAUNCH(ctx, k_ovl_posmap, grid_for(nb + 1), BLOCK, ctx->stream,
               ctx->acct.d, nb, ea.as<uint32_t>(), dl_a, n_acct,
               ed.as<uint32_t>(), io.map_out->as<uint32_t>());
    }
    if (io.d_old_roots && io.d_new_roots && nb)
        LAUNCH(ctx, k_ovl_carry_roots, grid_for(nb), BLOCK, ctx->stream,
               ctx->acct.d, nb, ea.as<uint32_t>(), dl_a, n_acct,
               ed.as<uint32_t>(), io.d_old_roots, io.d_new_roots);
    HIP_CHECK(ctx, m.sdel.alloc((m.n_del ? m.n_del : 1) * 32));
    if (n_acct)
        LAUNCH(ctx, k_ovl_gather_deleted, grid_for(n_acct), BLOCK, ctx->stream,
               dl_a, n_acct, edel.as<uint32_t>(), m.sdel.as<uint8_t>());
    return 0;
}

// Closed-form small-delta storage merge: delta ranks + wipe-range prefix
// sums (merge_plan.h) instead of O(ns) flags/scans/posmap. The host
// validates what k_ovl_delta_st_flags checks on device (the owner lookup
// against the resident accounts rides in k_sds_marks).
static int merge_storage_closed_form(delta_merge &m)
{
    sre_ctx *ctx = m.ctx;
    uint64_t ns = ctx->st.n, n_st = m.n_st;
    uint32_t n_del = m.n_del;
    const sre_storage_entry *dl_s = m.dl_s.as<sre_storage_entry>();
    if (uint32_t bad = st_delta_flags(m.st_delta, n_st,
                                      deleted_accounts(m.acct_delta, m.n_acct)))
        return fail_flags(ctx, bad);
    DBuf bpos(ctx), match(ctx), mex(ctx), eex(ctx), dwlo(ctx), dwhi(ctx),
        dwsum(ctx);
    HIP_CHECK(ctx, bpos.alloc((n_st ? n_st : 1) * 4));
    HIP_CHECK(ctx, match.alloc((n_st ? n_st : 1) * 4));
    if (n_st)
        LAUNCH(ctx, k_sds_marks, grid_for(n_st), BLOCK, ctx->stream, ctx->st.d,
               ns, dl_s, n_st, ctx->acct.d, ctx->acct.n,
               m.dl_a.as<sre_account_delta>(), m.n_acct, bpos.as<uint32_t>(),
               match.as<uint32_t>());
    HIP_CHECK(ctx, dwlo.alloc((n_del ? n_del : 1) * 4));
    HIP_CHECK(ctx, dwhi.alloc((n_del ? n_del : 1) * 4));
    if (n_del)
        LAUNCH(ctx, k_sds_wipes, grid_for(n_del), BLOCK, ctx->stream, ctx->st.d,
               ns, m.sdel.as<uint8_t>(), n_del, dwlo.as<uint32_t>(),
               dwhi.as<uint32_t>());
    std::vector<uint32_t> match_h, wlo_h, whi_h;
    if (to_host(ctx, match_h, match, n_st) || to_host(ctx, wlo_h, dwlo, n_del) ||
        to_host(ctx, whi_h, dwhi, n_del))
        return -1;
    merge_plan pl;
    if (uint32_t bad = plan_st_small(ns, m.st_delta, n_st, match_h, wlo_h, whi_h, pl))
        return fail_flags(ctx, bad); // nothing adopted
    m.new_ns = pl.new_n;
    if (alloc_merged(ctx, m.new_st, m.new_ns, sizeof(sre_storage_entry),
                     "apply_delta: out of memory (storage)") ||
        to_device(ctx, mex, pl.m_excl.data(), n_st + 1) ||
        to_device(ctx, eex, pl.eff_excl.data(), n_st + 1) ||
        to_device(ctx, dwsum, pl.wsum.data(), (uint64_t)n_del + 1))
        return -1;
    LAUNCH(ctx, k_sds_scatter, grid_for(ns), BLOCK, ctx->stream, ctx->st.d, ns,
           dl_s, n_st, mex.as<uint32_t>(), eex.as<uint32_t>(),
           dwlo.as<uint32_t>(), dwhi.as<uint32_t>(), dwsum.as<uint32_t>(), n_del,
           m.new_st.as<sre_storage_entry>());
    if (n_st)
        LAUNCH(ctx, k_sds_place, grid_for(n_st), BLOCK, ctx->stream, dl_s, n_st,
               bpos.as<uint32_t>(), mex.as<uint32_t>(), eex.as<uint32_t>(),
               dwlo.as<uint32_t>(), dwhi.as<uint32_t>(), dwsum.as<uint32_t>(),
               n_del, m.new_st.as<sre_storage_entry>());
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

static int merge_storage_general(delta_merge &m)
{
    sre_ctx *ctx = m.ctx;
    uint64_t ns = ctx->st.n, n_st = m.n_st;
    const sre_storage_entry *dl_s = m.dl_s.as<sre_storage_entry>();
    DBuf sa(ctx), sd(ctx), esa(ctx), esd(ctx);
    HIP_CHECK(ctx, sa.alloc((ns + 1) * 4));
    HIP_CHECK(ctx, sd.alloc((n_st + 1) * 4));
    LAUNCH(ctx, k_ovl_base_st_flags, grid_for(ns + 1), BLOCK, ctx->stream,
           ctx->st.d, ns, dl_s, n_st, m.sdel.as<uint8_t>(), (uint64_t)m.n_del,
           sa.as<uint32_t>());
    LAUNCH(ctx, k_ovl_delta_st_flags, grid_for(n_st + 1), BLOCK, ctx->stream,
           dl_s, n_st, m.sdel.as<uint8_t>(), (uint64_t)m.n_del, ctx->acct.d,
           ctx->acct.n, m.dl_a.as<sre_account_delta>(), m.n_acct,
           sd.as<uint32_t>(), m.err.as<uint32_t>());
    uint32_t Sk = 0, Tk = 0;
    HIP_CHECK(ctx, esa.alloc((ns + 1) * 4));
    HIP_CHECK(ctx, esd.alloc((n_st + 1) * 4));
    if (scan_u32(ctx, sa.as<uint32_t>(), esa.as<uint32_t>(), ns + 1, &Sk) ||
        scan_u32(ctx, sd.as<uint32_t>(), esd.as<uint32_t>(), n_st + 1, &Tk) ||
        check_err(ctx, m.err.as<uint32_t>()))
        return -1;
    m.new_ns = merged_count(Sk, Tk);
    if (alloc_merged(ctx, m.new_st, m.new_ns, sizeof(sre_storage_entry),
                     "apply_delta: out of memory (storage)"))
        return -1;
    uint64_t gmax = ns > n_st ? ns : n_st;
    if (gmax)
        LAUNCH(ctx, k_ovl_scatter_st, grid_for(gmax), BLOCK, ctx->stream,
               ctx->st.d, ns, esa.as<uint32_t>(), dl_s, n_st,
               esd.as<uint32_t>(), m.new_st.as<sre_storage_entry>());
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// General overlay merge of a delta into the resident state: accounts, then
// whichever storage merge fits, then adoption.
static int merge_delta(sre_ctx *ctx, const sre_account_delta *acct_delta,
                       uint64_t n_acct, const sre_storage_entry *st_delta,
                       uint64_t n_st, merge_io &io)
{
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    delta_merge m{ctx, acct_delta, n_acct, st_delta, n_st};
    if (alloc_err_flag(ctx, m.err) || to_device(ctx, m.dl_a, acct_delta, n_acct) ||
        to_device(ctx, m.dl_s, st_delta, n_st))
        return -1;
    revert_tmp rv{ctx};
    if (ctx->rv_on &&
        capture_revert(ctx, acct_delta, m.dl_a.as<sre_account_delta>(), n_acct,
                       m.dl_s.as<sre_storage_entry>(), n_st, rv))
        return -1;
    if (merge_accounts_general(m, io))
        return -1;
    uint64_t ns = ctx->st.n;
    if (ns && n_st == 0 && m.n_del == 0 && ctx->st.own) {
        // accounts-only delta over a storage-bearing state: the storage
        // array is untouched and m.new_st stays empty, so it is kept in
        // place (engine-owned only: a borrowed array may be released by
        // the caller after the delta)
    } else if (ns > sds_min_ns() && n_st <= (ns >> 8) && m.n_del <= 4096) {
        if (merge_storage_closed_form(m))
            return -1;
        io.st_closed_form = true;
    } else if (merge_storage_general(m)) {
        return -1;
    }
    adopt_merged(ctx, m.new_acct, m.new_na, m.new_st, m.new_ns, rv);
    return 0;
}

extern "C" int sre_apply_delta(sre_ctx *ctx,
                               const sre_account_delta *acct_delta,
                               uint64_t n_acct,
                               const sre_storage_entry *st_delta, uint64_t n_st)
{
    invalidate_retention(ctx); // a plain apply invalidates cell retention
    merge_io io;
    return merge_delta(ctx, acct_delta, n_acct, st_delta, n_st, io);
}

// Small-delta account merge + lcp repair (accounts-only dirty path): one
// pass over the base (closed-form ranks from tiny L2-resident delta
// arrays) replaces the general overlay merge's flags + scans + posmap
// passes, and the retained lcp is repaired at O(delta) boundary positions
// instead of recomputed over all na. Preconditions: ns == 0, lcp_valid.
static int apply_delta_small(sre_ctx *ctx, const sre_account_delta *acct_delta,
                             uint64_t nd, DBuf *map_out)
{
    uint64_t nb = ctx->acct.n;
    // the general path's k_ovl_delta_acct_flags validates this on device;
    // closed-form ranks would silently mis-merge on unsorted input
    if (uint32_t bad = acct_delta_order(acct_delta, nd))
        return fail_flags(ctx, bad);
    DBuf dl(ctx), bpos(ctx), match(ctx), mex(ctx), eex(ctx), npos(ctx),
        dpatch(ctx), err(ctx), out(ctx), no_st(ctx);
    if (to_device(ctx, dl, acct_delta, nd))
        return -1;
    revert_tmp rv{ctx};
    if (ctx->rv_on && capture_revert(ctx, acct_delta, dl.as<sre_account_delta>(),
                                     nd, nullptr, 0, rv))
        return -1;
    HIP_CHECK(ctx, bpos.alloc(nd * 4));
    HIP_CHECK(ctx, match.alloc(nd * 4));
    LAUNCH(ctx, k_sd_marks, grid_for(nd), BLOCK, ctx->stream, ctx->acct.d, nb,
           dl.as<sre_account_delta>(), nd, bpos.as<uint32_t>(),
           match.as<uint32_t>());
    std::vector<uint32_t> match_h, npos_h;
    if (to_host(ctx, match_h, match, nd))
        return -1;
    merge_plan pl = plan_acct_small(nb, acct_delta, nd, match_h);
    uint64_t new_na = pl.new_n;
    if (alloc_merged(ctx, out, new_na, sizeof(sre_account_entry),
                     "apply_delta_small: out of memory") ||
        to_device(ctx, mex, pl.m_excl.data(), nd + 1) ||
        to_device(ctx, eex, pl.eff_excl.data(), nd + 1))
        return -1;
    HIP_CHECK(ctx, map_out->alloc((nb + 1) * 4));
    LAUNCH(ctx, k_sd_scatter, grid_for(nb + 1), BLOCK, ctx->stream, ctx->acct.d,
           nb, dl.as<sre_account_delta>(), nd, mex.as<uint32_t>(),
           eex.as<uint32_t>(), out.as<sre_account_entry>(),
           map_out->as<uint32_t>());
    HIP_CHECK(ctx, npos.alloc(nd * 4));
    LAUNCH(ctx, k_sd_place, grid_for(nd), BLOCK, ctx->stream,
           dl.as<sre_account_delta>(), nd, bpos.as<uint32_t>(),
           mex.as<uint32_t>(), eex.as<uint32_t>(), out.as<sre_account_entry>(),
           npos.as<uint32_t>());
    // lcp repair into the ping-pong partner
    if (ctx->lcp_ret2.grow(ctx, new_na + 1))
        return -1;
    LAUNCH(ctx, k_sd_lcp_copy, grid_for(nb), BLOCK, ctx->stream,
           map_out->as<uint32_t>(), nb, (const int8_t *)ctx->lcp_ret.p,
           (int8_t *)ctx->lcp_ret2.p);
    if (to_host(ctx, npos_h, npos, nd))
        return -1;
    std::vector<uint32_t> patch = lcp_patch_list(acct_delta, nd, npos_h, new_na);
    if (to_device(ctx, dpatch, patch.data(), patch.size()) ||
        alloc_err_flag(ctx, err))
        return -1;
    LAUNCH(ctx, k_sd_lcp_patch, grid_for(patch.size()), BLOCK, ctx->stream,
           out.as<sre_account_entry>(), new_na, dpatch.as<uint32_t>(),
           patch.size(), (int8_t *)ctx->lcp_ret2.p, err.as<uint32_t>());
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (check_err(ctx, err.as<uint32_t>()))
        return -1;
    adopt_merged(ctx, out, new_na, no_st, 0, rv);
    std::swap(ctx->lcp_ret, ctx->lcp_ret2);
    ctx->lcp_valid = true;
    return 0;
}

// Full root, retaining the cell-top records and per-account storage roots
// for subsequent sre_incremental_root calls (dirty-path incremental). It
// times nothing and publishes no stats (they stay zeroed): no finish().
extern "C" int sre_root_retaining(sre_ctx *ctx, uint8_t out_root[32])
{
    root_call f{ctx};
    if (f.begin(true))
        return -1;
    invalidate_retention(ctx);
    if (ctx->acct.n == 0) {
        if (empty_state_root(ctx, out_root))
            return -1;
        ctx->cap_count = 0;
        ctx->cells_valid = true;
        return 0;
    }
    DBuf roots(ctx);
    armed_capture cap{ctx};
    if (ctx->roots_ret.grow(ctx, ctx->acct.n, 32) || f.arm_err())
        return -1;
    HIP_CHECK(ctx, roots.alloc(32));
    if (cap.arm(ctx->acct.n))
        return -1;
    // full storage pass into the RETAINED roots buffer (chained deltas
    // carry and patch it instead of recomputing every segment)
    if (run_storage_pass(ctx, (uint8_t *)ctx->roots_ret.p, &f.po, f.flag()) ||
        run_account_pass(ctx, (const uint8_t *)ctx->roots_ret.p, 0,
                         roots.as<uint8_t>(), nullptr, nullptr, &f.po, f.flag(),
                         cap.cap) ||
        check_err(ctx, f.flag()) || cap.read())
        return -1;
    ctx->cells_valid = true;
    HIP_CHECK(ctx, hipMemcpy(out_root, roots.p, 32, hipMemcpyDeviceToHost));
    return 0;
}

// What the steps of the dirty-path incremental root share (the shape of
// delta_merge): the delta, the call frame, which merge ran, and the buffers
// that live from the step that fills them to the end of the call.
struct inc_root {
    sre_ctx *ctx;
    const sre_account_delta *acct_delta;
    uint64_t n_acct;
    const sre_storage_entry *st_delta;
    uint64_t n_st;
    std::vector<uint8_t> *bitmap_out; // with updates: the final dirty cells
    root_call f{ctx};
    // no_storage: accounts-only state and delta, new_roots is null (the leaf
    // kernel substitutes EMPTY_ROOT). small / st_closed_form: the merges run.
    bool no_storage = false, small = false, st_closed_form = false;
    uint8_t *new_roots = nullptr;
    uint32_t n_active = 0;
    // map: old -> new positions; bitmap: dirty cells; dl / dls: the delta
    DBuf map{ctx}, bitmap{ctx}, dl{ctx}, dls{ctx}, recs{ctx}, depths{ctx},
        covered{ctx}, hist{ctx}, abhash{ctx}, alist{ctx}, roots{ctx};
};

// Step 1: merge the delta into the resident state (small or general merge),
// carrying the retained storage roots into the ping-pong partner buffer.
static int inc_merge(inc_root &r)
{
    sre_ctx *ctx = r.ctx;
    r.no_storage = (ctx->st.n == 0 && r.n_st == 0);
    // new roots buffer: the ping-pong partner of the retained one (no
    // per-step hipMalloc at steady state), EMPTY-filled upper bound,
    // carried across the merge
    uint64_t max_na = ctx->acct.n + r.n_acct;
    if (!r.no_storage && ctx->roots_ret2.grow(ctx, max_na, 32))
        return -1;
    r.new_roots = r.no_storage ? nullptr : (uint8_t *)ctx->roots_ret2.p;
    if (r.new_roots)
        LAUNCH(ctx, k_fill_empty_roots, grid_for(max_na ? max_na : 1), BLOCK,
               ctx->stream, r.new_roots, max_na ? max_na : 1);

    // small accounts-only deltas take the one-pass merge with lcp repair
    // (closed-form ranks; O(delta) boundary lcps patched) — the scan-floor
    // fix for the configs[4] shape. Everything else keeps the general
    // overlay merge.
    r.small = r.no_storage && r.n_acct > 0 && ctx->lcp_valid &&
              (r.n_acct <= (ctx->acct.n >> 6) ||
               (getenv("SRE_SD_FORCE") && r.n_acct <= ctx->acct.n));
    if (r.small)
        return apply_delta_small(ctx, r.acct_delta, r.n_acct, &r.map);
    // carry only when the pre-delta state HAS storage: while ns stays 0
    // every retained root is EMPTY_ROOT (and accounts-only fast-path
    // deltas may have drifted roots_ret's indexing — harmless, since
    // it is then never read)
    merge_io io;
    io.map_out = &r.map;
    if (r.new_roots && ctx->st.n > 0)
        io.d_old_roots = (const uint8_t *)ctx->roots_ret.p;
    io.d_new_roots = r.new_roots;
    if (merge_delta(ctx, r.acct_delta, r.n_acct, r.st_delta, r.n_st, io))
        return -1;
    r.st_closed_form = io.st_closed_form;
    ctx->lcp_valid = false; // recomputed by inc_seed_and_rehash
    return 0;
}

// Step 2: mark the 5-nibble cells the delta's rows fall into.
static int inc_mark_cells(inc_root &r)
{
    sre_ctx *ctx = r.ctx;
    HIP_CHECK(ctx, r.bitmap.alloc(N_CELLS));
    HIP_CHECK(ctx, hipMemsetAsync(r.bitmap.p, 0, N_CELLS, ctx->stream));
    if (to_device(ctx, r.dl, r.acct_delta, r.n_acct))
        return -1;
    if (r.n_acct)
        LAUNCH(ctx, k_mark_delta_cells, grid_for(r.n_acct), BLOCK, ctx->stream,
               r.dl.as<sre_account_delta>(), r.n_acct, r.bitmap.as<uint8_t>());
    if (r.n_st) {
        if (to_device(ctx, r.dls, r.st_delta, r.n_st))
            return -1;
        LAUNCH(ctx, k_mark_delta_cells_st, grid_for(r.n_st), BLOCK, ctx->stream,
               r.dls.as<sre_storage_entry>(), r.n_st, r.bitmap.as<uint8_t>());
    }
    return 0;
}

// Step 3: recompute ONLY the touched accounts' storage tries: gather their
// merged segments and scatter their fresh roots over the carried ones.
static int inc_touched_storage(inc_root &r)
{
    sre_ctx *ctx = r.ctx;
    if (!r.n_st)
        return 0;
    std::vector<key32> tkeys = storage_delta_accounts(r.st_delta, r.n_st);
    uint32_t nt = (uint32_t)tkeys.size();
    DBuf dtk(ctx), tlo(ctx), thi(ctx), taidx(ctx);
    if (to_device(ctx, dtk, tkeys.data(), nt))
        return -1;
    HIP_CHECK(ctx, tlo.alloc((uint64_t)nt * 4));
    HIP_CHECK(ctx, thi.alloc((uint64_t)nt * 4));
    HIP_CHECK(ctx, taidx.alloc((uint64_t)nt * 4));
    LAUNCH(ctx, k_touched_bounds, grid_for(nt), BLOCK, ctx->stream, ctx->st.d,
           ctx->st.n, ctx->acct.d, ctx->acct.n, dtk.as<uint8_t>(), nt,
           tlo.as<uint32_t>(), thi.as<uint32_t>(), taidx.as<uint32_t>(),
           r.new_roots, r.f.flag());
    std::vector<uint32_t> lo, hi;
    if (to_host(ctx, lo, tlo, nt) || to_host(ctx, hi, thi, nt))
        return -1;
    std::vector<uint32_t> offs = interval_offsets(lo, hi);
    if (offs[nt] &&
        run_storage_intervals(ctx, tlo.as<uint32_t>(), thi.as<uint32_t>(), offs,
                              r.new_roots, &r.f.po, r.f.flag()))
        return -1;
    return check_err(ctx, r.f.flag());
}

// Step 4: the account lcp (in the retained ping-pong buffer: repaired by the
// small merge, recomputed here after the general one, arming repair for the
// next delta). Then seed the clean cell tops from the retained rows and
// rehash the leaves of dirty cells and of positions no seed covers.
static int inc_seed_and_rehash(inc_root &r)
{
    sre_ctx *ctx = r.ctx;
    uint64_t na = ctx->acct.n;
    if (!r.small) {
        if (ctx->lcp_ret.grow(ctx, na + 1))
            return -1;
        LAUNCH(ctx, k_lcp_account, grid_for(na + 1), BLOCK, ctx->stream,
               ctx->acct.d, na, 0, (int8_t *)ctx->lcp_ret.p, r.f.flag());
        ctx->lcp_valid = true;
    }
    int8_t *lcp_p = (int8_t *)ctx->lcp_ret.p;
    HIP_CHECK(ctx, r.recs.alloc(na * sizeof(node_rec)));
    HIP_CHECK(ctx, r.depths.alloc(na));
    HIP_CHECK(ctx, r.covered.alloc(na));
    HIP_CHECK(ctx, r.hist.alloc(66 * 4));
    HIP_CHECK(ctx, r.roots.alloc(32));
    HIP_CHECK(ctx, hipMemsetAsync(r.depths.p, 0xFF, na, ctx->stream));
    HIP_CHECK(ctx, hipMemsetAsync(r.covered.p, 0, na, ctx->stream));
    HIP_CHECK(ctx, hipMemsetAsync(r.hist.p, 0, 66 * 4, ctx->stream));
    // with updates the seeded rows bring their branch hashes along
    if (ctx->retain_updates)
        HIP_CHECK(ctx, r.abhash.alloc(na * 32));
    // seed clean cell-tops; anything invalid dirties its cell
    if (ctx->cap_count)
        LAUNCH(ctx, k_revalidate_rows, grid_for(ctx->cap_count), BLOCK,
               ctx->stream, (const cap_row *)ctx->cap_rows.p, ctx->cap_count,
               r.map.as<uint32_t>(), lcp_p, r.bitmap.as<uint8_t>(),
               r.recs.as<node_rec>(), r.depths.as<uint8_t>(),
               r.covered.as<uint8_t>(), r.hist.as<uint32_t>(),
               r.abhash.as<uint8_t>());
    EvTimer leaf;
    HIP_CHECK(ctx, leaf.start(ctx->stream));
    // compact the recompute set (covered == 0: dirty cells leave their
    // positions uncovered, so this is exactly dirty ∪ uncovered) and
    // launch the leaf kernel over it instead of sweeping all na lanes
    {
        uint32_t nblk = grid_for(na);
        DBuf ac(ctx), ao(ctx);
        HIP_CHECK(ctx, ac.alloc((uint64_t)nblk * 4));
        HIP_CHECK(ctx, ao.alloc((uint64_t)nblk * 4));
        LAUNCH(ctx, k_active_hist, nblk, BLOCK, ctx->stream,
               r.covered.as<uint8_t>(), na, ac.as<uint32_t>());
        if (scan_u32(ctx, ac.as<uint32_t>(), ao.as<uint32_t>(), nblk,
                     &r.n_active))
            return -1;
        HIP_CHECK(ctx, r.alist.alloc(((uint64_t)r.n_active ? r.n_active : 1) * 4));
        LAUNCH(ctx, k_active_scatter, nblk, BLOCK, ctx->stream,
               r.covered.as<uint8_t>(), na, ao.as<uint32_t>(),
               r.alist.as<uint32_t>());
    }
    if (r.n_active)
        LAUNCH(ctx, k_leaf_account, grid_for(r.n_active), BLOCK, ctx->stream,
               ctx->acct.d, na, (const uint8_t *)r.new_roots, lcp_p, 0,
               r.recs.as<node_rec>(), r.depths.as<uint8_t>(),
               r.hist.as<uint32_t>(), r.roots.as<uint8_t>(), nullptr, nullptr,
               nullptr, nullptr, r.alist.as<uint32_t>(), r.n_active);
    HIP_CHECK(ctx, leaf.stop(ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIP_CHECK(ctx, leaf.ms(&ms));
    r.f.po.leaf_ms += ms;
    if (check_err(ctx, r.f.flag()))
        return -1;
    // final dirty-cell set (incl. revalidation misses)
    return r.bitmap_out ? to_host(ctx, *r.bitmap_out, r.bitmap, N_CELLS) : 0;
}

// Step 5: the account trie's levels, with a fresh capture for the next
// delta. k_revalidate_rows has consumed the retained rows, so capturing over
// the same buffer is safe (arm() swaps in a bigger one when na outgrew it).
static int inc_account_levels(inc_root &r)
{
    sre_ctx *ctx = r.ctx;
    armed_capture cap{ctx};
    // every rehashed leaf (k_leaf_account) and every seeded row
    // (k_revalidate_rows) adds exactly one to hist
    uint64_t level_inputs = 0;
    if (cap.arm(ctx->acct.n) ||
        run_account_levels(ctx, r.recs, r.depths, (const int8_t *)ctx->lcp_ret.p,
                           r.hist, r.abhash, 0, r.roots.as<uint8_t>(), nullptr,
                           nullptr, &r.f.po, r.f.flag(), cap.cap, {},
                           &level_inputs) ||
        check_err(ctx, r.f.flag()) || cap.read())
        return -1;
    ctx->inc_cnt[1] = level_inputs - r.n_active;
    ctx->inc_cnt[2] = r.n_active;
    ctx->inc_cnt[5] = ctx->cap_count;
    return 0;
}

// Dirty-path incremental root: apply a HashedPostState overlay delta
// (accounts + storage) and recompute only the 5-nibble cells it touches —
// reusing every clean cell-top record and every untouched account's
// retained storage root (the §3b walker-skip semantics expressed in this
// engine's level machinery). Requires a prior sre_root_retaining. With
// ctx->retain_updates armed by the caller, the seeded rows also seed bhash
// and the final dirty-cell bitmap goes to bitmap_out for the net diff.
// Retention is valid on entry, disarmed the moment the merge has adopted the
// new state and armed again only by the commit at the end: a step that fails
// in between returns with it disarmed; a rejected delta adopted nothing.
static int incremental_root_impl(sre_ctx *ctx, const sre_account_delta *acct_delta,
                                 uint64_t n_acct, const sre_storage_entry *st_delta,
                                 uint64_t n_st, uint8_t out_root[32],
                                 std::vector<uint8_t> *bitmap_out)
{
    inc_root r{ctx, acct_delta, n_acct, st_delta, n_st, bitmap_out};
    if (r.f.begin(true))
        return -1;
    if (!ctx->cells_valid) {
        set_err(ctx, "sre_incremental_root: needs sre_root_retaining first");
        return -1;
    }
    if (r.f.start_timer())
        return -1;
    ctx->inc_cnt[0] = ctx->cap_count;
    if (inc_merge(r))
        return -1;
    ctx->cells_valid = false;
    ctx->inc_cnt[3] = r.small;
    ctx->inc_cnt[4] = r.st_closed_form;
    if (ctx->acct.n == 0) {
        invalidate_retention(ctx);
        memcpy(out_root, EMPTY_ROOT_H, 32);
        return 0;
    }
    if (r.f.arm_err() || inc_mark_cells(r) || inc_touched_storage(r) ||
        inc_seed_and_rehash(r) || inc_account_levels(r))
        return -1;
    // commit: the ping-pong partner holds the post-delta storage roots
    if (!r.no_storage)
        std::swap(ctx->roots_ret, ctx->roots_ret2);
    ctx->cells_valid = true;
    // po counts only the subset storage leaves, not the account leaves
    // rehashed in step 4: the leaf/block totals would be partial numbers,
    // so they are published as zero
    r.f.po.leaf_count = r.f.po.leaf_blocks = r.f.po.branch_blocks = 0;
    if (r.f.publish())
        return -1;
    HIP_CHECK(ctx, hipMemcpy(out_root, r.roots.p, 32, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sre_incremental_root(sre_ctx *ctx,
                                    const sre_account_delta *acct_delta,
                                    uint64_t n_acct,
                                    const sre_storage_entry *st_delta,
                                    uint64_t n_st, uint8_t out_root[32])
{
    // the capture refresh runs without branch hashes -> the row snapshot
    // can no longer seed future update emission
    ctx->snap_valid = false;
    return incremental_root_impl(ctx, acct_delta, n_acct, st_delta, n_st,
                                 out_root, nullptr);
}

extern "C" int sre_root_retaining_with_updates(sre_ctx *ctx,
                                               uint8_t out_root[32])
{
    ctx->retain_updates = true;
    ctx->updates.clear();
    int rc = sre_root_retaining(ctx, out_root);
    ctx->retain_updates = false;
    if (rc)
        return rc;
    std::sort(ctx->updates.begin(), ctx->updates.end(), row_less);
    ctx->snap.clear();
    ctx->snap.reserve(ctx->updates.size());
    for (auto &r : ctx->updates) {
        r.removed = 0;
        ctx->snap.push_back(snap_of(r));
    }
    ctx->snap_valid = true;
    return 0;
}

extern "C" int sre_incremental_root_with_updates(
    sre_ctx *ctx, const sre_account_delta *acct_delta, uint64_t n_acct,
    const sre_storage_entry *st_delta, uint64_t n_st, uint8_t out_root[32])
{
    if (!ctx->snap_valid) {
        set_err(ctx, "sre_incremental_root_with_updates: needs "
                     "sre_root_retaining_with_updates first");
        return -1;
    }
    // region keys from the (sorted) delta, host side
    std::vector<key32> touched = storage_delta_accounts(st_delta, n_st);
    std::vector<key32> destroyed = deleted_accounts(acct_delta, n_acct);

    ctx->retain_updates = true;
    ctx->updates.clear();
    std::vector<uint8_t> bitmap;
    int rc = incremental_root_impl(ctx, acct_delta, n_acct, st_delta, n_st,
                                   out_root, &bitmap);
    ctx->retain_updates = false;
    if (rc) {
        ctx->updates.clear(); // no partial emission stays readable
        // a rejected delta adopted nothing and leaves the snapshot armed;
        // a failure after adoption disarmed the cells, and the snapshot
        // goes with them
        if (!ctx->cells_valid)
            ctx->snap_valid = false;
        return rc;
    }

    std::vector<sre_update_row> diff;
    std::vector<snap_row> nsnap;
    updates_net_diff(ctx->snap, std::move(ctx->updates), bitmap, touched,
                     destroyed, diff, nsnap);
    ctx->snap.swap(nsnap);
    ctx->updates.swap(diff);
    ctx->snap_valid = true;
    return 0;
}

// state_root_from_nodes equivalent (StateRootProvider, crates/storage/
// storage-api/src/trie.rs:26-40; TrieInput, crates/trie/common/src/
// input.rs:10): compute the root of (resident state + HashedPostState
// delta) using a supplied stored-node overlay instead of recomputing
// every storage trie. The engine consumes exactly what reth's walker
// would: kind-1 path-[] rows' root_hash seeds untouched accounts'
// storage roots (the stored-root skip of walker.rs:195-230); tries
// without a usable row (small tries whose root branch is unstored, or
// tries touched by the delta) are rebuilt from their entries; the
// account trie is rebuilt in full on-device (cheap: it is ~2% of the
// leaf work). kind-0 rows are accepted and ignored — the account-trie
// skip they enable on CPU saves nothing here. Removal rows are invalid
// input. The resident state is REPLACED by the merged result.
extern "C" int sre_root_from_nodes(sre_ctx *ctx,
                                   const sre_update_row *rows,
                                   uint64_t n_rows,
                                   const sre_account_delta *acct_delta,
                                   uint64_t n_acct,
                                   const sre_storage_entry *st_delta,
                                   uint64_t n_st, uint8_t out_root[32])
{
    root_call f{ctx};
    if (f.begin(true))
        return -1;
    invalidate_retention(ctx);
    if (f.start_timer())
        return -1;

    // supplied storage roots: kind-1 path-[] rows with root_hash
    std::vector<std::array<uint8_t, 64>> kv; // key || root
    for (uint64_t i = 0; i < n_rows; ++i) {
        if (rows[i].removed) {
            set_err(ctx, "sre_root_from_nodes: removal rows are not a "
                         "valid node overlay");
            return -1;
        }
        if (rows[i].kind == 1 && rows[i].path_len == 0 &&
            rows[i].root_hash_set) {
            std::array<uint8_t, 64> e;
            memcpy(e.data(), rows[i].acct_key, 32);
            memcpy(e.data() + 32, rows[i].root_hash, 32);
            kv.push_back(e);
        }
    }
    std::sort(kv.begin(), kv.end(),
              [](const std::array<uint8_t, 64> &a,
                 const std::array<uint8_t, 64> &b) {
                  return memcmp(a.data(), b.data(), 32) < 0;
              });
    // touched storage accounts (delta, sorted)
    std::vector<key32> tkeys = storage_delta_accounts(st_delta, n_st);

    merge_io io;
    if (merge_delta(ctx, acct_delta, n_acct, st_delta, n_st, io))
        return -1;
    uint64_t na = ctx->acct.n, ns = ctx->st.n;
    if (na == 0)
        return empty_state_root(ctx, out_root);

    DBuf acct_roots(ctx), roots(ctx);
    if (f.arm_err())
        return -1;
    HIP_CHECK(ctx, acct_roots.alloc(na * 32));
    HIP_CHECK(ctx, roots.alloc(32));
    LAUNCH(ctx, k_fill_empty_roots, grid_for(na), BLOCK, ctx->stream,
           acct_roots.as<uint8_t>(), na);
    if (ns) {
        // segment the resident storage; seed supplied roots / flag rebuilds
        storage_segs sg(ctx);
        if (segment_storage(ctx, ctx->st.d, ns, f.flag(), sg))
            return -1;
        const uint32_t n_seg = sg.n_seg;
        DBuf need(ctx), dkv(ctx), dtk(ctx);
        HIP_CHECK(ctx, need.alloc((uint64_t)n_seg * 4));
        if (to_device(ctx, dkv, kv.data(), kv.size()) ||
            to_device(ctx, dtk, tkeys.data(), tkeys.size()))
            return -1;
        LAUNCH(ctx, k_seg_need, grid_for(n_seg), BLOCK, ctx->stream, ctx->st.d,
               sg.seg_start.as<uint32_t>(), n_seg, dkv.as<uint8_t>(),
               (uint64_t)kv.size(), dtk.as<uint8_t>(),
               (uint64_t)tkeys.size(), sg.seg_acct.as<uint32_t>(),
               acct_roots.as<uint8_t>(), need.as<uint32_t>());
        std::vector<uint32_t> need_h, start_h, lo, hi;
        if (to_host(ctx, need_h, need, n_seg) ||
            to_host(ctx, start_h, sg.seg_start, n_seg))
            return -1;
        needed_intervals(need_h, start_h, ns, lo, hi);
        std::vector<uint32_t> offs = interval_offsets(lo, hi);
        if (offs.back()) {
            DBuf dlo(ctx), dhi(ctx);
            if (to_device(ctx, dlo, lo.data(), lo.size()) ||
                to_device(ctx, dhi, hi.data(), hi.size()))
                return -1;
            if (run_storage_intervals(ctx, dlo.as<uint32_t>(),
                                      dhi.as<uint32_t>(), offs,
                                      acct_roots.as<uint8_t>(), &f.po,
                                      f.flag()))
                return -1;
        }
        if (check_err(ctx, f.flag()))
            return -1;
    }
    if (run_account_pass(ctx, acct_roots.as<uint8_t>(), 0,
                         roots.as<uint8_t>(), nullptr, nullptr, &f.po,
                         f.flag()) ||
        f.finish())
        return -1;
    HIP_CHECK(ctx, hipMemcpy(out_root, roots.p, 32, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sre_root_with_updates(sre_ctx *ctx, uint8_t out_root[32])
{
    ctx->retain_updates = true;
    ctx->updates.clear();
    int rc = sre_root(ctx, out_root);
    ctx->retain_updates = false;
    if (rc)
        return rc;
    std::sort(ctx->updates.begin(), ctx->updates.end(), row_less);
    return 0;
}

extern "C" int64_t sre_updates_count(sre_ctx *ctx)
{
    return (int64_t)ctx->updates.size();
}

extern "C" int sre_updates_get(sre_ctx *ctx, sre_update_row *out, uint64_t max_rows)
{
    uint64_t n = ctx->updates.size();
    if (n > max_rows)
        n = max_rows;
    memcpy(out, ctx->updates.data(), n * sizeof(sre_update_row));
    return 0;
}

extern "C" int sre_get_stats(sre_ctx *ctx, sre_stats *out)
{
    *out = ctx->stats;
    return 0;
}

extern "C" int sre_get_path_counters(sre_ctx *ctx, uint64_t out[4])
{
    memcpy(out, ctx->path_cnt, sizeof(ctx->path_cnt));
    return 0;
}

extern "C" int sre_get_incremental_counters(sre_ctx *ctx, uint64_t out[6])
{
    memcpy(out, ctx->inc_cnt, sizeof(ctx->inc_cnt));
    return 0;
}

// ---------------------------------------------------------------------------
// plain-state upload (sre_upload_plain_state / sre_set_plain_state_device):
// hash addresses and slots, sort by hashed key, install as resident state.
// The device half of reth's AccountHashingStage / StorageHashingStage and of
// HashedPostState::from_bundle_state + into_sorted. Arithmetic shared with
// the host check lives in radix.h; DESIGN.md §14 has the reasoning.
// ---------------------------------------------------------------------------

#define PLAIN_ACCT_B 96u  // sizeof(sre_plain_account)
#define PLAIN_ST_B 84u    // sizeof(sre_plain_storage)
static_assert(sizeof(sre_plain_account) == PLAIN_ACCT_B, "sre_plain_account");
static_assert(sizeof(sre_plain_storage) == PLAIN_ST_B, "sre_plain_storage");
static_assert(HS_WAVES * HS_WAVE == BLOCK, "a tile is sorted by one block");

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi)
{
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ void store_hash(uint8_t *dst, const uint64_t s[25])
{
    uint4 *o = (uint4 *)dst;
    o[0] = make_uint4((uint32_t)s[0], (uint32_t)(s[0] >> 32), (uint32_t)s[1],
                      (uint32_t)(s[1] >> 32));
    o[1] = make_uint4((uint32_t)s[2], (uint32_t)(s[2] >> 32), (uint32_t)s[3],
                      (uint32_t)(s[3] >> 32));
}

// keccak256 of a 20-byte address given as five LE dwords: the single block
// is composed in registers (pad byte 0x01 at offset 20, 0x80 at offset 135).
__device__ __forceinline__ void keccak_address(uint32_t a0, uint32_t a1, uint32_t a2,
                                               uint32_t a3, uint32_t a4,
                                               uint64_t s[25])
{
#pragma unroll
    for (int k = 0; k < 25; ++k)
        s[k] = 0;
    s[0] = u64_of(a0, a1);
    s[1] = u64_of(a2, a3);
    s[2] = u64_of(a4, 0x01u);
    s[16] = 0x8000000000000000ull;
    keccak_f(s);
}

// One lane per plain account row: hashed address (32 B), sort key, row index.
__global__ void __launch_bounds__(BLOCK) k_hs_account_keys(
    const uint8_t *__restrict__ plain, uint64_t na, int keep,
    uint8_t *__restrict__ hk, uint64_t *__restrict__ keys,
    uint32_t *__restrict__ idx)
{
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= na)
        return;
    const uint8_t *row = plain + i * PLAIN_ACCT_B; // 16-B aligned
    uint4 a = *(const uint4 *)row;
    uint32_t a4 = *(const uint32_t *)(row + 16);
    uint64_t s[25];
    keccak_address(a.x, a.y, a.z, a.w, a4, s);
    store_hash(hk + i * 32, s);
    keys[i] = hs_account_key(s[0], keep);
    idx[i] = (uint32_t)i;
}

// One lane per plain storage row: hash the address, find its rank in the
// sorted accounts (a miss is an orphan row), hash the slot, emit the hashed
// slot key, the (rank, slot prefix) sort key and the row index.
__global__ void __launch_bounds__(BLOCK) k_hs_storage_keys(
    const uint8_t *__restrict__ plain, uint64_t ns,
    const sre_account_entry *__restrict__ acct, uint64_t na, int keep,
    uint8_t *__restrict__ hks, uint64_t *__restrict__ keys,
    uint32_t *__restrict__ idx, uint32_t *__restrict__ err)
{
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ns)
        return;
    const uint32_t *row = (const uint32_t *)(plain + i * PLAIN_ST_B); // 4-B aligned
    uint64_t s[25];
    keccak_address(row[0], row[1], row[2], row[3], row[4], s);
    uint64_t h[4] = {s[0], s[1], s[2], s[3]};
    uint64_t lo = 0, hi = na;
    while (lo < hi) {
        uint64_t mid = (lo + hi) / 2;
        const uint64_t *k = (const uint64_t *)&acct[mid];
        uint64_t w[4] = {k[0], k[1], k[2], k[3]};
        if (hs_cmp_words(w, h) < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    bool found = false;
    if (lo < na) {
        const uint64_t *k = (const uint64_t *)&acct[lo];
        uint64_t w[4] = {k[0], k[1], k[2], k[3]};
        found = hs_cmp_words(w, h) == 0;
    }
    if (!found)
        atomicOr(err, 1u << E_ORPHAN_STORAGE);
#pragma unroll
    for (int k = 0; k < 25; ++k)
        s[k] = 0;
    s[0] = u64_of(row[5], row[6]);
    s[1] = u64_of(row[7], row[8]);
    s[2] = u64_of(row[9], row[10]);
    s[3] = u64_of(row[11], row[12]);
    s[4] = 0x01ull;
    s[16] = 0x8000000000000000ull;
    keccak_f(s);
    store_hash(hks + i * 32, s);
    keys[i] = hs_storage_key(found ? (uint32_t)lo : 0u, s[0], keep);
    idx[i] = (uint32_t)i;
}

// hs_sort_pairs stage 1: one tile's 256-bin histogram of digit `pass`, one
// global write per bin.
__global__ void __launch_bounds__(BLOCK) k_hs_hist(
    const uint64_t *__restrict__ keys, uint64_t n, int pass, uint64_t ntiles,
    uint32_t *__restrict__ hist)
{
    __shared__ uint32_t bins[HS_BINS];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t tile = blockIdx.x;
    const uint32_t wave = threadIdx.x / HS_WAVE, lane = threadIdx.x % HS_WAVE;
#pragma unroll
    for (uint32_t r = 0; r < HS_ROUNDS; ++r) {
        uint64_t i = hs_item_index(tile, wave, r, lane);
        if (i < n)
            atomicAdd(&bins[hs_digit(keys[i], pass)], 1u);
    }
    __syncthreads();
    hist[hs_hist_slot(threadIdx.x, tile, ntiles)] = bins[threadIdx.x];
}

// Skip test on the scanned histogram matrix: a digit that holds all n pairs
// means the pass would move nothing.
__global__ void k_hs_one_bin(const uint32_t *__restrict__ offs, uint64_t ntiles,
                             uint64_t n, uint32_t *__restrict__ flag)
{
    uint32_t d = threadIdx.x;
    uint64_t first = offs[hs_hist_slot(d, 0, ntiles)];
    uint64_t end = d + 1 < HS_BINS ? offs[hs_hist_slot(d + 1, 0, ntiles)] : n;
    if (end - first == n)
        *flag = 1;
}

// hs_sort_pairs stage 3: stable scatter of one tile. The rank of a pair
// among the tile's pairs of its digit is built from wave64 peer masks (eight
// ballots per round) and per-(wave, digit) counters in LDS; see radix.h for
// the order that makes it stable.
__global__ void __launch_bounds__(BLOCK) k_hs_scatter(
    const uint64_t *__restrict__ keys_in, const uint32_t *__restrict__ idx_in,
    uint64_t n, int pass, uint64_t ntiles, const uint32_t *__restrict__ offs,
    uint64_t *__restrict__ keys_out, uint32_t *__restrict__ idx_out)
{
    __shared__ uint32_t wcount[HS_WAVES][HS_BINS];
    const uint64_t tile = blockIdx.x;
    const uint32_t wave = threadIdx.x / HS_WAVE, lane = threadIdx.x % HS_WAVE;
#pragma unroll
    for (uint32_t w = 0; w < HS_WAVES; ++w)
        wcount[w][threadIdx.x] = 0;
    __syncthreads();

    uint64_t key[HS_ROUNDS], peers[HS_ROUNDS];
    uint32_t id[HS_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < HS_ROUNDS; ++r) {
        uint64_t i = hs_item_index(tile, wave, r, lane);
        bool valid = i < n;
        key[r] = valid ? keys_in[i] : 0;
        id[r] = valid ? idx_in[i] : 0;
        uint32_t d = hs_digit(key[r], pass);
        uint64_t p = __ballot(valid);
#pragma unroll
        for (int b = 0; b < HS_RADIX_BITS; ++b) {
            bool bit = (d >> b) & 1u;
            uint64_t m = __ballot(bit);
            p &= bit ? m : ~m;
        }
        peers[r] = valid ? p : 0;
        // the lowest peer counts the round's pairs of this digit for its wave
        if (valid && lane == (uint32_t)__builtin_ctzll(p))
            atomicAdd(&wcount[wave][d], (uint32_t)__popcll(p));
    }
    __syncthreads();
    // per digit: the tile's first slot, then the four waves in order
    {
        uint32_t d = threadIdx.x;
        uint32_t g = offs[hs_hist_slot(d, tile, ntiles)];
#pragma unroll
        for (uint32_t w = 0; w < HS_WAVES; ++w) {
            uint32_t c = wcount[w][d];
            wcount[w][d] = g;
            g += c;
        }
    }
    __syncthreads();
    // rounds in order: the lowest peer claims the round's slots of its digit
    // (LDS atomics of one wave complete in issue order, so a later round
    // sees the earlier rounds' claims) and hands the base to its peers
#pragma unroll
    for (uint32_t r = 0; r < HS_ROUNDS; ++r) {
        uint64_t p = peers[r];
        bool valid = p != 0;
        uint32_t d = hs_digit(key[r], pass);
        uint32_t leader = valid ? (uint32_t)__builtin_ctzll(p) : 0u;
        uint32_t base = 0;
        if (valid && lane == leader)
            base = atomicAdd(&wcount[wave][d], (uint32_t)__popcll(p));
        base = __shfl(base, (int)leader, HS_WAVE);
        if (valid) {
            uint64_t pos = base + hs_rank_in_mask(p, lane);
            keys_out[pos] = key[r];
            idx_out[pos] = id[r];
        }
    }
}

// Tie runs = maximal runs of equal adjacent sort keys, length >= 2.
// cnt[0] += rows inside runs, cnt[1] += runs.
__global__ void __launch_bounds__(BLOCK) k_hs_tie_count(
    const uint64_t *__restrict__ keys, uint64_t n, unsigned long long *cnt)
{
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool in = i < n;
    uint64_t k = in ? keys[i] : 0;
    bool eqp = in && i > 0 && keys[i - 1] == k;
    bool eqn = in && i + 1 < n && keys[i + 1] == k;
    uint64_t rows = __ballot(eqp || eqn), heads = __ballot(eqn && !eqp);
    if (threadIdx.x % HS_WAVE == 0) {
        if (rows)
            atomicAdd(&cnt[0], (unsigned long long)__popcll(rows));
        if (heads)
            atomicAdd(&cnt[1], (unsigned long long)__popcll(heads));
    }
}

// One thread per run head insertion-sorts the run's row indices by the full
// 32-byte hashed key (hk[32 * row]); an exact tie keeps row order and raises
// the duplicate bit. Right for any run length, fast for short ones.
__global__ void __launch_bounds__(BLOCK) k_hs_tie_sort(
    const uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, uint64_t n,
    const uint8_t *__restrict__ hk, uint32_t dup_bit, uint32_t *__restrict__ err)
{
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n)
        return;
    uint64_t k = keys[i];
    if (i > 0 && keys[i - 1] == k)
        return;
    uint64_t end = i + 1;
    while (end < n && keys[end] == k)
        ++end;
    bool dup = false;
    for (uint64_t a = i + 1; a < end; ++a) {
        uint32_t v = idx[a];
        const uint64_t *pv = (const uint64_t *)(hk + (uint64_t)v * 32);
        uint64_t hv[4] = {pv[0], pv[1], pv[2], pv[3]};
        uint64_t b = a;
        while (b > i) {
            uint32_t u = idx[b - 1];
            const uint64_t *pu = (const uint64_t *)(hk + (uint64_t)u * 32);
            uint64_t hu[4] = {pu[0], pu[1], pu[2], pu[3]};
            int c = hs_cmp_words(hu, hv);
            if (c == 0) {
                dup = true;
                c = u < v ? -1 : 1;
            }
            if (c < 0)
                break;
            idx[b] = u;
            --b;
        }
        idx[b] = v;
    }
    if (dup)
        atomicOr(err, 1u << dup_bit);
}

// out[i] = (hashed key, nonce, balance, code_hash) of plain row idx[i].
// 16-B loads from the 96-B plain rows; the 104-B output stride allows 8 B.
__global__ void __launch_bounds__(BLOCK) k_hs_gather_accounts(
    const uint8_t *__restrict__ plain, const uint8_t *__restrict__ hk,
    const uint32_t *__restrict__ idx, uint64_t na,
    sre_account_entry *__restrict__ out)
{
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= na)
        return;
    uint64_t src = idx[i];
    const uint4 *h = (const uint4 *)(hk + src * 32);
    const uint4 *r = (const uint4 *)(plain + src * PLAIN_ACCT_B);
    uint4 h0 = h[0], h1 = h[1], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4],
          r5 = r[5];
    uint64_t *o = (uint64_t *)&out[i];
    o[0] = u64_of(h0.x, h0.y);
    o[1] = u64_of(h0.z, h0.w);
    o[2] = u64_of(h1.x, h1.y);
    o[3] = u64_of(h1.z, h1.w);
    o[4] = u64_of(r1.z, r1.w); // nonce at byte 24
    o[5] = u64_of(r2.x, r2.y);
    o[6] = u64_of(r2.z, r2.w);
    o[7] = u64_of(r3.x, r3.y);
    o[8] = u64_of(r3.z, r3.w);
    o[9] = u64_of(r4.x, r4.y);
    o[10] = u64_of(r4.z, r4.w);
    o[11] = u64_of(r5.x, r5.y);
    o[12] = u64_of(r5.z, r5.w);
}

// out[i] = (account key of the row's rank, hashed slot, value) of plain
// row idx[i]; flags zero values. The 84-B plain rows allow 4-B loads only;
// the hashed keys and the 96-B output rows move as 16 B.
__global__ void __launch_bounds__(BLOCK) k_hs_gather_storage(
    const uint8_t *__restrict__ plain, const uint8_t *__restrict__ hks,
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx,
    uint64_t ns, const sre_account_entry *__restrict__ acct,
    sre_storage_entry *__restrict__ out, uint32_t *__restrict__ err)
{
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ns)
        return;
    uint64_t src = idx[i];
    uint64_t rank = keys[i] >> 32;
    const uint64_t *ak = (const uint64_t *)&acct[rank];
    uint64_t a0 = ak[0], a1 = ak[1], a2 = ak[2], a3 = ak[3];
    const uint4 *h = (const uint4 *)(hks + src * 32);
    uint4 h0 = h[0], h1 = h[1];
    const uint32_t *v = (const uint32_t *)(plain + src * PLAIN_ST_B) + 13;
    uint4 v0 = make_uint4(v[0], v[1], v[2], v[3]);
    uint4 v1 = make_uint4(v[4], v[5], v[6], v[7]);
    if (!(v0.x | v0.y | v0.z | v0.w | v1.x | v1.y | v1.z | v1.w))
        atomicOr(err, 1u << E_ZERO_VALUE);
    uint4 *o = (uint4 *)&out[i];
    o[0] = make_uint4((uint32_t)a0, (uint32_t)(a0 >> 32), (uint32_t)a1,
                      (uint32_t)(a1 >> 32));
    o[1] = make_uint4((uint32_t)a2, (uint32_t)(a2 >> 32), (uint32_t)a3,
                      (uint32_t)(a3 >> 32));
    o[2] = h0;
    o[3] = h1;
    o[4] = v0;
    o[5] = v1;
}

// Test gate (read per call, inert when unset): keep only the top K bits of
// the hashed prefix in the sort keys so that ties carry the sort.
static int hs_key_bits()
{
    const char *e = getenv("SRE_HS_KEY_BITS");
    return e ? atoi(e) : -1;
}

static int read_u32(sre_ctx *ctx, const uint32_t *d, uint32_t *out)
{
    HIP_CHECK(ctx, hipMemcpyAsync(out, d, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// (u64 key, u32 row index) pairs, ping-ponged between two buffer pairs.
struct hs_pairs {
    DBuf k[2], x[2];
    int cur = 0;
    explicit hs_pairs(sre_ctx *c) : k{DBuf(c), DBuf(c)}, x{DBuf(c), DBuf(c)} {}
    hipError_t alloc(uint64_t n)
    {
        for (int j = 0; j < 2; ++j) {
            hipError_t e = k[j].alloc(n * 8);
            if (e == hipSuccess)
                e = x[j].alloc(n * 4);
            if (e != hipSuccess)
                return e;
        }
        return hipSuccess;
    }
    uint64_t *keys() { return k[cur].as<uint64_t>(); }
    uint32_t *idx() { return x[cur].as<uint32_t>(); }
};

// Stable LSD radix sort of n pairs by key, 8-bit digits. Per pass: per-tile
// histograms, exclusive scan of the [digit][tile] matrix, stable scatter; a
// pass whose histogram has one bin is skipped. cnt[1] / cnt[2] count the
// executed / skipped passes. Generic: knows nothing about what a key means.
static int hs_sort_pairs(sre_ctx *ctx, hs_pairs &pr, uint64_t n, uint64_t cnt[6])
{
    if (n == 0)
        return 0;
    const uint64_t ntiles = hs_num_tiles(n), cells = ntiles * HS_BINS;
    DBuf hist(ctx), offs(ctx), flag(ctx);
    HIP_CHECK(ctx, hist.alloc(cells * 4));
    HIP_CHECK(ctx, offs.alloc(cells * 4));
    HIP_CHECK(ctx, flag.alloc(4));
    for (int pass = 0; pass < HS_PASSES; ++pass) {
        HIP_CHECK(ctx, hipMemsetAsync(flag.p, 0, 4, ctx->stream));
        LAUNCH(ctx, k_hs_hist, (uint32_t)ntiles, BLOCK, ctx->stream, pr.keys(), n,
               pass, ntiles, hist.as<uint32_t>());
        if (scan_u32(ctx, hist.as<uint32_t>(), offs.as<uint32_t>(), cells, nullptr))
            return -1;
        LAUNCH(ctx, k_hs_one_bin, 1, HS_BINS, ctx->stream, offs.as<uint32_t>(),
               ntiles, n, flag.as<uint32_t>());
        uint32_t one_bin = 0;
        if (read_u32(ctx, flag.as<uint32_t>(), &one_bin))
            return -1;
        if (one_bin) {
            cnt[2]++;
            continue;
        }
        LAUNCH(ctx, k_hs_scatter, (uint32_t)ntiles, BLOCK, ctx->stream, pr.keys(),
               pr.idx(), n, pass, ntiles, offs.as<uint32_t>(),
               pr.k[pr.cur ^ 1].as<uint64_t>(), pr.x[pr.cur ^ 1].as<uint32_t>());
        pr.cur ^= 1;
        cnt[1]++;
    }
    return 0;
}

// Order every tie run of the sorted pairs by the full hashed key.
static int hs_resolve_ties(sre_ctx *ctx, hs_pairs &pr, uint64_t n, const uint8_t *hk,
                           uint32_t dup_bit, uint32_t *d_err, uint64_t cnt[6])
{
    if (n < 2)
        return 0;
    DBuf tc(ctx);
    HIP_CHECK(ctx, tc.alloc(16));
    HIP_CHECK(ctx, hipMemsetAsync(tc.p, 0, 16, ctx->stream));
    LAUNCH(ctx, k_hs_tie_count, grid_for(n), BLOCK, ctx->stream, pr.keys(), n,
           tc.as<unsigned long long>());
    unsigned long long h[2] = {0, 0};
    HIP_CHECK(ctx, hipMemcpyAsync(h, tc.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    cnt[3] += h[0];
    cnt[4] += h[1];
    if (h[1])
        LAUNCH(ctx, k_hs_tie_sort, grid_for(n), BLOCK, ctx->stream, pr.keys(),
               pr.idx(), n, hk, dup_bit, d_err);
    return 0;
}

static int plain_state_device(sre_ctx *ctx, const uint8_t *d_pa, uint64_t na,
                              const uint8_t *d_ps, uint64_t ns)
{
    if (check_cap(ctx, na) || check_cap(ctx, ns))
        return -1;
    if ((na && !d_pa) || (ns && !d_ps) || ((uintptr_t)d_pa & 15) ||
        ((uintptr_t)d_ps & 3)) {
        set_err(ctx, "plain state: null or misaligned row pointer (accounts "
                     "need 16-byte, storage 4-byte alignment)");
        return -1;
    }
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int keep = hs_key_bits();
    uint64_t cnt[6] = {na + 2 * ns, 0, 0, 0, 0, 0};
    DBuf err(ctx);
    if (alloc_err_flag(ctx, err))
        return -1;
    uint32_t *d_err = err.as<uint32_t>();

    // Build into temporaries; the resident state is touched only at the end.
    DBuf new_acct(ctx), new_st(ctx);
    if (new_acct.alloc((na ? na : 1) * sizeof(sre_account_entry)) != hipSuccess ||
        new_st.alloc((ns ? ns : 1) * sizeof(sre_storage_entry)) != hipSuccess) {
        set_err(ctx, "plain state: out of memory (sorted rows)");
        return -1;
    }
    sre_account_entry *acct = new_acct.as<sre_account_entry>();
    sre_storage_entry *st = new_st.as<sre_storage_entry>();

    if (na) {
        DBuf hk(ctx);
        hs_pairs pr(ctx);
        HIP_CHECK(ctx, hk.alloc(na * 32));
        HIP_CHECK(ctx, pr.alloc(na));
        LAUNCH(ctx, k_hs_account_keys, grid_for(na), BLOCK, ctx->stream, d_pa, na,
               keep, hk.as<uint8_t>(), pr.keys(), pr.idx());
        if (hs_sort_pairs(ctx, pr, na, cnt) ||
            hs_resolve_ties(ctx, pr, na, hk.as<uint8_t>(), E_DUP_ADDRESS, d_err, cnt))
            return -1;
        LAUNCH(ctx, k_hs_gather_accounts, grid_for(na), BLOCK, ctx->stream, d_pa,
               hk.as<uint8_t>(), pr.idx(), na, acct);
        if (check_err(ctx, d_err))
            return -1;
    }
    if (ns) {
        DBuf hks(ctx);
        hs_pairs pr(ctx);
        HIP_CHECK(ctx, hks.alloc(ns * 32));
        HIP_CHECK(ctx, pr.alloc(ns));
        LAUNCH(ctx, k_hs_storage_keys, grid_for(ns), BLOCK, ctx->stream, d_ps, ns,
               (const sre_account_entry *)acct, na, keep, hks.as<uint8_t>(),
               pr.keys(), pr.idx(), d_err);
        if (check_err(ctx, d_err)) // an orphan row has no rank to sort by
            return -1;
        if (hs_sort_pairs(ctx, pr, ns, cnt) ||
            hs_resolve_ties(ctx, pr, ns, hks.as<uint8_t>(), E_DUP_STORAGE, d_err, cnt))
            return -1;
        LAUNCH(ctx, k_hs_gather_storage, grid_for(ns), BLOCK, ctx->stream, d_ps,
               hks.as<uint8_t>(), pr.keys(), pr.idx(), ns,
               (const sre_account_entry *)acct, st, d_err);
        if (check_err(ctx, d_err))
            return -1;
    }
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));

    invalidate_retention(ctx);
    clear_revert(ctx);
    ctx->acct.adopt(ctx, new_acct, na);
    ctx->st.adopt(ctx, new_st, ns);
    memcpy(ctx->hs_cnt, cnt, sizeof(cnt));
    return 0;
}

extern "C" int sre_set_plain_state_device(sre_ctx *ctx, const void *d_acct,
                                          uint64_t na, const void *d_st, uint64_t ns)
{
    return plain_state_device(ctx, (const uint8_t *)d_acct, na,
                              (const uint8_t *)d_st, ns);
}

extern "C" int sre_upload_plain_state(sre_ctx *ctx, const sre_plain_account *accounts,
                                      uint64_t na, const sre_plain_storage *storage,
                                      uint64_t ns)
{
    if (check_cap(ctx, na) || check_cap(ctx, ns))
        return -1;
    if ((na && !accounts) || (ns && !storage)) {
        set_err(ctx, "sre_upload_plain_state: null row pointer");
        return -1;
    }
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DBuf pa(ctx), ps(ctx);
    if (na) {
        HIP_CHECK(ctx, pa.alloc(na * PLAIN_ACCT_B));
        HIP_CHECK(ctx, hipMemcpy(pa.p, accounts, na * PLAIN_ACCT_B,
                                 hipMemcpyHostToDevice));
    }
    if (ns) {
        HIP_CHECK(ctx, ps.alloc(ns * PLAIN_ST_B));
        HIP_CHECK(ctx, hipMemcpy(ps.p, storage, ns * PLAIN_ST_B,
                                 hipMemcpyHostToDevice));
    }
    return plain_state_device(ctx, pa.as<uint8_t>(), na, ps.as<uint8_t>(), ns);
}

extern "C" int sre_resident_counts(sre_ctx *ctx, uint64_t *na, uint64_t *ns)
{
    *na = ctx->acct.n;
    *ns = ctx->st.n;
    return 0;
}

// Copy a resident array (owned or borrowed) to the host.
static int download_rows(sre_ctx *ctx, const char *what, const void *d, uint64_t have,
                         size_t row, void *out, uint64_t n)
{
    if (n != have) {
        set_err(ctx, std::string(what) + ": n = " + std::to_string(n) +
                         " but " + std::to_string(have) + " rows are resident");
        return -1;
    }
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (n)
        HIP_CHECK(ctx, hipMemcpy(out, d, n * row, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sre_download_accounts(sre_ctx *ctx, sre_account_entry *out, uint64_t n)
{
    return download_rows(ctx, "sre_download_accounts", ctx->acct.d, ctx->acct.n,
                         sizeof(sre_account_entry), out, n);
}

extern "C" int sre_download_storage(sre_ctx *ctx, sre_storage_entry *out, uint64_t n)
{
    return download_rows(ctx, "sre_download_storage", ctx->st.d, ctx->st.n,
                         sizeof(sre_storage_entry), out, n);
}

extern "C" int sre_get_hash_sort_counters(sre_ctx *ctx, uint64_t out[6])
{
    memcpy(out, ctx->hs_cnt, sizeof(ctx->hs_cnt));
    return 0;
}

// ---- revert capture and unwind (include/sre.h) ----------------------------

extern "C" int sre_set_revert_capture(sre_ctx *ctx, int on)
{
    ctx->rv_on = on != 0;
    if (!ctx->rv_on)
        clear_revert(ctx);
    return 0;
}

extern "C" int sre_revert_counts(sre_ctx *ctx, uint64_t *n_acct, uint64_t *n_st)
{
    *n_acct = ctx->rv_have ? ctx->rv_acct.n : 0;
    *n_st = ctx->rv_have ? ctx->rv_st.n : 0;
    return 0;
}

extern "C" int sre_revert_get(sre_ctx *ctx, sre_account_delta *acct, uint64_t n_acct,
                              sre_storage_entry *st, uint64_t n_st)
{
    uint64_t ha = ctx->rv_have ? ctx->rv_acct.n : 0;
    uint64_t hs = ctx->rv_have ? ctx->rv_st.n : 0;
    if (n_acct != ha || n_st != hs) {
        set_err(ctx, "sre_revert_get: n = (" + std::to_string(n_acct) + ", " +
                         std::to_string(n_st) + ") but the stored revert has (" +
                         std::to_string(ha) + ", " + std::to_string(hs) + ") rows");
        return -1;
    }
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ha)
        HIP_CHECK(ctx, hipMemcpy(acct, ctx->rv_acct.d, ha * sizeof(sre_account_delta),
                                 hipMemcpyDeviceToHost));
    if (hs)
        HIP_CHECK(ctx, hipMemcpy(st, ctx->rv_st.d, hs * sizeof(sre_storage_entry),
                                 hipMemcpyDeviceToHost));
    return 0;
}

// The stored revert as host rows: the merges take host pointers and plan on
// the host, and the copies outlive the stored revert, which the unwind
// overwrites with the redo when capture is on.
static int unwind_rows(sre_ctx *ctx, const char *who,
                       std::vector<sre_account_delta> &acct,
                       std::vector<sre_storage_entry> &st)
{
    if (!ctx->rv_have) {
        set_err(ctx, std::string(who) + ": no-revert-captured (turn capture on "
                                        "before the delta to unwind)");
        return -1;
    }
    acct.resize(ctx->rv_acct.n);
    st.resize(ctx->rv_st.n);
    return sre_revert_get(ctx, acct.data(), acct.size(), st.data(), st.size());
}

extern "C" int sre_unwind(sre_ctx *ctx, uint8_t out_root[32])
{
    std::vector<sre_account_delta> acct;
    std::vector<sre_storage_entry> st;
    if (unwind_rows(ctx, "sre_unwind", acct, st))
        return -1;
    return sre_incremental_root(ctx, acct.data(), acct.size(), st.data(), st.size(),
                                out_root);
}

extern "C" int sre_unwind_with_updates(sre_ctx *ctx, uint8_t out_root[32])
{
    std::vector<sre_account_delta> acct;
    std::vector<sre_storage_entry> st;
    if (unwind_rows(ctx, "sre_unwind_with_updates", acct, st))
        return -1;
    return sre_incremental_root_with_updates(ctx, acct.data(), acct.size(),
                                             st.data(), st.size(), out_root);
}

extern "C" int sre_get_revert_counters(sre_ctx *ctx, uint64_t out[4])
{
    memcpy(out, ctx->rv_cnt, sizeof(ctx->rv_cnt));
    return 0;
}
