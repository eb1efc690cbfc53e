// Host-side multiproof assembly (sre_account_proof / sre_storage_proof):
// the captured-row layout, a host Keccak-256, the hex-prefix / RLP leaf and
// extension encoders, the RLP list parser and the semantic walk that picks
// the proof nodes out of the captured ones. Plain C++17, no HIP and no
// engine context, so tests/proof_main.cpp checks it as a sanitizer-built
// host program. Failures leave as a reason string; the caller stores it.
#pragma once

#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../include/sre.h"

// One captured path node: the branch group whose member interval contains
// a target's entry index (filled by k_proof_capture / the leaf kernels).
struct proof_row {
    uint32_t target;
    int16_t d, P;
    uint32_t br_len;
    uint32_t s, e;      // member interval (leaf index range)
    uint8_t key0[32];   // first key of the interval (ext path nibbles)
    uint8_t rlp[536];
};
static_assert(sizeof(proof_row) == 588, "proof_row layout");

// Host-side Keccak-256 (FIPS-202 restatement, independent of oracle/) —
// used only to derive extension-node child references while assembling
// proof node lists host-side; all bulk hashing stays on the GPU.
static void h_keccak_f(uint64_t s[25])
{
    static const uint64_t RC[24] = {
        0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL,
        0x8000000080008000ULL, 0x000000000000808bULL, 0x0000000080000001ULL,
        0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL,
        0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
        0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
        0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL,
        0x000000000000800aULL, 0x800000008000000aULL, 0x8000000080008081ULL,
        0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    static const int ROT[25] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3, 10, 43,
                                25, 39, 41, 45, 15, 21, 8,  18, 2,  61, 56, 14};
    auto rotl = [](uint64_t v, int r) {
        return r ? (v << r) | (v >> (64 - r)) : v;
    };
    for (int r = 0; r < 24; ++r) {
        uint64_t c[5], dd[5], b[25];
        for (int x = 0; x < 5; ++x)
            c[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];
        for (int x = 0; x < 5; ++x)
            dd[x] = c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1);
        for (int i = 0; i < 25; ++i)
            s[i] ^= dd[i % 5];
        for (int x = 0; x < 5; ++x)
            for (int y = 0; y < 5; ++y)
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(s[x + 5 * y],
                                                        ROT[x + 5 * y]);
        for (int y = 0; y < 5; ++y)
            for (int x = 0; x < 5; ++x)
                s[x + 5 * y] = b[x + 5 * y] ^
                               ((~b[(x + 1) % 5 + 5 * y]) &
                                b[(x + 2) % 5 + 5 * y]);
        s[0] ^= RC[r];
    }
}

static void h_keccak256(const uint8_t *msg, size_t len, uint8_t out[32])
{
    uint64_t s[25] = {0};
    auto absorb = [&](const uint8_t *blk) {
        for (int i = 0; i < 17; ++i) {
            uint64_t w;
            memcpy(&w, blk + 8 * i, 8);
            s[i] ^= w;
        }
        h_keccak_f(s);
    };
    size_t off = 0;
    for (; len - off >= 136; off += 136)
        absorb(msg + off);
    uint8_t blk[136] = {0};
    if (len > off) // msg may be null for the empty message
        memcpy(blk, msg + off, len - off);
    blk[len - off] = 0x01;
    blk[135] |= 0x80;
    absorb(blk);
    memcpy(out, s, 32);
}

static inline int h_nib(const uint8_t *key, int i)
{
    return (i & 1) ? (key[i >> 1] & 0xF) : (key[i >> 1] >> 4);
}

// RLP string of n < 256 bytes: a single byte < 0x80 stays bare, 56 bytes
// and more take the 0xb8 length form. Returns bytes written.
static int h_rlp_str(uint8_t *dst, const uint8_t *p, int n)
{
    int w = 0;
    if (n >= 56)
        dst[w++] = 0xb8;
    if (n != 1 || p[0] >= 0x80)
        dst[w++] = (uint8_t)(n < 56 ? 0x80 + n : n);
    memcpy(dst + w, p, n);
    return w + n;
}

// RLP string item of the hex-prefix-encoded path key[from..to) (HP per the
// yellow paper; in-repo shape proof_v2/node.rs:30-68). Returns bytes written.
static int h_hp_item(uint8_t *dst, const uint8_t *key, int from, int to,
                     int leaf)
{
    int n = to - from;
    int hl = 1 + n / 2;
    uint8_t hp[34];
    int odd = n & 1;
    hp[0] = (uint8_t)((leaf ? 0x20 : 0x00) | (odd ? 0x10 | h_nib(key, from) : 0));
    int p = 1, i = from + odd;
    for (; i < to; i += 2)
        hp[p++] = (uint8_t)((h_nib(key, i) << 4) | h_nib(key, i + 1));
    return h_rlp_str(dst, hp, hl);
}

// RLP of a big-endian unsigned integer (nonce / balance), minimal form.
static int h_rlp_uint(uint8_t *dst, const uint8_t *be, int len)
{
    int s = 0;
    while (s < len && be[s] == 0)
        s++;
    return h_rlp_str(dst, be + s, len - s); // zero is the empty string
}

static int h_rlp_list_hdr(uint8_t *dst, int payload)
{
    int w = 0;
    if (payload >= 56)
        dst[w++] = 0xf8;
    dst[w++] = (uint8_t)(payload < 56 ? 0xc0 + payload : payload);
    return w;
}

// Leaf node RLP: [HP(key[from..64), leaf), val as an RLP string]
static int h_leaf(uint8_t *dst, const uint8_t *key, int from,
                  const uint8_t *val, int vp)
{
    uint8_t hp[40], sv[124];
    int hl = h_hp_item(hp, key, from, 64, 1), sl = h_rlp_str(sv, val, vp);
    int w = h_rlp_list_hdr(dst, hl + sl);
    memcpy(dst + w, hp, hl);
    memcpy(dst + w + hl, sv, sl);
    return w + hl + sl;
}

// Account leaf node RLP: [HP(short,1), RLP_string(RLP([nonce,balance,
// storage_root,code_hash]))] (trie.rs:472-476; proof_v2/value.rs:55-139).
static int h_leaf_node(uint8_t *dst, const uint8_t *key, int from,
                       const sre_account_entry *a,
                       const uint8_t storage_root[32])
{
    uint8_t val[120], body[112], nb[8];
    for (int i = 0; i < 8; ++i)
        nb[i] = (uint8_t)(a->nonce >> (8 * (7 - i)));
    int bp = h_rlp_uint(body, nb, 8);
    bp += h_rlp_uint(body + bp, a->balance, 32);
    body[bp++] = 0xa0;
    memcpy(body + bp, storage_root, 32);
    bp += 32;
    body[bp++] = 0xa0;
    memcpy(body + bp, a->code_hash, 32);
    bp += 32;
    int vp = h_rlp_list_hdr(val, bp);
    memcpy(val + vp, body, bp);
    return h_leaf(dst, key, from, val, vp + bp);
}

// Storage leaf node RLP: [HP(short,1), RLP_string(RLP(U256 value))]
// (trie.rs:819-825 encode_fixed_size; proof_v2/value.rs:55).
static int h_storage_leaf(uint8_t *dst, const uint8_t *slot_key, int from,
                          const uint8_t value_be[32])
{
    uint8_t val[40];
    return h_leaf(dst, slot_key, from, val, h_rlp_uint(val, value_be, 32));
}

// build the ext-wrapper bytes for a captured row (path nibbles from the
// row's own first key — valid for on-path and sibling rows alike)
static void h_row_ext(const proof_row *r, std::vector<uint8_t> &out)
{
    uint8_t cref[33], hp[40];
    int crl = (int)r->br_len, hl = h_hp_item(hp, r->key0, r->P + 1, r->d, 0);
    if (crl >= 32) { // by hash; a shorter child is embedded as it is
        cref[0] = 0xa0;
        h_keccak256(r->rlp, crl, cref + 1);
        crl = 33;
    } else {
        memcpy(cref, r->rlp, crl);
    }
    out.resize(2 + hl + crl);
    int w = h_rlp_list_hdr(out.data(), hl + crl);
    memcpy(out.data() + w, hp, hl);
    memcpy(out.data() + w + hl, cref, crl);
    out.resize(w + hl + crl);
}

// ---- proof assembly: RLP list parser + semantic walk -----------------
// The emitted proof is exactly the node chain a verifier walks from the
// root by the target's nibbles (eth_getProof / ProofRetainer semantics):
// present keys end at the target leaf, absent keys end at the first
// divergence (empty branch slot, mismatching extension/leaf path). Inline
// (<32 B) nodes are traversed in place and never emitted.
struct h_item {
    const uint8_t *p; // a string's payload; a list's whole encoding
    int len;
    bool is_list;
};

// Header of the RLP item at b[i..end): *hdr header bytes, *pl payload bytes.
// -1 when the header would run past end or holds a length no trie node has
// (they are a few hundred bytes); the payload is not checked against end.
static int h_rlp_head(const uint8_t *b, int i, int end, int *hdr, int *pl,
                      bool *is_list)
{
    if (i >= end)
        return -1;
    uint8_t c = b[i];
    *is_list = c >= 0xc0;
    int base = *is_list ? 0xc0 : 0x80;
    *hdr = c < 0x80 ? 0 : 1;
    *pl = c < 0x80 ? 1 : c - base;
    if (c < base + 56)
        return 0;
    int n = *pl - 55; // long form: n big-endian length bytes follow
    if (n > 3 || i + 1 + n > end)
        return -1;
    *hdr = 1 + n;
    *pl = 0;
    for (int k = 0; k < n; ++k)
        *pl = (*pl << 8) | b[i + 1 + k];
    return 0;
}

// Items of the RLP list b[0..len); -1 for anything that is not exactly one
// well-formed list. Never reads at or past b + len.
static int h_rlp_list_items(const uint8_t *b, int len, std::vector<h_item> &out)
{
    int hdr, pl;
    bool is_list;
    if (h_rlp_head(b, 0, len, &hdr, &pl, &is_list) || !is_list ||
        hdr + pl != len)
        return -1;
    for (int i = hdr; i < len; i += hdr + pl) {
        h_item it{};
        if (h_rlp_head(b, i, len, &hdr, &pl, &it.is_list) || i + hdr + pl > len)
            return -1;
        it.p = it.is_list ? b + i : b + i + hdr;
        it.len = it.is_list ? hdr + pl : pl;
        out.push_back(it);
    }
    return 0;
}

typedef std::array<uint8_t, 32> hkey;
typedef std::map<hkey, std::pair<const uint8_t *, int>> node_map;

static void map_add(node_map &m, const uint8_t *b, int len)
{
    hkey k;
    h_keccak256(b, len, k.data());
    m.emplace(k, std::make_pair(b, len));
}

// returns 0 = reached the target leaf (present), 1 = divergence proven
// (absent), -1 = internal error with *why set (emit sets it for its own
// failures). Emits each hash-referenced node visited.
template <typename EmitFn>
static int proof_walk_emit(const uint8_t root[32], const node_map &byhash,
                           const uint8_t *key, EmitFn &&emit, const char **why)
{
    auto fail = [&](const char *reason) {
        *why = reason;
        return -1;
    };
    auto find = [&](const uint8_t *hash) {
        hkey k;
        memcpy(k.data(), hash, 32);
        return byhash.find(k);
    };
    auto it = find(root);
    if (it == byhash.end())
        return fail("proof: root node missing from capture");
    const uint8_t *cur = it->second.first;
    int clen = it->second.second;
    bool emit_cur = true;
    int pos = 0;
    for (int guard = 0; guard < 200; ++guard) {
        if (emit_cur && emit(cur, clen))
            return -1;
        std::vector<h_item> items;
        if (h_rlp_list_items(cur, clen, items))
            return fail("proof: malformed node");
        const h_item *next = nullptr;
        if (items.size() == 17) {
            if (pos >= 64)
                return fail("proof: branch below leaf depth");
            const h_item &c = items[h_nib(key, pos)];
            if (!c.is_list && c.len == 0)
                return 1; // empty child slot: absence proven
            pos++;
            next = &c;
        } else if (items.size() == 2) {
            const uint8_t *hp = items[0].p;
            int hl = items[0].len;
            if (items[0].is_list || hl < 1) // no hex-prefix flag byte
                return fail("proof: malformed node");
            int flag = hp[0] >> 4;
            bool is_leaf = (flag & 2) != 0;
            int np = (hl - 1) * 2 + ((flag & 1) ? 1 : 0);
            bool match = pos + np <= 64;
            // the path starts at hp's nibble 1 (odd length) or 2 (even)
            for (int k = 0; match && k < np; ++k)
                match = h_nib(hp, k + 2 - (flag & 1)) == h_nib(key, pos + k);
            if (!match)
                return 1; // path mismatch: absence proven
            pos += np;
            if (is_leaf) {
                if (pos != 64)
                    return fail("proof: leaf at wrong depth");
                return 0; // target leaf reached
            }
            next = &items[1];
        } else {
            return fail("proof: unexpected node arity");
        }
        if (!next->is_list && next->len == 32) {
            auto jt = find(next->p);
            if (jt == byhash.end())
                return fail("proof: child node missing from capture");
            cur = jt->second.first;
            clen = jt->second.second;
            emit_cur = true;
        } else { // inline embedded node: traverse, do not emit
            cur = next->p;
            clen = next->len;
            emit_cur = false;
        }
    }
    return fail("proof: walk did not terminate");
}

// Where a call's proofs go: node bytes back to back in nodes, one length per
// node in lens; nb / nl run on across the call's targets. full is the reason
// reported when either runs out (it names the entry point).
struct proof_sink {
    uint8_t *nodes;
    uint64_t cap_nodes;
    uint32_t *lens;
    uint64_t cap_lens;
    const char *full;
    uint64_t nb = 0, nl = 0;
};

// One target's proof. The node universe is the target's captured branches
// (rows, root-first), their extension wrappers, and the already-encoded
// candidate leaves; the walk from root by key picks the proof out of it and
// appends it to out, its node count to *count. Returns as proof_walk_emit.
static int proof_assemble(const uint8_t root[32], const uint8_t *key,
                          const std::vector<const proof_row *> &rows,
                          const std::vector<std::vector<uint8_t>> &leaves,
                          proof_sink &out, uint32_t *count, const char **why)
{
    node_map byhash;
    std::vector<std::vector<uint8_t>> exts;
    exts.reserve(rows.size()); // byhash points into these: no reallocation
    for (const proof_row *r : rows) {
        map_add(byhash, r->rlp, (int)r->br_len);
        if (r->d > r->P + 1) {
            exts.emplace_back();
            h_row_ext(r, exts.back());
            map_add(byhash, exts.back().data(), (int)exts.back().size());
        }
    }
    for (const auto &l : leaves)
        map_add(byhash, l.data(), (int)l.size());
    uint32_t cnt = 0;
    auto emit = [&](const uint8_t *node, int len) -> int {
        if (out.nl >= out.cap_lens || out.nb + (uint64_t)len > out.cap_nodes) {
            *why = out.full;
            return -1;
        }
        memcpy(out.nodes + out.nb, node, len);
        out.nb += len;
        out.lens[out.nl++] = (uint32_t)len;
        cnt++;
        return 0;
    };
    int rc = proof_walk_emit(root, byhash, key, emit, why);
    if (rc >= 0)
        *count = cnt;
    return rc;
}
