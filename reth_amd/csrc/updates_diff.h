// Host-side TrieUpdates ordering and the incremental NET diff
// (sre_root_retaining_with_updates / sre_incremental_root_with_updates),
// plus the sorted 32-byte key lists the delta entry points derive on the
// host. Plain C++17, no HIP and no engine context, so
// tests/updates_diff_main.cpp checks it as a sanitizer-built host program.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/sre.h"

// ---- sorted 32-byte key lists ------------------------------------------
typedef std::array<uint8_t, 32> key32;

static key32 key32_of(const uint8_t *k)
{
    key32 a;
    memcpy(a.data(), k, 32);
    return a;
}

// is k a member of the ascending list v?
static bool key_in(const std::vector<key32> &v, const uint8_t *k)
{
    auto it = std::lower_bound(v.begin(), v.end(), k,
                               [](const key32 &a, const uint8_t *b) {
                                   return memcmp(a.data(), b, 32) < 0;
                               });
    return it != v.end() && memcmp(it->data(), k, 32) == 0;
}

// distinct account keys of a storage delta sorted by (acct_key, slot_key):
// ascending, and contiguous in memory for upload (32 B per key)
static std::vector<key32> storage_delta_accounts(const sre_storage_entry *st,
                                                 uint64_t n_st)
{
    std::vector<key32> keys;
    for (uint64_t i = 0; i < n_st; ++i)
        if (i == 0 || memcmp(st[i].acct_key, st[i - 1].acct_key, 32) != 0)
            keys.push_back(key32_of(st[i].acct_key));
    return keys;
}

// keys of the accounts a (key-sorted) account delta deletes
static std::vector<key32> deleted_accounts(const sre_account_delta *ad,
                                           uint64_t n_acct)
{
    std::vector<key32> keys;
    for (uint64_t i = 0; i < n_acct; ++i)
        if (ad[i].deleted)
            keys.push_back(key32_of(ad[i].key));
    return keys;
}

// ---- row order and snapshot --------------------------------------------
// same ordering as reth's TrieUpdates::into_sorted (updates.rs): account
// rows first (path-sorted), then storage rows grouped by account key
static bool row_less(const sre_update_row &a, const sre_update_row &b)
{
    if (a.kind != b.kind)
        return a.kind < b.kind;
    if (a.kind == 1) {
        int c = memcmp(a.acct_key, b.acct_key, 32);
        if (c)
            return c < 0;
    }
    int minl = a.path_len < b.path_len ? a.path_len : b.path_len;
    for (int k = 0; k < minl; ++k) {
        uint8_t na_ = (a.path[k / 2] >> ((k & 1) ? 0 : 4)) & 0xf;
        uint8_t nb_ = (b.path[k / 2] >> ((k & 1) ? 0 : 4)) & 0xf;
        if (na_ != nb_)
            return na_ < nb_;
    }
    return a.path_len < b.path_len;
}

// One stored row of the CURRENT trie, as (sort key, 64-bit content hash):
// the retained row-set snapshot that lets the incremental mode emit a NET
// TrieUpdates diff (upserts/removals) per delta. Content equality by h64
// (FNV-1a over masks+hashes+root fields; collision odds are ~1e-19 per
// pair — far below the GPU's own soft-error rate).
struct snap_row {
    uint8_t kind, path_len;
    uint8_t acct_key[32];
    uint8_t path[32];
    uint64_t h64;
};

// FNV-1a over a row's content (masks + hashes + root fields): the snapshot
// compares rows by this to suppress unchanged re-emits from the net diff.
static uint64_t row_h64(const sre_update_row &r)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t n) {
        const uint8_t *b = (const uint8_t *)p;
        for (size_t i = 0; i < n; ++i) {
            h ^= b[i];
            h *= 1099511628211ull;
        }
    };
    mix(&r.state_mask, 2);
    mix(&r.tree_mask, 2);
    mix(&r.hash_mask, 2);
    mix(&r.num_hashes, 1);
    mix(&r.root_hash_set, 1);
    mix(r.root_hash, 32);
    mix(&r.hashes[0][0], 32ull * r.num_hashes);
    return h;
}

static snap_row snap_of(const sre_update_row &r)
{
    snap_row s{};
    s.kind = r.kind;
    s.path_len = r.path_len;
    memcpy(s.acct_key, r.acct_key, 32);
    memcpy(s.path, r.path, 32);
    s.h64 = row_h64(r);
    return s;
}

// 3-way key compare, the same total order as row_less: paths are packed
// high-nibble-first and zero-padded, so a 32-byte memcmp + length
// tiebreak IS the nibble-lexicographic prefix-first order.
static int snap_cmp(const snap_row &a, const snap_row &b)
{
    if (a.kind != b.kind)
        return a.kind < b.kind ? -1 : 1;
    if (a.kind == 1) {
        int c = memcmp(a.acct_key, b.acct_key, 32);
        if (c)
            return c;
    }
    int c = memcmp(a.path, b.path, 32);
    if (c)
        return c;
    return (int)a.path_len - (int)b.path_len;
}

// NET diff: emitted rows vs the retained snapshot. The engine re-emits
// every row in the rebuilt region (depth <= 4 account rows, dirty/uncovered
// cells, rebuilt storage tries); unchanged re-emits are suppressed by
// content hash, region rows missing from the emission become removals
// (walker.rs:363-369 semantics), destroyed accounts get whole-trie markers
// (updates.rs:154-157).
//   snap      the retained snapshot, sorted by snap_cmp
//   E         the rows this pass emitted, in any order
//   bitmap    dirty 5-nibble account-trie cells; empty = the delta emptied
//             the state, everything is rebuilt region
//   touched   accounts whose storage trie was rebuilt   (ascending)
//   destroyed accounts the delta deleted                (ascending)
// Out: diff sorted by row_less, and the new snapshot.
static void updates_net_diff(const std::vector<snap_row> &snap,
                             std::vector<sre_update_row> E,
                             const std::vector<uint8_t> &bitmap,
                             const std::vector<key32> &touched,
                             const std::vector<key32> &destroyed,
                             std::vector<sre_update_row> &diff,
                             std::vector<snap_row> &nsnap)
{
    std::sort(E.begin(), E.end(), row_less);
    std::vector<snap_row> Es;
    Es.reserve(E.size());
    for (auto &r : E) {
        r.removed = 0;
        Es.push_back(snap_of(r));
    }
    auto in_region = [&](const snap_row &s) {
        if (s.kind == 0) {
            if (s.path_len <= 4 || bitmap.empty())
                return true;
            uint32_t cell = ((uint32_t)s.path[0] << 12) |
                            ((uint32_t)s.path[1] << 4) |
                            ((uint32_t)s.path[2] >> 4);
            return bitmap[cell] != 0;
        }
        return key_in(touched, s.acct_key);
    };

    diff.clear();
    nsnap.clear();
    nsnap.reserve(snap.size() + Es.size());
    size_t i = 0, j = 0;
    while (i < snap.size() || j < Es.size()) {
        int c = i >= snap.size() ? 1
                : j >= Es.size() ? -1
                                 : snap_cmp(snap[i], Es[j]);
        if (c >= 0) { // emitted row: new (c > 0), changed or unchanged
            if (c > 0 || snap[i].h64 != Es[j].h64)
                diff.push_back(E[j]);
            nsnap.push_back(Es[j]);
            i += c == 0;
            j++;
        } else { // snapshot row not re-emitted this pass
            const snap_row &s = snap[i];
            if (s.kind == 1 && key_in(destroyed, s.acct_key)) {
                // dropped wholesale; the removed=2 marker covers the trie
            } else if (in_region(s)) {
                sre_update_row rr{};
                rr.kind = s.kind;
                rr.path_len = s.path_len;
                memcpy(rr.path, s.path, 32);
                if (s.kind == 1)
                    memcpy(rr.acct_key, s.acct_key, 32);
                rr.removed = 1;
                diff.push_back(rr);
            } else {
                nsnap.push_back(s); // untouched region: row kept
            }
            i++;
        }
    }
    for (const auto &k : destroyed) { // StorageTrieUpdates::set_deleted(true)
        sre_update_row rr{};
        rr.kind = 1;
        memcpy(rr.acct_key, k.data(), 32);
        rr.removed = 2;
        diff.push_back(rr);
    }
    std::sort(diff.begin(), diff.end(), row_less);
}
