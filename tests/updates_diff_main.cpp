// Stand-alone host check of reth_amd/csrc/updates_diff.h (built and run by
// tests/test_updates_diff_cpu.py): row_less and snap_cmp are one order, and
// updates_net_diff agrees with a std::map model of the stored row set.
// Self-contained, fixed seed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "updates_diff.h"

static const int N_PAIRS = 200000, N_SCENARIOS = 2000, N_CELLS = 1 << 20;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static int below(int n) { return (int)(rnd() % (uint64_t)n); }

static long n_checked = 0, n_failed = 0;

static void check(bool ok, const char *what, long at)
{
    ++n_checked;
    if (!ok && n_failed++ < 10)
        fprintf(stderr, "%s (at %ld)\n", what, at);
}

typedef std::vector<uint8_t> nibbles;

// the four account keys, ascending with a: they differ in a middle, the
// last or the first byte
static void acct_key(int a, uint8_t k[32])
{
    memset(k, 0x55, 32);
    if (a == 0)
        k[13] = 0x54;
    if (a == 2)
        k[31] = 0x56;
    if (a == 3)
        k[0] = 0xd5;
}

// a row with this key and no content: packed path, zero beyond path_len
static sre_update_row key_row(int kind, int acct, const nibbles &path)
{
    sre_update_row r{};
    r.kind = (uint8_t)kind;
    acct_key(acct, r.acct_key);
    r.path_len = (uint8_t)path.size();
    for (size_t k = 0; k < path.size(); ++k)
        r.path[k / 2] |= (uint8_t)(path[k] << ((k & 1) ? 0 : 4));
    return r;
}

static void random_content(sre_update_row &r)
{
    r.state_mask = (uint16_t)rnd();
    r.tree_mask = (uint16_t)rnd();
    r.hash_mask = (uint16_t)rnd();
    r.num_hashes = (uint8_t)below(4);
    r.root_hash_set = (uint8_t)below(2);
    for (int k = 0; k < 32; ++k)
        r.root_hash[k] = (uint8_t)rnd();
    for (int h = 0; h < r.num_hashes; ++h)
        for (int k = 0; k < 32; ++k)
            r.hashes[h][k] = (uint8_t)rnd();
}

// ---- order agreement ---------------------------------------------------
static nibbles random_path(int len, int alphabet)
{
    nibbles p(len);
    for (auto &n : p)
        n = (uint8_t)(alphabet == 16 ? below(16) : 15 * below(2));
    return p;
}

static int sign(int v) { return (v > 0) - (v < 0); }

static void check_orders()
{
    for (int k = 0; k < N_PAIRS; ++k) {
        // nibbles from {0, f} or from all 16; b shares a random-length
        // prefix with a three times out of four, often all of a or of b
        int alphabet = (k & 1) ? 16 : 2;
        nibbles pa = random_path(below(65), alphabet);
        nibbles pb = random_path(below(65), alphabet);
        if (k & 6) {
            size_t share = (k & 8) ? (size_t)below(65) : pa.size();
            for (size_t i = 0; i < share && i < pa.size() && i < pb.size(); ++i)
                pb[i] = pa[i];
        }
        int ka = below(2), kb = (k & 16) ? ka : below(2);
        int aa = below(4), ab = (k & 32) ? aa : below(4);
        sre_update_row a = key_row(ka, aa, pa), b = key_row(kb, ab, pb);
        snap_row sa = snap_of(a), sb = snap_of(b);
        int ab_ = snap_cmp(sa, sb), ba_ = snap_cmp(sb, sa);
        check(row_less(a, b) == (ab_ < 0) && row_less(b, a) == (ba_ < 0) &&
                  sign(ab_) == -sign(ba_) && !(row_less(a, b) && row_less(b, a)),
              "row_less / snap_cmp disagree", k);
    }
}

// ---- net diff against a model ------------------------------------------
// kind, account (kind 1 only), then one char per path nibble: the order of
// these strings is the into_sorted order, stated without row_less or snap_cmp
typedef std::string model_key;
typedef std::map<model_key, sre_update_row> model;

static model_key key_of(int kind, int acct, const nibbles &path)
{
    model_key k{(char)kind, (char)(kind ? acct : 0)};
    return k.append(path.begin(), path.end());
}

static uint32_t cell_of(const nibbles &p) // 5-nibble cell of a deep account row
{
    return (uint32_t)p[0] << 16 | p[1] << 12 | p[2] << 8 | p[3] << 4 | p[4];
}

static bool same_rows(const model &m, const std::vector<snap_row> &s)
{
    if (m.size() != s.size())
        return false;
    size_t i = 0;
    for (const auto &kv : m) {
        const sre_update_row &r = kv.second;
        const snap_row &q = s[i++];
        if (q.kind != r.kind || q.path_len != r.path_len ||
            memcmp(q.path, r.path, 32) || q.h64 != row_h64(r) ||
            (r.kind == 1 && memcmp(q.acct_key, r.acct_key, 32)))
            return false;
    }
    return true;
}

static bool same_models(const model &a, const model &b)
{
    if (a.size() != b.size())
        return false;
    for (auto i = a.begin(), j = b.begin(); i != a.end(); ++i, ++j)
        if (i->first != j->first || row_h64(i->second) != row_h64(j->second))
            return false;
    return true;
}

// which way each snapshot / emitted row went, counted from the model's side
enum {
    UNCHANGED, CHANGED, NEW, GONE_DESTROYED, GONE_SHALLOW, GONE_ALL_REGION,
    GONE_DIRTY_CELL, GONE_TOUCHED, KEPT_CLEAN_CELL, KEPT_UNTOUCHED, N_WAYS
};
static long ways[N_WAYS];

static void check_net_diff()
{
    std::vector<uint8_t> cells(N_CELLS, 0);
    for (int sc = 0; sc < N_SCENARIOS; ++sc) {
        // accounts: destroyed, touched or neither
        bool is_destroyed[4], is_touched[4];
        std::vector<key32> touched, destroyed;
        for (int a = 0; a < 4; ++a) {
            int what = below(4);
            is_destroyed[a] = what == 0;
            is_touched[a] = what == 1 || what == 2;
            uint8_t k[32];
            acct_key(a, k);
            if (is_destroyed[a])
                destroyed.push_back(key32_of(k));
            if (is_touched[a])
                touched.push_back(key32_of(k));
        }
        // a pool of keys for both row sets to draw from, so they collide
        struct pooled {
            int kind, acct;
            nibbles path;
        };
        std::vector<pooled> pool(8 + below(40));
        for (auto &p : pool) {
            p.kind = below(2);
            p.acct = below(4);
            static const int lens[] = {0, 1, 3, 4, 5, 6, 8};
            p.path = random_path(lens[below(7)], 2);
        }
        // dirty cells: none (all of the state is region), or about half of
        // the cells the pool's deep account rows lie in
        bool no_bitmap = below(8) == 0;
        std::vector<uint32_t> dirty;
        for (const auto &p : pool)
            if (p.kind == 0 && p.path.size() > 4 && below(2))
                dirty.push_back(cell_of(p.path));
        for (uint32_t c : dirty)
            cells[c] = 1;
        const std::vector<uint8_t> none;
        const std::vector<uint8_t> &bitmap = no_bitmap ? none : cells;

        model old_rows, emitted;
        for (int k = below(33); k > 0; --k) {
            const pooled &p = pool[below((int)pool.size())];
            sre_update_row r = key_row(p.kind, p.acct, p.path);
            random_content(r);
            old_rows[key_of(p.kind, p.acct, p.path)] = r;
        }
        for (int k = below(33); k > 0; --k) {
            const pooled &p = pool[below((int)pool.size())];
            if (p.kind == 1 && is_destroyed[p.acct])
                continue; // a destroyed account's trie emits nothing
            model_key key = key_of(p.kind, p.acct, p.path);
            sre_update_row r = key_row(p.kind, p.acct, p.path);
            auto was = old_rows.find(key);
            if (was != old_rows.end() && below(2))
                r = was->second; // re-emitted unchanged
            else
                random_content(r);
            r.removed = (uint8_t)below(3); // whatever the emitter left there
            emitted[key] = r;
        }

        // the model: old rows, minus destroyed accounts' rows, minus region
        // rows not re-emitted, plus the emitted rows
        model want;
        for (const auto &kv : old_rows) {
            int kind = kv.first[0], acct = kv.first[1];
            nibbles path(kv.first.begin() + 2, kv.first.end());
            auto em = emitted.find(kv.first);
            if (em != emitted.end()) {
                ways[row_h64(em->second) == row_h64(kv.second) ? UNCHANGED
                                                               : CHANGED]++;
                continue; // the emitted row replaces it below
            }
            int way;
            if (kind == 1)
                way = is_destroyed[acct] ? GONE_DESTROYED
                      : is_touched[acct] ? GONE_TOUCHED
                                         : KEPT_UNTOUCHED;
            else if (path.size() <= 4)
                way = GONE_SHALLOW;
            else if (no_bitmap)
                way = GONE_ALL_REGION;
            else
                way = cells[cell_of(path)] ? GONE_DIRTY_CELL : KEPT_CLEAN_CELL;
            ways[way]++;
            if (way == KEPT_UNTOUCHED || way == KEPT_CLEAN_CELL)
                want.insert(kv);
        }
        for (const auto &kv : emitted) {
            if (!old_rows.count(kv.first))
                ways[NEW]++;
            want[kv.first] = kv.second;
        }

        // inputs as the engine holds them: the snapshot sorted, the emission
        // in no particular order (here: reversed)
        std::vector<snap_row> snap, nsnap;
        for (const auto &kv : old_rows)
            snap.push_back(snap_of(kv.second));
        std::vector<sre_update_row> E, diff;
        for (auto it = emitted.rbegin(); it != emitted.rend(); ++it)
            E.push_back(it->second);
        updates_net_diff(snap, E, bitmap, touched, destroyed, diff, nsnap);

        check(same_rows(want, nsnap), "new snapshot != model", sc);

        // the diff applied to the old set, in order
        model applied = old_rows;
        bool sorted = true, all_changed = true;
        std::map<int, int> markers;
        for (size_t k = 0; k < diff.size(); ++k) {
            const sre_update_row &r = diff[k];
            if (k && row_less(r, diff[k - 1]))
                sorted = false;
            int acct = -1;
            for (int a = 0; a < 4; ++a) {
                uint8_t key[32];
                acct_key(a, key);
                if (r.kind == 1 && !memcmp(key, r.acct_key, 32))
                    acct = a;
            }
            nibbles path(r.path_len);
            for (size_t i = 0; i < path.size(); ++i)
                path[i] = (r.path[i / 2] >> ((i & 1) ? 0 : 4)) & 0xf;
            model_key key = key_of(r.kind, acct, path);
            if (r.removed == 0) {
                auto was = old_rows.find(key);
                if (was != old_rows.end() &&
                    row_h64(was->second) == row_h64(r))
                    all_changed = false;
                applied[key] = r;
            } else if (r.removed == 1) {
                applied.erase(key);
            } else {
                markers[acct]++;
                for (auto it = applied.begin(); it != applied.end();)
                    if (it->first[0] == 1 && it->first[1] == acct)
                        it = applied.erase(it);
                    else
                        ++it;
            }
        }
        check(same_models(applied, want), "old rows + diff != model", sc);
        check(sorted, "diff not sorted by row_less", sc);
        check(all_changed, "diff upserts an unchanged row", sc);
        bool one_each = markers.size() == destroyed.size();
        for (int a = 0; a < 4; ++a)
            if (is_destroyed[a] && markers[a] != 1)
                one_each = false;
        check(one_each, "not one removed=2 marker per destroyed key", sc);

        for (uint32_t c : dirty)
            cells[c] = 0;
    }
    // every branch of the merge loop was taken
    static const char *names[N_WAYS] = {
        "unchanged", "changed", "new", "gone: destroyed", "gone: shallow",
        "gone: no bitmap", "gone: dirty cell", "gone: touched",
        "kept: clean cell", "kept: untouched"};
    for (int w = 0; w < N_WAYS; ++w)
        check(ways[w] > 0, names[w], ways[w]);
}

int main()
{
    check_orders();
    check_net_diff();
    printf("checked %ld failed %ld\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
