// Stand-alone host check of reth_amd/csrc/revert_plan.h (built and run by
// tests/test_revert_plan_cpu.py): the row decisions and the position
// formulas of the revert capture, against a std::map model of "the revert
// of a delta restores the pre-delta state". The program plays the capture
// kernels (k_rv_acct, k_rv_st, k_rv_seg_base, k_rv_copy_segs) with a
// lower bound that, like the device one, stays in range on unsorted input.
// Self-contained, fixed seed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "revert_plan.h"

static const int N_RANDOM = 3000, N_BAD = 1500;

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

// the scenarios the capture has to get right; each must be hit at least once
enum {
    DESTROYED_FIRST, DESTROYED_LAST, ADJ_DESTROYED, ROWS_BEFORE, ROWS_BETWEEN,
    ROWS_AFTER, EMPTY_SEGMENT, ZERO_EMITTED, NOTHING_AT_ALL, UNSORTED, DUPLICATE,
    N_NAMED
};
static long named[N_NAMED];

typedef std::pair<int, int> slot_t;             // (account, slot)
typedef std::map<int, int> accounts_t;          // key -> nonce
typedef std::map<slot_t, int> storage_t;        // (account, slot) -> value != 0
struct arow { int key, nonce; bool deleted; };  // account delta row
struct srow { int acct, slot, value; };         // storage delta row, 0 deletes

struct delta_t {
    std::vector<arow> a;
    std::vector<srow> s;
};

// lb_keys of the engine: first index whose key is not below `key`; on
// unsorted rows still a value in [0, n]
template <typename Row, typename Less>
static uint64_t lb(const std::vector<Row> &rows, Less below_key)
{
    uint64_t lo = 0, hi = rows.size();
    while (lo < hi) {
        uint64_t mid = (lo + hi) / 2;
        if (below_key(rows[mid]))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// ---- the model: overlay semantics and the definition of the revert -------
static void apply(accounts_t &acc, storage_t &st, const delta_t &d)
{
    for (const arow &r : d.a) {
        if (r.deleted) {
            acc.erase(r.key);
            st.erase(st.lower_bound({r.key, -1}), st.lower_bound({r.key + 1, -1}));
        } else {
            acc[r.key] = r.nonce;
        }
    }
    for (const srow &r : d.s) {
        if (r.value)
            st[{r.acct, r.slot}] = r.value;
        else
            st.erase({r.acct, r.slot});
    }
}

static delta_t model_revert(const accounts_t &acc, const storage_t &st,
                            const delta_t &d)
{
    delta_t out;
    std::map<slot_t, int> rows;
    std::set<int> inserted;
    for (const arow &r : d.a) {
        auto it = acc.find(r.key);
        if (it != acc.end()) {
            out.a.push_back({r.key, it->second, false});
            if (r.deleted)
                for (auto s = st.lower_bound({r.key, -1});
                     s != st.end() && s->first.first == r.key; ++s)
                    rows[s->first] = s->second;
        } else if (!r.deleted) {
            inserted.insert(r.key);
            out.a.push_back({r.key, 0, true});
        }
    }
    for (const srow &r : d.s) {
        if (inserted.count(r.acct) || !acc.count(r.acct))
            continue;
        auto it = st.find({r.acct, r.slot});
        if (it != st.end())
            rows[it->first] = it->second;
        else if (r.value)
            rows[{r.acct, r.slot}] = 0;
    }
    for (auto &kv : rows)
        out.s.push_back({kv.first.first, kv.first.second, kv.second});
    return out;
}

// ---- the capture pass, played on the host with revert_plan.h -------------
// valid: the delta meets the input contract; then the rows must equal the
// model. Otherwise only the bounds are checked.
static void run(const accounts_t &acc, const storage_t &st, const delta_t &d,
                bool valid, long at)
{
    std::vector<int> A;
    for (auto &kv : acc)
        A.push_back(kv.first);
    std::vector<std::pair<slot_t, int>> S(st.begin(), st.end());
    size_t na = A.size(), ns = S.size(), n_acct = d.a.size(), n_st = d.s.size();

    // k_rv_acct
    std::vector<uint32_t> ka(n_acct), fa(n_acct + 1, 0), src_a(n_acct),
        seglo(n_acct), seglen(n_acct + 1, 0);
    for (size_t k = 0; k < n_acct; ++k) {
        int key = d.a[k].key;
        uint64_t p = lb(A, [key](int a) { return a < key; });
        bool resident = p < na && A[p] == key;
        ka[k] = rv_acct_row(resident, d.a[k].deleted);
        fa[k] = ka[k] != RV_NONE;
        src_a[k] = (uint32_t)p;
        uint64_t lo = 0, hi = 0;
        if (resident && d.a[k].deleted) {
            lo = lb(S, [key](const std::pair<slot_t, int> &r) {
                return r.first.first < key;
            });
            hi = lb(S, [key](const std::pair<slot_t, int> &r) {
                return r.first.first <= key;
            });
        }
        seglo[k] = (uint32_t)lo;
        seglen[k] = (uint32_t)(hi - lo);
    }
    // k_rv_st
    std::vector<uint32_t> ks(n_st), fs(n_st + 1, 0), src_s(n_st), owner(n_st);
    for (size_t j = 0; j < n_st; ++j) {
        const srow &r = d.s[j];
        uint64_t q = lb(d.a, [&r](const arow &a) { return a.key < r.acct; });
        bool destroyed = q < n_acct && d.a[q].key == r.acct && d.a[q].deleted;
        uint64_t a = lb(A, [&r](int k) { return k < r.acct; });
        bool owner_resident = a < na && A[a] == r.acct;
        slot_t key(r.acct, r.slot);
        uint64_t p = lb(S, [&key](const std::pair<slot_t, int> &s) {
            return s.first < key;
        });
        bool slot_resident = p < ns && S[p].first == key;
        ks[j] = rv_st_row(owner_resident, destroyed, slot_resident, r.value != 0);
        fs[j] = ks[j] != RV_NONE;
        src_s[j] = (uint32_t)p;
        owner[j] = (uint32_t)q;
    }
    // the three scans
    std::vector<uint32_t> ea(n_acct + 1, 0), es(n_st + 1, 0), segsum(n_acct + 1, 0);
    for (size_t k = 0; k < n_acct; ++k) {
        ea[k + 1] = ea[k] + fa[k];
        segsum[k + 1] = segsum[k] + seglen[k];
    }
    for (size_t j = 0; j < n_st; ++j)
        es[j + 1] = es[j] + fs[j];
    uint64_t wiped = segsum[n_acct], total = (uint64_t)es[n_st] + wiped;

    // emit
    delta_t got;
    got.a.resize(ea[n_acct]);
    for (size_t k = 0; k < n_acct; ++k)
        if (ka[k] == RV_OLD)
            got.a[ea[k]] = {d.a[k].key, acc.at(A[src_a[k]]), false};
        else if (ka[k] == RV_GONE)
            got.a[ea[k]] = {d.a[k].key, 0, true};
    got.s.assign(total, {-1, -1, -1});
    std::vector<int> written(total, 0);
    bool in_bounds = true;
    for (size_t j = 0; j < n_st; ++j) {
        if (ks[j] == RV_NONE)
            continue;
        uint64_t pos = rv_delta_row_pos(es.data(), j, segsum.data(), owner[j]);
        if (pos >= total || (ks[j] == RV_OLD && src_s[j] >= ns)) {
            in_bounds = false;
            continue;
        }
        got.s[pos] = {d.s[j].acct, d.s[j].slot,
                      ks[j] == RV_OLD ? S[src_s[j]].second : 0};
        ++written[pos];
    }
    // k_rv_seg_base
    std::vector<uint32_t> segp(n_acct, 0);
    for (size_t k = 0; k < n_acct; ++k)
        if (seglen[k]) {
            int key = d.a[k].key;
            segp[k] = (uint32_t)lb(d.s, [key](const srow &r) { return r.acct < key; });
        }
    // k_rv_copy_segs, flat over the wiped rows
    for (uint64_t w = 0; w < wiped; ++w) {
        uint64_t k = rv_segment_of(segsum.data(), n_acct, w);
        if (k >= n_acct || segsum[k] > w || w >= segsum[k + 1]) {
            in_bounds = false;
            continue;
        }
        uint64_t from = seglo[k] + (w - segsum[k]);
        uint64_t pos = rv_segment_row_pos(w, es.data(), segp[k]);
        if (from >= ns || pos >= total) {
            in_bounds = false;
            continue;
        }
        got.s[pos] = {S[from].first.first, S[from].first.second, S[from].second};
        ++written[pos];
    }
    check(in_bounds, "a position or a source index out of bounds", at);
    if (!valid)
        return;

    bool once = true;
    for (int w : written)
        once &= w == 1;
    check(once, "an output position written twice or never", at);
    delta_t want = model_revert(acc, st, d);
    bool same = want.a.size() == got.a.size() && want.s.size() == got.s.size();
    for (size_t i = 0; same && i < want.a.size(); ++i)
        same = want.a[i].key == got.a[i].key && want.a[i].nonce == got.a[i].nonce &&
               want.a[i].deleted == got.a[i].deleted;
    for (size_t i = 0; same && i < want.s.size(); ++i)
        same = want.s[i].acct == got.s[i].acct && want.s[i].slot == got.s[i].slot &&
               want.s[i].value == got.s[i].value;
    check(same, "revert rows != model", at);
    accounts_t acc2 = acc;
    storage_t st2 = st;
    apply(acc2, st2, d);
    apply(acc2, st2, got);
    check(acc2 == acc && st2 == st, "delta then revert != pre state", at);

    // which named scenarios this one is
    std::vector<int> seg_keys; // destroyed accounts with rows, ascending
    for (size_t k = 0; k < n_acct; ++k) {
        if (!(d.a[k].deleted && acc.count(d.a[k].key)))
            continue;
        if (seglen[k])
            seg_keys.push_back(d.a[k].key);
        else
            ++named[EMPTY_SEGMENT];
        if (d.a[k].key == A.front())
            ++named[DESTROYED_FIRST];
        if (d.a[k].key == A.back())
            ++named[DESTROYED_LAST];
    }
    for (size_t i = 1; i < seg_keys.size(); ++i) {
        auto it = acc.find(seg_keys[i - 1]);
        if (++it != acc.end() && it->first == seg_keys[i])
            ++named[ADJ_DESTROYED];
    }
    for (size_t j = 0; j < n_st && !seg_keys.empty(); ++j) {
        if (ks[j] == RV_NONE)
            continue;
        if (d.s[j].acct < seg_keys.front())
            ++named[ROWS_BEFORE];
        else if (d.s[j].acct > seg_keys.back())
            ++named[ROWS_AFTER];
        else
            ++named[ROWS_BETWEEN];
    }
    if (es[n_st] == 0 && wiped)
        ++named[ZERO_EMITTED];
    if (total == 0 && ea[n_acct] == 0 && n_acct + n_st)
        ++named[NOTHING_AT_ALL];
}

// ---- scenarios -------------------------------------------------------------
static void random_state(accounts_t &acc, storage_t &st, int space)
{
    for (int n = below(20); n > 0; --n)
        acc[below(space)] = 100 + below(900);
    for (auto &kv : acc)
        for (int n = below(4) ? below(6) : 0; n > 0; --n)
            st[{kv.first, below(8)}] = 1 + below(99);
}

// a delta that meets the input contract over (acc, st)
static delta_t random_delta(const accounts_t &acc, int space)
{
    delta_t d;
    std::map<int, arow> a;
    for (int n = below(8); n > 0; --n) {
        int k = below(space);
        a[k] = {k, 1000 + below(900), below(2) == 0};
    }
    for (auto &kv : a)
        d.a.push_back(kv.second);
    std::map<slot_t, int> s;
    for (int n = below(12); n > 0; --n) {
        int k = below(space);
        auto it = a.find(k);
        if (it != a.end() && it->second.deleted)
            continue; // a row for a destroyed account is rejected
        bool owned = acc.count(k) || it != a.end();
        s[{k, below(8)}] = owned && below(3) ? 1 + below(99) : 0;
    }
    for (auto &kv : s)
        d.s.push_back({kv.first.first, kv.first.second, kv.second});
    return d;
}

int main()
{
    for (int sc = 0; sc < N_RANDOM; ++sc) {
        accounts_t acc;
        storage_t st;
        int space = 12 + 30 * (sc & 1);
        random_state(acc, st, space);
        run(acc, st, random_delta(acc, space), true, sc);
    }
    // unsorted and duplicate rows, and rows for destroyed accounts: nothing
    // to compare, every position stays below the total
    for (int sc = 0; sc < N_BAD; ++sc) {
        accounts_t acc;
        storage_t st;
        random_state(acc, st, 16);
        delta_t d = random_delta(acc, 16);
        for (int n = 1 + below(3); n > 0; --n) {
            int what = below(4);
            if (what == 0 && d.a.size() >= 2) {
                std::swap(d.a[below((int)d.a.size())], d.a[below((int)d.a.size())]);
                ++named[UNSORTED];
            } else if (what == 1 && !d.a.empty()) {
                arow dup = d.a[below((int)d.a.size())];
                d.a.insert(d.a.begin() + below((int)d.a.size()), dup);
                ++named[DUPLICATE];
            } else if (what == 2 && d.s.size() >= 2) {
                std::swap(d.s[below((int)d.s.size())], d.s[below((int)d.s.size())]);
                ++named[UNSORTED];
            } else if (!d.s.empty()) {
                srow dup = d.s[below((int)d.s.size())];
                d.s.insert(d.s.begin() + below((int)d.s.size()), dup);
                ++named[DUPLICATE];
            } else if (!acc.empty()) { // a row for a destroyed account
                int k = acc.begin()->first;
                d.a = {{k, 0, true}, {k, 0, true}};
                d.s = {{k, 3, 5}, {k, 3, 0}};
                ++named[DUPLICATE];
            }
        }
        run(acc, st, d, false, 100000 + sc);
    }
    // by hand. Accounts 1..5; 1 has 3 rows, 2 has 2, 3 none, 4 has 1, 5 has 2.
    accounts_t acc = {{1, 11}, {2, 12}, {3, 13}, {4, 14}, {5, 15}};
    storage_t st = {{{1, 0}, 7}, {{1, 3}, 8}, {{1, 5}, 9}, {{2, 1}, 6}, {{2, 2}, 5},
                    {{4, 4}, 4}, {{5, 0}, 3}, {{5, 7}, 2}};
    // the first and the last account destroyed, delta rows between
    run(acc, st, {{{1, 0, true}, {5, 0, true}}, {{2, 1, 0}, {3, 9, 1}, {4, 4, 44}}},
        true, -1);
    // two adjacent destroyed accounts, rows before and after
    run(acc, st, {{{2, 0, true}, {3, 0, true}, {4, 0, true}},
                  {{1, 0, 70}, {1, 1, 71}, {5, 7, 0}}}, true, -2);
    // a destroyed account without storage next to one with, nothing emitted
    run(acc, st, {{{3, 0, true}, {4, 0, true}}, {}}, true, -3);
    run(acc, st, {{{3, 0, true}}, {}}, true, -4);
    // every no-row branch at once: nothing at all comes out
    run(acc, st, {{{0, 0, true}, {9, 0, true}}, {{1, 6, 0}, {7, 1, 0}}}, true, -5);
    // an inserted account with rows; everything destroyed
    run(acc, st, {{{0, 5, false}}, {{0, 1, 5}, {0, 2, 6}, {5, 0, 33}}}, true, -6);
    run(acc, st, {{{1, 0, true}, {2, 0, true}, {3, 0, true}, {4, 0, true},
                   {5, 0, true}}, {}}, true, -7);
    run({}, {}, {{{1, 1, false}}, {{1, 1, 1}}}, true, -8);
    run(acc, st, {{}, {}}, true, -9);

    static const char *names[N_NAMED] = {
        "first account destroyed", "last account destroyed",
        "two adjacent destroyed accounts", "delta rows before the segments",
        "delta rows between segments", "delta rows after the segments",
        "empty segment", "segments but no emitted delta row",
        "a delta without any revert row", "unsorted delta", "duplicate delta rows"};
    for (int w = 0; w < N_NAMED; ++w)
        check(named[w] > 0, names[w], named[w]);
    printf("checked %ld failed %ld\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
