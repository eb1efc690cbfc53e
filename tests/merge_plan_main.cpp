// Stand-alone host check of reth_amd/csrc/merge_plan.h (built and run by
// tests/test_merge_plan_cpu.py): the plans of the closed-form account and
// storage merges and the position formulas their kernels share, against a
// std::map model of "post-state wins, zero value deletes, destroyed account
// wipes its rows". The program plays the mark kernels (bpos, match, wlo,
// whi) with std::lower_bound. Self-contained, fixed seed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "merge_plan.h"

static const int N_ACCT = 2000, N_ST = 2000, N_REJ = 1400, N_IV = 200;

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

// the scenarios the issue names; each must be hit at least once
enum {
    EMPTY_BASE, EMPTY_DELTA, DELETE_ALL, DELTA_BEFORE, DELTA_AFTER, MOD_FIRST,
    MOD_LAST, ADJ_WIPES, WIPE_AT_0, WIPE_AT_END, MATCH_IN_WIPE, ZERO_ABSENT,
    UNSORTED, DUPLICATE, DEAD_ACCT_ROW, COUNT_LIMIT, N_NAMED
};
static long named[N_NAMED];

// keys from a space small enough to collide: they vary in bytes 13 and 31,
// ascending with v
static void key_of(int v, uint8_t k[32])
{
    memset(k, 0x55, 32);
    k[13] = (uint8_t)(v >> 8);
    k[31] = (uint8_t)v;
}

typedef std::vector<int> ivec;
static ivec random_set(int n, int space) // ascending, unique, <= n values
{
    ivec v(n);
    for (auto &x : v)
        x = below(space);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

template <typename Row> static uint32_t lower(const std::vector<Row> &rows,
                                              const void *key, size_t klen)
{
    return (uint32_t)(std::lower_bound(rows.begin(), rows.end(), key,
                                       [klen](const Row &r, const void *k) {
                                           return memcmp(&r, k, klen) < 0;
                                       }) -
                      rows.begin());
}

// ---- accounts: the small merge and its lcp patch list --------------------
struct arow {
    int key;
    bool deleted;
};

static void run_acct(const ivec &base, const std::vector<arow> &delta, long at)
{
    size_t nb = base.size(), nd = delta.size();
    std::vector<sre_account_entry> B(nb);
    std::vector<sre_account_delta> D(nd);
    std::map<int, uint64_t> want; // key -> nonce
    for (size_t i = 0; i < nb; ++i) {
        memset(&B[i], 0, sizeof(B[i]));
        key_of(base[i], B[i].key);
        want[base[i]] = B[i].nonce = 1000 + i;
    }
    for (size_t k = 0; k < nd; ++k) {
        memset(&D[k], 0, sizeof(D[k]));
        key_of(delta[k].key, D[k].key);
        D[k].deleted = delta[k].deleted;
        D[k].nonce = 5000 + k;
        if (delta[k].deleted)
            want.erase(delta[k].key);
        else
            want[delta[k].key] = D[k].nonce;
    }
    // k_sd_marks
    std::vector<uint32_t> bpos(nd), match(nd), npos(nd);
    for (size_t k = 0; k < nd; ++k) {
        bpos[k] = lower(B, D[k].key, 32);
        match[k] = bpos[k] < nb && !memcmp(B[bpos[k]].key, D[k].key, 32);
    }
    bool accepted = acct_delta_order(D.data(), nd) == 0;
    merge_plan pl = plan_acct_small(nb, D.data(), nd, match);

    // k_sd_scatter and k_sd_place, with the formulas they call
    std::vector<sre_account_entry> out(pl.new_n);
    std::vector<int> hits(pl.new_n, 0), origin(pl.new_n, -1);
    bool perm = accepted && count_fits(pl.new_n);
    for (size_t i = 0; i < nb; ++i) {
        uint32_t p = lower(D, B[i].key, 32);
        if (p < nd && !memcmp(D[p].key, B[i].key, 32))
            continue;
        uint64_t j = merged_pos(i, pl.m_excl[p], pl.eff_excl[p]);
        if (j >= pl.new_n) {
            perm = false;
            continue;
        }
        hits[j]++;
        out[j] = B[i];
        origin[j] = (int)i;
    }
    for (size_t k = 0; k < nd; ++k) {
        npos[k] = (uint32_t)merged_pos(bpos[k], pl.m_excl[k], pl.eff_excl[k]);
        if (D[k].deleted)
            continue;
        if (npos[k] >= pl.new_n) {
            perm = false;
            continue;
        }
        hits[npos[k]]++;
        memcpy(out[npos[k]].key, D[k].key, 32);
        out[npos[k]].nonce = D[k].nonce;
    }
    for (int h : hits)
        perm = perm && h == 1;
    check(perm, "account positions are not a permutation of 0..new_n-1", at);
    bool asc = true, same = want.size() == out.size();
    for (size_t j = 1; j < out.size(); ++j)
        asc = asc && memcmp(out[j - 1].key, out[j].key, 32) < 0;
    check(asc, "placed account keys do not ascend strictly", at);
    size_t j = 0;
    for (auto it = want.begin(); same && it != want.end(); ++it, ++j) {
        uint8_t k[32];
        key_of(it->first, k);
        same = !memcmp(out[j].key, k, 32) && out[j].nonce == it->second;
    }
    check(same, "merged accounts != model", at);

    // patch list: sorted, unique, both ends, and every position whose left
    // neighbour is not the row it had in the base
    std::vector<uint32_t> patch = lcp_patch_list(D.data(), nd, npos, pl.new_n);
    bool pok = !patch.empty() && patch.front() == 0 && patch.back() == pl.new_n;
    for (size_t t = 1; t < patch.size(); ++t)
        pok = pok && patch[t - 1] < patch[t];
    for (size_t q = 1; q < out.size(); ++q) {
        bool kept = origin[q - 1] >= 0 && origin[q] == origin[q - 1] + 1;
        if (!kept && !std::binary_search(patch.begin(), patch.end(), (uint32_t)q))
            pok = false;
    }
    check(pok, "lcp patch list misses a changed junction", at);

    named[EMPTY_BASE] += nb == 0;
    named[EMPTY_DELTA] += nd == 0;
    named[DELETE_ALL] += nb > 0 && pl.new_n == 0;
    if (nb && nd) {
        named[DELTA_BEFORE] += delta.back().key < base.front();
        named[DELTA_AFTER] += delta.front().key > base.back();
        for (const arow &r : delta) {
            named[MOD_FIRST] += !r.deleted && r.key == base.front();
            named[MOD_LAST] += !r.deleted && r.key == base.back();
        }
    }
}

static std::vector<arow> random_acct_delta(int max_n, int space)
{
    std::vector<arow> d;
    for (int v : random_set(below(max_n + 1), space))
        d.push_back({v, below(3) == 0});
    return d;
}

// ---- storage: the closed-form merge with wipe ranges ----------------------
struct srow {
    int acct, slot;
    bool zero;
};
typedef std::vector<std::pair<int, int>> pvec; // (acct, slot), ascending

static sre_storage_entry st_entry(int acct, int slot, uint8_t value)
{
    sre_storage_entry e;
    memset(&e, 0, sizeof(e));
    key_of(acct * 90, e.acct_key); // accounts 0..5: byte 13 varies too
    key_of(slot * 37, e.slot_key);
    e.value[31] = value;
    return e;
}

static std::vector<key32> dead_keys(const ivec &dead)
{
    std::vector<key32> keys;
    for (int a : dead)
        keys.push_back(key32_of(st_entry(a, 0, 0).acct_key));
    return keys;
}

static std::vector<sre_storage_entry> st_rows(const std::vector<srow> &delta)
{
    std::vector<sre_storage_entry> D;
    for (size_t k = 0; k < delta.size(); ++k)
        D.push_back(st_entry(delta[k].acct, delta[k].slot,
                             delta[k].zero ? 0 : (uint8_t)(128 + k % 100)));
    return D;
}

// a valid scenario: no delta row for an account in dead
static void run_st(const pvec &base, const ivec &dead,
                   const std::vector<srow> &delta, long at)
{
    size_t ns = base.size(), nd = delta.size(), ndel = dead.size();
    std::vector<sre_storage_entry> B, D = st_rows(delta);
    std::map<std::pair<int, int>, uint8_t> want;
    for (size_t i = 0; i < ns; ++i) {
        B.push_back(st_entry(base[i].first, base[i].second, (uint8_t)(1 + i)));
        if (!std::binary_search(dead.begin(), dead.end(), base[i].first))
            want[base[i]] = B[i].value[31];
    }
    for (size_t k = 0; k < nd; ++k)
        if (delta[k].zero)
            want.erase({delta[k].acct, delta[k].slot});
        else
            want[{delta[k].acct, delta[k].slot}] = D[k].value[31];
    // k_sds_marks and k_sds_wipes
    std::vector<uint32_t> bpos(nd), match(nd), wlo(ndel), whi(ndel);
    for (size_t k = 0; k < nd; ++k) {
        bpos[k] = lower(B, &D[k], 64);
        match[k] = bpos[k] < ns && !memcmp(&B[bpos[k]], &D[k], 64) ? SDS_MATCH : 0;
        named[ZERO_ABSENT] += delta[k].zero && !match[k];
    }
    std::vector<key32> dk = dead_keys(dead);
    for (size_t a = 0; a < ndel; ++a) {
        wlo[a] = whi[a] = lower(B, dk[a].data(), 32);
        while (whi[a] < ns && !memcmp(B[whi[a]].acct_key, dk[a].data(), 32))
            ++whi[a];
    }
    merge_plan pl;
    bool perm = st_delta_flags(D.data(), nd, dk) == 0 &&
                plan_st_small(ns, D.data(), nd, match, wlo, whi, pl) == 0 &&
                count_fits(pl.new_n);

    // k_sds_scatter and k_sds_place, with the formulas they call
    std::vector<sre_storage_entry> out(perm ? pl.new_n : 0);
    std::vector<int> hits(out.size(), 0);
    auto place = [&](uint64_t j, const sre_storage_entry &e) {
        if (j >= out.size()) {
            perm = false;
            return;
        }
        hits[j]++;
        out[j] = e;
    };
    for (size_t i = 0; perm && i < ns; ++i) {
        bool wiped;
        uint64_t wb = wipes_before(wlo.data(), whi.data(), pl.wsum.data(),
                                   (uint32_t)ndel, i, &wiped);
        uint32_t p = lower(D, &B[i], 64);
        if (wiped || (p < nd && !memcmp(&D[p], &B[i], 64)))
            continue;
        place(merged_pos(i, pl.m_excl[p], pl.eff_excl[p], wb), B[i]);
    }
    for (size_t k = 0; perm && k < nd; ++k) {
        bool wiped;
        uint64_t wb = wipes_before(wlo.data(), whi.data(), pl.wsum.data(),
                                   (uint32_t)ndel, bpos[k], &wiped);
        if (!delta[k].zero)
            place(merged_pos(bpos[k], pl.m_excl[k], pl.eff_excl[k], wb), D[k]);
    }
    for (int h : hits)
        perm = perm && h == 1;
    check(perm, "storage positions are not a permutation of 0..new_n-1", at);
    bool asc = true, same = want.size() == out.size();
    for (size_t j = 1; j < out.size(); ++j)
        asc = asc && memcmp(&out[j - 1], &out[j], 64) < 0;
    check(asc, "placed storage keys do not ascend strictly", at);
    size_t j = 0;
    for (auto it = want.begin(); same && it != want.end(); ++it, ++j) {
        sre_storage_entry e = st_entry(it->first.first, it->first.second, it->second);
        same = !memcmp(&out[j], &e, sizeof(e));
    }
    check(same, "merged storage != model", at);

    named[EMPTY_BASE] += ns == 0;
    named[EMPTY_DELTA] += nd == 0 && ndel == 0;
    named[DELETE_ALL] += ns > 0 && perm && pl.new_n == 0;
    for (size_t a = 0; a < ndel; ++a) {
        bool rows = whi[a] > wlo[a];
        named[WIPE_AT_0] += rows && wlo[a] == 0;
        named[WIPE_AT_END] += rows && whi[a] == ns;
        named[ADJ_WIPES] += rows && a + 1 < ndel && whi[a + 1] > wlo[a + 1] &&
                            whi[a] == wlo[a + 1];
    }
    if (ns && nd) {
        named[DELTA_BEFORE] += memcmp(&D[nd - 1], &B[0], 64) < 0;
        named[DELTA_AFTER] += memcmp(&D[0], &B[ns - 1], 64) > 0;
        named[MOD_FIRST] += !delta[0].zero && !memcmp(&D[0], &B[0], 64);
        named[MOD_LAST] += !delta[nd - 1].zero && !memcmp(&D[nd - 1], &B[ns - 1], 64);
    }
}

static const int N_A = 6, N_SLOT = 16;

static pvec random_pairs(int max_n)
{
    pvec v;
    for (int x : random_set(below(max_n + 1), N_A * N_SLOT))
        v.push_back({x / N_SLOT, x % N_SLOT});
    return v;
}

static void random_st(pvec &base, ivec &dead, std::vector<srow> &delta)
{
    base = random_pairs(64);
    dead = random_set(below(4), N_A);
    delta.clear();
    for (const auto &p : random_pairs(24))
        if (!std::binary_search(dead.begin(), dead.end(), p.first))
            delta.push_back({p.first, p.second, below(3) == 0});
}

// ---- what must be rejected -----------------------------------------------
static void check_rejected()
{
    for (int sc = 0; sc < N_REJ; ++sc) {
        int kind = sc % 7;
        if (kind < 2) { // account delta: two rows swapped / one row twice
            std::vector<arow> d = random_acct_delta(24, 100);
            while (d.size() < 2)
                d = random_acct_delta(24, 100);
            size_t k = (size_t)below((int)d.size() - 1);
            if (kind == 0)
                std::swap(d[k], d[k + 1]);
            else
                d[k + 1].key = d[k].key;
            std::vector<sre_account_delta> D(d.size());
            for (size_t q = 0; q < d.size(); ++q)
                key_of(d[q].key, D[q].key);
            check(acct_delta_order(D.data(), D.size()) == 1u << E_UNSORTED_ACCT,
                  "unsorted / duplicate account delta accepted", sc);
            named[kind == 0 ? UNSORTED : DUPLICATE]++;
            continue;
        }
        pvec base;
        ivec dead;
        std::vector<srow> delta;
        do
            random_st(base, dead, delta);
        while (delta.size() < 2 || dead.empty());
        size_t k = (size_t)below((int)delta.size() - 1);
        uint32_t want = 1u << E_UNSORTED_STORAGE;
        if (kind == 2) {
            std::swap(delta[k], delta[k + 1]);
            named[UNSORTED]++;
        } else if (kind == 3) {
            delta[k + 1] = delta[k];
            named[DUPLICATE]++;
        } else if (kind == 4 || kind == 5) {
            // a row of a destroyed account, kind 5: one that matches a
            // resident row inside that account's wipe range. merged_pos would
            // subtract such a row twice (matched and wiped), so the plan
            // relies on this check.
            int a = dead[below((int)dead.size())], slot = below(N_SLOT);
            if (kind == 5) {
                base.push_back({a, slot});
                std::sort(base.begin(), base.end());
                base.erase(std::unique(base.begin(), base.end()), base.end());
                named[MATCH_IN_WIPE]++;
            }
            delta.push_back({a, slot, false});
            std::sort(delta.begin(), delta.end(), [](const srow &x, const srow &y) {
                return std::make_pair(x.acct, x.slot) < std::make_pair(y.acct, y.slot);
            });
            want = 1u << E_ORPHAN_STORAGE;
            named[DEAD_ACCT_ROW]++;
        }
        std::vector<sre_storage_entry> D = st_rows(delta);
        if (kind < 6) {
            check(st_delta_flags(D.data(), D.size(), dead_keys(dead)) == want,
                  "bad storage delta: wrong flags", sc);
            continue;
        }
        // k_sds_marks reported an orphan row: no plan
        std::vector<uint32_t> match(D.size(), 0), none;
        match[k] = SDS_ORPHAN | (below(2) ? SDS_MATCH : 0);
        merge_plan pl;
        check(plan_st_small(base.size(), D.data(), D.size(), match, none, none, pl) ==
                  1u << E_ORPHAN_STORAGE,
              "orphan mark not rejected", sc);
    }
}

// merged counts are 64-bit and a count of 2^32-1 does not fit
static void check_count_limit()
{
    sre_account_delta ins;
    memset(&ins, 0, sizeof(ins));
    merge_plan pa = plan_acct_small(0xFFFFFFFEull, &ins, 1, {0});
    check(pa.new_n == 0xFFFFFFFFull && !count_fits(pa.new_n),
          "account count at the limit accepted", 0);
    sre_storage_entry row = st_entry(0, 0, 1);
    merge_plan ps;
    uint32_t bad = plan_st_small(0xFFFFFFFEull, &row, 1, {0}, {}, {}, ps);
    check(!bad && ps.new_n == 0xFFFFFFFFull && !count_fits(ps.new_n),
          "storage count at the limit accepted", 0);
    check(merged_count(0xFFFFFFFFu, 0xFFFFFFFFu) == 0x1FFFFFFFEull &&
              !count_fits(merged_count(0xFFFFFFFEu, 1)),
          "general merged count wraps or fits at the limit", 0);
    check(count_fits(merged_count(0xFFFFFFFDu, 1)), "largest count rejected", 0);
    named[COUNT_LIMIT]++;
}

// ---- interval offsets ------------------------------------------------------
static void check_intervals()
{
    for (int sc = 0; sc < N_IV; ++sc) {
        uint32_t n_seg = (uint32_t)below(12), row = 0;
        std::vector<uint32_t> need(n_seg), start(n_seg), lo, hi, rows;
        for (uint32_t s = 0; s < n_seg; ++s) {
            start[s] = row;
            need[s] = below(2);
            for (int len = 1 + below(5); len > 0; --len, ++row)
                if (need[s])
                    rows.push_back(row); // what the gather must collect
        }
        needed_intervals(need, start, row, lo, hi);
        std::vector<uint32_t> offs = interval_offsets(lo, hi), got(rows.size());
        bool ok = offs.size() == lo.size() + 1 && offs.back() == rows.size();
        for (size_t t = 0; ok && t < lo.size(); ++t)
            for (uint32_t r = lo[t]; r < hi[t]; ++r)
                got[offs[t] + (r - lo[t])] = r;
        check(ok && got == rows, "interval offsets != concatenation", sc);
    }
}

int main()
{
    for (int sc = 0; sc < N_ACCT; ++sc)
        run_acct(random_set(below(65), 100 + 300 * (sc & 1)),
                 random_acct_delta(24, 100 + 300 * (sc & 1)), sc);
    for (int sc = 0; sc < N_ST; ++sc) {
        pvec base;
        ivec dead;
        std::vector<srow> delta;
        random_st(base, dead, delta);
        run_st(base, dead, delta, sc);
    }
    // the named scenarios, built by hand: 7 account and 5 storage ones
    run_acct({}, {{5, false}, {7, true}}, -1);
    run_acct({1, 2, 3}, {}, -2);
    run_acct({1, 2, 300}, {{1, true}, {2, true}, {300, true}}, -3);
    run_acct({10, 11}, {{3, false}, {4, true}}, -4);
    run_acct({10, 11}, {{12, false}, {299, false}}, -5);
    run_acct({10, 11, 12}, {{10, false}}, -6);
    run_acct({10, 11, 12}, {{12, false}}, -7);
    // two adjacent wipe ranges, the first at index 0; a zero row for an
    // absent slot; the last row modified
    run_st({{0, 1}, {0, 2}, {1, 1}, {1, 3}, {2, 1}}, {0, 1},
           {{2, 1, false}, {2, 5, true}}, -8);
    run_st({{0, 1}, {1, 1}, {1, 2}}, {1}, {{0, 0, false}}, -9); // wipe ends at ns
    run_st({}, {}, {{0, 1, false}, {0, 2, false}}, -10);
    run_st({{0, 1}, {0, 2}}, {}, {}, -11);
    run_st({{0, 1}, {1, 1}}, {0}, {{1, 1, true}}, -12); // everything goes
    check_rejected();
    check_count_limit();
    check_intervals();
    static const char *names[N_NAMED] = {
        "empty base", "empty delta", "delete everything", "delta before the base",
        "delta after the base", "modify first row", "modify last row",
        "two adjacent wipe ranges", "wipe range at index 0",
        "wipe range ending at ns", "delta row matching a row inside a wipe range",
        "zero-value row for an absent slot", "unsorted delta", "duplicate delta",
        "row for a destroyed account", "count reaching 2^32-1"};
    for (int w = 0; w < N_NAMED; ++w)
        check(named[w] > 0, names[w], named[w]);
    printf("checked %ld failed %ld\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
