// Where every row of a delta merge lands: the host-side plans of the
// closed-form ("small") account and storage merges, the position formulas
// their kernels run, the interval offsets of the subset storage pass and
// the 64-bit merged counts. No engine context and no device-only code, so
// tests/merge_plan_main.cpp checks it as a sanitizer-built host program.
#ifndef SRE_MERGE_PLAN_H
#define SRE_MERGE_PLAN_H

#include "updates_diff.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MERGE_HD __host__ __device__ __forceinline__
#else
#define MERGE_HD inline
#endif

// bit numbers of the validation failures (device error flag and host checks)
enum {
    E_OK = 0,
    E_UNSORTED_ACCT = 1,
    E_UNSORTED_STORAGE = 2,
    E_ORPHAN_STORAGE = 3,
    E_ZERO_VALUE = 4,
    E_INTERNAL = 5,
    E_DUP_ADDRESS = 6,
    E_DUP_STORAGE = 7,
};

// k_sds_marks' per-row word, read back by the host
enum : uint32_t {
    SDS_MATCH = 1,  // (acct, slot) is resident: the row replaces/deletes it
    SDS_ORPHAN = 2, // nonzero row whose account is neither resident nor upserted
};

// leaf intervals are u32 (node_rec.s/e): a resident or merged row count must
// stay below 2^32-1 (sre.h capacity contract — reject, never truncate)
MERGE_HD bool count_fits(uint64_t n) { return n < 0xFFFFFFFFull; }

// rows of a general merge: surviving base rows + effective delta rows, two
// u32 scan totals that are widened before they are added
MERGE_HD uint64_t merged_count(uint32_t kept, uint32_t added)
{
    return (uint64_t)kept + added;
}

// ---- position formulas (host plans and the k_sd_* / k_sds_* kernels) ----
// Base rows removed by wipe ranges before base index i. Range a is
// [wlo[a], whi[a]), ascending and disjoint; wsum[a] = rows in ranges < a.
// *wiped = i itself lies in a range.
MERGE_HD uint64_t wipes_before(const uint32_t *wlo, const uint32_t *whi,
                               const uint32_t *wsum, uint32_t ndel, uint64_t i,
                               bool *wiped)
{
    // last range with wlo <= i
    int lo = 0, hi = (int)ndel;
    while (lo < hi) {
        int mid = (lo + hi) / 2;
        if ((uint64_t)wlo[mid] <= i)
            lo = mid + 1;
        else
            hi = mid;
    }
    int r = lo - 1;
    *wiped = false;
    if (r < 0)
        return 0;
    uint32_t clip = i < whi[r] ? (uint32_t)i : whi[r];
    *wiped = i < whi[r];
    return wsum[r] + (clip > wlo[r] ? clip - wlo[r] : 0);
}

// Output position of base row i, or of the delta row whose lower bound in
// the base is i: m and eff are m_excl / eff_excl at the row's delta rank
// (matched resp. effective delta rows before it), wb = wipes_before(i).
MERGE_HD uint64_t merged_pos(uint64_t i, uint32_t m, uint32_t eff, uint64_t wb = 0)
{
    return i - m - wb + eff;
}

// ---- plans ---------------------------------------------------------------
// What both closed-form merges upload: exclusive prefix counts over the
// delta rows (n + 1 each) and the merged row count, in 64 bits.
struct merge_plan {
    std::vector<uint32_t> m_excl, eff_excl;
    std::vector<uint32_t> wsum; // storage only: rows in wipe ranges < a
    uint64_t new_n = 0;
};

// E_* bits of an account delta that is not strictly ascending by key
static uint32_t acct_delta_order(const sre_account_delta *d, uint64_t nd)
{
    for (uint64_t k = 1; k < nd; ++k)
        if (memcmp(d[k - 1].key, d[k].key, 32) >= 0)
            return 1u << E_UNSORTED_ACCT;
    return 0;
}

// small account merge over nb resident rows; match[k] = delta key k is resident
static merge_plan plan_acct_small(uint64_t nb, const sre_account_delta *d,
                                  uint64_t nd, const std::vector<uint32_t> &match)
{
    merge_plan pl;
    pl.m_excl.assign(nd + 1, 0);
    pl.eff_excl.assign(nd + 1, 0);
    for (uint64_t k = 0; k < nd; ++k) {
        pl.m_excl[k + 1] = pl.m_excl[k] + (match[k] ? 1 : 0);
        pl.eff_excl[k + 1] = pl.eff_excl[k] + (d[k].deleted ? 0 : 1);
    }
    pl.new_n = nb - pl.m_excl[nd] + pl.eff_excl[nd];
    return pl;
}

// lcp positions the small account merge recomputes: both ends, each delta
// row's output position (insert/replace position; for a delete the junction
// where its successor now sits) and the position after a row that produced
// an entry. Sorted, unique.
static std::vector<uint32_t> lcp_patch_list(const sre_account_delta *d, uint64_t nd,
                                            const std::vector<uint32_t> &npos,
                                            uint64_t new_na)
{
    std::vector<uint32_t> patch;
    patch.reserve(2 * nd + 2);
    patch.push_back(0);
    patch.push_back((uint32_t)new_na);
    for (uint64_t k = 0; k < nd; ++k) {
        patch.push_back(npos[k]);
        if (!d[k].deleted)
            patch.push_back(npos[k] + 1);
    }
    std::sort(patch.begin(), patch.end());
    patch.erase(std::unique(patch.begin(), patch.end()), patch.end());
    return patch;
}

// What the host checks of a storage delta before the closed-form merge
// (k_ovl_delta_st_flags checks the same on device for the general merge):
// E_* bits for unsorted or duplicate (acct, slot) rows and for a row of an
// account the same delta destroys (dead: ascending keys).
static uint32_t st_delta_flags(const sre_storage_entry *st, uint64_t n_st,
                               const std::vector<key32> &dead)
{
    uint32_t bad = 0;
    for (uint64_t i = 0; i < n_st; ++i) {
        if (i && memcmp(&st[i - 1], &st[i], 64) >= 0)
            bad |= 1u << E_UNSORTED_STORAGE;
        if (key_in(dead, st[i].acct_key))
            bad |= 1u << E_ORPHAN_STORAGE;
    }
    return bad;
}

// closed-form storage merge over ns resident rows: match[k] = SDS_* word of
// delta row k, [wlo[a], whi[a]) = resident rows of destroyed account a.
// Returns E_* bits (an orphan row); the plan is valid when they are 0.
static uint32_t plan_st_small(uint64_t ns, const sre_storage_entry *st, uint64_t n_st,
                              const std::vector<uint32_t> &match,
                              const std::vector<uint32_t> &wlo,
                              const std::vector<uint32_t> &whi, merge_plan &pl)
{
    for (uint64_t k = 0; k < n_st; ++k)
        if (match[k] & SDS_ORPHAN)
            return 1u << E_ORPHAN_STORAGE;
    size_t ndel = wlo.size();
    pl.wsum.assign(ndel + 1, 0);
    for (size_t a = 0; a < ndel; ++a)
        pl.wsum[a + 1] = pl.wsum[a] + (whi[a] - wlo[a]);
    pl.m_excl.assign(n_st + 1, 0);
    pl.eff_excl.assign(n_st + 1, 0);
    for (uint64_t k = 0; k < n_st; ++k) {
        bool nz = false; // zero value = slot deletion: no output row
        for (int q = 0; q < 32; ++q)
            nz |= st[k].value[q] != 0;
        pl.m_excl[k + 1] = pl.m_excl[k] + ((match[k] & SDS_MATCH) ? 1 : 0);
        pl.eff_excl[k + 1] = pl.eff_excl[k] + (nz ? 1 : 0);
    }
    pl.new_n = ns - pl.m_excl[n_st] - pl.wsum[ndel] + pl.eff_excl[n_st];
    return 0;
}

// ---- subset storage pass -------------------------------------------------
// offs[t] = offset of interval [lo[t], hi[t]) in the gathered array,
// offs[n] = the total (disjoint intervals of a u32-counted array: it fits)
static std::vector<uint32_t> interval_offsets(const std::vector<uint32_t> &lo,
                                              const std::vector<uint32_t> &hi)
{
    std::vector<uint32_t> offs(lo.size() + 1, 0);
    for (size_t t = 0; t < lo.size(); ++t)
        offs[t + 1] = offs[t] + (hi[t] - lo[t]);
    return offs;
}

// the segments s with need[s] set, as intervals: segment s is
// [start[s], start[s + 1]), the last one ends at ns
static void needed_intervals(const std::vector<uint32_t> &need,
                             const std::vector<uint32_t> &start, uint64_t ns,
                             std::vector<uint32_t> &lo, std::vector<uint32_t> &hi)
{
    for (size_t s = 0; s < need.size(); ++s)
        if (need[s]) {
            lo.push_back(start[s]);
            hi.push_back(s + 1 < need.size() ? start[s + 1] : (uint32_t)ns);
        }
}

#endif
