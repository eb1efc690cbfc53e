// The revert of a delta (include/sre.h, "revert capture"): which delta row
// leaves which revert row, and where every revert storage row lands. The
// capture kernels (k_rv_* in sre.hip) call these functions; no engine
// context and no device-only code, so tests/revert_plan_main.cpp checks
// them as a sanitizer-built host program against a std::map model.
#ifndef SRE_REVERT_PLAN_H
#define SRE_REVERT_PLAN_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define REVERT_HD __host__ __device__ __forceinline__
#else
#define REVERT_HD inline
#endif

// what one delta row contributes to the revert
enum : uint32_t {
    RV_NONE = 0, // no row: the forward row was a no-op, or the revert of
                 // its account (a destroy) already covers it
    RV_OLD = 1,  // the resident row as it was (account: deleted = 0)
    RV_GONE = 2, // the key was not resident: account row with deleted = 1,
                 // storage row with value 0
};

// Account delta row: `resident` = its key is in the pre-delta accounts.
REVERT_HD uint32_t rv_acct_row(bool resident, bool deleted)
{
    if (resident)
        return RV_OLD; // upserted or destroyed: put the old row back
    return deleted ? RV_NONE : RV_GONE;
}

// Storage delta row. owner_resident = its account is in the pre-delta
// accounts; owner_destroyed = the same delta destroys that account (the
// merges reject such a delta; the row is dropped here so that it cannot
// share an account with a copied segment); slot_resident = (acct, slot) is
// in the pre-delta storage; nonzero = the forward value.
REVERT_HD uint32_t rv_st_row(bool owner_resident, bool owner_destroyed,
                             bool slot_resident, bool nonzero)
{
    if (!owner_resident || owner_destroyed)
        return RV_NONE; // inserted by this delta (its revert destroys the
                        // account) or unknown (a no-op deletion)
    if (slot_resident)
        return RV_OLD;
    return nonzero ? RV_GONE : RV_NONE;
}

// ---- positions of the revert storage rows --------------------------------
// Two sorted sources share the output: delta rows that emit (flag 1; es =
// exclusive prefix sum of the flags, n_st + 1 entries) and the resident
// segments of destroyed accounts. Segments are indexed by ACCOUNT DELTA ROW
// k (length 0 unless row k destroys a resident account); segsum is the
// exclusive prefix sum of the lengths, n_acct + 1 entries, segsum[n_acct] =
// W, the wiped rows in all. The output holds es[n_st] + W rows.
//
// In bounds for ANY input, sorted or not, as long as the sums do not wrap:
// an emitting row j has es[j] < es[n_st] and any segsum entry is <= W; a
// flat wiped row w is < W and any es entry is <= es[n_st]. The engine
// validates the account delta's order before it captures, which makes the
// segments disjoint (W <= resident rows < 2^32), so nothing wraps.

// Emitting delta row j: (emitted rows before it) + (wiped rows of destroyed
// accounts with a smaller key). q = lower bound of the row's account key
// among the account delta keys, 0..n_acct.
REVERT_HD uint64_t rv_delta_row_pos(const uint32_t *es, uint64_t j,
                                    const uint32_t *segsum, uint64_t q)
{
    return (uint64_t)es[j] + segsum[q];
}

// The segment holding flat wiped row w (w < segsum[nseg]): the last k with
// segsum[k] <= w. Its length is nonzero by construction.
REVERT_HD uint64_t rv_segment_of(const uint32_t *segsum, uint64_t nseg, uint64_t w)
{
    uint64_t lo = 0, hi = nseg; // first k with segsum[k + 1] > w
    while (lo < hi) {
        uint64_t mid = (lo + hi) / 2;
        if ((uint64_t)segsum[mid + 1] <= w)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < nseg ? lo : nseg - 1;
}

// Flat wiped row w of a segment: (wiped rows before it) + (emitted delta
// rows with a smaller account key). p = lower bound of the segment's
// account key among the storage delta rows' account keys, 0..n_st.
REVERT_HD uint64_t rv_segment_row_pos(uint64_t w, const uint32_t *es, uint64_t p)
{
    return w + es[p];
}

#endif
