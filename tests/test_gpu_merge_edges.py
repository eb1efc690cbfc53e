"""Block edges of the closed-form small-delta merges (k_sd_scatter for
accounts, k_sds_scatter for storage).

Both kernels copy a full 256-row block flat, to a constant-shifted
destination, when no delta key falls in the block's span, no wipe range
overlaps it and the delta key at the block's rank is not its last row;
every other block goes row by row. At bench scale nearly every block is
flat; at test scale with random deltas nearly none is, and the edges — a
delta key ON a block's first or last row, a delete of a last row, an
insert exactly between two blocks, nb a multiple of 256, wipe ranges that
start, end or lie on block edges — are hit only by luck.

Here the delta keys are placed against the blocks of the sorted pre-delta
arrays on purpose. The block rule is restated in plain Python
(_account_blocks / _storage_blocks) and every test first asserts that its
delta really leaves at least one full block flat with a nonzero shift and
at least one full block not flat. Roots are compared with the oracle on
the dict-merged state, then one more small delta next to the first is
chained so the repaired lcp / carried roots and the refreshed retention
are consumed. On the incremental calls the reuse counters must equal the
key-only model of tests/dense_cells.py as well: the merge's position map
drives the rebase of every retained row, and a wrong entry there can
cost reuse without changing the root.
"""
import bisect
import copy
import os

import numpy as np
import pytest

from oracle import bind
from reth_amd import gen
from tests import dense_cells as dc
from tests.test_gpu_incremental import _acct_dict, _arrays_of, _mk_delta
from tests.test_gpu_incremental_updates import _rowmap, _apply_diff

pytestmark = pytest.mark.gpu

BLOCK = 256
COUNTERS = ("examined", "seeded", "rehashed", "captured")


@pytest.fixture(scope="module")
def eng():
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()


@pytest.fixture()
def st_closed_form():
    old = os.environ.get("SRE_ST_SMALL_MIN")
    os.environ["SRE_ST_SMALL_MIN"] = "0"
    yield
    if old is None:
        os.environ.pop("SRE_ST_SMALL_MIN", None)
    else:
        os.environ["SRE_ST_SMALL_MIN"] = old


def _prefix(flags):
    out = [0]
    for f in flags:
        out.append(out[-1] + int(f))
    return out


def _reach(blocks, want_shift="nonzero"):
    """blocks: [(flat, shift)] per full block"""
    flat = [s for f, s in blocks if f]
    if want_shift == "nonzero":
        assert any(s != 0 for s in flat), f"no shifted flat block: {blocks}"
    else:
        assert flat and all(s == 0 for s in flat), blocks
    assert any(not f for f, _ in blocks), f"no per-row block: {blocks}"


# ---------------------------------------------------------------------------
# accounts
# ---------------------------------------------------------------------------

def _account_blocks(base, rows):
    """k_sd_scatter's rule per full block of the sorted base keys."""
    rows = sorted(rows)
    dkeys = [r[0] for r in rows]
    present = set(base)
    m_excl = _prefix(k in present for k in dkeys)
    eff_excl = _prefix(not r[4] for r in rows)
    out = []
    for i0 in range(0, len(base) - BLOCK + 1, BLOCK):
        last = i0 + BLOCK - 1
        plo = bisect.bisect_left(dkeys, base[i0])
        phi = bisect.bisect_left(dkeys, base[last])
        lastmatch = plo < len(dkeys) and dkeys[plo] == base[last]
        out.append((plo == phi and not lastmatch, eff_excl[plo] - m_excl[plo]))
    return out


def _after(k, n=1):
    for _ in range(n):
        k = dc.key_after(k)
    return k


def _shifter(K):
    # two inserts inside block 0 (no case below nets -2), so the untouched
    # blocks after them are copied to a shifted destination
    return [dc.ins(_after(K[10]), 9), dc.ins(_after(K[11]), 8)]


def _c_modify_first_row(K, acc, b):
    return [dc.mod(acc, K[BLOCK * b])]


def _c_modify_last_row(K, acc, b):  # the lastmatch guard
    return [dc.mod(acc, K[BLOCK * b + 255])]


def _c_delete_last_row(K, acc, b):
    return [dc.dele(K[BLOCK * b + 255])]


def _c_delete_first_row(K, acc, b):
    return [dc.dele(K[BLOCK * b])]


def _c_insert_between_blocks(K, acc, b):
    return [dc.ins(_after(K[BLOCK * b + 255]))]


def _c_insert_before_first_and_after_last(K, acc, b):
    return [dc.ins(bytes(32)), dc.ins(b"\xff" * 32, 1),
            dc.mod(acc, K[BLOCK * b + 100])]


def _c_insert_run_and_delete_both_neighbours(K, acc, b):
    r = BLOCK * b + 255  # patch positions of the deletes and inserts coincide
    rows = [dc.dele(K[r])] + [dc.ins(_after(K[r], n), n) for n in (1, 2, 3)]
    if r + 1 < len(K):
        rows.append(dc.dele(K[r + 1]))
    return rows


def _c_delete_run_across_block_edge(K, acc, b):
    return [dc.dele(K[i])
            for i in range(BLOCK * b + 253, min(BLOCK * b + 259, len(K)))]


ACCOUNT_CASES = {f.__name__[3:]: f for f in (
    _c_modify_first_row, _c_modify_last_row, _c_delete_last_row,
    _c_delete_first_row, _c_insert_between_blocks,
    _c_insert_before_first_and_after_last,
    _c_insert_run_and_delete_both_neighbours,
    _c_delete_run_across_block_edge)}


def _followup(acc, rows):
    """A small delta right next to the previous one."""
    K = sorted(acc)
    p = min(bisect.bisect_left(K, sorted(rows)[0][0]), len(K) - 1)
    out = {}
    for q in (p - 1, p, p + 1):
        if 0 <= q < len(K):
            out[K[q]] = dc.mod(acc, K[q], 5)
    k = _after(K[max(p - 1, 0)])
    if k not in acc:
        out[k] = dc.ins(k, 4)
    return sorted(out.values())


def _run_account_case(eng, nb, make_rows, updates=False, want_shift="nonzero"):
    acct, _ = gen.gen_state_numpy(nb, 0, bind.keccak256_batch)
    acc = _acct_dict(acct)
    assert len(acc) == nb
    eng.upload(acct, np.zeros(0, bind.STORAGE_DTYPE))

    def step(rows, want_small):
        assert 0 < len(rows) <= len(acc) >> 6
        pre = list(acc)
        dc.apply_rows(acc, rows)
        exp = dc.model(pre, list(acc), rows, [])
        d, _ = _mk_delta(rows, [])
        oroot, orows = bind.state_root_with_updates(*_arrays_of(acc))
        if updates:
            root, diff = eng.incremental_root_with_updates(d)
            step.cur = _apply_diff(step.cur, diff)
            assert step.cur == _rowmap(orows), "diff does not reproduce rows"
        else:
            root = eng.incremental_root(d)
        assert root == oroot
        got = eng.incremental_counters()
        assert got["small_acct_merge"] == want_small
        # the position map feeds the rebase of every retained row: a wrong
        # entry at a block edge may only cost reuse, which no root shows
        assert {k: got[k] for k in COUNTERS} == {k: exp[k] for k in COUNTERS}

    if updates:
        _, rows0 = eng.root_retaining_with_updates()
        step.cur = _rowmap(rows0)
    else:
        eng.root_retaining()
    # warm value-only delta: general merge, arms the retained lcp
    step([dc.mod(acc, sorted(acc)[5])], 0)
    K = sorted(acc)
    rows = make_rows(K, acc)
    _reach(_account_blocks(K, rows), want_shift)
    step(rows, 1)
    step(_followup(acc, rows), 1)


@pytest.mark.parametrize("nb", [1024, 1025, 1061])
@pytest.mark.parametrize("case", sorted(ACCOUNT_CASES))
def test_account_merge_block_edges(eng, case, nb):
    for b in (1, 3):
        _run_account_case(
            eng, nb,
            lambda K, acc: ACCOUNT_CASES[case](K, acc, b) + _shifter(K))


@pytest.mark.parametrize("nb", [1024, 1025, 1061])
@pytest.mark.parametrize("sign", ["positive", "negative", "zero"])
def test_account_merge_net_shift(eng, sign, nb):
    # all delta keys inside block 0: blocks 1..3 are flat copies to a
    # destination shifted by the net row count (unaligned unless zero)
    def rows(K, acc):
        ins = [dc.ins(_after(K[20])), dc.ins(_after(K[21]), 1)]
        dels = [dc.dele(K[40]), dc.dele(K[41])]
        return {"positive": ins, "negative": dels,
                "zero": ins[:1] + dels[:1]}[sign]
    _run_account_case(eng, nb, rows,
                      want_shift="zero" if sign == "zero" else "nonzero")


@pytest.mark.parametrize("nb", [1024, 1061])
@pytest.mark.parametrize("case", ["modify_last_row",
                                  "insert_run_and_delete_both_neighbours"])
def test_account_merge_block_edges_with_updates(eng, case, nb):
    _run_account_case(
        eng, nb, lambda K, acc: ACCOUNT_CASES[case](K, acc, 3) + _shifter(K),
        updates=True)


# ---------------------------------------------------------------------------
# storage
# ---------------------------------------------------------------------------

# slots per account, in account-key order: segment edges land on purpose
#   A0 [0,256) one aligned block      A1 [256,512)
#   A2 [512,1112) blocks 2,3 whole + a tail into block 4
#   A3 [1112,1212) strictly inside block 4
#   A4 [1212,1280) ends on block 4's last row
#   A5 [1280,1535)                     A6 [1535,1575) starts on block 5's last row
#   A7 no storage   A8 [1575,1605)   A9 [1605,1650) adjacent segments
SLOTS = [256, 256, 600, 100, 68, 255, 40, 0, 30, 45] + [85] * 30


@pytest.fixture(scope="module")
def st_state():
    # two sibling cells of 20 accounts: A0..A9 share the lower one, so a
    # destroyed account dirties it while the upper cell's retained subtree,
    # which embeds carried storage roots, must be reused
    keys = sorted(dc.key_in(dc.PAIR_BIG if i < 20 else dc.PAIR_SMALL,
                            b"edge-acct" + bytes([i]))
                  for i in range(len(SLOTS)))
    assert dc.cell(keys[19]) == dc.PAIR_BIG < dc.cell(keys[20])
    acc = {}
    for i, (k, n) in enumerate(zip(keys, SLOTS)):
        slots = {bind.keccak256(b"edge-slot" + bytes([i]) + j.to_bytes(2, "big")):
                 1 + j for j in range(n)}
        acc[k] = [i, 1000 + i, dc.KE, slots]
    rows = _st_rows(acc)
    lo = {k: next((p for p, r in enumerate(rows) if r[0] == k), None)
          for k in keys}
    assert [lo[k] for k in keys[:7]] == [0, 256, 512, 1112, 1212, 1280, 1535]
    assert lo[keys[7]] is None and lo[keys[8]] == 1575 and lo[keys[9]] == 1605
    assert 4096 <= len(rows) <= 5000
    return acc, keys


def _st_rows(acc):
    return [(k, s) for k in sorted(acc) for s in sorted(acc[k][3])]


def _storage_blocks(base, strows, destroyed):
    """k_sds_scatter's rule per full block of the sorted (acct, slot) rows."""
    strows = sorted(strows)
    dkeys = [(a, s) for a, s, _ in strows]
    present = set(base)
    m_excl = _prefix(k in present for k in dkeys)
    eff_excl = _prefix(v != 0 for _, _, v in strows)
    wiped = _prefix(r[0] in destroyed for r in base)  # wiped rows before i
    out = []
    for i0 in range(0, len(base) - BLOCK + 1, BLOCK):
        last = i0 + BLOCK - 1
        plo = bisect.bisect_left(dkeys, base[i0])
        phi = bisect.bisect_left(dkeys, base[last])
        lastmatch = plo < len(dkeys) and dkeys[plo] == base[last]
        untouched = wiped[last + 1] == wiped[i0]
        out.append((plo == phi and not lastmatch and untouched,
                    eff_excl[plo] - m_excl[plo] - wiped[i0]))
    return out


def _slot_after(row):
    return (row[0], dc.key_after(row[1]))


def _st_cases(acc, A):
    R = _st_rows(acc)
    shifter = (*_slot_after(R[3]), 77)  # an insert inside block 0
    return {
        "destroy_one_aligned_block": ([A[0]], []),
        "destroy_whole_blocks_plus_tail": ([A[2]], []),
        "destroy_inside_a_block": ([A[3]], []),
        "destroy_ending_on_block_last_row": ([A[4]], []),
        "destroy_starting_on_block_last_row": ([A[6]], []),
        "destroy_adjacent_and_storageless": ([A[7], A[8], A[9]], []),
        "destroy_first_and_last_segment": ([A[0], A[-1]], []),
        "slot_delete_block_first_and_last_row":
            ([], [(*R[512], 0), (*R[767], 0)]),
        "slot_upsert_block_last_row": ([], [(*R[1023], 999), shifter]),
        "slot_insert_between_blocks":
            ([], [(*_slot_after(R[767]), 5), (*_slot_after(R[255]), 6),
                  (*R[1400], 321)]),  # inserts alone leave every block flat
    }


ST_CASES = ["destroy_one_aligned_block", "destroy_whole_blocks_plus_tail",
            "destroy_inside_a_block", "destroy_ending_on_block_last_row",
            "destroy_starting_on_block_last_row",
            "destroy_adjacent_and_storageless",
            "destroy_first_and_last_segment",
            "slot_delete_block_first_and_last_row",
            "slot_upsert_block_last_row", "slot_insert_between_blocks"]


@pytest.mark.parametrize("incremental", [False, True],
                         ids=["apply_delta", "incremental"])
@pytest.mark.parametrize("case", ST_CASES)
def test_storage_merge_block_edges(eng, st_state, st_closed_form, case,
                                   incremental):
    state, A = st_state
    acc = copy.deepcopy(state)
    destroyed, strows = _st_cases(acc, A)[case]
    base = _st_rows(acc)
    assert len(strows) <= len(base) >> 8
    _reach(_storage_blocks(base, strows, set(destroyed)))
    # the chained delta: slot churn at the far end and next to a wipe
    tail = A[-2]
    follow = [(tail, sorted(state[tail][3])[0], 0),
              (tail, bind.keccak256(b"edge-follow"), 3),
              (A[1], dc.key_after(sorted(state[A[1]][3])[-1]), 4)]

    eng.upload(*_arrays_of(acc))
    if incremental:
        assert eng.root_retaining() == bind.state_root(*_arrays_of(acc))
    for rows, srows in (([dc.dele(k) for k in destroyed], strows),
                        ([], follow)):
        pre = list(acc)
        dc.apply_rows(acc, rows, srows)
        d, s = _mk_delta(rows, srows)
        if incremental:
            root = eng.incremental_root(d, s)
            got = eng.incremental_counters()
            assert got["small_st_merge"] == 1
            exp = dc.model(pre, list(acc), rows, srows)
            assert {k: got[k] for k in COUNTERS} == \
                {k: exp[k] for k in COUNTERS}
        else:
            eng.apply_delta(d, s)
            root = eng.root()
        assert root == bind.state_root(*_arrays_of(acc))
