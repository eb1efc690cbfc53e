"""What every root-type call leaves in stats() and incremental_counters().

A characterisation of the host driver's call prologue and epilogue, so that
restructuring them cannot change what a caller reads afterwards:

  - root, root_with_updates, subtree_roots and root_from_nodes publish the
    stats of the call;
  - root_retaining and root_retaining_with_updates zero the stats and
    publish nothing;
  - incremental_root and incremental_root_with_updates publish levels,
    branch_count and the times, zero leaf_count / leaf_blocks /
    branch_blocks, and fill the six incremental counters;
  - account_proof, storage_proof and storage_roots leave stats() alone;
  - a rejected incremental call leaves zeroed stats, the examined counter
    and a state that root_retaining can rebuild from.

Every integer in EXPECTED is a deterministic function of the inputs built
here. They were read off a run of this file's scenarios on the parent
commit of the change that introduced this test (the driver before its call
frame and incremental steps were factored out), not off the code under
test. Roots are checked against the CPU oracle.
"""
import os

import pytest

from oracle import bind
from tests.test_gpu_incremental import _arrays_of, _mk_delta

pytestmark = pytest.mark.gpu

KE = bind.keccak256(b"")
INT_FIELDS = ("leaf_count", "leaf_blocks", "branch_count", "branch_blocks",
              "levels")
MS_FIELDS = ("total_ms", "leaf_hash_ms", "branch_hash_ms", "sort_ms")


def _storage_state():
    """96 accounts, every third one (32) with 4 slots."""
    accounts = {}
    for i in range(96):
        slots = {}
        if i % 3 == 0:
            slots = {bind.keccak256(b"cs-slot" + bytes([i, j])): 1000 + 7 * i + j
                     for j in range(4)}
        accounts[bind.keccak256(b"cs-acct" + bytes([i]))] = \
            [i, 10 ** 9 + i, KE, slots]
    return accounts


def _plain_state():
    """256 accounts, no storage."""
    return {bind.keccak256(b"cp-acct" + bytes([i])): [i, 5000 + i, KE, {}]
            for i in range(256)}


def _storage_delta(accounts):
    """3 account rows (one an insert) + 2 slot rows in 2 touched accounts;
    applied to `accounts`."""
    keys = sorted(accounts)
    with_slots = [k for k in keys if accounts[k][3]]
    plain = [k for k in keys if not accounts[k][3]]
    rows = []
    for k in (plain[3], plain[40]):
        accounts[k][1] += 11
        rows.append((k, accounts[k][0], accounts[k][1], accounts[k][2], 0))
    nk = bind.keccak256(b"cs-new")
    assert nk not in accounts
    accounts[nk] = [1, 77, KE, {}]
    rows.append((nk, 1, 77, KE, 0))
    strows = []
    for n, k in enumerate((with_slots[2], with_slots[20])):
        sk = bind.keccak256(b"cs-fresh" + bytes([n]))
        accounts[k][3][sk] = 31 + n
        strows.append((k, sk, 31 + n))
    return _mk_delta(rows, strows)


def _plain_delta(accounts, step, n_rows=2):
    """n_rows account rows: balance changes and one insert; applied to
    `accounts`."""
    keys = sorted(accounts)
    rows = []
    for j in range(n_rows - 1):
        k = keys[17 + 50 * step + 9 * j]
        accounts[k][1] += 3
        rows.append((k, accounts[k][0], accounts[k][1], accounts[k][2], 0))
    nk = bind.keccak256(b"cp-new" + bytes([step]))
    assert nk not in accounts
    accounts[nk] = [2, 9 + step, KE, {}]
    rows.append((nk, 2, 9 + step, KE, 0))
    return _mk_delta(rows, [])


def _ints(eng):
    s = eng.stats()
    return {f: s[f] for f in INT_FIELDS}


def _published(eng):
    """The integer stats of a call that publishes; its time must be set."""
    assert eng.stats()["total_ms"] > 0
    return _ints(eng)


def _want(accounts):
    return bind.state_root(*_arrays_of(accounts))


# ---- scenarios: each returns {label: observed integers} -------------------

def observe_full(eng, make_state):
    accounts = make_state()
    acct, st = _arrays_of(accounts)
    want = bind.state_root(acct, st)
    seen = {}
    eng.upload(acct, st)
    assert eng.root() == want
    seen["root"] = _published(eng)
    root, rows = eng.root_with_updates()
    assert root == want
    seen["root_with_updates"] = _published(eng)
    seen["root_with_updates"]["rows"] = len(rows)
    assert eng.finish_top(*eng.subtree_roots()) == want
    seen["subtree_roots"] = _published(eng)
    assert eng.root_from_nodes(rows) == want
    seen["root_from_nodes"] = _published(eng)
    return seen


def observe_retaining(eng, make_state):
    accounts = make_state()
    acct, st = _arrays_of(accounts)
    want = bind.state_root(acct, st)
    seen = {}
    eng.upload(acct, st)
    assert eng.root() == want  # nonzero stats for the next call to zero
    assert eng.root_retaining() == want
    seen["root_retaining"] = eng.stats()
    assert eng.root() == want
    root, _ = eng.root_retaining_with_updates()
    assert root == want
    seen["root_retaining_with_updates"] = eng.stats()
    return seen


def _incremental_call(eng, with_updates, d, s):
    if with_updates:
        root, rows = eng.incremental_root_with_updates(d, s)
        extra = {"rows": len(rows)}
    else:
        root, extra = eng.incremental_root(d, s), {}
    got = _published(eng)
    got.update(eng.incremental_counters())
    got.update(extra)
    return root, got


def observe_incremental_storage(eng, with_updates):
    accounts = _storage_state()
    eng.upload(*_arrays_of(accounts))
    want = _want(accounts)
    if with_updates:
        assert eng.root_retaining_with_updates()[0] == want
    else:
        assert eng.root_retaining() == want
    d, s = _storage_delta(accounts)
    root, got = _incremental_call(eng, with_updates, d, s)
    assert root == _want(accounts)
    return {"delta": got}


def observe_incremental_plain(eng, with_updates):
    """Chained deltas of 2, 2 and 6 rows. The first follows root_retaining,
    which leaves no repaired lcp, so it takes the general merge. The second
    is within na/64 rows and takes the small merge with or without
    SRE_SD_FORCE. The third is above na/64: general unless forced."""
    accounts = _plain_state()
    eng.upload(*_arrays_of(accounts))
    want = _want(accounts)
    if with_updates:
        assert eng.root_retaining_with_updates()[0] == want
    else:
        assert eng.root_retaining() == want
    seen = {}
    for step, n_rows in enumerate((2, 2, 6)):
        d, s = _plain_delta(accounts, step, n_rows)
        root, got = _incremental_call(eng, with_updates, d, s)
        assert root == _want(accounts), step
        seen[f"delta{step}"] = got
    return seen


def observe_rejected(eng, state):
    """An unsorted account delta after one good delta. Over the storage
    state the general merge rejects it; over the accounts-only state the
    small merge's host check does."""
    accounts = STATES[state]()
    eng.upload(*_arrays_of(accounts))
    assert eng.root_retaining() == _want(accounts)
    if state == "storage":
        d, s = _storage_delta(accounts)
    else:
        d, s = _plain_delta(accounts, 0)
    assert eng.incremental_root(d, s) == _want(accounts)
    good = eng.incremental_counters()
    keys = sorted(accounts)
    rows = [(k, accounts[k][0], accounts[k][1] + 1, accounts[k][2], 0)
            for k in (keys[5], keys[9])]
    bad, _ = _mk_delta(rows, [])
    bad = bad[::-1].copy()  # descending keys
    with pytest.raises(RuntimeError, match="accounts-not-sorted"):
        eng.incremental_root(bad)
    seen = {"stats": eng.stats(), "counters": eng.incremental_counters()}
    # the one counter a rejected call fills: the rows retained on entry
    assert seen["counters"]["examined"] == good["captured"]
    assert eng.root_retaining() == _want(accounts)
    return seen


STATES = {"storage": _storage_state, "plain": _plain_state}


# ---- expectations, from the parent commit (see the module docstring) ------

ZERO_STATS = {f: 0 for f in INT_FIELDS + MS_FIELDS}


def _full(leaf_count, leaf_blocks, branch_count, branch_blocks, levels, **more):
    return dict(leaf_count=leaf_count, leaf_blocks=leaf_blocks,
                branch_count=branch_count, branch_blocks=branch_blocks,
                levels=levels, **more)


def _inc(levels, branch_count, examined, seeded, rehashed, captured, small,
         rows):
    """An incremental call: the three partial totals are published as 0;
    `rows` is the length of the net diff (with-updates calls only)."""
    return dict(leaf_count=0, leaf_blocks=0, branch_blocks=0, levels=levels,
                branch_count=branch_count, examined=examined, seeded=seeded,
                rehashed=rehashed, captured=captured, small_acct_merge=small,
                small_st_merge=0, rows=rows)


EXPECTED_FULL = {
    "storage": {
        "root": _full(224, 320, 71, 115, 6),
        "root_with_updates": _full(224, 320, 71, 115, 6, rows=19),
        "subtree_roots": _full(224, 320, 70, 127, 5),
        # tries whose root row is in `rows` are seeded, not rebuilt
        "root_from_nodes": _full(196, 292, 57, 101, 5),
    },
    "plain": {
        "root": _full(256, 512, 87, 132, 5),
        "root_with_updates": _full(256, 512, 87, 132, 5, rows=21),
        "subtree_roots": _full(256, 512, 86, 144, 4),
        "root_from_nodes": _full(256, 512, 87, 132, 5),
    },
}
EXPECTED_INC_STORAGE = _inc(5, 34, 0, 0, 97, 0, 0, rows=2)
EXPECTED_INC_PLAIN = {  # keyed by SRE_SD_FORCE
    False: {"delta0": _inc(5, 87, 2, 2, 255, 2, 0, rows=3),
            "delta1": _inc(5, 87, 2, 2, 256, 2, 1, rows=3),
            "delta2": _inc(5, 88, 2, 2, 257, 2, 0, rows=5)},
    True: {"delta0": _inc(5, 87, 2, 2, 255, 2, 0, rows=3),
           "delta1": _inc(5, 87, 2, 2, 256, 2, 1, rows=3),
           "delta2": _inc(5, 88, 2, 2, 257, 2, 1, rows=5)},
}
# a rejected call has zeroed every counter and filled `examined` only
EXPECTED_REJECTED_EXAMINED = {"storage": 0, "plain": 2}


def _expect(want, with_updates):
    return want if with_updates else {k: v for k, v in want.items()
                                      if k != "rows"}


@pytest.fixture(scope="module")
def eng():
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()


@pytest.fixture()
def force_small():
    os.environ["SRE_SD_FORCE"] = "1"  # read per call
    yield
    os.environ.pop("SRE_SD_FORCE", None)


@pytest.mark.parametrize("state", sorted(STATES))
def test_full_root_calls_publish_their_stats(eng, state):
    seen = observe_full(eng, STATES[state])
    print(state, seen)
    assert seen == EXPECTED_FULL[state]


@pytest.mark.parametrize("state", sorted(STATES))
def test_retaining_calls_publish_nothing(eng, state):
    seen = observe_retaining(eng, STATES[state])
    print(state, seen)
    assert seen == {"root_retaining": ZERO_STATS,
                    "root_retaining_with_updates": ZERO_STATS}


@pytest.mark.parametrize("with_updates", [False, True])
def test_incremental_general_merge_subset_storage(eng, with_updates):
    seen = observe_incremental_storage(eng, with_updates)
    print(with_updates, seen)
    assert seen == {"delta": _expect(EXPECTED_INC_STORAGE, with_updates)}


def _check_plain(seen, with_updates, forced):
    want = EXPECTED_INC_PLAIN[forced]
    assert seen == {k: _expect(v, with_updates) for k, v in want.items()}
    assert [seen[f"delta{i}"]["small_acct_merge"] for i in range(3)] == \
        [0, 1, int(forced)]


@pytest.mark.parametrize("with_updates", [False, True])
def test_incremental_accounts_only(eng, with_updates):
    seen = observe_incremental_plain(eng, with_updates)
    print(with_updates, seen)
    _check_plain(seen, with_updates, False)


@pytest.mark.parametrize("with_updates", [False, True])
def test_incremental_accounts_only_forced_small(eng, force_small, with_updates):
    seen = observe_incremental_plain(eng, with_updates)
    print(with_updates, seen)
    _check_plain(seen, with_updates, True)


def test_proofs_and_storage_roots_leave_stats_alone(eng):
    accounts = _storage_state()
    acct, st = _arrays_of(accounts)
    eng.upload(acct, st)
    assert eng.root() == bind.state_root(acct, st)
    before = eng.stats()
    assert before["total_ms"] > 0 and before["leaf_count"] == len(acct) + len(st)
    keys = sorted(accounts)
    owner = next(k for k in keys if accounts[k][3])
    assert len(eng.account_proof([keys[0], keys[50], b"\x55" * 32])) == 3
    assert eng.stats() == before
    roots, proofs = eng.storage_proof([owner, keys[1]],
                                      [sorted(accounts[owner][3])[0], KE])
    assert len(roots) == len(proofs) == 2
    assert eng.stats() == before
    assert eng.storage_roots(len(acct)).shape == (len(acct), 32)
    assert eng.stats() == before


@pytest.mark.parametrize("state", sorted(STATES))
def test_rejected_incremental_call(eng, state):
    seen = observe_rejected(eng, state)
    print(state, seen)
    assert seen["stats"] == ZERO_STATS
    want = dict.fromkeys(seen["counters"], 0)
    want["examined"] = EXPECTED_REJECTED_EXAMINED[state]
    assert len(want) == 6 and seen["counters"] == want
