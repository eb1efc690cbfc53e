"""Dirty-path incremental root on dense cells (tests/dense_cells.py): every
retained record is a multi-account subtree, so seeding a prebuilt subtree,
the position rebase, multi-position coverage, the sparse leaf list and the
re-capture of records that were themselves seeded all carry weight here.

Per delta the root must equal the oracle's on the dict-merged state AND the
engine's incremental counters (sre_get_incremental_counters) must equal the
key-only reuse model exactly: reusing more than the model would be a stale
subtree, reusing less a lost fast path — the root alone shows neither,
because an unseeded position is simply rehashed.

Each account scenario runs four ways: the general account merge (a single
storage slot in the state keeps the call off the accounts-only paths), the
small one-pass merge under its natural gate (delta <= na/64 after a warm-up
delta armed the retained lcp), the same merge forced by SRE_SD_FORCE, and
the with-updates form, whose net TrieUpdates diff must reproduce the
oracle's row set without touching any row of a reused cell.
"""
import copy
import os

import pytest

from oracle import bind
from tests import dense_cells as dc
from tests.test_gpu_incremental import _arrays_of, _mk_delta
from tests.test_gpu_incremental_updates import _rowmap, _apply_diff

pytestmark = pytest.mark.gpu

COUNTERS = ("examined", "seeded", "rehashed", "captured")


@pytest.fixture(scope="module")
def eng():
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def std_state():
    return dc.build_state()


@pytest.fixture(scope="module")
def slot_state():
    return dc.build_state(scale=0.55, slots=True)


def _setenv(name, value):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    return old


@pytest.fixture(params=["general", "natural", "forced", "updates"])
def way(request):
    old = _setenv("SRE_SD_FORCE", "1" if request.param == "forced" else None)
    yield request.param
    _setenv("SRE_SD_FORCE", old)


@pytest.fixture(params=[None, "0"], ids=["st_general", "st_closed_form"])
def st_gate(request):
    old = _setenv("SRE_ST_SMALL_MIN", request.param)
    yield request.param
    _setenv("SRE_ST_SMALL_MIN", old)


def _warmed(scenario):
    """One value-only delta first: the first call after root_retaining
    takes the general merge and arms the retained lcp."""
    def steps(acc):
        yield [dc.mod(acc, dc.keys_of(acc, dc.LONE)[0])], []
        yield from scenario(acc)
    return steps


def _oracle(acc):
    return bind.state_root_with_updates(*_arrays_of(acc))


def _run(eng, state, scenario, updates, small_acct, small_st):
    """Drive one scenario. small_acct / small_st(step, exp, rows, strows)
    give the merge the gates must select on that step."""
    acc = copy.deepcopy(state)
    eng.upload(*_arrays_of(acc))
    oroot, orows = _oracle(acc)
    if updates:
        root, rows0 = eng.root_retaining_with_updates()
        cur = _rowmap(rows0)
        assert cur == _rowmap(orows)
    else:
        root = eng.root_retaining()
    assert root == oroot
    assert eng.incremental_counters()["examined"] == 0, "reset by every call"
    steps = n_small = deep_rows = 0
    for rows, strows, exp in dc.walk(acc, _warmed(scenario)):
        d, s = _mk_delta(rows, strows)
        if updates:
            root, diff = eng.incremental_root_with_updates(d, s)
        else:
            root = eng.incremental_root(d, s)
        oroot, orows = _oracle(acc)
        assert root == oroot, f"step {steps}"
        got = eng.incremental_counters()
        print(f"step {steps}: delta {len(rows)}+{len(strows)} got {got} "
              f"want { {k: exp[k] for k in COUNTERS} }")
        assert {k: got[k] for k in COUNTERS} == \
            {k: exp[k] for k in COUNTERS}, f"step {steps}"
        assert got["small_acct_merge"] == small_acct(steps, exp, rows, strows), \
            f"step {steps}"
        assert got["small_st_merge"] == small_st(steps, exp, rows, strows), \
            f"step {steps}"
        n_small += got["small_acct_merge"]
        if updates:
            for k in exp["destroyed"]:
                assert k in {bytes(r["acct_key"])
                             for r in diff[diff["removed"] == 2]}, \
                    "destroyed account without a whole-trie marker"
            deep = dc.deep_account_rows(_rowmap(diff[diff["removed"] != 2]))
            deep_rows += len(deep)
            stale = [k for k, c in deep.items() if c in exp["reused"]]
            assert not stale, f"step {steps}: diff touches a reused cell"
            cur = _apply_diff(cur, diff)
            assert cur == _rowmap(orows), \
                f"step {steps}: diff does not reproduce rows"
        steps += 1
    assert steps >= 5  # warm-up + at least 4 chained deltas
    return n_small, deep_rows


def _never(step, exp, rows, strows):
    return 0


@pytest.mark.parametrize("name", sorted(dc.ACCOUNT_SCENARIOS))
def test_dense_account_scenarios(eng, std_state, way, name):
    scenario = dc.ACCOUNT_SCENARIOS[name]
    state = std_state
    if way == "general":
        # one slot anywhere keeps ns > 0: no accounts-only shortcut
        state = copy.deepcopy(std_state)
        anchor = dc.keys_of(state, dc.LONE)[-1]
        state[anchor][3][bind.keccak256(b"anchor-slot")] = 5
        small = _never
    elif way == "forced":
        def small(step, exp, rows, strows):
            return int(step > 0 and len(rows) > 0)
    else:
        def small(step, exp, rows, strows):
            return int(step > 0 and 0 < len(rows) <= exp["na_pre"] >> 6)
    n_small, deep_rows = _run(eng, state, scenario, way == "updates",
                              small, _never)
    if way != "general":
        assert n_small >= 1, "the small account merge never ran"
    if way == "updates":
        assert deep_rows > 0, "no diff row at path_len >= 5"


@pytest.mark.parametrize("updates", [False, True], ids=["plain", "updates"])
@pytest.mark.parametrize("name", sorted(dc.STORAGE_SCENARIOS))
def test_dense_storage_scenarios(eng, slot_state, st_gate, updates, name):
    # a storage-only delta dirties its account's cell; the sibling seeds
    # embed storage roots that were carried, not recomputed
    def small_st(step, exp, rows, strows):
        if st_gate is None:
            return 0
        keep = not strows and not any(r[4] for r in rows)
        assert keep or len(strows) <= exp["ns_pre"] >> 8
        return int(not keep)
    _run(eng, slot_state, dc.STORAGE_SCENARIOS[name], updates, _never,
         small_st)


def test_dense_counters_read_zero_after_other_calls(eng, std_state):
    eng.upload(*_arrays_of(std_state))
    eng.root_retaining()
    acc = copy.deepcopy(std_state)
    d, s = _mk_delta([dc.mod(acc, dc.deep_key(acc, dc.FULL_BIG))], [])
    eng.incremental_root(d, s)
    assert eng.incremental_counters()["seeded"] > 0
    eng.root()
    assert set(eng.incremental_counters().values()) == {0}
