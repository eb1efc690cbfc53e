"""Non-vacuity of tests/dense_cells.py (no GPU): the builder must really
produce every cell kind the dense incremental GPU tests rely on, and every
scenario must both reuse and rebuild something — otherwise those tests
could lose their coverage without failing."""
import copy

import pytest

from oracle import bind, pyref
from tests import dense_cells as dc
from tests.test_gpu_incremental import _arrays_of
from tests.test_gpu_incremental_updates import _rowmap


@pytest.fixture(scope="module")
def state():
    return dc.build_state()


@pytest.fixture(scope="module")
def rows(state):
    root, rows = bind.state_root_with_updates(*_arrays_of(state))
    return root, _rowmap(rows)


def _acct_paths(rowmap, c):
    """path lengths of the stored account rows inside cell c"""
    return sorted(k[2] for k, rc in dc.deep_account_rows(rowmap).items()
                  if rc == c)


def test_state_holds_every_cell_kind(state):
    assert 900 <= len(state) <= 1500
    pop = dc.populated(state)
    cap = dc.captured(state)
    assert all(pop[dc.FULL << 4 | c] for c in range(16)), "full sibling group"
    assert {c for c in pop if c >> 4 == dc.PAIR} == {dc.PAIR_BIG, dc.PAIR_SMALL}
    assert pop[dc.LONE] and dc.LONE not in cap
    assert sum(1 for c in pop if c >> 4 == dc.LONE >> 4) == 1
    # the neighbouring group shares exactly 3 nibbles with the full group
    assert dc.NEIGH >> 4 == dc.FULL >> 4 and dc.NEIGH != dc.FULL
    assert {dc.NEIGH_A, dc.NEIGH_B} <= cap and not pop[dc.NEIGH_GAP]
    assert all(pop[c] for c in dc.EDGES) and set(dc.EDGES) <= cap
    keys = sorted(state)
    assert dc.cell(keys[0]) == 0x00000 and dc.cell(keys[-1]) == 0xFFFFF
    assert pop[dc.FULL_LEAF] == 1 and dc.FULL_LEAF in cap
    assert pop[dc.FULL_SMALL] == 3
    assert len({dc.nibbles(k)[5] for k in dc.keys_of(state, dc.FULL_SMALL)}) == 3
    assert pop[dc.FULL_BIG] >= 40
    ext = [dc.nibbles(k) for k in dc.keys_of(state, dc.FULL_EXT)]
    assert len(ext) >= 2 and all(n[:10] == ext[0][:10] for n in ext)
    assert len({n[10] for n in ext}) >= 2, "the branch sits right at depth 10"
    # more than one account in (nearly) every retained cell
    assert sum(1 for c in cap if pop[c] > 1) >= len(cap) - 1


def test_oracle_matches_pyref_on_dense_state(state, rows):
    want = pyref.state_root({k: tuple(v) for k, v in state.items()})
    assert rows[0] == want
    assert bind.state_root(*_arrays_of(state)) == want


def test_update_rows_reach_below_the_cell_tops(rows):
    _, rowmap = rows
    acct = [k for k in rowmap if k[0] == 0]
    assert sum(1 for k in acct if k[2] == 4) >= 4
    assert sum(1 for k in acct if k[2] >= 5) >= 20
    # stored cell top; unstored cell top; extension over a stored branch
    assert _acct_paths(rowmap, dc.FULL_BIG)[0] == 5
    assert _acct_paths(rowmap, dc.FULL_SMALL) == []
    assert _acct_paths(rowmap, dc.FULL_EXT)[0] == 10


def _check_scenario(state, scenario, min_steps=4):
    acc = copy.deepcopy(state)
    cur = _rowmap(bind.state_root_with_updates(*_arrays_of(acc))[1])
    steps = deep_changes = 0
    for rows, strows, exp in dc.walk(acc, scenario):
        steps += 1
        assert exp["reused"], f"step {steps}: nothing reused"
        assert exp["rehashed"] > 0 and exp["seeded"] < len(dc.populated(acc)), \
            f"step {steps}: everything reused"
        new = _rowmap(bind.state_root_with_updates(*_arrays_of(acc))[1])
        changed = {k for k in set(cur) | set(new) if cur.get(k) != new.get(k)}
        deep = dc.deep_account_rows(changed)
        deep_changes += len(deep)
        # the oracle agrees with the model: no row inside a reused cell moves
        assert not [k for k, c in deep.items() if c in exp["reused"]], \
            f"step {steps}: a row of a clean cell changed"
        cur = new
    assert steps >= min_steps
    return deep_changes


@pytest.mark.parametrize("name", sorted(dc.ACCOUNT_SCENARIOS))
def test_account_scenarios_reuse_and_rebuild(state, name):
    deep = _check_scenario(state, dc.ACCOUNT_SCENARIOS[name])
    assert deep > 0, "no update row at path_len >= 5 changes in this scenario"


def _depth4_rows_after_first_delta(state, scenario, grp):
    """the oracle's path_len-4 account row of group `grp` before and after
    the scenario's first delta (None where it is not stored)"""
    acc = copy.deepcopy(state)

    def row():
        rowmap = _rowmap(bind.state_root_with_updates(*_arrays_of(acc))[1])
        hit = [v for k, v in rowmap.items() if k[0] == 0 and k[2] == 4
               and k[3] == grp.to_bytes(2, "big")]
        return hit[0] if hit else None
    before = row()
    next(dc.walk(acc, scenario))  # applies the first delta to acc
    return before, row()


def test_deleting_one_pair_cell_removes_the_depth4_row(state):
    before, after = _depth4_rows_after_first_delta(
        state, dc.sc_delete_one_cell_of_pair, dc.PAIR)
    assert before is not None and after is None


def test_small_cell_top_flips_the_parent_tree_mask(state):
    before, after = _depth4_rows_after_first_delta(
        state, dc.sc_small_cell_top_becomes_stored, dc.FULL)
    bit = 1 << (dc.FULL_SMALL & 0xF)
    assert before[1] & bit == 0 and after[1] & bit == bit  # tree_mask


@pytest.mark.parametrize("name", sorted(dc.STORAGE_SCENARIOS))
def test_storage_scenarios_reuse_and_rebuild(name):
    st_state = dc.build_state(scale=0.55, slots=True)
    assert 450 <= len(st_state) <= 700
    nslots = [len(v[3]) for v in st_state.values()]
    assert min(nslots) == 0 and max(nslots) == 8 and sum(nslots) <= 5000
    _check_scenario(st_state, dc.STORAGE_SCENARIOS[name])
