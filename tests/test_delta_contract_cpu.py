"""Non-vacuity of tests/delta_contract.py (no GPU): every builder must
produce the kind of bad delta it names, every twin and control must be a
valid delta of the same shape that really changes the state — otherwise
the follow-up steps of tests/test_gpu_rejections.py (the twin after a
rejected call gives the oracle root) could pass on an engine that ignores
deltas altogether."""
import copy

import numpy as np
import pytest

from oracle import bind
from reth_amd import gen
from tests import delta_contract as dc
from tests import dense_cells
from tests.test_gpu_incremental import _arrays_of, _dict_of

STATES = {"S": (96, 8), "A": (128, 0)}


@pytest.fixture(scope="module", params=sorted(STATES) + ["D"])
def state(request):
    if request.param == "D":  # the dense-cell state of the retention cases
        accounts = dense_cells.build_state(scale=0.55, slots=True)
        assert len(dense_cells.captured(accounts)) >= 20
        return accounts, bind.state_root(*_arrays_of(accounts))
    acct, st = gen.gen_state_numpy(*STATES[request.param],
                                   bind.keccak256_batch)
    accounts = _dict_of(acct, st)
    # random keys: nothing is captured, which is why D exists
    assert not dense_cells.captured(accounts)
    return accounts, bind.state_root(acct, st)


def _root_after(accounts, delta):
    acc = copy.deepcopy(accounts)
    dc.apply(acc, delta)
    return bind.state_root(*_arrays_of(acc))


@pytest.mark.parametrize("kind", list(dc.KINDS))
def test_bad_delta_and_twin(state, kind):
    accounts, root0 = state
    case = dc.KINDS[kind](accounts, np.random.default_rng(1))
    assert case.kind == kind
    assert dc.verdict(accounts, *case.bad) == case.token
    assert dc.verdict(accounts, *case.twin) is None
    assert dc.shape(case.twin) == dc.shape(case.bad)
    assert _root_after(accounts, case.twin) != root0


def test_each_kind_has_exactly_its_defect(state):
    # mending the one defect a builder plants gives a valid delta: sorting
    # cures K1/K3, nothing but the twin cures the rest — so no bad delta
    # carries a second defect that could earn its rejection instead
    accounts, _ = state
    for kind, build in dc.KINDS.items():
        rows, strows = build(accounts, np.random.default_rng(2)).bad
        mended = dc.verdict(accounts, sorted(rows), sorted(strows))
        if kind in ("K1", "K3-within", "K3-across"):
            assert mended is None, kind
        else:
            assert mended == dc.KINDS[kind](
                accounts, np.random.default_rng(2)).token, kind


def test_unknown_keys_sit_where_they_say(state):
    accounts, _ = state
    keys = sorted(accounts)
    assert dc.unknown_key(accounts, "before") < keys[0]
    assert keys[0] < dc.unknown_key(accounts, "between") < keys[-1]
    assert dc.unknown_key(accounts, "after") > keys[-1]
    for where in ("before", "between", "after"):
        case = dc.k6_row_for_unknown(accounts, np.random.default_rng(3), where)
        (f, *_), = case.bad[0]
        # the inserted account shifts at least half of the positions, and
        # nothing is deleted
        assert sum(1 for k in keys if k > f) >= len(keys) // 2
        assert dc.shape(case.bad)[2] == 0


@pytest.mark.parametrize("name", list(dc.CONTROLS))
def test_controls_are_accepted(state, name):
    accounts, root0 = state
    delta = dc.CONTROLS[name](accounts, np.random.default_rng(4))
    assert dc.verdict(accounts, *delta) is None
    changed = _root_after(accounts, delta) != root0
    assert changed == (name != "C1")


def test_good_deltas_change_the_state():
    acct, st = gen.gen_state_numpy(*STATES["S"], bind.keccak256_batch)
    accounts = _dict_of(acct, st)
    rng = np.random.default_rng(5)
    root = bind.state_root(acct, st)
    seen = set()
    for step in range(6):
        for max_st in (1, 2, 3):
            d = dc.good_delta(accounts, rng, step, max_st)
            assert dc.verdict(accounts, *d) is None
            assert 1 <= len(d[1]) <= max_st
        dc.apply(accounts, d)
        seen.add((dc.shape(d)[0] > 0, dc.shape(d)[2]))
        new = bind.state_root(*_arrays_of(accounts))
        assert new != root
        root = new
    # slot-only, destroying and inserting flavours all occurred
    assert seen == {(False, 0), (True, 1), (True, 0)}
