"""tests/revert_model.py against tests/delta_contract.py (no GPU): the revert
of a valid delta is a valid delta over the post state, applying it restores
the pre state exactly, and the revert of the revert restores the post
state — over chained deltas of every flavour, and on hand-written deltas
for every branch of the definition that emits no row. The GPU tests compare
the engine's capture with this model row for row, so the model has to be
right on its own."""
import copy

import numpy as np
import pytest

from oracle import bind
from reth_amd import gen
from tests import delta_contract as dc
from tests import revert_model as rm
from tests.test_gpu_incremental import _dict_of
from tests.util import random_accounts

KE = dc.KE


def _states():
    acct, st = gen.gen_state_numpy(96, 8, bind.keccak256_batch)
    yield "S", _dict_of(acct, st)
    # tuples in, lists out: normalise before comparing dicts
    yield "R", rm.normalised(random_accounts(3, 60))


@pytest.fixture(scope="module", params=["S", "R"])
def state(request):
    return dict(_states())[request.param]


def _round_trip(pre, delta):
    """the three properties for one delta; returns the post state"""
    post = copy.deepcopy(pre)
    dc.apply(post, delta)
    rev = rm.revert_of(pre, delta)
    assert dc.verdict(post, *rev) is None
    assert [r[0] for r in rev[0]] == sorted(r[0] for r in rev[0])
    back = copy.deepcopy(post)
    dc.apply(back, rev)
    assert back == pre
    redo = rm.revert_of(post, rev)
    assert dc.verdict(back, *redo) is None
    again = copy.deepcopy(back)
    dc.apply(again, redo)
    assert again == post
    cnt = rm.counts_of(pre, delta)
    assert cnt["acct_rows"] == len(rev[0])
    assert cnt["st_rows"] + cnt["wiped_rows"] == len(rev[1])
    assert cnt["acct_rows"] + cnt["st_rows"] + cnt["no_row"] == \
        len(delta[0]) + len(delta[1])
    return post


def test_chained_good_deltas(state):
    accounts = copy.deepcopy(state)
    rng = np.random.default_rng(21)
    seen = set()
    for step in range(27):
        delta = dc.good_delta(accounts, rng, step, max_st=3)
        cnt = rm.counts_of(accounts, delta)
        seen.add((step % 3, cnt["wiped_rows"] > 0, cnt["no_row"] > 0))
        accounts = _round_trip(accounts, delta)
    # slot upserts and deletes; a wiped segment; an inserted account whose
    # storage rows leave no revert row
    assert seen == {(0, False, False), (1, True, False), (2, False, True)}


def _some(accounts):
    c, d = dc._pick(accounts, np.random.default_rng(22), 2, want_slots=True)
    return c, d


def test_delete_of_an_absent_account_leaves_no_row(state):
    u = dc.unknown_key(state, "between")
    delta = ([(u, 0, 0, KE, 1)], [])
    assert rm.revert_of(state, delta) == ([], [])
    assert rm.counts_of(state, delta) == {
        "acct_rows": 0, "st_rows": 0, "wiped_rows": 0, "no_row": 1}
    assert _round_trip(state, delta) == state


def test_rows_of_an_inserted_account_leave_no_row(state):
    delta = dc.c2_row_for_inserted(state, np.random.default_rng(23))
    (f, *_), = delta[0]
    assert rm.revert_of(state, delta) == ([(f, 0, 0, KE, 1)], [])
    assert rm.counts_of(state, delta)["no_row"] == 1
    post = _round_trip(state, delta)
    assert f in post and post[f][3]


def test_zero_row_for_an_unknown_account_leaves_no_row(state):
    delta = dc.c1_zero_row_for_unknown(state, np.random.default_rng(24))
    assert rm.revert_of(state, delta) == ([], [])
    assert rm.counts_of(state, delta)["no_row"] == 1
    assert _round_trip(state, delta) == state


def test_zero_row_for_an_absent_slot_leaves_no_row(state):
    c, _ = _some(state)
    absent = dc._fresh_slot(b"rm-absent", c[:4])
    assert absent not in state[c][3]
    delta = ([], [(c, absent, 0)])
    assert rm.revert_of(state, delta) == ([], [])
    assert rm.counts_of(state, delta)["no_row"] == 1
    assert _round_trip(state, delta) == state


def test_every_emitting_branch_by_hand(state):
    c, d = _some(state)
    have = sorted(state[c][3])[0]
    fresh = dc._fresh_slot(b"rm-fresh", c[:4])
    f = dc._fresh_account(state, b"rm")
    rows = sorted([(d, 0, 0, KE, 1), dc._bump(state, c, 5), (f, 2, 9, KE, 0)])
    strows = sorted([(c, have, 0), (c, fresh, 77)])
    rrows, rst = rm.revert_of(state, (rows, strows))
    n, b, ch, slots = state[d]
    assert sorted(rrows) == sorted([(d, n, b, ch, 0),
                                    (c,) + tuple(state[c][:3]) + (0,),
                                    (f, 0, 0, KE, 1)])
    assert rst == sorted([(c, have, state[c][3][have]), (c, fresh, 0)] +
                         [(d, sk, v) for sk, v in slots.items()])
    assert rm.counts_of(state, (rows, strows)) == {
        "acct_rows": 3, "st_rows": 2, "wiped_rows": len(slots), "no_row": 0}
    _round_trip(state, (rows, strows))
