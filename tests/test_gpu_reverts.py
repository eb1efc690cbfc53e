"""Revert capture and unwind on the GPU (include/sre.h
sre_set_revert_capture ... sre_unwind_with_updates).

The expected revert of a delta comes from tests/revert_model.py (checked
without a GPU in test_revert_model_cpu.py); the engine's capture has to
equal it row for row, and its four counters the model's. States, deltas and
the gates that select a merge path are those of tests/test_gpu_rejections.py:

  S = gen_state_numpy(96, 8): general storage merge, and with
      SRE_ST_SMALL_MIN=0 the closed-form one (n_st <= 768 >> 8 = 3);
  A = gen_state_numpy(128, 0) with SRE_SD_FORCE=1: the one-pass account
      merge. It exists for accounts-only deltas over accounts-only states,
      and every flavour of delta_contract.good_delta carries storage rows,
      so this path gets an accounts-only delta written here that walks all
      three account decisions;
  B = 2,503 accounts and 11,400 slots for the shapes at which the capture
      kernels can go wrong (several blocks of the segment copy, more than
      one tile of the scan).

The merge path is proven from incremental_counters(); the entries that do
not publish them run a delta that went through incremental_root on a fresh
upload of the same state first (the gates look at counts only).
"""
import copy
import ctypes
import os

import numpy as np
import pytest

from oracle import bind, pyref
from reth_amd import gen, plain
from reth_amd.engine import DELTA_DTYPE, STORAGE_DTYPE
from tests import delta_contract as dc
from tests import revert_model as rm
from tests.test_gpu_incremental import _arrays_of, _dict_of
from tests.test_gpu_incremental_updates import _apply_diff
from tests.test_gpu_rejections import (ENTRIES, NEEDS_CELLS, NO_DELTA, PATHS,
                                       _call, _oracle_root, _oracle_rows,
                                       _raw_delta, _took)

pytestmark = pytest.mark.gpu

KE = dc.KE
GATES = {p: PATHS[p][1] for p in ("general", "closed", "small")}
NO_REVERT = "no-revert-captured"


@pytest.fixture(scope="module")
def eng():
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _capture_off_afterwards(eng):
    yield
    eng.capture_reverts(False)


@pytest.fixture()
def gate(request):
    env = GATES[request.param]
    os.environ.update(env)
    yield request.param
    for k in env:
        os.environ.pop(k, None)


def _big_state():
    """B: random accounts with 4 slots each, plus an account of 700 slots
    at either end of the key order and a storage-less one in the middle."""
    acct, st = gen.gen_state_numpy(2500, 4, bind.keccak256_batch)
    accounts = _dict_of(acct, st)
    keys = sorted(accounts)
    first, last = bytes(31) + b"\x01", b"\xff" * 32
    assert first < keys[0] and keys[-1] < last
    for k, tag in ((first, b"f"), (last, b"l")):
        accounts[k] = [1, 5, KE, {dc._fresh_slot(tag, i.to_bytes(2, "big")): 1 + i
                                  for i in range(700)}]
    bare = (int.from_bytes(keys[1200], "big") + 1).to_bytes(32, "big")
    assert bare not in accounts
    accounts[bare] = [2, 6, KE, {}]
    return accounts, first, last, bare


@pytest.fixture(scope="module")
def states():
    out = {}
    for name in ("S", "A"):
        acct, st = gen.gen_state_numpy(
            *{"S": (96, 8), "A": (128, 0)}[name], bind.keccak256_batch)
        out[name] = (acct, st, _dict_of(acct, st))
    big, first, last, bare = _big_state()
    out["B"] = _arrays_of(big) + (big,)
    out["B-keys"] = (first, last, bare)
    return out


def _accounts_only_delta(accounts, tag):
    """the three account decisions in one valid accounts-only delta: two
    upserts and a destroy of resident keys, an insert, and deleted = 1 for
    a key that is not resident"""
    rng = np.random.default_rng(31)
    a, b, c = dc._pick(accounts, rng, 3)
    f = dc._fresh_account(accounts, tag)
    u = dc.unknown_key(accounts, "between")
    return sorted([dc._bump(accounts, a, 3), dc._bump(accounts, b, 4),
                   (c, 0, 0, KE, 1), (f, 1, 9, KE, 0), (u, 0, 0, KE, 1)]), []


def _delta_for(path, accounts, flavour):
    if path == "small":
        return _accounts_only_delta(accounts, b"rv" + bytes([flavour]))
    return dc.good_delta(accounts, np.random.default_rng(40 + flavour), flavour)


def _arm(eng, state):
    """fresh upload with everything armed; returns the node rows"""
    acct, st, _ = state
    eng.upload(acct, st)
    _, nodes = eng.root_with_updates()
    eng.root_retaining_with_updates()
    eng.incremental_root_with_updates(NO_DELTA)  # arms the small path's lcp
    return nodes


def _revert_is(eng, pre, delta):
    """revert() and revert_counters() equal the model's, byte for byte"""
    want_a, want_s = _raw_delta(rm.revert_of(pre, delta))
    got_a, got_s = eng.revert()
    assert got_a.dtype == DELTA_DTYPE and got_s.dtype == STORAGE_DTYPE
    assert eng.revert_counts() == (len(want_a), len(want_s))
    assert got_a.tobytes() == want_a.tobytes()
    assert got_s.tobytes() == want_s.tobytes()
    assert eng.revert_counters() == rm.counts_of(pre, delta)


def _state_is(eng, accounts):
    """root, resident rows and storage roots are the oracle's"""
    arrays = _arrays_of(accounts)
    acct, st = eng.download()
    assert acct.tobytes() == arrays[0].tobytes()
    assert st.tobytes() == arrays[1].tobytes()
    if len(accounts):
        assert np.array_equal(eng.storage_roots(len(accounts)),
                              bind.storage_roots(*arrays))


# ---- row-for-row equality --------------------------------------------------

def _equality_cases():
    for path in GATES:
        for entry in ENTRIES[path]:
            for flavour in ((0,) if path == "small" else (0, 1, 2)):
                yield pytest.param(path, entry, flavour,
                                   id=f"{path}-{entry}-f{flavour}")


@pytest.mark.parametrize("gate,entry,flavour", list(_equality_cases()),
                         indirect=["gate"])
def test_revert_equals_model(eng, states, gate, entry, flavour):
    path = gate
    state = states[PATHS[path][0]]
    pre = state[2]
    delta = _delta_for(path, pre, flavour)
    eng.capture_reverts(True)
    if entry != "incremental_root":
        # the path this delta takes, read off an entry that reports it
        _arm(eng, state)
        _call(eng, "incremental_root", delta)
        assert _took(eng.incremental_counters(), path)
    nodes = _arm(eng, state)
    assert eng.revert_counts() == (0, 0)  # the upload dropped the last one
    root, _ = _call(eng, entry, delta, nodes)
    if entry == "incremental_root":
        assert _took(eng.incremental_counters(), path)
    _revert_is(eng, pre, delta)
    post = copy.deepcopy(pre)
    dc.apply(post, delta)
    if root is not None:
        assert root == _oracle_root(post)
    _state_is(eng, post)


# ---- round trip ------------------------------------------------------------

@pytest.mark.parametrize("gate,flavour",
                         [(p, f) for p in GATES
                          for f in ((0,) if p == "small" else (0, 1, 2))],
                         indirect=["gate"])
def test_unwind_and_redo(eng, states, gate, flavour):
    path = gate
    state = states[PATHS[path][0]]
    pre = state[2]
    delta = _delta_for(path, pre, flavour)
    post = copy.deepcopy(pre)
    dc.apply(post, delta)
    _arm(eng, state)
    eng.capture_reverts(True)
    assert eng.incremental_root(*_raw_delta(delta)) == _oracle_root(post)
    assert _took(eng.incremental_counters(), path)
    # back ...
    assert eng.unwind() == _oracle_root(pre)
    _state_is(eng, pre)
    # ... and the unwind captured too: the stored revert is now the redo
    _revert_is(eng, post, rm.revert_of(pre, delta))
    assert eng.unwind() == _oracle_root(post)
    _state_is(eng, post)


@pytest.mark.parametrize("gate", ["general", "closed"], indirect=True)
def test_unwind_with_updates_gives_the_earlier_rows(eng, states, gate):
    state = states["S"]
    pre = state[2]
    delta = dc.good_delta(pre, np.random.default_rng(50), 1)
    post = copy.deepcopy(pre)
    dc.apply(post, delta)
    _arm(eng, state)
    eng.capture_reverts(True)
    root, diff = eng.incremental_root_with_updates(*_raw_delta(delta))
    want_pre, rows_pre = _oracle_rows(pre)
    want_post, rows_post = _oracle_rows(post)
    assert root == want_post
    assert _apply_diff(copy.deepcopy(rows_pre), diff) == rows_post
    root, diff = eng.unwind_with_updates()
    assert root == want_pre
    assert _apply_diff(copy.deepcopy(rows_post), diff) == rows_pre
    _state_is(eng, pre)


# ---- chain -----------------------------------------------------------------

@pytest.mark.parametrize("with_updates", [False, True])
def test_chain_of_fetched_reverts_newest_first(eng, states, with_updates):
    state = states["S"]
    accounts = copy.deepcopy(state[2])
    rng = np.random.default_rng(60)
    _arm(eng, state)
    eng.capture_reverts(True)
    history, reverts = [copy.deepcopy(accounts)], []
    for step in range(6):
        delta = dc.good_delta(accounts, rng, step)
        root, _ = eng.incremental_root_with_updates(*_raw_delta(delta))
        _revert_is(eng, accounts, delta)
        reverts.append(eng.revert())
        dc.apply(accounts, delta)
        assert root == _oracle_root(accounts)
        history.append(copy.deepcopy(accounts))
    _, cur = _oracle_rows(accounts)
    for step in reversed(range(6)):
        earlier = history[step]
        if with_updates:
            root, diff = eng.incremental_root_with_updates(*reverts[step])
            want, want_rows = _oracle_rows(earlier)
            assert _apply_diff(cur, diff) == want_rows
            assert root == want
        else:
            assert eng.incremental_root(*reverts[step]) == _oracle_root(earlier)
        _state_is(eng, earlier)


# ---- shapes at which the capture kernels can go wrong ----------------------

def _slot_rows(accounts, k, tag):
    """an old slot changed, an old slot deleted, a fresh one set, and a zero
    for an absent one"""
    have = sorted(accounts[k][3])
    return [(k, have[0], 4242), (k, have[1], 0),
            (k, dc._fresh_slot(tag, k[:4]), 17),
            (k, dc._fresh_slot(tag + b"z", k[:4]), 0)]


def _shape_delta(states, which):
    accounts = states["B"][2]
    first, last, bare = states["B-keys"]
    keys = [k for k in sorted(accounts) if k not in (first, last, bare)]
    u = dc.unknown_key(accounts, "between")
    if which == "ends":
        # the 700-slot accounts at either end go (each segment spans several
        # 256-thread blocks of the copy), with delta rows between them, for
        # an inserted account among them, and a zero row for an unknown one
        f = dc._fresh_account(accounts, b"shape")
        rows = [(first, 0, 0, KE, 1), (last, 0, 0, KE, 1), (f, 1, 1, KE, 0),
                (u, 0, 0, KE, 1)]
        strows = _slot_rows(accounts, keys[700], b"e1") + \
            [(f, dc._fresh_slot(b"e2", b"a"), 5), (f, dc._fresh_slot(b"e2", b"b"), 6),
             (bytes(31) + b"\x02", dc._fresh_slot(b"e3", b"u"), 0)]
    elif which == "adjacent":
        # two adjacent destroyed accounts, a third further on, the
        # storage-less one; delta rows before, between and after the segments
        rows = [(keys[100], 0, 0, KE, 1), (keys[101], 0, 0, KE, 1),
                (bare, 0, 0, KE, 1), (keys[2000], 0, 0, KE, 1)]
        strows = _slot_rows(accounts, keys[5], b"a1") + \
            _slot_rows(accounts, keys[1000], b"a2") + \
            _slot_rows(accounts, keys[2400], b"a3") + \
            [(u, dc._fresh_slot(b"a4", b"u"), 0)]
    elif which == "many-slots":
        # > 2,048 storage rows: past one tile of the scan, with a destroyed
        # 700-slot segment in the middle of the output
        rows = [(keys[1101], 0, 0, KE, 1), (last, 0, 0, KE, 1)]
        strows = []
        for i, k in enumerate(keys[:2200:2]):
            have = sorted(accounts[k][3])
            strows += [(k, have[i % 4], 0 if i % 3 == 0 else 900 + i),
                       (k, dc._fresh_slot(b"m", k[:4]), i % 5)]
        strows.append((first, sorted(accounts[first][3])[350], 0))
        assert len(strows) > 2048
    else:
        # > 2,048 account rows: upserts, inserts, destroys, and deletes of
        # absent keys, all mixed
        assert which == "many-accounts"
        rows = []
        for i, k in enumerate(keys[:2300]):
            if i % 7 == 3:
                rows.append((k, 0, 0, KE, 1))
            else:
                rows.append(dc._bump(accounts, k, 1 + i))
            if i % 9 == 0:
                nk = (int.from_bytes(k, "big") + 1).to_bytes(32, "big")
                assert nk not in accounts
                rows.append((nk, i, 3, KE, i % 2))
        rows += [(first, 0, 0, KE, 1)]
        strows = [(last, sorted(accounts[last][3])[0], 0)]
        assert len(rows) > 2048
    delta = (sorted(rows), sorted(strows))
    assert dc.verdict(accounts, *delta) is None
    return delta


@pytest.mark.parametrize("gate,which", [
    ("general", "ends"), ("closed", "ends"), ("general", "adjacent"),
    ("closed", "adjacent"), ("general", "many-slots"),
    ("general", "many-accounts")], indirect=["gate"])
def test_shapes(eng, states, gate, which):
    state = states["B"]
    pre = state[2]
    delta = _shape_delta(states, which)
    want = rm.counts_of(pre, delta)
    print("model counters", want)
    post = copy.deepcopy(pre)
    dc.apply(post, delta)
    acct, st, _ = state
    eng.upload(acct, st)
    assert eng.root_retaining() == _oracle_root(pre)
    eng.capture_reverts(True)
    assert eng.incremental_root(*_raw_delta(delta)) == _oracle_root(post)
    assert _took(eng.incremental_counters(), gate)
    _revert_is(eng, pre, delta)
    assert eng.unwind() == _oracle_root(pre)
    _state_is(eng, pre)


def test_borrowed_storage_at_an_8_byte_offset(eng, states):
    # the segment copy moves 16 bytes per lane when the resident storage
    # array allows it; a borrowed array that is only 8-byte aligned takes
    # the 8-byte form
    import torch
    acct, st, pre = states["B"]
    first, last, _ = states["B-keys"]
    delta = ([(first, 0, 0, KE, 1), (last, 0, 0, KE, 1)], [])

    def offset_by_8(rows):
        raw = torch.zeros(rows.nbytes + 16, dtype=torch.uint8, device="cuda")
        off = (8 - raw.data_ptr() % 16) % 16
        view = raw[off:off + rows.nbytes].view(len(rows), rows.itemsize)
        view.copy_(torch.from_numpy(rows.view(np.uint8).reshape(view.shape)))
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        return view

    a_t, s_t = offset_by_8(acct), offset_by_8(st)
    torch.cuda.synchronize()
    try:
        eng.set_device_tensors(a_t, s_t)
        assert eng.root_retaining() == _oracle_root(pre)
        eng.capture_reverts(True)
        post = copy.deepcopy(pre)
        dc.apply(post, delta)
        assert eng.incremental_root(*_raw_delta(delta)) == _oracle_root(post)
        _revert_is(eng, pre, delta)
        assert eng.revert_counters()["wiped_rows"] == 1400
        assert eng.unwind() == _oracle_root(pre)
        _state_is(eng, pre)
    finally:
        eng.release_borrowed()


def test_emptying_the_state_and_back(eng, states):
    state = states["S"]
    pre = state[2]
    delta = ([(k, 0, 0, KE, 1) for k in sorted(pre)], [])
    _arm(eng, state)
    eng.capture_reverts(True)
    root = eng.incremental_root(*_raw_delta(delta))
    assert root == pyref.EMPTY_ROOT_HASH and eng.resident_counts() == (0, 0)
    _revert_is(eng, pre, delta)
    assert eng.revert_counters()["wiped_rows"] == dc.n_slots(pre)
    # an emptied state keeps no retention (sre.h): arm it again, then unwind
    with pytest.raises(RuntimeError, match=NEEDS_CELLS):
        eng.unwind()
    assert eng.root_retaining() == root
    assert eng.unwind() == _oracle_root(pre)
    _state_is(eng, pre)


# ---- contract --------------------------------------------------------------

def _bytes_of(eng):
    a, s = eng.revert()
    return a.tobytes(), s.tobytes(), eng.revert_counts(), eng.revert_counters()


def test_capture_is_off_by_default(states):
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    try:
        acct, st, pre = states["S"]
        e.upload(acct, st)
        e.root_retaining()
        with pytest.raises(RuntimeError, match=NO_REVERT):
            e.unwind()
        with pytest.raises(RuntimeError, match=NO_REVERT):
            e.unwind_with_updates()
        delta = dc.good_delta(pre, np.random.default_rng(70), 1)
        post = copy.deepcopy(pre)
        dc.apply(post, delta)
        assert e.incremental_root(*_raw_delta(delta)) == _oracle_root(post)
        assert e.revert_counts() == (0, 0)
        assert e.revert_counters() == {"acct_rows": 0, "st_rows": 0,
                                       "wiped_rows": 0, "no_row": 0}
        with pytest.raises(RuntimeError, match=NO_REVERT):
            e.unwind()
        # nothing changed: the next delta still chains
        assert e.incremental_root(NO_DELTA) == _oracle_root(post)
    finally:
        e.close()


@pytest.mark.parametrize("gate,kind",
                         [(p, k) for p in ("general", "closed", "small")
                          for k in PATHS[p][2]], indirect=["gate"])
def test_rejected_delta_leaves_the_stored_revert(eng, states, gate, kind):
    path = gate
    state = states[PATHS[path][0]]
    pre = state[2]
    first = _delta_for(path, pre, 1)
    post = copy.deepcopy(pre)
    dc.apply(post, first)
    _arm(eng, state)
    eng.capture_reverts(True)
    eng.incremental_root(*_raw_delta(first))
    before = _bytes_of(eng)
    assert before[2] != (0, 0)
    case = dc.KINDS[kind](post, np.random.default_rng(71))
    assert dc.verdict(post, *case.bad) == case.token
    with pytest.raises(RuntimeError, match=case.token):
        eng.incremental_root(*_raw_delta(case.bad))
    assert _bytes_of(eng) == before
    # cell retention stayed armed (sre.h): the unwind still works
    assert eng.unwind() == _oracle_root(pre)
    _state_is(eng, pre)


def test_what_clears_the_stored_revert(eng, states):
    state = states["S"]
    acct, st, pre = state
    delta = dc.good_delta(pre, np.random.default_rng(72), 1)

    def stored():
        _arm(eng, state)
        eng.capture_reverts(True)
        eng.apply_delta(*_raw_delta(delta))
        assert eng.revert_counts() != (0, 0)

    stored()
    eng.upload(acct, st)
    assert eng.revert_counts() == (0, 0)
    stored()
    eng.upload_plain(*plain.gen_plain_numpy(4, np.array([1, 0, 2, 0])))
    assert eng.revert_counts() == (0, 0) and eng.resident_counts() == (4, 3)
    stored()
    eng.capture_reverts(False)
    assert eng.revert_counts() == (0, 0)
    assert eng.revert_counters()["acct_rows"] == 0
    eng.root_retaining()
    with pytest.raises(RuntimeError, match=NO_REVERT):
        eng.unwind()


def test_revert_get_with_a_wrong_count(eng, states):
    state = states["S"]
    pre = state[2]
    delta = dc.good_delta(pre, np.random.default_rng(73), 1)
    _arm(eng, state)
    eng.capture_reverts(True)
    eng.incremental_root(*_raw_delta(delta))
    before = _bytes_of(eng)
    na, ns = before[2]
    ctx = ctypes.c_void_p(eng._ctx)
    for wa, ws in ((na + 1, ns), (na, ns - 1), (0, 0)):
        a = np.full(wa + 1, 0xAB, dtype=np.uint8).repeat(DELTA_DTYPE.itemsize)
        s = np.full(ws + 1, 0xAB, dtype=np.uint8).repeat(STORAGE_DTYPE.itemsize)
        rc = eng._lib.sre_revert_get(
            ctx, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(wa),
            s.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(ws))
        msg = eng._lib.sre_last_error(ctx).decode()
        assert rc != 0 and "sre_revert_get" in msg and "internal" not in msg
        assert (a == 0xAB).all() and (s == 0xAB).all()  # nothing written
    assert _bytes_of(eng) == before


def test_unwind_needs_armed_retention(eng, states):
    state = states["S"]
    pre = state[2]
    delta = dc.good_delta(pre, np.random.default_rng(74), 1)
    _arm(eng, state)
    eng.capture_reverts(True)
    eng.apply_delta(*_raw_delta(delta))  # disarms all retention (sre.h)
    _revert_is(eng, pre, delta)
    before = _bytes_of(eng)
    with pytest.raises(RuntimeError, match=NEEDS_CELLS):
        eng.unwind()
    assert _bytes_of(eng) == before
    # "a fresh sre_root_retaining followed by applying the revert"
    post = copy.deepcopy(pre)
    dc.apply(post, delta)
    assert eng.root_retaining() == _oracle_root(post)
    assert eng.unwind() == _oracle_root(pre)
    _state_is(eng, pre)
