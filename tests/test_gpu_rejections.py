"""What a rejected call leaves behind — the "Failed calls" paragraph of
include/sre.h, pinned per kind of bad input, per merge path and per entry
point.

The bad deltas, their good twins and the expected tokens come from
tests/delta_contract.py (a key-only model; its non-vacuity is checked
without a GPU in test_delta_contract_cpu.py). The states are the smallest
that reach every merge path:

  S = gen_state_numpy(96, 8): 768 slots; with SRE_ST_SMALL_MIN=0 the
      closed-form storage merge takes n_st <= 768 >> 8 = 3 rows;
  A = gen_state_numpy(128, 0): accounts only; with SRE_SD_FORCE=1 the
      one-pass account merge runs once a first incremental step has
      armed the retained lcp;
  D = the dense-cell state of tests/dense_cells.py, for the entries that
      leave cell retention armed: S and A capture no cell at all (see
      PATHS), so only D shows that the armed retention is still usable.

Which path a rejected call would have taken cannot be read off the
rejected call. It is read off its twin — a valid delta with the same
(n_acct, n_st, destroyed) counts, which are all the gates look at — on a
fresh upload, before the bad delta is tried.

Per case the assertions run in a fixed order: (1) the message, (2) the
resident state through calls that do not look at retention, (3) retention,
(4) re-arm and go on. An engine that adopted a delta before rejecting it
fails (2) and never reaches (3), where its stale retained positions
would be used.
"""
import copy
import ctypes
import os

import numpy as np
import pytest

from oracle import bind, pyref
from reth_amd import gen
from reth_amd.engine import DELTA_DTYPE
from tests import delta_contract as dc
from tests import dense_cells
from tests.test_gpu_incremental import _arrays_of, _dict_of
from tests.test_gpu_incremental_updates import _apply_diff, _rowmap

pytestmark = pytest.mark.gpu

STATES = {"S": (96, 8), "A": (128, 0)}

# merge path -> (state, environment gates, kinds that can reach it)
PATHS = {
    "general": ("S", {}, tuple(dc.KINDS)),
    "closed": ("S", {"SRE_ST_SMALL_MIN": "0"}, tuple(dc.KINDS)),
    "small": ("A", {"SRE_SD_FORCE": "1"}, dc.ACCOUNT_KINDS),
    # S and A are random keccak keys: no two of their accounts share four
    # nibbles, so nothing is captured and "the failed call
    # neither refreshed nor dropped the capture" compares 0 with 0 there.
    # D is the dense-cell state (tests/dense_cells.py: 608 accounts, 2426
    # slots, 24 captured cells of several accounts each); on it the twin
    # after a rejection has to seed retained subtrees, which gives the
    # oracle root only if they still describe the resident arrays.
    "general-dense": ("D", {}, ("K1", "K5", "K6-before", "K6-between",
                                "K6-after")),
    "closed-dense": ("D", {"SRE_ST_SMALL_MIN": "0"},
                     ("K1", "K5", "K6-before", "K6-between", "K6-after")),
}

# include/sre.h "Failed calls" -> what a REJECTED call leaves armed:
# entry: (cell retention, row snapshot)
ARMED_AFTER_REJECTION = {
    # "sre_apply_delta and sre_root_from_nodes disarm all retention on
    #  entry, rejected or not"
    "apply_delta": (False, False),
    "root_from_nodes": (False, False),
    # "plain sre_incremental_root disarms the row snapshot on entry,
    #  rejected or not, and leaves cell retention armed when it rejects"
    "incremental_root": (True, False),
    # "a rejected sre_incremental_root_with_updates leaves both armed"
    "incremental_root_with_updates": (True, True),
}
# the small account merge exists inside the incremental calls only
INCREMENTAL = ("incremental_root", "incremental_root_with_updates")
ENTRIES = {
    "general": tuple(ARMED_AFTER_REJECTION),
    "closed": tuple(ARMED_AFTER_REJECTION),
    "small": INCREMENTAL,
    "general-dense": INCREMENTAL,  # the entries that leave cells armed
    "closed-dense": INCREMENTAL,
}

NEEDS_CELLS = "needs sre_root_retaining first"
NEEDS_SNAP = "needs sre_root_retaining_with_updates first"
NO_DELTA = np.zeros(0, DELTA_DTYPE)


@pytest.fixture(scope="module")
def eng():
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def states():
    out = {}
    for name, (na, slots) in STATES.items():
        acct, st = gen.gen_state_numpy(na, slots, bind.keccak256_batch)
        out[name] = (acct, st, _dict_of(acct, st))
    dense = dense_cells.build_state(scale=0.55, slots=True)
    out["D"] = _arrays_of(dense) + (dense,)
    return out


@pytest.fixture()
def gate(request):
    """Selects a merge path through the engine's test gates (getenv is read
    per call) and restores the environment afterwards."""
    env = PATHS[request.param][1]
    os.environ.update(env)
    yield request.param
    for k in env:
        os.environ.pop(k, None)


def _raw_delta(delta):
    """_mk_delta without the sort: the rows reach the engine in the order
    they are written down."""
    rows, strows = delta
    d = np.zeros(len(rows), dtype=DELTA_DTYPE)
    for i, (k, n, b, ch, dead) in enumerate(rows):
        d[i]["key"] = np.frombuffer(k, np.uint8)
        d[i]["nonce"] = n
        d[i]["balance"] = np.frombuffer(b.to_bytes(32, "big"), np.uint8)
        d[i]["code_hash"] = np.frombuffer(ch, np.uint8)
        d[i]["deleted"] = dead
    s = np.zeros(len(strows), dtype=bind.STORAGE_DTYPE)
    for i, (a, sk, v) in enumerate(strows):
        s[i]["acct_key"] = np.frombuffer(a, np.uint8)
        s[i]["slot_key"] = np.frombuffer(sk, np.uint8)
        s[i]["value"] = np.frombuffer(v.to_bytes(32, "big"), np.uint8)
    return d, s


def _oracle_root(accounts):
    return bind.state_root(*_arrays_of(accounts))


def _oracle_rows(accounts):
    root, rows = bind.state_root_with_updates(*_arrays_of(accounts))
    return root, _rowmap(rows)


def _updates_count(eng):
    return eng._lib.sre_updates_count(ctypes.c_void_p(eng._ctx))


def _took(cnt, path):
    """the incremental counters of a successful call show `path`"""
    merge = path.split("-")[0]
    return (cnt["small_acct_merge"], cnt["small_st_merge"]) == \
        (int(merge == "small"), int(merge == "closed"))


def _call(eng, entry, delta, nodes=None):
    """One delta through `entry`; returns (root or None, diff or None)."""
    d, s = _raw_delta(delta)
    if entry == "apply_delta":
        eng.apply_delta(d, s)
        return None, None
    if entry == "incremental_root":
        return eng.incremental_root(d, s), None
    if entry == "incremental_root_with_updates":
        return eng.incremental_root_with_updates(d, s)
    return eng.root_from_nodes(nodes, d, s), None


def _rejected(eng, entry, case, nodes=None):
    """step 1: the call raises with the model's token and does not blame
    the engine"""
    with pytest.raises(RuntimeError) as ei:
        _call(eng, entry, case.bad, nodes)
    msg = str(ei.value)
    assert case.token in msg, msg
    assert "internal" not in msg, msg


def _state_is(eng, accounts):
    """step 2: the resident state, through calls that do not read retention"""
    arrays = _arrays_of(accounts)
    assert eng.root() == bind.state_root(*arrays)
    assert np.array_equal(eng.storage_roots(len(accounts)),
                          bind.storage_roots(*arrays))


_path_proven = set()


def _prove_path(eng, state, path, kind, twin):
    """The twin, on a fresh upload, takes `path` (once per path and kind:
    builders and states are deterministic)."""
    if (path, kind) in _path_proven:
        return
    acct, st, accounts = state
    accounts = copy.deepcopy(accounts)
    eng.upload(acct, st)
    eng.root_retaining()
    eng.incremental_root(NO_DELTA)  # arms the lcp repair of the small path
    root, _ = _call(eng, "incremental_root", twin)
    cnt = eng.incremental_counters()
    dc.apply(accounts, twin)
    assert root == _oracle_root(accounts)
    assert _took(cnt, path), (path, kind, cnt)
    _path_proven.add((path, kind))


def _cases():
    for path, (_, _, kinds) in PATHS.items():
        for entry in ENTRIES[path]:
            for kind in kinds:
                yield pytest.param(path, entry, kind,
                                   id=f"{path}-{entry}-{kind}")


@pytest.mark.parametrize("gate,entry,kind", list(_cases()), indirect=["gate"])
def test_rejected_delta(eng, states, gate, entry, kind):
    path = gate
    state = states[PATHS[path][0]]
    acct, st, accounts = state
    accounts = copy.deepcopy(accounts)
    case = dc.KINDS[kind](accounts, np.random.default_rng(11))
    assert dc.verdict(accounts, *case.bad) == case.token
    _prove_path(eng, state, path, kind, case.twin)

    eng.upload(acct, st)
    _, nodes = eng.root_with_updates()
    root0, rows0 = eng.root_retaining_with_updates()  # cells AND snapshot armed
    want0, cur = _oracle_rows(accounts)
    assert root0 == want0 and _rowmap(rows0) == cur
    # the last successful incremental call before the rejection
    root, diff = eng.incremental_root_with_updates(NO_DELTA)
    assert root == root0 and len(diff) == 0
    captured = eng.incremental_counters()["captured"]
    dense = PATHS[path][0] == "D"
    assert captured == len(dense_cells.captured(accounts)) and \
        (captured > 0) == dense

    # 1. the message
    _rejected(eng, entry, case, nodes)
    # 2. nothing the caller can observe later has changed
    if entry == "incremental_root_with_updates":
        assert _updates_count(eng) == 0
    _state_is(eng, accounts)
    # 3. retention is exactly as the header says
    cells, snap = ARMED_AFTER_REJECTION[entry]
    twin = _raw_delta(case.twin)
    if not snap:
        with pytest.raises(RuntimeError, match=NEEDS_SNAP):
            eng.incremental_root_with_updates(*twin)
    if not cells:
        with pytest.raises(RuntimeError, match=NEEDS_CELLS):
            eng.incremental_root(*twin)
        _state_is(eng, accounts)
    else:
        if snap:
            root, diff = eng.incremental_root_with_updates(*twin)
        else:
            root, diff = eng.incremental_root(*twin), None
        cnt = eng.incremental_counters()
        dc.apply(accounts, case.twin)
        want, want_rows = _oracle_rows(accounts)
        assert root == want
        # the failed call neither refreshed nor dropped the capture
        assert cnt["examined"] == captured
        assert (cnt["seeded"] > 0) == dense, cnt
        assert _took(cnt, path), cnt
        if snap:
            assert _apply_diff(cur, diff) == want_rows
    # 4. re-arm and go on: the twin where it has not run yet, else the
    # twin of a second case built on the state as it is now
    assert eng.root_retaining() == _oracle_root(accounts)
    follow = case.twin
    if cells:
        follow = dc.KINDS[kind](accounts, np.random.default_rng(12)).twin
    root, _ = _call(eng, "incremental_root", follow)
    dc.apply(accounts, follow)
    assert root == _oracle_root(accounts)
    _state_is(eng, accounts)


@pytest.mark.parametrize("gate", ["general", "closed"], indirect=True)
def test_from_nodes_removal_row_leaves_the_state(eng, states, gate):
    acct, st, accounts = states["S"]
    eng.upload(acct, st)
    _, nodes = eng.root_with_updates()
    eng.root_retaining_with_updates()
    bad = nodes.copy()
    bad[len(bad) // 2]["removed"] = 1
    twin = dc.k6_row_for_unknown(accounts, np.random.default_rng(13),
                                 "between").twin
    with pytest.raises(RuntimeError, match="removal rows") as ei:
        eng.root_from_nodes(bad, *_raw_delta(twin))
    assert "internal" not in str(ei.value)
    _state_is(eng, accounts)
    with pytest.raises(RuntimeError, match=NEEDS_SNAP):
        eng.incremental_root_with_updates(*_raw_delta(twin))
    with pytest.raises(RuntimeError, match=NEEDS_CELLS):
        eng.incremental_root(*_raw_delta(twin))
    accounts = copy.deepcopy(accounts)
    dc.apply(accounts, twin)
    assert eng.root_from_nodes(nodes, *_raw_delta(twin)) == \
        _oracle_root(accounts)


def _control_cases():
    for path in ("general", "closed"):
        for entry in ENTRIES[path]:
            for name in dc.CONTROLS:
                yield pytest.param(path, entry, name,
                                   id=f"{path}-{entry}-{name}")


@pytest.mark.parametrize("gate,entry,name", list(_control_cases()),
                         indirect=["gate"])
def test_accepted_controls(eng, states, gate, entry, name):
    # C1: "a zero-valued storage row for an unknown account is a no-op
    # deletion and is accepted"; C2: the owner is upserted by the delta
    acct, st, accounts = states["S"]
    accounts = copy.deepcopy(accounts)
    delta = dc.CONTROLS[name](accounts, np.random.default_rng(14))
    eng.upload(acct, st)
    _, nodes = eng.root_with_updates()
    _, rows0 = eng.root_retaining_with_updates()
    cur = _rowmap(rows0)
    root, diff = _call(eng, entry, delta, nodes)
    if entry.startswith("incremental"):
        assert _took(eng.incremental_counters(), gate)
    dc.apply(accounts, delta)
    want, want_rows = _oracle_rows(accounts)
    assert root in (None, want)
    if diff is not None:
        assert _apply_diff(cur, diff) == want_rows
    _state_is(eng, accounts)


# ---- a chain with failures in it -----------------------------------------

def _proof_refs(accounts, targets, pair):
    tup = {k: tuple(v) for k, v in accounts.items()}
    want = []
    for t in targets:
        with pyref.accelerated(bind.keccak256):
            want.append(pyref.account_proof(tup, t))
    with pyref.accelerated(bind.keccak256):
        want_st = pyref.storage_proof({pair[0]: tup[pair[0]]}, *pair)
    return want, want_st


def _read_only_calls(eng, accounts, rng, rows_too):
    arrays = _arrays_of(accounts)
    want = bind.state_root(*arrays)
    _state_is(eng, accounts)
    assert eng.finish_top(*eng.subtree_roots()) == want
    keys = sorted(accounts)
    targets = [keys[int(rng.integers(len(keys)))],
               dc.unknown_key(accounts, "between")]
    ak = next(k for k in keys[int(rng.integers(len(keys) // 2)):]
              if accounts[k][3])
    pair = (ak, sorted(accounts[ak][3])[0])
    want_proofs, (want_sroot, want_snodes) = _proof_refs(accounts, targets,
                                                         pair)
    assert eng.account_proof(targets) == want_proofs
    sroots, sproofs = eng.storage_proof([pair[0]], [pair[1]])
    assert sroots == [want_sroot] and sproofs == [want_snodes]
    if rows_too:
        root, rows = eng.root_with_updates()
        assert root == want
        assert _rowmap(rows) == _rowmap(
            bind.state_root_with_updates(*arrays)[1])


@pytest.mark.parametrize("with_updates", [True, False],
                         ids=["with_updates", "plain"])
@pytest.mark.parametrize("gate", ["general", "closed"], indirect=True)
def test_chain_with_failures(eng, states, gate, with_updates):
    path = gate
    acct, st, accounts = states["S"]
    accounts = copy.deepcopy(accounts)
    entry = "incremental_root_with_updates" if with_updates \
        else "incremental_root"
    rng = np.random.default_rng(15)
    # 5 rejections per run, 4 runs: every kind comes up at least twice
    run = 2 * (path == "closed") + (not with_updates)
    kinds = list(dc.KINDS)
    eng.upload(acct, st)
    if with_updates:
        _, rows0 = eng.root_retaining_with_updates()
        cur = _rowmap(rows0)
    else:
        eng.root_retaining()
    for step in range(6):
        # the closed-form gate is n_st <= ns >> 8 on the state of the moment
        max_st = min(3, dc.n_slots(accounts) >> 8) if path == "closed" else 3
        good = dc.good_delta(accounts, rng, step, max_st)
        root, diff = _call(eng, entry, good)
        cnt = eng.incremental_counters()
        dc.apply(accounts, good)
        want, want_rows = _oracle_rows(accounts)
        assert root == want, f"step {step}"
        assert _took(cnt, path), f"step {step}: {cnt}"
        if with_updates:
            cur = _apply_diff(cur, diff)
            assert cur == want_rows, f"step {step}"
        if step == 5:
            break
        kind = kinds[(5 * run + step) % len(kinds)]
        _rejected(eng, entry, dc.KINDS[kind](accounts, rng))
        if with_updates:
            assert _updates_count(eng) == 0
        _read_only_calls(eng, accounts, rng, with_updates)


# ---- argument rejections of the read-only calls ---------------------------

@pytest.fixture()
def resident(eng, states):
    acct, st, accounts = states["S"]
    eng.upload(acct, st)
    root = bind.state_root(acct, st)
    assert eng.root() == root
    return accounts, root


def _targets(accounts):
    keys = sorted(accounts)
    return [keys[5], dc.unknown_key(accounts, "between"), keys[-1]]


def _pairs(accounts):
    keys = sorted(accounts)
    a, b = keys[7], keys[40]
    return ([a, b, b], [sorted(accounts[a][3])[0], sorted(accounts[b][3])[-1],
                        bind.keccak256(b"no such slot")])


def _good_account_proof(eng, accounts, **caps):
    targets = _targets(accounts)
    tup = {k: tuple(v) for k, v in accounts.items()}
    got = eng.account_proof(targets, **caps)
    for t, nodes in zip(targets, got):
        with pyref.accelerated(bind.keccak256):
            assert nodes == pyref.account_proof(tup, t), t.hex()
    return got


def _good_storage_proof(eng, accounts, **caps):
    aks, sks = _pairs(accounts)
    roots, proofs = eng.storage_proof(aks, sks, **caps)
    for a, s, root, nodes in zip(aks, sks, roots, proofs):
        with pyref.accelerated(bind.keccak256):
            want = pyref.storage_proof({a: tuple(accounts[a])}, a, s)
        assert (root, nodes) == want, (a.hex(), s.hex())
    return proofs


@pytest.mark.parametrize("n", [0, 4097])
def test_account_proof_target_count(eng, resident, n):
    accounts, root = resident
    targets = [bind.keccak256(i.to_bytes(2, "big")) for i in range(n)]
    with pytest.raises(RuntimeError, match=r"sre_account_proof: 1\.\.4096 targets"):
        eng.account_proof(targets, cap_nodes=4096, cap_lens=8)
    assert eng.root() == root
    _good_account_proof(eng, accounts)


@pytest.mark.parametrize("n", [0, 4097])
def test_storage_proof_target_count(eng, resident, n):
    accounts, root = resident
    targets = [bind.keccak256(i.to_bytes(2, "big")) for i in range(n)]
    with pytest.raises(RuntimeError, match=r"sre_storage_proof: 1\.\.4096 targets"):
        eng.storage_proof(targets, targets, cap_nodes=4096, cap_lens=8)
    assert eng.root() == root
    _good_storage_proof(eng, accounts)


@pytest.mark.parametrize("which", ["account", "storage"])
def test_proof_output_capacity(eng, resident, which):
    accounts, root = resident
    good = _good_account_proof if which == "account" else _good_storage_proof
    proofs = good(eng, accounts)
    need_lens = sum(len(p) for p in proofs)
    need_nodes = sum(len(n) for p in proofs for n in p)
    assert need_lens >= 4 and need_nodes > 32 * need_lens
    msg = f"sre_{which}_proof: output capacity exceeded"
    for caps in ({"cap_lens": need_lens - 1, "cap_nodes": need_nodes},
                 {"cap_lens": need_lens, "cap_nodes": need_nodes - 1}):
        with pytest.raises(RuntimeError, match=msg):
            good(eng, accounts, **caps)
        assert eng.root() == root
    # what the query needs, to the byte, is enough
    assert good(eng, accounts, cap_lens=need_lens,
                cap_nodes=need_nodes) == proofs


@pytest.mark.parametrize("off", [-1, 1])
def test_storage_roots_count(eng, resident, off):
    accounts, root = resident
    with pytest.raises(RuntimeError,
                       match="sre_storage_roots: n != uploaded account count"):
        eng.storage_roots(len(accounts) + off)
    _state_is(eng, accounts)


def test_keccak_long_len_past_stride(eng, resident):
    import torch
    accounts, root = resident
    msgs = np.random.default_rng(16).integers(0, 256, (5, 200), dtype=np.uint8)
    t = torch.from_numpy(msgs).cuda()
    out = torch.zeros((5, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="sre_keccak_long_device: len > stride"):
        eng.keccak_long_device(t, 201, out)
    assert eng.root() == root
    got = eng.keccak_long_device(t, 200, out).cpu().numpy()
    for row, m in zip(got, msgs):
        assert bytes(row) == bind.keccak256(m.tobytes())


@pytest.mark.parametrize("fn", ["sre_upload_accounts", "sre_upload_storage",
                                "sre_set_accounts_device",
                                "sre_set_storage_device"])
def test_entry_limit_checked_before_anything_is_read(eng, resident, fn):
    # 2^32 - 1 entries announced over an 8-entry buffer: the limit check
    # comes before any copy or allocation, so the buffer is never read
    import torch
    accounts, root = resident
    itemsize = 104 if "accounts" in fn else 96
    if "device" in fn:
        buf = torch.zeros((8, itemsize), dtype=torch.uint8, device="cuda")
        ptr = ctypes.c_void_p(buf.data_ptr())
    else:
        buf = np.zeros((8, itemsize), dtype=np.uint8)
        ptr = buf.ctypes.data_as(ctypes.c_void_p)
    ctx = ctypes.c_void_p(eng._ctx)
    rc = getattr(eng._lib, fn)(ctx, ptr, ctypes.c_uint64(2**32 - 1))
    assert rc != 0
    assert "2^32-1" in eng._lib.sre_last_error(ctx).decode()
    _state_is(eng, accounts)
